"""Scenes and the numpy restatement for tests/test_raster_k.py (the K-fragment rasteriser, libfoho_rastk.so).

Scenes are (verts_ndc (V,3) float32 [x_ndc, y_ndc, z_view], faces (F,3) int64).  The oracle of every comparison is
oracle.clib.rasterize on verts[faces]; its results are computed once per (scene, frame, blur, K, cull) and shared."""
import functools

import numpy as np
import torch

from followmyhold_amd import synthetic
from oracle import clib
from oracle import ref_ops as R

BLUR = R.blur_radius_from_sigma()
K_ALL = 128          # the oracle's whole fragment set of a pixel, as long as the pixel holds fewer


@functools.lru_cache(maxsize=None)
def two_spheres(H, W, seed=2):
    """A 320-face icosphere and a second one, scaled and shifted so that the two overlap; every vertex jittered from a fixed seed
    (an unjittered icosphere is symmetric: mirror faces would share depths exactly).  640 faces, up to 4 layers plus edge fragments."""
    v, f = synthetic.icosphere(2, 0.4)
    assert len(f) == 320
    rng = np.random.default_rng(seed)
    v2 = v * np.float32(0.7) + np.array([0.12, 0.06, 0.05], np.float32)
    vv = np.concatenate([v, v2]).astype(np.float32)
    vv = vv + rng.normal(scale=0.004, size=vv.shape).astype(np.float32) + np.array([0.05, -0.02, -2.0], np.float32)
    ff = np.concatenate([f, f + len(v)]).astype(np.int64)
    ndc = R.world_to_ndc(torch.from_numpy(vv), R.Camera(50.0, H, W)).contiguous()
    return ndc.numpy().astype(np.float32), ff


@functools.lru_cache(maxsize=None)
def long_lists(H=32, W=32, n_small=600, seed=3):
    """One triangle covering the frame and n_small small faces stacked over the 8x8 tile (1, 1), every face at a depth of its own:
    that tile's list holds n_small + 1 faces (ten LDS chunks of 64) and its pixels hold far more than 128 fragments."""
    rng = np.random.default_rng(seed)
    verts = [[-3.0, -3.0, 5.0], [3.0, -3.0, 5.0], [0.0, 3.0, 5.0]]
    faces = [[0, 1, 2]]
    cx, cy = 1.0 - 24.0 / W, 1.0 - 24.0 / H            # centre of tile (1, 1)
    for i in range(n_small):
        a0 = rng.uniform(0, 2 * np.pi)
        c = np.array([cx, cy]) + rng.normal(scale=0.04, size=2)
        z = 1.0 + 0.004 * i + rng.uniform(0, 0.001)
        for j in range(3):
            a = a0 + 2 * np.pi * j / 3
            verts.append([c[0] + 0.22 * np.cos(a), c[1] + 0.22 * np.sin(a), z])
        faces.append([3 * i + 3, 3 * i + 4, 3 * i + 5])
    order = rng.permutation(len(faces))                 # face ids are not in depth order
    return np.asarray(verts, np.float32), np.asarray(faces, np.int64)[order]


@functools.lru_cache(maxsize=None)
def near_plane():
    """The straddling faces of tests/test_oracle_kat.py (one vertex behind the plane z = 0.005: two sub-triangles; two behind: one)
    and a plain face behind them."""
    P3 = np.array([[[0.0, -0.0009, 0.002], [0.006, 0.004, 0.011], [-0.005, 0.005, 0.013]],
                   [[0.0, 0.0006, 0.012], [-0.004, -0.0015, 0.002], [0.004, -0.0012, 0.003]]], np.float64)
    v = np.concatenate([P3[..., :2] / P3[..., 2:3], P3[..., 2:3]], -1).reshape(-1, 3).astype(np.float32)
    far = np.array([[-0.9, -0.9, 0.5], [0.9, -0.9, 0.5], [0.0, 0.9, 0.5]], np.float32)
    return np.concatenate([v, far]), np.arange(9, dtype=np.int64).reshape(3, 3)


def coplanar_pair():
    a = np.array([[-0.5, -0.5, 3.0], [0.5, -0.5, 3.0], [0.0, 0.5, 3.0]], np.float32)
    return np.concatenate([a, a]), np.arange(6, dtype=np.int64).reshape(2, 3)


_ORACLE = {}


def oracle(name, verts, faces, H, W, blur, K, cull=False):
    """clib.rasterize(verts[faces]) -> (pix_to_face, zbuf, bary, dists), cached under `name` (arrays are not hashable)."""
    key = (name, H, W, float(blur), int(K), bool(cull))
    if key not in _ORACLE:
        _ORACLE[key] = clib.rasterize(verts[faces], H, W, blur, K=K, cull_backfaces=cull)
    return _ORACLE[key]


def tie_pixels(p2f, zb):
    """(H,W) bool: pixels on which two fragments of the oracle's K-buffer share a depth exactly."""
    z = np.where(p2f >= 0, zb, np.nan)
    zs = np.sort(z, axis=-1)                             # NaN (background) sorts last
    with np.errstate(invalid="ignore"):
        return (zs[..., 1:] == zs[..., :-1]).any(-1)


def select_sort(full, K):
    """The (z, face id, sub) rule on the oracle's whole fragment set `full` = rasterize(..., K=K_ALL): per pixel the K smallest keys
    (z bits << 32 | face id), ascending, padded with -1.  A pixel holds one fragment per face at most (the neighbour rule), so
    the sub-triangle bit never decides.  Only valid where the pixel holds fewer than K_ALL fragments (the caller checks)."""
    p2f, zb, ba, di = full
    H, W, KA = p2f.shape
    hit = p2f >= 0
    zbits = zb.view(np.uint32).astype(np.uint64)
    assert (zb[hit] >= 0).all()                         # non-negative floats order as their bits
    key = np.where(hit, (zbits << np.uint64(32)) | p2f.astype(np.uint64), np.uint64(2 ** 64 - 1))
    assert K <= KA
    order = np.argsort(key, axis=-1, kind="stable")[..., :K]
    take = lambda a: np.take_along_axis(a, order, axis=-1)
    keep = take(hit) & (np.arange(K) < hit.sum(-1, keepdims=True))
    o_p2f = np.where(keep, take(p2f), -1)
    o_zb = np.where(keep, take(zb), np.float32(-1))
    o_di = np.where(keep, take(di), np.float32(-1))
    o_ba = np.where(keep[..., None], np.take_along_axis(ba, order[..., None], axis=-2), np.float32(-1))
    return o_p2f, o_zb, o_ba, o_di
