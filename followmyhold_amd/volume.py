"""Hierarchical final decode: the (res+1)^3 grid of the last `latent2sdf` (PL:1623-1642) queried only near the surface.

A dense decode of the 385^3 grid is 57 M decoder rows, and FlexiCubes reads values only at the corners of cubes whose corners
differ in sign (inside <=> -logit < 0 <=> logit > 0); everywhere else it reads the sign.  `hierarchical_grid_logits` decodes a
coarse (min_res+1)^3 grid, then, level by level at twice the resolution, only the points inside coarse cells whose corners are
mixed (dilated by `band` cells); every other point gets the midpoint mean of its enclosing coarse corners, which has their
common sign.  At the final level a closure loop decodes the corners of every sign-changing cube that still has an undecoded
corner (and of its 26 neighbours) until there is none.

Contract: the decoder computes each query row on its own (HipGeoDecoder: GEMM rows, LayerNorm and attention per row), and every
point is queried at the coordinates the dense path uses (generate_dense_grid_points, then .half().float(), PL:303).  So every
decoded value equals the dense decode's bit for bit, every cube that changes sign in the result has all 8 corners decoded, and
FlexiCubes builds the dense path's mesh index for index.  If `max_rounds` closure rounds do not settle, every remaining point is
decoded (`fallback`): an unverified band is never returned.

Known limit: a surface component lying entirely inside cells that the coarse level sees as one sign is missed (FlashVDM's
hierarchical decoding has the same limit).  That is why the mode is opt-in and the dense decode stays the default.

The kernels are libfoho_vol.so's (csrc/foho_vol.hip, C ABI csrc/foho_vol.h): mark, select, close, count, emit, fill, scatter.
There is no CPU path: the binding raises when the library is missing or of another version.
"""
import ctypes
import os

import numpy as np
import torch

from ._lib import FohoError, vp

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libfoho_vol.so")
VERSION = 100           # FOHO_VOL_VERSION of csrc/foho_vol.h
CLOSE_ALL = 1           # FOHO_VOL_CLOSE_ALL
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise FohoError(f"{SO_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)")
        L = ctypes.CDLL(SO_PATH)
        L.foho_vol_version.restype = ctypes.c_int
        if L.foho_vol_version() != VERSION:
            raise FohoError(f"{SO_PATH} is version {L.foho_vol_version()}, this binding is {VERSION}: rebuild (make -C followmyhold_amd/csrc)")
        L.foho_vol_last_error.restype = ctypes.c_char_p
        i32, i64 = ctypes.c_int32, ctypes.c_int64
        sig = {"foho_vol_mark": [vp, i32, i32, vp, vp, vp], "foho_vol_select": [vp, vp, i32, vp, vp, vp],
               "foho_vol_close": [vp, vp, i32, i32, vp, vp, vp, vp], "foho_vol_count": [vp, i64, vp, vp, vp],
               "foho_vol_emit": [vp, i32, i32, vp, vp, vp, vp, vp], "foho_vol_fill": [vp, i32, vp, vp],
               "foho_vol_scatter": [vp, vp, i64, vp, vp]}
        for name, args in sig.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = ctypes.c_int, args
        L.foho_vol_count_blocks.restype, L.foho_vol_count_blocks.argtypes = ctypes.c_int64, [ctypes.c_int64]
        _lib = L
    return _lib


def _check(status, what):
    if status != 0:
        raise FohoError(f"{what} failed ({status}): {lib().foho_vol_last_error().decode()}")


def _p(t):
    return None if t is None else vp(t.data_ptr())


def _stream(device):
    return vp(torch.cuda.current_stream(device).cuda_stream)


def _mask(n, device, fill=0):
    return torch.full(((n + 63) // 64,), fill, dtype=torch.int64, device=device)


def check_levels(res, min_res=None):
    """(res, min_res) after validation: res / min_res a power of two, min_res >= 8.  min_res defaults to res / 4."""
    res = int(res)
    min_res = res // 4 if min_res is None else int(min_res)
    if min_res < 8 or res < min_res or res % min_res or (res // min_res) & (res // min_res - 1):
        raise FohoError(f"hierarchical decode: final resolution {res} over min_res {min_res} must be a power of two, with min_res >= 8")
    if res > 1024:
        raise FohoError(f"hierarchical decode: resolution {res} above 1024")
    return res, min_res


def axis_tables(bmin, bmax, res):
    """(3, res+1) float32: per axis the coordinates generate_dense_grid_points gives the final grid (numpy float32 linspace),
    rounded to fp16 and back like the query points of the dense path (PL:303, HipGeoDecoder.grid_queries)."""
    t = np.stack([np.linspace(bmin[k], bmax[k], int(res) + 1, dtype=np.float32) for k in range(3)])
    return torch.from_numpy(t).half().float()


class _Compactor:
    """Point mask -> (ascending int32 indices, fp16-rounded xyz): foho_vol_count, one read-back of the count, foho_vol_emit."""

    def __init__(self, tables, res, device):
        self.tables, self.res, self.device = tables, res, device
        self.total = torch.zeros(1, dtype=torch.int32, device=device)

    def __call__(self, sel, r):
        L = lib()
        n_points = (r + 1) ** 3
        boff = torch.empty(int(L.foho_vol_count_blocks(n_points)), dtype=torch.int32, device=self.device)
        st = _stream(self.device)
        _check(L.foho_vol_count(_p(sel), n_points, _p(boff), _p(self.total), st), "foho_vol_count")
        n = int(self.total.item())
        idx = torch.empty(n, dtype=torch.int32, device=self.device)
        xyz = torch.empty(n, 3, dtype=torch.float32, device=self.device)
        if n:
            _check(L.foho_vol_emit(_p(sel), r, self.res, _p(self.tables), _p(boff), _p(idx), _p(xyz), st), "foho_vol_emit")
        return idx, xyz


def hierarchical_grid_logits(decode, bmin, bmax, res, min_res=None, band=1, max_rounds=8, device=None):
    """decode: points (N, 3) float32 -> logits (N,) float32 on `device` (default: the current GPU).

    -> (logits (res+1)^3 float32 in the flattened "ij" layout of the dense path, stats): decoded values equal the dense decode at
    those points; every other point carries a fill value of the right sign (see the module's docstring for the contract and its
    limit).  stats: levels, decoded per level, closure rounds and the points each decoded, total decoded, decoded fraction,
    fallback."""
    res, min_res = check_levels(res, min_res)
    band, max_rounds = int(band), int(max_rounds)
    if band < 0 or max_rounds < 0:
        raise FohoError(f"hierarchical decode: band {band} and max_rounds {max_rounds} must be >= 0")
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    L = lib()
    st = _stream(device)
    tables = axis_tables(bmin, bmax, res).to(device)
    emit = _Compactor(tables, res, device)

    def run(sel, r):
        idx, xyz = emit(sel, r)
        vals = decode(xyz).reshape(-1).to(torch.float32).contiguous() if idx.numel() else idx.float()
        if vals.numel() != idx.numel():
            raise FohoError(f"hierarchical decode: the decoder returned {vals.numel()} values for {idx.numel()} points")
        return idx, vals

    # level 0: the dense (min_res+1)^3 grid
    r = min_res
    dec = _mask((r + 1) ** 3, device, -1)
    idx, vals = run(_mask((r + 1) ** 3, device, -1), r)
    field = torch.empty((r + 1) ** 3, dtype=torch.float32, device=device)
    _check(L.foho_vol_scatter(_p(idx), _p(vals), idx.numel(), _p(field), st), "foho_vol_scatter")
    stats = {"levels": [r], "decoded_per_level": [int(idx.numel())]}
    # levels 1..L: points inside active coarse cells
    while r < res:
        cells = r ** 3
        mixed, active = _mask(cells, device), _mask(cells, device)
        _check(L.foho_vol_mark(_p(field), r, band, _p(mixed), _p(active), st), "foho_vol_mark")
        n_fine = (2 * r + 1) ** 3
        sel, fdec = _mask(n_fine, device), _mask(n_fine, device)
        _check(L.foho_vol_select(_p(active), _p(dec), r, _p(sel), _p(fdec), st), "foho_vol_select")
        del mixed, active
        idx, vals = run(sel, 2 * r)
        fine = torch.empty(n_fine, dtype=torch.float32, device=device)
        _check(L.foho_vol_fill(_p(field), r, _p(fine), st), "foho_vol_fill")
        _check(L.foho_vol_scatter(_p(idx), _p(vals), idx.numel(), _p(fine), st), "foho_vol_scatter")
        field, dec, r = fine, fdec, 2 * r
        stats["levels"].append(r)
        stats["decoded_per_level"].append(int(idx.numel()))
    # closure at the final level
    cubes = res ** 3
    bad, near, sel = _mask(cubes, device), _mask(cubes, device), _mask((res + 1) ** 3, device)
    rounds, closure, fallback = 0, [], False
    while True:
        _check(L.foho_vol_close(_p(field), _p(dec), res, 0, _p(bad), _p(near), _p(sel), st), "foho_vol_close")
        idx, xyz = emit(sel, res)
        if idx.numel() == 0:
            break
        fallback = rounds == max_rounds
        if fallback:                       # not settled: this round's points and every other point still undecoded
            _check(L.foho_vol_close(_p(field), _p(dec), res, CLOSE_ALL, None, None, _p(sel), st), "foho_vol_close")
            idx2, xyz2 = emit(sel, res)
            idx, order = torch.sort(torch.cat([idx, idx2]))           # one ascending list, like every other decode's
            xyz = torch.cat([xyz, xyz2])[order]
        vals = decode(xyz).reshape(-1).to(torch.float32).contiguous()
        if vals.numel() != idx.numel():
            raise FohoError(f"hierarchical decode: the decoder returned {vals.numel()} values for {idx.numel()} points")
        _check(L.foho_vol_scatter(_p(idx), _p(vals), idx.numel(), _p(field), st), "foho_vol_scatter")
        closure.append(int(idx.numel()))
        if fallback:
            break
        rounds += 1
    total = sum(stats["decoded_per_level"]) + sum(closure)
    stats.update(closure_rounds=rounds, closure_decoded=closure, decoded=total, decoded_fraction=total / (res + 1) ** 3,
                 fallback=fallback, band=band, max_rounds=max_rounds)
    return field, stats
