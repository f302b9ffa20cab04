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
The guidance loop's band decode (pipeline.latent2sdf_band) runs the same scheme on the 65^3 grid, for several
images in lockstep through hierarchical_grid_logits_batch.

There is no CPU path: the binding raises when the library is missing or of another version.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L_
from ._lib import FohoError, _p, _stream, vp

SO_PATH = L_.side_path("vol")
VERSION = L_.SIDE_VERSIONS["vol"]      # FOHO_VOL_VERSION of csrc/foho_vol.h
CLOSE_ALL = 1           # FOHO_VOL_CLOSE_ALL
_i32, _i64, _rc = ctypes.c_int32, ctypes.c_int64, ctypes.c_int
_SIGNATURES = {
    "foho_vol_mark": (_rc, [vp, _i32, _i32, vp, vp, vp]), "foho_vol_select": (_rc, [vp, vp, _i32, vp, vp, vp]),
    "foho_vol_close": (_rc, [vp, vp, _i32, _i32, vp, vp, vp, vp]), "foho_vol_count": (_rc, [vp, _i64, vp, vp, vp]),
    "foho_vol_emit": (_rc, [vp, _i32, _i32, vp, vp, vp, vp, vp]), "foho_vol_fill": (_rc, [vp, _i32, vp, vp]),
    "foho_vol_scatter": (_rc, [vp, vp, _i64, vp, vp]), "foho_vol_count_blocks": (_i64, [_i64])}


def lib():
    return L_.load_side("vol", _SIGNATURES)


def _check(status, what):
    L_.check_side(lib(), "foho_vol", status, what)


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
    """Point masks of several images -> per image (ascending int32 indices, fp16-rounded xyz): foho_vol_count per image into its own
    slot of one int32[B] tensor, ONE read-back of all the counts, foho_vol_emit per image.  `reads` counts the read-backs."""

    def __init__(self, tables, res, n_images, device):
        self.tables, self.res, self.device = tables, res, device
        self.totals = torch.zeros(max(int(n_images), 1), dtype=torch.int32, device=device)
        self.reads = 0

    def __call__(self, sels, r):
        """sels: {image: point mask over the (r+1)^3 points of level r} -> {image: (idx, xyz)}."""
        L = lib()
        n_points = (r + 1) ** 3
        nb = int(L.foho_vol_count_blocks(n_points))
        st = _stream(self.device)
        boff = {}
        for b, sel in sels.items():
            boff[b] = torch.empty(nb, dtype=torch.int32, device=self.device)
            _check(L.foho_vol_count(_p(sel), n_points, _p(boff[b]), _p(self.totals[b:b + 1]), st), "foho_vol_count")
        if not sels:
            return {}
        counts = self.totals.tolist()
        self.reads += 1
        out = {}
        for b, sel in sels.items():
            n = int(counts[b])
            idx = torch.empty(n, dtype=torch.int32, device=self.device)
            xyz = torch.empty(n, 3, dtype=torch.float32, device=self.device)
            if n:
                _check(L.foho_vol_emit(_p(sel), r, self.res, _p(self.tables), _p(boff[b]), _p(idx), _p(xyz), st), "foho_vol_emit")
            out[b] = (idx, xyz)
        return out


def _decoded(decode, xyz, n):
    vals = decode(xyz).reshape(-1).to(torch.float32).contiguous() if n else xyz.new_empty(0)
    if vals.numel() != n:
        raise FohoError(f"hierarchical decode: the decoder returned {vals.numel()} values for {n} points")
    return vals


def hierarchical_grid_logits(decode, bmin, bmax, res, min_res=None, band=1, max_rounds=8, device=None):
    """decode: points (N, 3) float32 -> logits (N,) float32 on `device` (default: the current GPU).

    -> (logits (res+1)^3 float32 in the flattened "ij" layout of the dense path, stats): decoded values equal the dense decode at
    those points; every other point carries a fill value of the right sign (see the module's docstring for the contract and its
    limit).  stats: levels, decoded per level, closure rounds and the points each decoded, total decoded, decoded fraction,
    fallback."""
    fields, stats, _ = hierarchical_grid_logits_batch([decode], bmin, bmax, res, min_res=min_res, band=band, max_rounds=max_rounds,
                                                      device=device)
    return fields[0], stats[0]


def hierarchical_grid_logits_batch(decodes, bmin, bmax, res, min_res=None, band=1, max_rounds=8, device=None):
    """hierarchical_grid_logits for B images in lockstep: decodes[b] is image b's decode callable.  Every level and every closure round
    reads the point counts of all images back at once (one host read each, not one per image); an image whose closure has settled
    decodes nothing in later rounds.  Each image's kernels and decoder calls are the ones its own hierarchical_grid_logits makes, in
    the same order, so its field and stats are the same.

    -> (list of B fields, list of B stats, host reads)."""
    res, min_res = check_levels(res, min_res)
    band, max_rounds = int(band), int(max_rounds)
    if band < 0 or max_rounds < 0:
        raise FohoError(f"hierarchical decode: band {band} and max_rounds {max_rounds} must be >= 0")
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    B = len(decodes)
    imgs = range(B)
    L = lib()
    st = _stream(device)
    tables = axis_tables(bmin, bmax, res).to(device)
    emit = _Compactor(tables, res, B, device)

    # level 0: the dense (min_res+1)^3 grid -- the same points for every image
    r = min_res
    dec = [_mask((r + 1) ** 3, device, -1) for _ in imgs]
    idx, xyz = emit({0: _mask((r + 1) ** 3, device, -1)}, r)[0] if B else (None, None)
    field, stats = [], []
    for b in imgs:
        vals = _decoded(decodes[b], xyz, idx.numel())
        field.append(torch.empty((r + 1) ** 3, dtype=torch.float32, device=device))
        _check(L.foho_vol_scatter(_p(idx), _p(vals), idx.numel(), _p(field[b]), st), "foho_vol_scatter")
        stats.append({"levels": [r], "decoded_per_level": [int(idx.numel())]})
    # levels 1..L: points inside active coarse cells
    while r < res:
        cells, n_fine = r ** 3, (2 * r + 1) ** 3
        sels, fdec = {}, []
        for b in imgs:
            mixed, active = _mask(cells, device), _mask(cells, device)
            _check(L.foho_vol_mark(_p(field[b]), r, band, _p(mixed), _p(active), st), "foho_vol_mark")
            sels[b], fd = _mask(n_fine, device), _mask(n_fine, device)
            _check(L.foho_vol_select(_p(active), _p(dec[b]), r, _p(sels[b]), _p(fd), st), "foho_vol_select")
            fdec.append(fd)
            del mixed, active
        got = emit(sels, 2 * r)
        for b in imgs:
            idx, xyz = got[b]
            vals = _decoded(decodes[b], xyz, idx.numel())
            fine = torch.empty(n_fine, dtype=torch.float32, device=device)
            _check(L.foho_vol_fill(_p(field[b]), r, _p(fine), st), "foho_vol_fill")
            _check(L.foho_vol_scatter(_p(idx), _p(vals), idx.numel(), _p(fine), st), "foho_vol_scatter")
            field[b] = fine
            stats[b]["levels"].append(2 * r)
            stats[b]["decoded_per_level"].append(int(idx.numel()))
        dec, r = fdec, 2 * r
    # closure at the final level, for the images that have not settled yet
    cubes = res ** 3
    bad, near, sel = _mask(cubes, device), _mask(cubes, device), {b: _mask((res + 1) ** 3, device) for b in imgs}
    rounds, closure, fallback = [0] * B, [[] for _ in imgs], [False] * B
    open_ = list(imgs)
    while open_:
        for b in open_:
            _check(L.foho_vol_close(_p(field[b]), _p(dec[b]), res, 0, _p(bad), _p(near), _p(sel[b]), st), "foho_vol_close")
        got = emit({b: sel[b] for b in open_}, res)
        open_ = [b for b in open_ if got[b][0].numel()]
        falls = [b for b in open_ if rounds[b] == max_rounds]
        for b in falls:                    # not settled: this round's points and every other point still undecoded
            fallback[b] = True
            _check(L.foho_vol_close(_p(field[b]), _p(dec[b]), res, CLOSE_ALL, None, None, _p(sel[b]), st), "foho_vol_close")
        rest = emit({b: sel[b] for b in falls}, res)
        for b in open_:
            idx, xyz = got[b]
            if b in rest:
                idx2, xyz2 = rest[b]
                idx, order = torch.sort(torch.cat([idx, idx2]))           # one ascending list, like every other decode's
                xyz = torch.cat([xyz, xyz2])[order]
            vals = _decoded(decodes[b], xyz, idx.numel())
            _check(L.foho_vol_scatter(_p(idx), _p(vals), idx.numel(), _p(field[b]), st), "foho_vol_scatter")
            closure[b].append(int(idx.numel()))
            if not fallback[b]:
                rounds[b] += 1
        open_ = [b for b in open_ if not fallback[b]]
    for b in imgs:
        total = sum(stats[b]["decoded_per_level"]) + sum(closure[b])
        stats[b].update(closure_rounds=rounds[b], closure_decoded=closure[b], decoded=total, decoded_fraction=total / (res + 1) ** 3,
                        fallback=fallback[b], band=band, max_rounds=max_rounds)
    return field, stats, emit.reads
