"""numpy restatement of the hierarchical final decode (followmyhold_amd/volume.py, csrc/foho_vol.hip) for the tests to compare
against: mark (mixed cells, dilated by `band`), select / emit (points in active cells that are not exact yet, ascending), fill
(midpoint means in the kernel's summation order, float32), close (corners of the 27 cubes around every sign-changing cube
with an undecoded corner; after `max_rounds` rounds every undecoded point).  Fields are (n, n, n) float32 arrays, x slowest."""
import numpy as np


def axis_tables(bmin, bmax, res):
    """(3, res+1) float32: generate_dense_grid_points' per-axis coordinates, rounded to fp16 and back."""
    return np.stack([np.linspace(bmin[k], bmax[k], res + 1, dtype=np.float32) for k in range(3)]).astype(np.float16).astype(np.float32)


def inside(f):
    return f > 0                      # -logit < 0: FlexiCubes' inside


def mixed_cells(f):
    """(r, r, r) bool: cells whose 8 corners of the (r+1)^3 field are not all of one side."""
    ins = inside(f)
    cnt = np.zeros(tuple(s - 1 for s in f.shape), np.int32)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                cnt += ins[a:a + cnt.shape[0], b:b + cnt.shape[1], c:c + cnt.shape[2]]
    return (cnt != 0) & (cnt != 8)


def dilate(m, band):
    """Chebyshev dilation by `band` cells (separable: a box is the product of three intervals)."""
    out = m.copy()
    for ax in range(3):
        src, acc = out, out.copy()
        n = m.shape[ax]
        for d in range(1, band + 1):
            if d >= n:
                break
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[ax], hi[ax] = slice(0, n - d), slice(d, n)
            acc[tuple(lo)] |= src[tuple(hi)]
            acc[tuple(hi)] |= src[tuple(lo)]
        out = acc
    return out


def _cells_to_points(cells, fine):
    """Bool over points touching a True cell.  fine=True: cells of resolution r -> points of the (2r+1)^3 level (point I lies in
    cells (I-1)//2 .. I//2); fine=False: cubes of resolution R -> their corners, the (R+1)^3 points (point I: cubes I-1, I)."""
    out = cells
    for ax in range(3):
        n = out.shape[ax]
        m = 2 * n + 1 if fine else n + 1
        shape = list(out.shape)
        shape[ax] = m
        res = np.zeros(shape, bool)
        for I in range(m):
            lo, hi = (max((I - 1) >> 1, 0), min(I >> 1, n - 1)) if fine else (max(I - 1, 0), min(I, n - 1))
            sl = [slice(None)] * 3
            sl[ax] = I
            src = [slice(None)] * 3
            src[ax] = slice(lo, hi + 1)
            res[tuple(sl)] = out[tuple(src)].any(axis=ax)
        out = res
    return out


def fill(c):
    """(2r+1)^3 float32 from the (r+1)^3 coarse field: values at even indices, means of 2 / 4 / 8 corners otherwise, summed with the
    x-corner outermost and the z-corner innermost, then scaled by 1/2, 1/4 or 1/8 -- foho_vol_fill's arithmetic."""
    r = c.shape[0] - 1
    f = np.empty((2 * r + 1,) * 3, np.float32)
    for oi in (0, 1):
        for oj in (0, 1):
            for ok in (0, 1):
                ni, nj, nk = r + 1 - oi, r + 1 - oj, r + 1 - ok
                s = None
                for a in range(oi + 1):
                    for b in range(oj + 1):
                        for d in range(ok + 1):
                            v = c[a:a + ni, b:b + nj, d:d + nk]
                            s = v.copy() if s is None else (s + v).astype(np.float32)
                odd = oi + oj + ok
                if odd:
                    s = (s * np.float32(0.5 ** odd)).astype(np.float32)
                f[oi::2, oj::2, ok::2] = s
    return f


def coords(flat_idx, r, tables):
    """xyz (N, 3) float32 of level points (flattened (r+1)^3 indices) on the final grid's tables."""
    G = r + 1
    R = tables.shape[1] - 1
    s = R // r
    i, j, k = flat_idx // (G * G), (flat_idx // G) % G, flat_idx % G
    return np.stack([tables[0][i * s], tables[1][j * s], tables[2][k * s]], 1).astype(np.float32)


def hierarchical(decode, bmin, bmax, res, min_res=None, band=1, max_rounds=8):
    """decode: (N, 3) float32 -> (N,) float32.  -> (field (res+1)^3 float32, decoded point mask, stats, index lists): the index
    lists are the ascending flat indices every decode got, level by level then round by round ((level r, indices) pairs)."""
    min_res = res // 4 if min_res is None else min_res
    tab = axis_tables(bmin, bmax, res)
    r = min_res
    idx = np.arange((r + 1) ** 3)
    field = np.asarray(decode(coords(idx, r, tab)), np.float32).reshape((r + 1,) * 3)
    dec = np.ones_like(field, bool)
    lists = [(r, idx)]
    stats = {"levels": [r], "decoded_per_level": [idx.size]}
    while r < res:
        active = dilate(mixed_cells(field), band)
        carried = np.zeros((2 * r + 1,) * 3, bool)
        carried[::2, ::2, ::2] = dec
        sel = _cells_to_points(active, True) & ~carried
        idx = np.flatnonzero(sel)
        fine = fill(field)
        if idx.size:
            fine.reshape(-1)[idx] = np.asarray(decode(coords(idx, 2 * r, tab)), np.float32).reshape(-1)
        field, dec, r = fine, sel | carried, 2 * r
        lists.append((r, idx))
        stats["levels"].append(r)
        stats["decoded_per_level"].append(idx.size)
    rounds, closure, fallback = 0, [], False
    while True:
        all_dec = np.ones((res,) * 3, bool)
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    all_dec &= dec[a:a + res, b:b + res, c:c + res]
        bad = mixed_cells(field) & ~all_dec
        add = _cells_to_points(dilate(bad, 1), False) & ~dec
        if not add.any():
            break
        fallback = rounds == max_rounds
        if fallback:
            add = ~dec
        idx = np.flatnonzero(add)
        field.reshape(-1)[idx] = np.asarray(decode(coords(idx, res, tab)), np.float32).reshape(-1)
        dec |= add
        lists.append((res, idx))
        closure.append(idx.size)
        if fallback:
            break
        rounds += 1
    total = sum(stats["decoded_per_level"]) + sum(closure)
    stats.update(closure_rounds=rounds, closure_decoded=closure, decoded=total, decoded_fraction=total / (res + 1) ** 3, fallback=fallback)
    return field, dec, stats, lists


def dense(decode, bmin, bmax, res):
    tab = axis_tables(bmin, bmax, res)
    return np.asarray(decode(coords(np.arange((res + 1) ** 3), res, tab)), np.float32).reshape((res + 1,) * 3)
