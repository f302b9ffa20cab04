"""Sparse FlexiCubes: the mesh of `ops.flexicubes(x_dense, s, res)` from the field and three per-axis coordinate tables.

`ops.flexicubes` wants the dense (res+1)^3 x 3 array of grid positions (685 MB at res 384, built on the host) and a workspace of
9 B per cube + 8 B per grid edge (1.9 GB at res 384), and walks every cube and edge.  FlexiCubes reads positions only at the corners
of the cubes whose corners differ in sign.  `flexicubes_sparse` marks those cubes (a bit mask and prefix sums, about 8 MB at res
384), reads their number back, and extracts on the compact list: the same vertices bit for bit, the same faces and l_dev, in the
same order.  Work and memory outside the field are proportional to the number of surface cubes.

Two host reads per extraction: the number of surface cubes (it sizes the workspace and the outputs: at most 4 vertices and 6
triangles per cube, so there is no retry loop), then the vertex and triangle counts.

`flexicubes_sparse` is forward only: it is the extractor of the no-gradient final step and refuses a field that requires grad.
`flexicubes_sparse_grad` is the same extraction as a torch.autograd.Function: it keeps the mark buffer and the cube workspace (22 B per
surface cube) and its backward is foho_sflexi_bwd, dL/ds by gather -- the thread that owns a grid point sums the point's at most 24
terms in a fixed order and stores once, so the gradient is bitwise repeatable (ops.flexicubes' backward adds with float atomics).  There
is no gradient to the axis tables.

The kernels are libfoho_sflexi.so's (csrc/foho_sflexi.hip, C ABI csrc/foho_sflexi.h).  There is no CPU path: the binding raises
when the library is missing or of another version.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L_
from ._lib import FohoError, _p, _stream, vp

SO_PATH = L_.side_path("sflexi")
VERSION = L_.SIDE_VERSIONS["sflexi"]      # FOHO_SFLEXI_VERSION of csrc/foho_sflexi.h
MAX_RES = 1024          # FOHO_SFLEXI_MAX_RES
MAX_CUBES = 1 << 26     # FOHO_SFLEXI_MAX_CUBES
OVER_VERTS, OVER_FACES, OVER_CUBES = 1, 2, 4
_i32, _sz, _rc = ctypes.c_int32, ctypes.c_size_t, ctypes.c_int
_SIGNATURES = {
    "foho_sflexi_mark_bytes": (_sz, [_i32]), "foho_sflexi_cube_bytes": (_sz, [_i32]), "foho_sflexi_workspace_bytes": (_sz, [_i32, _i32]),
    "foho_sflexi_mark": (_rc, [vp, _i32, vp, _sz, vp, vp]),
    "foho_sflexi_extract": (_rc, [vp, vp, _i32, vp, _sz, _i32, vp, _i32, vp, _i32, vp, vp, vp, _sz, vp]),
    "foho_sflexi_bwd": (_rc, [vp, vp, _i32, vp, _sz, _i32, vp, _i32, vp, vp, _sz, vp])}


def lib():
    return L_.load_side("sflexi", _SIGNATURES)


def _check(status, what):
    L_.check_side(lib(), "foho_sflexi", status, what)


def grid_axes(bbox_min, bbox_max, res):
    """(3, res+1) float32: per axis the coordinates generate_dense_grid_points gives the grid (numpy float32 linspace), NOT rounded to
    fp16: the extractor of the dense route gets the unrounded grid (volume.axis_tables rounds, because its tables feed decoder
    queries)."""
    return torch.from_numpy(np.stack([np.linspace(bbox_min[k], bbox_max[k], int(res) + 1, dtype=np.float32) for k in range(3)]))


def _extract(who, axes, s, res):
    """The two calls behind `who` (flexicubes_sparse / flexicubes_sparse_grad) -> ((verts, faces, l_dev), stats, kept), kept = what
    foho_sflexi_bwd needs: (axes, field, mark buffer, cube workspace or None, surface cubes)."""
    if not isinstance(s, torch.Tensor) or not s.is_cuda:
        raise FohoError(f"{who} needs a CUDA/HIP field (there is no CPU fallback)")
    if res < 1 or res > MAX_RES:
        raise FohoError(f"{who}: resolution {res} outside 1 .. {MAX_RES}")
    G = res + 1
    dev = s.device
    ss = s.detach().to(torch.float32).contiguous().reshape(-1)
    ax = torch.as_tensor(axes).detach().to(device=dev, dtype=torch.float32).contiguous()
    if ax.shape != (3, G) or ss.numel() != G ** 3:
        raise FohoError(f"{who}: expected {(3, G)} axis tables and {G ** 3} SDF values")
    L = lib()
    st = _stream(dev)
    n_marks = L.foho_sflexi_mark_bytes(res)
    marks = torch.empty(n_marks, dtype=torch.uint8, device=dev)
    n_dev = torch.empty(1, dtype=torch.int32, device=dev)
    _check(L.foho_sflexi_mark(_p(ss), res, _p(marks), n_marks, _p(n_dev), st), "foho_sflexi_mark")
    n = int(n_dev.item())                    # host read 1: the surface cubes size everything below
    if n > MAX_CUBES:
        raise FohoError(f"{who}: {n} surface cubes, above {MAX_CUBES}: not a surface (use ops.flexicubes)")
    stats = {"cubes": n, "vertices": 0, "faces": 0, "workspace_bytes": int(n_marks)}
    if n == 0:
        out = (torch.empty(0, 3, device=dev), torch.empty(0, 3, dtype=torch.int64, device=dev), torch.empty(0, device=dev))
        return out, stats, (ax, ss, marks, None, 0)
    n_ws = L.foho_sflexi_cube_bytes(n)
    ws = torch.empty(n_ws, dtype=torch.uint8, device=dev)
    verts_cap, faces_cap = 4 * n, 6 * n
    verts = torch.empty(verts_cap, 3, device=dev)
    faces = torch.empty(faces_cap, 3, dtype=torch.int64, device=dev)
    ldev = torch.empty(verts_cap, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    _check(L.foho_sflexi_extract(_p(ax), _p(ss), res, _p(marks), n_marks, n, _p(verts), verts_cap, _p(faces), faces_cap, _p(ldev),
                                 _p(counts), _p(ws), n_ws, st), "foho_sflexi_extract")
    nv, nf, over = counts.tolist()           # host read 2
    if over:
        raise FohoError(f"{who}: overflow bits {over} with capacities sized from the cube count ({n} cubes, {nv} vertices, {nf} faces)")
    stats.update(vertices=nv, faces=nf, workspace_bytes=int(n_marks + n_ws))
    out = (verts[:nv].clone(), faces[:nf].clone(), ldev[:nv].clone())       # the capacity-sized buffers are not kept alive
    return out, stats, (ax, ss, marks, ws, n)


def flexicubes_sparse(axes, s, res, return_stats=False):
    """axes: (3, res+1) float32 (grid_axes); s: (res+1)^3 values, negative inside, in the "ij" layout of generate_dense_grid_points.
    -> (verts (V,3), faces (F,3) int64, l_dev (V,)) on s's device, equal to ops.flexicubes(x, s, res) for the x those axes mesh to;
    with return_stats also {"cubes", "vertices", "faces", "workspace_bytes"} (workspace_bytes: mark buffer + cube workspace)."""
    if isinstance(s, torch.Tensor) and s.is_cuda and s.requires_grad:
        raise FohoError("flexicubes_sparse is forward only (the no-gradient final step): a field that requires grad goes through ops.flexicubes")
    out, stats, _ = _extract("flexicubes_sparse", axes, s, int(res))
    return out + (stats,) if return_stats else out


class _SparseFlexiFn(torch.autograd.Function):
    """flexicubes_sparse's forward with the mark buffer and the cube workspace kept; the backward is foho_sflexi_bwd."""

    @staticmethod
    def forward(ctx, s, axes, res, box):
        out, box["stats"], (ax, ss, marks, ws, n) = _extract("flexicubes_sparse_grad", axes, s, res)
        ctx.kept = (ax, ss, marks, ws)
        ctx.res, ctx.n, ctx.nv = res, n, out[0].shape[0]
        ctx.s_meta = (s.shape, s.dtype)
        ctx.mark_non_differentiable(out[1], out[2])
        return out

    @staticmethod
    def backward(ctx, g_verts, _gf, _gl):
        ax, ss, marks, ws = ctx.kept
        gs = torch.zeros_like(ss)
        if ctx.n > 0 and ctx.nv > 0:         # no surface cube: zeros, nothing launched
            g = g_verts.detach().to(torch.float32).contiguous()
            L = lib()
            _check(L.foho_sflexi_bwd(_p(ax), _p(ss), ctx.res, _p(marks), marks.numel(), ctx.n, _p(g), ctx.nv, _p(gs), _p(ws), ws.numel(),
                                     _stream(ss.device)), "foho_sflexi_bwd")
        # the gradient in the shape and dtype of the caller's field (a (G,G,G) or half-precision SDF is a legal input)
        return gs.view(ctx.s_meta[0]).to(ctx.s_meta[1]), None, None, None


def flexicubes_sparse_grad(axes, s, res, return_stats=False):
    """flexicubes_sparse -- the same arguments, the same outputs bit for bit, the same two host reads, the same stats -- differentiable
    with respect to s: (verts * g).sum().backward() leaves dL/ds in s.grad, in s's shape and dtype, bitwise equal from run to run and
    from stream to stream.  faces and l_dev carry no gradient; axes that require grad are refused (there is no gradient to them)."""
    if isinstance(axes, torch.Tensor) and axes.requires_grad:
        raise FohoError("flexicubes_sparse_grad: there is no gradient to the axis tables (pass them detached); ops.flexicubes has a "
                        "gradient to the grid positions")
    box = {}
    out = _SparseFlexiFn.apply(s, axes, int(res), box)
    return tuple(out) + (box["stats"],) if return_stats else tuple(out)
