"""Weighted FlexiCubes: `ops.flexicubes` with the three weight sets and the training-mode triangulation, forward and gradient.

`ops.flexicubes` extracts Dual Marching Cubes -- FlexiCubes with every weight at 1.  `flexicubes_weighted` takes the normalised,
strictly positive weights alpha (res^3, 8) per cube corner, beta (res^3, 12) per cube edge and gamma (res^3,) per cube (None = ones):
alpha moves the crossings, beta moves a dual vertex inside its cube, gamma chooses the quad split, or, with training=True, blends the
quad's centre vertex (appended behind the dual vertices, four triangles a quad).  l_dev is differentiable.  Semantics, orderings, the
tie rule and the l_dev convention: csrc/foho_wflexi.h.  With unit weights and training=False the outputs are bitwise ops.flexicubes'.

Gradients reach x, s, alpha, beta and, in training mode, gamma, without float atomics: they are bitwise repeatable.

The kernels are libfoho_wflexi.so's (csrc/foho_wflexi.hip, C ABI csrc/foho_wflexi.h).  There is no CPU path: the binding raises when
the library is missing or of another version.
"""
import ctypes

import torch

from . import _lib as L_
from ._lib import FohoError, _p, _stream, vp

SO_PATH = L_.side_path("wflexi")
VERSION = L_.SIDE_VERSIONS["wflexi"]      # FOHO_WFLEXI_VERSION of csrc/foho_wflexi.h
MAX_RES = 256                             # FOHO_WFLEXI_MAX_RES
OVER_VERTS, OVER_FACES = 1, 2
_i32, _sz, _rc = ctypes.c_int32, ctypes.c_size_t, ctypes.c_int
_SIGNATURES = {
    "foho_wflexi_workspace_bytes": (_sz, [_i32, _i32]), "foho_wflexi_bwd_bytes": (_sz, [_i32]),
    # x s alpha beta gamma, res training, verts verts_cap, faces faces_cap, l_dev counts, workspace bytes, stream
    "foho_wflexi_fwd": (_rc, [vp, vp, vp, vp, vp, _i32, _i32, vp, _i32, vp, _i32, vp, vp, vp, _sz, vp]),
    # x s alpha beta gamma, res training, verts n_verts n_all n_cubes, grad_verts grad_l_dev, grad_s grad_x grad_alpha grad_beta grad_gamma,
    # workspace bytes verts_cap, scratch bytes, stream
    "foho_wflexi_bwd": (_rc, [vp, vp, vp, vp, vp, _i32, _i32, vp, _i32, _i32, _i32, vp, vp, vp, vp, vp, vp, vp, vp, _sz, _i32, vp, _sz, vp])}


def lib():
    return L_.load_side("wflexi", _SIGNATURES)


def _check(status, what):
    L_.check_side(lib(), "foho_wflexi", status, what)


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


class _WFlexiFn(torch.autograd.Function):
    """foho_wflexi_fwd with the workspace kept; the backward is foho_wflexi_bwd."""

    @staticmethod
    def forward(ctx, x, s, alpha, beta, gamma, res, training, verts_cap, faces_cap):
        L = lib()
        xx, ss = _f32(x), _f32(s).reshape(-1)
        al, be, ga = (None if w is None else _f32(w) for w in (alpha, beta, gamma))
        if ga is not None:
            ga = ga.reshape(-1)
        dev = xx.device
        st = _stream(dev)
        counts = torch.zeros(5, dtype=torch.int32, device=dev)
        while True:
            nws = L.foho_wflexi_workspace_bytes(res, verts_cap)
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            verts = torch.empty(verts_cap, 3, device=dev)
            faces = torch.empty(faces_cap, 3, dtype=torch.int64, device=dev)
            ldev = torch.empty(verts_cap, device=dev)
            _check(L.foho_wflexi_fwd(_p(xx), _p(ss), _p(al), _p(be), _p(ga), res, int(training), _p(verts), verts_cap, _p(faces), faces_cap,
                                     _p(ldev), _p(counts), _p(ws), nws, st), "foho_wflexi_fwd")
            nv, n_all, nf, over, n_cubes = counts.tolist()     # the output sizes are data dependent: one host sync per extraction
            if not over:
                break
            verts_cap, faces_cap = max(verts_cap, n_all), max(faces_cap, nf)
        v_out, f_out, l_out = verts[:n_all], faces[:nf], ldev[:nv]
        ctx.save_for_backward(xx, ss, al, be, ga, ws, v_out)
        ctx.cfg = (res, int(training), nv, n_all, n_cubes, verts_cap)
        ctx.meta = [None if t is None else (t.shape, t.dtype) for t in (x, s, alpha, beta, gamma)]
        ctx.mark_non_differentiable(f_out)
        return v_out, f_out, l_out

    @staticmethod
    def backward(ctx, g_verts, _gf, g_ldev):
        xx, ss, al, be, ga, ws, verts = ctx.saved_tensors
        res, training, nv, n_all, n_cubes, verts_cap = ctx.cfg
        need = ctx.needs_input_grad[:5]
        dev = xx.device
        want = [need[0], need[1], need[2] and al is not None, need[3] and be is not None, need[4] and ga is not None and bool(training)]
        like = (xx, ss, al, be, ga)
        grads = [torch.zeros_like(t) if w else None for w, t in zip(want, like)]
        if n_cubes > 0 and any(want):
            L = lib()
            nsc = L.foho_wflexi_bwd_bytes(n_cubes) if (want[0] or want[1]) else 0
            scratch = torch.empty(nsc, dtype=torch.uint8, device=dev) if nsc else None
            gv = _f32(g_verts)
            gl = None if g_ldev is None else _f32(g_ldev)
            _check(L.foho_wflexi_bwd(_p(xx), _p(ss), _p(al), _p(be), _p(ga), res, training, _p(verts), nv, n_all, n_cubes, _p(gv), _p(gl),
                                     _p(grads[1]), _p(grads[0]), _p(grads[2]), _p(grads[3]), _p(grads[4]), _p(ws), ws.numel(), verts_cap,
                                     _p(scratch), nsc, _stream(dev)), "foho_wflexi_bwd")
        # gradients in the shape and dtype the caller's tensors have
        out = [None if g is None else g.view(m[0]).to(m[1]) for g, m in zip(grads, ctx.meta)]
        return tuple(out) + (None, None, None, None)


def flexicubes_weighted(x, s, res, alpha=None, beta=None, gamma=None, training=False, verts_cap=None, faces_cap=None):
    """x ((res+1)^3, 3) grid positions, s ((res+1)^3 values, negative inside), alpha (res^3, 8), beta (res^3, 12), gamma (res^3,) or None
    -> (verts, faces (F,3) int64, l_dev (V,)).  training=False: V dual vertices, two triangles a quad, no gradient to gamma.
    training=True: the V dual vertices, then one centre per quad; four triangles a quad.  The first capacities that are too small cost
    one more extraction."""
    res = int(res)
    for t in (x, s, alpha, beta, gamma):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise FohoError("flexicubes_weighted needs CUDA/HIP tensors (there is no CPU fallback)")
    if res < 1 or res > MAX_RES:
        raise FohoError(f"flexicubes_weighted: resolution {res} outside 1 .. {MAX_RES} (the weights are dense)")
    G, C = res + 1, res ** 3
    if tuple(x.shape) != (G ** 3, 3) or s.numel() != G ** 3:
        raise FohoError(f"flexicubes_weighted: expected {(G ** 3, 3)} grid positions and {G ** 3} SDF values")
    for name, w, shape in (("alpha", alpha, (C, 8)), ("beta", beta, (C, 12)), ("gamma", gamma, (C,))):
        if w is not None and tuple(w.shape) != shape:
            raise FohoError(f"flexicubes_weighted: {name} is {tuple(w.shape)}, expected {shape}")
    verts_cap = int(verts_cap or 16 * res * res)
    faces_cap = int(faces_cap or 32 * res * res)
    return tuple(_WFlexiFn.apply(x, s, alpha, beta, gamma, res, bool(training), verts_cap, faces_cap))
