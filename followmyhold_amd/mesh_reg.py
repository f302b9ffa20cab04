"""Mesh regularisers: Laplacian smoothing (uniform, cot, cotcurv), normal consistency and edge length of one mesh, fused, with the
gradient to the vertices -- what `pytorch3d.loss.mesh_laplacian_smoothing`, `mesh_normal_consistency` and `mesh_edge_loss` compute
(their published formulas, restated in csrc/foho_mreg.h; parity with pytorch3d is unpinned).

`MeshTopology(faces, V)` builds the index tables of one connectivity once, with torch sorts and uniques on the device of `faces` (a CPU
tensor works too; one host synchronisation for the sizes and the range check).  `mesh_regularizers(verts, topo, ...)` is one call of
foho_mreg_run: at most three launches, no float atomics, terms, total and gradient bitwise repeatable.  The gradient is computed in the
forward and scaled by the incoming cotangent in the backward (once differentiable).

The kernels are libfoho_mreg.so's (csrc/foho_mreg.hip, C ABI csrc/foho_mreg.h).  There is no CPU path: the binding raises when the
library is missing or of another version, and for CPU vertices.
"""
import ctypes

import torch

from . import _lib as L_
from ._lib import FohoError, _p, _stream, vp

SO_PATH = L_.side_path("mreg")
VERSION = L_.SIDE_VERSIONS["mreg"]      # FOHO_MREG_VERSION of csrc/foho_mreg.h
METHODS = {"uniform": 0, "cot": 1, "cotcurv": 2}      # FOHO_MREG_UNIFORM, _COT, _COTCURV
TERMS = ("lap", "nc", "edge")           # the order of `terms` (FOHO_MREG_LAP, _NC, _EDGE); out[3] is the total
MAX_SHIFTED = (1 << 29) - 1             # faces and pairs are stored << 2 in an int32
_i32, _sz, _rc, _f = ctypes.c_int32, ctypes.c_size_t, ctypes.c_int, ctypes.c_float
_SIGNATURES = {
    "foho_mreg_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    # verts faces, V F E P, nbr_off nbr_idx nbr_edge, edge_off edge_fc, pairs vp_off vp_ent, method, w_lap w_nc w_edge target_length,
    # out grad, workspace bytes, stream
    "foho_mreg_run": (_rc, [vp, vp, _i32, _i32, _i32, _i32, vp, vp, vp, vp, vp, vp, vp, vp, _i32, _f, _f, _f, _f, vp, vp, vp, _sz, vp])}


def lib():
    return L_.load_side("mreg", _SIGNATURES)


def _check(status, what):
    L_.check_side(lib(), "foho_mreg", status, what)


def _offsets(owner, n):
    """(n + 1,) offsets of the lists of entries sorted by `owner` (values in [0, n))."""
    off = torch.zeros(n + 1, dtype=torch.int64, device=owner.device)
    if owner.numel():
        off[1:] = torch.cumsum(torch.bincount(owner, minlength=n), 0)
    return off


class MeshTopology:
    """The index tables of one connectivity (csrc/foho_mreg.h), int32 on the device of `faces`:
      edges (E, 2)                     the unique undirected edges, lower end first, ascending -- the rows of Meshes.edges_packed()
      nbr_off, nbr_idx, nbr_edge       per vertex its neighbours, ascending, and the edge id of every entry
      edge_off, edge_fc                per edge the ascending list of (face << 2 | corner opposite the edge)
      pairs (P, 4)                     (v0, v1, a, b) per pair of faces on one edge, by (edge, first entry, second entry)
      vp_off, vp_ent                   per vertex the ascending list of (pair << 2 | column of `pairs`)
    Faces with an index outside [0, V), or with one vertex twice, raise FohoError."""

    def __init__(self, faces, V):
        V = int(V)
        f = faces.detach().to(torch.int64).reshape(-1, 3)
        dev, F = f.device, int(f.shape[0])
        if V < 0:
            raise FohoError(f"MeshTopology: {V} vertices")
        if F > MAX_SHIFTED:
            raise FohoError(f"MeshTopology: {F} faces, at most {MAX_SHIFTED}")
        if F:
            lo_hi = torch.stack([f.min(), f.max(), ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])).sum()]).tolist()
            if lo_hi[0] < 0 or lo_hi[1] >= V:
                raise FohoError(f"MeshTopology: face indices {lo_hi[0]} .. {lo_hi[1]} outside [0, {V})")
            if lo_hi[2]:
                raise FohoError(f"MeshTopology: {lo_hi[2]} faces hold one vertex twice")
        ar = lambda n: torch.arange(n, dtype=torch.int64, device=dev)
        # half-edge c of a face is the side opposite corner c
        h0, h1 = torch.cat([f[:, 1], f[:, 2], f[:, 0]]), torch.cat([f[:, 2], f[:, 0], f[:, 1]])
        ent = (ar(F).repeat(3) << 2) | ar(3).repeat_interleave(F)
        key = torch.minimum(h0, h1) * max(V, 1) + torch.maximum(h0, h1)
        ukey, eid = torch.unique(key, return_inverse=True)               # sorted: edges by ascending (lower, higher)
        E = int(ukey.numel())
        e0, e1 = ukey // max(V, 1), ukey % max(V, 1)
        order = torch.argsort(eid * (4 * max(F, 1)) + ent)               # by (edge, entry)
        edge_fc, fc_edge = ent[order], eid[order]
        edge_off = _offsets(fc_edge, E)
        # neighbours: both directions of every edge, by (vertex, neighbour)
        src, dst, ide = torch.cat([e0, e1]), torch.cat([e1, e0]), ar(E).repeat(2)
        order = torch.argsort(src * max(V, 1) + dst)
        nbr_idx, nbr_edge, nbr_off = dst[order], ide[order], _offsets(src[order], V)
        # pairs: entry t of an edge's list with every later entry of the same list
        later = edge_off[1:][fc_edge] - 1 - ar(3 * F)
        P = int(later.sum()) if F else 0
        if P > MAX_SHIFTED:
            raise FohoError(f"MeshTopology: {P} pairs of faces on one edge, at most {MAX_SHIFTED}")
        first = ar(3 * F).repeat_interleave(later)
        start = torch.cumsum(later, 0) - later
        second = first + 1 + (ar(P) - start.repeat_interleave(later))
        opp = lambda t: f[edge_fc[t] >> 2, edge_fc[t] & 3]
        pairs = torch.stack([e0[fc_edge[first]], e1[fc_edge[first]], opp(first), opp(second)], 1) if P else torch.zeros(0, 4, dtype=torch.int64, device=dev)
        pent = ar(4 * P)                                                  # (pair << 2 | column) is the flat index of `pairs`
        owner = pairs.reshape(-1)
        order = torch.argsort(owner * (4 * max(P, 1)) + pent)
        vp_ent, vp_off = pent[order], _offsets(owner[order], V)

        i32 = lambda t: t.to(torch.int32).contiguous()
        self.V, self.F, self.E, self.P = V, F, E, P
        self.faces = i32(f)
        self.edges = i32(torch.stack([e0, e1], 1))
        self.nbr_off, self.nbr_idx, self.nbr_edge = i32(nbr_off), i32(nbr_idx), i32(nbr_edge)
        self.edge_off, self.edge_fc = i32(edge_off), i32(edge_fc)
        self.pairs, self.vp_off, self.vp_ent = i32(pairs), i32(vp_off), i32(vp_ent)

    TABLES = ("faces", "edges", "nbr_off", "nbr_idx", "nbr_edge", "edge_off", "edge_fc", "pairs", "vp_off", "vp_ent")
    device = property(lambda self: self.faces.device)

    def to(self, device):
        if torch.device(device) == self.device:
            return self
        t = object.__new__(MeshTopology)
        t.V, t.F, t.E, t.P = self.V, self.F, self.E, self.P
        for k in self.TABLES:
            setattr(t, k, getattr(self, k).to(device))
        return t

    def table_bytes(self):
        return sum(getattr(self, k).numel() * 4 for k in self.TABLES if k != "edges")


def run(verts32, topo, method, w_lap, w_nc, w_edge, target_length, want_grad=True):
    """foho_mreg_run on contiguous float32 device vertices -> out (4,) [lap, nc, edge, total], grad (V, 3) or None."""
    L = lib()
    dev = verts32.device
    nws = L.foho_mreg_workspace_bytes(topo.V, topo.E, topo.P)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    out = torch.empty(4, device=dev)
    grad = torch.empty(topo.V, 3, device=dev) if want_grad else None
    _check(L.foho_mreg_run(_p(verts32), _p(topo.faces), topo.V, topo.F, topo.E, topo.P, _p(topo.nbr_off), _p(topo.nbr_idx), _p(topo.nbr_edge),
                           _p(topo.edge_off), _p(topo.edge_fc), _p(topo.pairs), _p(topo.vp_off), _p(topo.vp_ent), method, w_lap, w_nc, w_edge,
                           target_length, _p(out), _p(grad), _p(ws), nws, _stream(dev)), "foho_mreg_run")
    return out, grad


class _MeshRegFn(torch.autograd.Function):
    """One foho_mreg_run: the gradient is computed in the forward and scaled by the incoming cotangent in the backward."""

    @staticmethod
    def forward(ctx, verts, topo, method, w_lap, w_nc, w_edge, target_length):
        out, grad = run(verts.detach().to(torch.float32).contiguous(), topo, method, w_lap, w_nc, w_edge, target_length,
                        want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(grad)
        ctx.dtype = verts.dtype
        terms = out[:3]
        ctx.mark_non_differentiable(terms)
        return out[3].clone(), terms

    @staticmethod
    def backward(ctx, g_total, _g_terms):
        (grad,) = ctx.saved_tensors
        return (grad * g_total.to(torch.float32)).to(ctx.dtype), None, None, None, None, None, None


def mesh_regularizers(verts, topo, w_lap=0.0, lap_method="uniform", w_nc=0.0, w_edge=0.0, target_length=0.0):
    """verts (V, 3) on the device, topo = MeshTopology(faces, V) -> (total, terms).  total = w_edge edge + w_lap lap + w_nc nc, a
    differentiable float32 scalar; terms = detached (3,) [lap, nc, edge], a term whose weight is 0 reported as 0 (and not computed).
    float64 or non-contiguous vertices are converted; the gradient comes back in their dtype."""
    if not (isinstance(verts, torch.Tensor) and verts.is_cuda):
        raise FohoError("mesh_regularizers needs CUDA/HIP vertices (there is no CPU fallback)")
    if not isinstance(topo, MeshTopology):
        raise FohoError("mesh_regularizers: topo must be a MeshTopology (mesh_reg.MeshTopology(faces, V))")
    if lap_method not in METHODS:
        raise FohoError(f"mesh_regularizers: lap_method {lap_method!r}, expected one of {sorted(METHODS)}")
    if tuple(verts.shape) != (topo.V, 3):
        raise FohoError(f"mesh_regularizers: verts is {tuple(verts.shape)}, the topology has {topo.V} vertices")
    if topo.device != verts.device:
        raise FohoError(f"mesh_regularizers: the topology is on {topo.device}, the vertices on {verts.device} (MeshTopology.to)")
    total, terms = _MeshRegFn.apply(verts, topo, METHODS[lap_method], float(w_lap), float(w_nc), float(w_edge), float(target_length))
    return total, terms
