"""Referee of the mesh regularisers (ops.mesh_regularizers, csrc/foho_mreg.h): the definitions evaluated by torch autograd in float64 --
or, with dtype=torch.float32, the same formulas as the float32 yardstick.  Written without the table builder: edges and pairs come from
plain loops over the faces, the Laplacian is a dense V x V matrix, W, S and a are detached.

  evaluate(verts, faces, method, target_length, dtype)  ->  {"lap" | "nc" | "edge": (value, gradient (V, 3))} as float64 numpy
  meshes: mesh(name) -> (verts float32, faces int64), the seeded test meshes
"""
import functools
import math

import numpy as np
import torch

from followmyhold_amd import synthetic

METHODS = ("uniform", "cot", "cotcurv")
TERMS = ("lap", "nc", "edge")


# ---------------------------------------------------------------- connectivity by brute force
def brute_edges(faces):
    """{(i, j) with i < j: [(face, corner opposite), ...]} in face order."""
    out = {}
    for fi, f in enumerate(np.asarray(faces).tolist()):
        for c in range(3):
            i, j = f[(c + 1) % 3], f[(c + 2) % 3]
            out.setdefault((min(i, j), max(i, j)), []).append((fi, c))
    return out


def brute_pairs(faces):
    """[(v0, v1, a, b)]: for every edge, every unordered pair of its faces; v0 < v1, a and b the opposite vertices."""
    fl = np.asarray(faces).tolist()
    out = []
    for (i, j), lst in sorted(brute_edges(faces).items()):
        for x in range(len(lst)):
            for y in range(x + 1, len(lst)):
                out.append((i, j, fl[lst[x][0]][lst[x][1]], fl[lst[y][0]][lst[y][1]]))
    return out


# ---------------------------------------------------------------- the terms
def cot_weights(v, faces):
    """W (V, V) dense, a (V,): the cotangent weights and the area sums of vertices v (no gradient)."""
    v = v.detach()
    V = v.shape[0]
    f = torch.tensor(np.asarray(faces), dtype=torch.int64).reshape(-1, 3)
    W, a = torch.zeros(V, V, dtype=v.dtype), torch.zeros(V, dtype=v.dtype)
    if f.shape[0] == 0:
        return W, a
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    A, B, C = (p1 - p2).norm(dim=1), (p0 - p2).norm(dim=1), (p0 - p1).norm(dim=1)
    s = 0.5 * (A + B + C)
    area = (s * (s - A) * (s - B) * (s - C)).clamp(min=1e-12).sqrt()
    A2, B2, C2 = A * A, B * B, C * C
    cot = torch.stack([B2 + C2 - A2, A2 + C2 - B2, A2 + B2 - C2], 1) / area[:, None] / 4.0
    for c in range(3):
        i, j = f[:, (c + 1) % 3], f[:, (c + 2) % 3]
        W.index_put_((i, j), cot[:, c], accumulate=True)
        W.index_put_((j, i), cot[:, c], accumulate=True)
        a.index_put_((f[:, c],), area, accumulate=True)
    return W, a


def residual(v, faces, method, weights_from=None, corrupt=None):
    """r (V, 3) and the mask of the vertices with a neighbour; W, S, a from `weights_from` (default: v itself), detached."""
    V = v.shape[0]
    adj = torch.zeros(V, V, dtype=v.dtype)
    for i, j in brute_edges(faces):
        adj[i, j] = adj[j, i] = 1.0
    deg = adj.sum(1)
    if method == "uniform":
        scale = torch.where(deg > 0, 1.0 / deg.clamp(min=1.0), torch.zeros_like(deg))
        if corrupt == "row_weight":
            scale[int(deg.argmax())] *= 1.01
        r = (scale[:, None] * (adj @ v) - v) * (deg > 0).to(v.dtype)[:, None]
        return r, deg > 0
    W, a = cot_weights(v if weights_from is None else weights_from, faces)
    if corrupt == "row_weight":       # one weight of one row (the whole row times 1.01 would cancel in cot's normalisation)
        i = int(deg.argmax())
        W[i, int(W[i].abs().argmax())] *= 1.01
    S = W.sum(1)
    if method == "cot":
        n = torch.where(S > 0, 1.0 / S, S)
        r = n[:, None] * (W @ v) - v
    elif method == "cotcurv":
        q = torch.where(a > 0, 1.0 / a, a)
        r = (W @ v - S[:, None] * v) * (0.25 * q)[:, None]
    else:
        raise ValueError(method)
    return r, deg > 0


def lap_term(v, faces, method, weights_from=None, corrupt=None):
    if v.shape[0] == 0 or len(faces) == 0:
        return v.sum() * 0.0
    r, _ = residual(v, faces, method, weights_from, corrupt)
    return r.norm(dim=1).sum() / v.shape[0]


def pair_normals(v, faces, corrupt=None):
    p = brute_pairs(faces)
    if corrupt == "drop_pair":
        p = p[:-1]
    if not p:
        return None, None
    p = torch.tensor(p, dtype=torch.int64)
    v0, v1, a, b = (v[p[:, k]] for k in range(4))
    return torch.cross(v1 - v0, a - v0, dim=1), torch.cross(v1 - v0, b - v0, dim=1)


def nc_term(v, faces, corrupt=None):
    n0, n1 = pair_normals(v, faces, corrupt)
    if n0 is None:
        return v.sum() * 0.0
    m1 = n1 if corrupt == "flip_sign" else -n1
    cos = (n0 * m1).sum(1) / (n0.norm(dim=1).clamp(min=1e-8) * m1.norm(dim=1).clamp(min=1e-8))
    return (1.0 - cos).mean()


def edge_term(v, faces, target_length=0.0):
    e = sorted(brute_edges(faces))
    if not e:
        return v.sum() * 0.0
    e = torch.tensor(e, dtype=torch.int64)
    return (((v[e[:, 0]] - v[e[:, 1]]).norm(dim=1) - target_length) ** 2).mean()


def evaluate(verts, faces, method="uniform", target_length=0.0, dtype=torch.float64, corrupt=None, terms=TERMS):
    """{term: (value, gradient)} as float64 numpy, every term evaluated and differentiated alone in `dtype`."""
    out = {}
    for t in terms:
        v = torch.tensor(np.asarray(verts), dtype=dtype).reshape(-1, 3).requires_grad_(True)
        val = {"lap": lambda: lap_term(v, faces, method, corrupt=corrupt), "nc": lambda: nc_term(v, faces, corrupt),
               "edge": lambda: edge_term(v, faces, target_length)}[t]()
        (g,) = torch.autograd.grad(val, v, allow_unused=True)
        g = torch.zeros_like(v) if g is None else g
        out[t] = (float(val.detach()), g.double().numpy())
    return out


# ---------------------------------------------------------------- error measures and conditions
def err_term(got, ref):
    return abs(float(got) - ref) / abs(ref)


def err_grad(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


def lap_condition(verts, faces, method):
    """c = min |r_i| / mean |r_i| over the vertices with a neighbour, in float64."""
    r, has = residual(torch.tensor(np.asarray(verts), dtype=torch.float64), faces, method)
    n = r.norm(dim=1)[has]
    return float(n.min() / n.mean())


def nc_condition(verts, faces):
    """The smallest |n0| or |n1| of a pair over their mean, in float64."""
    n0, n1 = pair_normals(torch.tensor(np.asarray(verts), dtype=torch.float64), faces)
    n = torch.cat([n0.norm(dim=1), n1.norm(dim=1)])
    return float(n.min() / n.mean())


# ---------------------------------------------------------------- meshes
def tetrahedron(R=1.0):
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64) * (R / math.sqrt(3.0))
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int64)


def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int64)


def grid(n=5):
    """Planar regular n x n grid in z = 0, every cell split along the same diagonal."""
    v = np.array([[i, j, 0.0] for i in range(n) for j in range(n)], dtype=np.float64)
    f = []
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j, (i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1
            f += [(a, b, c), (a, c, d)]
    return v, np.array(f, dtype=np.int64)


def double_cone(valence=100, h=0.8):
    ang = 2 * math.pi * np.arange(valence) / valence
    v = np.concatenate([np.stack([np.cos(ang), np.sin(ang), np.zeros(valence)], 1), [[0, 0, h], [0, 0, -h]]])
    f = [(i, (i + 1) % valence, valence) for i in range(valence)] + [((i + 1) % valence, i, valence + 1) for i in range(valence)]
    return v, np.array(f, dtype=np.int64)


def _mean_edge(v, f):
    e = np.array(sorted(brute_edges(f)))
    return float(np.linalg.norm(v[e[:, 0]] - v[e[:, 1]], axis=1).mean())


def jittered(v, f, jitter, seed):
    """Vertices moved by seeded normal noise of standard deviation jitter x the mean edge length; float32."""
    v = np.asarray(v, dtype=np.float64)
    rng = np.random.default_rng(seed)
    return (v + rng.normal(size=v.shape) * (jitter * _mean_edge(v, f))).astype(np.float32), np.asarray(f, dtype=np.int64)


def _compact(v, f):
    used = np.unique(f)
    remap = np.full(len(v), -1, dtype=np.int64)
    remap[used] = np.arange(len(used))
    return v[used], remap[f]


#        name       (jitter, seed)
JITTER = {"torus": (0.3, 2), "ico3": (0.3, 1), "cone": (0.1, 2), "open": (0.05, 2), "fin": (0.05, 2), "zero": (0.05, 2)}


@functools.lru_cache(maxsize=None)
def mesh(name):
    """The seeded test meshes: (verts float32 (V, 3), faces int64 (F, 3)), read-only."""
    if name == "tet":
        v, f = tetrahedron(1.0)
        v = v.astype(np.float32)
    elif name == "torus":
        v, f = jittered(*synthetic.torus(16, 16), *JITTER[name])
    elif name == "torus_iso":                                    # one vertex more, in no face
        v, f = mesh("torus")
        v = np.concatenate([v, np.array([[0.1, 0.2, 0.3]], dtype=np.float32)])
    elif name == "ico3":
        v, f = jittered(*synthetic.icosphere(3), *JITTER[name])
    elif name == "cone":
        v, f = jittered(*double_cone(100), *JITTER[name])
    elif name == "open":                                         # icosphere(2) without its cap: boundary edges
        v, f = synthetic.icosphere(2)
        f = f[v[f].mean(1)[:, 2] < 0.7]
        v, f = jittered(*_compact(v, f), *JITTER[name])
    elif name in ("fin", "zero"):
        v, f = synthetic.icosphere(1)
        a, b = int(f[0, 0]), int(f[0, 1])
        v, f = jittered(v, f, *JITTER[name])
        if name == "fin":                                        # a third face on edge (a, b)
            extra = (1.6 * 0.5 * (v[a] + v[b])).astype(np.float32)
        else:                                                    # a vertex on top of a, and the zero-area face (a, new, b)
            extra = v[a].copy()
        v = np.concatenate([v, extra[None]])
        f = np.concatenate([f, np.array([[a, len(v) - 1, b]], dtype=np.int64)])
    elif name == "ico5":
        v, f = synthetic.make_object("20k")
    else:
        raise ValueError(name)
    v, f = np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int64)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f
