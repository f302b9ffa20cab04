"""The mesh regularisers (ops.mesh_regularizers, libfoho_mreg.so: Laplacian smoothing uniform / cot / cotcurv, normal consistency, edge
length, fused, with the gradient to the vertices) against a float64 referee.

tests/mesh_reg_ref64.py evaluates the definitions of csrc/foho_mreg.h by torch autograd in float64 over a dense V x V Laplacian, with
edges and pairs from plain loops over the faces (nothing of mesh_reg.MeshTopology).  Error measures against it:
  term, total    |d| / |ref|
  gradient       max |d| / max |ref|

Meshes (mesh_reg_ref64.mesh; jitter = seeded normal noise, in mean edge lengths), V / F / pairs:
  tet         4 / 4 / 6          regular tetrahedron, no jitter: less than one wave, known answers
  torus       256 / 512 / 768    torus(16, 16), jitter 0.3: exactly one workgroup
  torus_iso   257 / 512 / 768    the same and one vertex in no face: a second workgroup with one thread, degree 0
  ico3        642 / 1280 / 1920  icosphere(3), jitter 0.3: three workgroups in the ordered sums
  cone        102 / 200 / 300    double cone, both apexes of valence 100, jitter 0.1: a list longer than any fixed-size buffer
  open        147 / 276 / 406    icosphere(2) without its cap, jitter 0.05: boundary edges give no pair
  fin         43 / 81 / 122      icosphere(1) and a third face on one edge, jitter 0.05: three pairs on that edge
  zero        43 / 81 / 122      icosphere(1), a vertex on top of another and the zero-area face between them
  ico5        10242 / 20480      the workload's object: repeatability only

Condition on the inputs (asserted in float64): c = min |r_i| / mean |r_i| >= 1e-2 over the vertices with a neighbour for every
Laplacian case, every pair's |n0|, |n1| >= 1e-3 of their mean for every normal-consistency case -- the unit direction r / |r| loses
accuracy as 1 / |r|.  `zero` is outside the condition for cot, cotcurv (area clamp) and the pair normals (n = 0 exactly).

Tolerances.  TOL_F32 is the worst error of the referee's own formulas evaluated in float32 torch on the CPU against float64, over
the conditioned cases (zero: uniform and edge only; the normal-consistency gradient of tet is exactly 0 and has no relative measure):
  measured  term          8.73e-7 (cone cotcurv; the others 1.2e-8 .. 3.5e-7)
            grad_uniform  2.62e-6 (open; 3.6e-7 .. 1.8e-6)
            grad_cot      5.28e-5 (cone cotcurv; cot and cotcurv 7e-7 .. 4.7e-5, growing as c falls: c = 0.03 .. 0.64)
            grad_nc       1.05e-6 (fin; 2.1e-7 .. 7.9e-7)
            grad_edge     1.92e-7 (ico3; 1.2e-7 .. 1.6e-7)
TOL, the kernel's bound, is 4 x TOL_F32 rounded up to one significant digit: the kernel sums in another order than the referee (per
list, per workgroup tree, then the partials in index order).  Neither number comes from what the kernel achieves; a kernel that needs
more is a finding.

CPU: the referee against central differences, known answers that involve no restatement, the identities of the gradients, three
corrupted referees that the measures must catch, the conditions, the float32 yardstick, MeshTopology on CPU tensors against brute
force, the C ABI.  GPU: every mesh above against the referee, the edge term against facade.mesh_edge_loss in float64, weights, the
cotangent, repeatability, the facade."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_reg_ref64 as R  # noqa: E402

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "followmyhold_amd", "csrc", "foho_mreg.h")
QUANT = ("term", "grad_uniform", "grad_cot", "grad_nc", "grad_edge")
TOL_F32 = {"term": 8.8e-7, "grad_uniform": 2.7e-6, "grad_cot": 5.3e-5, "grad_nc": 1.1e-6, "grad_edge": 2.0e-7}   # measured, see above
TOL = {"term": 4e-6, "grad_uniform": 2e-5, "grad_cot": 3e-4, "grad_nc": 5e-6, "grad_edge": 8e-7}                 # 4 x TOL_F32, one digit, up
TOL_EXACT = 1e-12          # float64 referee against a closed-form answer or an identity
TARGET = 0.1               # target_length of the edge term in the referee cases
CASES = ("tet", "torus", "torus_iso", "ico3", "cone", "open", "fin", "zero")
CONDITIONED = tuple(n for n in CASES if n != "zero")


def grad_key(term, method):
    return {"lap": "grad_uniform" if method == "uniform" else "grad_cot", "nc": "grad_nc", "edge": "grad_edge"}[term]


def runs(name):
    """The (method, term) evaluations of a mesh: every method's Laplacian, normal consistency and the edge term once."""
    return [(m, "lap") for m in R.METHODS] + [("uniform", "nc"), ("uniform", "edge")]


def in_yardstick(name, method, term):
    return not (name == "zero" and (method != "uniform" or term == "nc"))


@functools.lru_cache(maxsize=None)
def ref(name, method):
    """The float64 referee of a mesh, computed once: {term: (value, gradient)}; read-only."""
    v, f = R.mesh(name)
    out = R.evaluate(v, f, method, TARGET, terms=R.TERMS if method == "uniform" else ("lap",))
    for _, g in out.values():
        g.setflags(write=False)
    return out


def measure(name, method, term, value, grad):
    """{quantity: error} of one term's value and gradient against the referee."""
    rv, rg = ref(name, method)[term]
    e = {"term": R.err_term(value, rv)}
    if np.abs(rg).max() > 0:
        e[grad_key(term, method)] = R.err_grad(grad, rg)
    return e


def _report(what, e, tol=TOL):
    print(f"{what}: " + "  ".join(f"{k} {v:.2e} ({v / tol[k]:.2f} of the bound)" for k, v in e.items()))


def _within(e, tol=TOL):
    return all(v <= tol[k] for k, v in e.items())


# ---------------------------------------------------------------- CPU: the referee and the rule
def test_tolerances_follow_from_the_yardstick():
    for k in QUANT:
        lead = 10.0 ** np.floor(np.log10(4 * TOL_F32[k]))
        assert TOL[k] == pytest.approx(np.ceil(4 * TOL_F32[k] / lead - 1e-9) * lead, rel=1e-12)


@pytest.mark.parametrize("name", CONDITIONED)
def test_inputs_meet_the_conditions(name):
    """A condition, not a measurement (if one breaks, change the jitter or the seed, never the floor)."""
    v, f = R.mesh(name)
    c = {m: R.lap_condition(v, f, m) for m in R.METHODS}
    n = R.nc_condition(v, f)
    print(f"{name}: c " + "  ".join(f"{m} {x:.3f}" for m, x in c.items()) + f"  pair normals {n:.3f}")
    assert all(x >= 1e-2 for x in c.values()) and n >= 1e-3
    assert R.lap_condition(*R.mesh("zero"), "uniform") >= 1e-2


def test_referee_matches_central_differences():
    """Every term on `fin` (an edge with three faces included), W, S and a held at the unperturbed vertices as the gradient holds them.
    h = 1e-5 on coordinates of size 1: the truncation is O(h^2) ~ 1e-10 of the third derivative, the rounding 2.2e-16 / h ~ 2e-11;
    bound 1e-7 of the largest gradient entry."""
    v, f = R.mesh("fin")
    v0 = torch.tensor(np.array(v), dtype=torch.float64)
    h = 1e-5
    rng = np.random.default_rng(7)
    coords = [(int(k), int(a)) for k, a in zip(rng.integers(0, len(v), 10), rng.integers(0, 3, 10))] + [(len(v) - 1, 0), (int(f[0, 0]), 2)]
    fns = {(m, "lap"): (lambda x, m=m: R.lap_term(x, f, m, weights_from=v0)) for m in R.METHODS}
    fns[("uniform", "nc")] = lambda x: R.nc_term(x, f)
    fns[("uniform", "edge")] = lambda x: R.edge_term(x, f, TARGET)
    for (m, t), fn in fns.items():
        g = ref("fin", m)[t][1]
        worst = 0.0
        for k, a in coords:
            xp, xm = v0.clone(), v0.clone()
            xp[k, a] += h
            xm[k, a] -= h
            fd = (float(fn(xp)) - float(fn(xm))) / (2 * h)
            worst = max(worst, abs(fd - g[k, a]) / np.abs(g).max())
        print(f"{m} {t}: central differences against the referee {worst:.2e}")
        assert worst <= 1e-7


def test_referee_gives_the_known_answers():
    """Answers that restate nothing: a regular tetrahedron of circumradius R about the origin (every neighbour mean is -v_i / 3, so
    |r_i| = 4R / 3 for uniform, and for cot by symmetry of the weights; every dihedral angle has cos(n0, -n1) = -1/3); the unit cube of
    12 triangles (6 diagonals inside a face: 0; 12 cube edges: 1; 12 of 18 pairs); a planar regular grid."""
    for Rr in (1.0, 0.37):
        v, f = R.tetrahedron(Rr)
        for m in ("uniform", "cot"):
            assert R.evaluate(v, f, m, terms=("lap",))["lap"][0] == pytest.approx(4 * Rr / 3, rel=TOL_EXACT)
        assert R.evaluate(v, f, terms=("nc",))["nc"][0] == pytest.approx(4 / 3, rel=TOL_EXACT)
    assert R.evaluate(*R.cube(), terms=("nc",))["nc"][0] == pytest.approx(12 / 18, rel=TOL_EXACT)
    v, f = R.grid(5)
    assert abs(R.evaluate(v, f, terms=("nc",))["nc"][0]) <= TOL_EXACT
    r, _ = R.residual(torch.tensor(v), f, "uniform")
    interior = [i * 5 + j for i in range(1, 4) for j in range(1, 4)]
    assert float(r[interior].abs().max()) <= TOL_EXACT and float(r.abs().max()) > 0.1


@pytest.mark.parametrize("name", ("torus", "fin"))
def test_referee_gradients_obey_the_identities(name):
    """Translation invariance: sum_k g_k = 0 for every term.  The Laplacian residual is linear in v with constant weights, so its term
    is homogeneous of degree 1: sum_k v_k . g_k = the term; normal consistency is scale invariant: sum_k v_k . g_k = 0."""
    v = np.array(R.mesh(name)[0], dtype=np.float64)
    for m, t in runs(name):
        val, g = ref(name, m)[t]
        scale = np.abs(g).sum()
        assert np.abs(g.sum(0)).max() <= TOL_EXACT * scale, (m, t)
        if t == "lap":
            assert (v * g).sum() == pytest.approx(val, rel=1e-11), (m, t)
        if t == "nc":
            assert abs((v * g).sum()) <= TOL_EXACT * scale


@pytest.mark.parametrize("corrupt,which", [("row_weight", [(m, "lap") for m in R.METHODS]), ("drop_pair", [("uniform", "nc")]),
                                           ("flip_sign", [("uniform", "nc")])])
def test_corrupted_referees_are_caught(corrupt, which):
    """Teeth: one weight of one row off by 1 %, one pair dropped, the sign of -n1 flipped -- each leaves the bound by a factor of ten
    or more in the value or in the gradient (one weight of 1536 moves the mean |r| of the torus by 3e-6, and its row's direction by
    7e-3)."""
    for name in ("torus", "fin"):
        v, f = R.mesh(name)
        for m, t in which:
            bad = R.evaluate(v, f, m, TARGET, corrupt=corrupt, terms=(t,))[t]
            e = measure(name, m, t, *bad)
            _report(f"{name} {m} {t}: {corrupt}", e)
            assert not _within(e) and max(x / TOL[k] for k, x in e.items()) > 10, e


def test_float32_yardstick():
    """The referee's formulas in float32 torch against float64 on exactly the cases' inputs: what float32 arithmetic achieves on them.
    Its worst values are TOL_F32 (a case that exceeds one means the header's figures are stale, not that the bound may grow unseen)."""
    worst = dict.fromkeys(QUANT, 0.0)
    for name in CASES:
        v, f = R.mesh(name)
        for m in R.METHODS:
            terms = [t for mm, t in runs(name) if mm == m and in_yardstick(name, m, t)]
            if not terms:
                continue
            r32 = R.evaluate(v, f, m, TARGET, dtype=torch.float32, terms=terms)
            for t in terms:
                assert np.isfinite(r32[t][1]).all()
                e = measure(name, m, t, *r32[t])
                _report(f"{name} {m} {t}: float32 against float64", e, TOL_F32)
                worst.update({k: max(worst[k], x) for k, x in e.items()})
    _report("worst", worst, TOL_F32)
    for k in QUANT:
        assert 0.8 * TOL_F32[k] <= worst[k] <= TOL_F32[k], (k, worst[k])


# ---------------------------------------------------------------- CPU: the table builder
@pytest.mark.parametrize("name", ("torus", "open", "fin", "torus_iso", "cone"))
def test_topology_tables_against_brute_force(name):
    """MeshTopology on CPU tensors: a closed mesh, an open one, an edge with three faces, an isolated vertex, valence 100."""
    from followmyhold_amd import facade
    from followmyhold_amd.mesh_reg import MeshTopology
    v, f = R.mesh(name)
    V = len(v)
    t = MeshTopology(torch.tensor(f), V)
    edges, pairs = R.brute_edges(f), R.brute_pairs(f)
    assert (t.V, t.F, t.E, t.P) == (V, len(f), len(edges), len(pairs))
    assert all(getattr(t, k).dtype == torch.int32 and not getattr(t, k).is_cuda for k in t.TABLES)
    # edges: the rows of Meshes.edges_packed(), in its order
    packed = facade.Meshes([torch.tensor(v)], [torch.tensor(f)]).edges_packed()
    assert t.edges.tolist() == packed.tolist() == [list(e) for e in sorted(edges)]
    # neighbour lists: ascending, symmetric, complete, every entry with its edge
    off, idx, eid = t.nbr_off.tolist(), t.nbr_idx.tolist(), t.nbr_edge.tolist()
    assert off[0] == 0 and off[-1] == 2 * t.E == len(idx) and len(off) == V + 1
    nbrs = [idx[off[i]:off[i + 1]] for i in range(V)]
    want = [[] for _ in range(V)]
    for i, j in edges:
        want[i].append(j)
        want[j].append(i)
    assert nbrs == [sorted(w) for w in want]
    assert all(i in nbrs[j] for i in range(V) for j in nbrs[i])
    el = t.edges.tolist()
    assert all(el[eid[k]] == [min(i, j), max(i, j)] for i in range(V) for k, j in zip(range(off[i], off[i + 1]), nbrs[i]))
    if name == "torus_iso":
        assert nbrs[-1] == []
    if name == "cone":
        assert max(map(len, nbrs)) == 100
    # per edge: the ascending (face << 2 | opposite corner) list
    eoff, efc = t.edge_off.tolist(), t.edge_fc.tolist()
    assert eoff[0] == 0 and eoff[-1] == 3 * t.F == len(efc)
    for e, key in enumerate(sorted(edges)):
        assert efc[eoff[e]:eoff[e + 1]] == sorted(fi << 2 | c for fi, c in edges[key])
    # pairs: sum over the edges of C(k, 2), the brute-force set
    assert t.P == sum(len(l) * (len(l) - 1) // 2 for l in edges.values())
    assert sorted(map(tuple, t.pairs.tolist())) == sorted(pairs)
    if name == "fin":
        assert max(map(len, edges.values())) == 3
    if name == "open":
        assert min(map(len, edges.values())) == 1
    # per vertex: the ascending, complete (pair << 2 | slot) lists
    voff, vent = t.vp_off.tolist(), t.vp_ent.tolist()
    flat = t.pairs.reshape(-1).tolist()
    assert voff[0] == 0 and voff[-1] == 4 * t.P == len(vent) and sorted(vent) == list(range(4 * t.P))
    for i in range(V):
        lst = vent[voff[i]:voff[i + 1]]
        assert lst == sorted(lst) and all(flat[x] == i for x in lst)


def test_topology_refuses_bad_faces_and_takes_empty_meshes():
    from followmyhold_amd._lib import FohoError
    from followmyhold_amd.mesh_reg import MeshTopology
    for bad in ([[0, 1, 4]], [[0, -1, 2]], [[0, 1, 1]]):
        with pytest.raises(FohoError):
            MeshTopology(torch.tensor(bad), 4)
    for V, f in ((0, torch.zeros(0, 3, dtype=torch.int64)), (5, torch.zeros(0, 3, dtype=torch.int64))):
        t = MeshTopology(f, V)
        assert (t.V, t.F, t.E, t.P) == (V, 0, 0, 0) and t.nbr_off.tolist() == [0] * (V + 1) == t.vp_off.tolist()


# ---------------------------------------------------------------- CPU: the C ABI
def _mreg():
    from followmyhold_amd import _lib, mesh_reg
    _lib.build()
    return mesh_reg.lib()


def test_cabi_header_is_what_the_library_exports():
    """foho_mreg.h's prototypes are `nm -D libfoho_mreg.so`, and the ctypes table types them as the header does."""
    from test_cabi import prototypes
    from followmyhold_amd import _lib, mesh_reg
    L = _mreg()
    protos = prototypes(HEADER)
    names = sorted(p[0] for p in protos)
    assert names == ["foho_mreg_last_error", "foho_mreg_run", "foho_mreg_version", "foho_mreg_workspace_bytes"]
    out = subprocess.run(["nm", "-D", "--defined-only", mesh_reg.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in out.splitlines() if len(l.split()) >= 3 and l.split()[-2] in ("T", "t", "W", "V", "B", "D"))
    assert [n for n in exported if not n.startswith(("_init", "_fini", "__bss_start", "_edata", "_end", "__hip_"))] == names
    assert L.foho_mreg_version() == 100 == mesh_reg.VERSION == _lib.SIDE_VERSIONS["mreg"]
    scalars = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    assert set(mesh_reg._SIGNATURES) == set(names) - {"foho_mreg_version", "foho_mreg_last_error"}
    for fn, ret, params in protos:
        if fn in mesh_reg._SIGNATURES:
            restype, argtypes = mesh_reg._SIGNATURES[fn]
            assert restype is scalars[ret] and len(argtypes) == len(params)
            assert all(t is (ctypes.c_void_p if c.endswith("*") else scalars[c]) for c, t in zip(params, argtypes)), fn


def test_cabi_refuses_bad_arguments_before_any_launch():
    """-1 and a message for null pointers, negative sizes, an unknown method and a short workspace; nothing is dereferenced or launched
    (the pointers below are not addresses of anything)."""
    L = _mreg()
    V, F, E, P = 4, 4, 6, 6
    need = L.foho_mreg_workspace_bytes(V, E, P)
    assert need >= 32 * V + 8 * E + 64 * P and L.foho_mreg_workspace_bytes(-1, E, P) == 0 == L.foho_mreg_workspace_bytes(V, E, -2)
    assert L.foho_mreg_workspace_bytes(0, 0, 0) > 0
    p = 4096

    def call(verts=p, sizes=(V, F, E, P), tables=(p,) * 8, method=0, out=p, grad=p, ws=p, nws=need):
        return L.foho_mreg_run(verts, p, *sizes, *tables, method, 1.0, 1.0, 1.0, 0.0, out, grad, ws, nws, None)

    for kw, word in ((dict(verts=None), b"null"), (dict(out=None), b"null"), (dict(ws=None), b"null"), (dict(tables=(None,) + (p,) * 7), b"null"),
                     (dict(tables=(p,) * 5 + (None, p, p)), b"null"), (dict(sizes=(-1, F, E, P)), b"negative"), (dict(sizes=(V, F, E, -1)), b"negative"),
                     (dict(method=3), b"method"), (dict(method=-1), b"method"), (dict(nws=need - 1), b"workspace"), (dict(nws=0), b"workspace")):
        assert call(**kw) == -1, kw
        msg = L.foho_mreg_last_error()
        assert msg and word in msg, (kw, msg)


def test_cpu_vertices_raise():
    from followmyhold_amd import facade, ops
    from followmyhold_amd._lib import FohoError
    v, f = R.mesh("tet")
    with pytest.raises(FohoError):
        ops.mesh_regularizers(torch.tensor(v), ops.MeshTopology(torch.tensor(f), 4), w_lap=1.0)
    with pytest.raises(FohoError):
        facade.mesh_laplacian_smoothing(facade.Meshes([torch.tensor(v)], [torch.tensor(f)]))


# ---------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _device_mesh(name):
    from followmyhold_amd import ops
    v, f = R.mesh(name)
    return torch.tensor(v).cuda(), ops.MeshTopology(torch.tensor(f).cuda(), len(v))


_KW = {"lap": lambda m: dict(w_lap=1.0, lap_method=m), "nc": lambda m: dict(w_nc=1.0), "edge": lambda m: dict(w_edge=1.0, target_length=TARGET)}


def _single(name, method, term, verts=None):
    """One term alone through autograd -> value, gradient (numpy), terms (list)."""
    from followmyhold_amd import ops
    v, topo = _device_mesh(name)
    x = (v if verts is None else verts).clone().requires_grad_(True)
    total, terms = ops.mesh_regularizers(x, topo, **_KW[term](method))
    total.backward()
    return total.item(), x.grad.cpu().numpy(), terms.tolist()


@gpu
@pytest.mark.parametrize("name", CONDITIONED)
def test_gpu_terms_and_gradients_against_the_referee(name):
    for m, t in runs(name):
        val, g, terms = _single(name, m, t)
        e = measure(name, m, t, val, g)
        _report(f"{name} {m} {t}", e)
        assert _within(e), (m, t, e)
        assert terms[R.TERMS.index(t)] == val and sum(x != 0 for x in terms) == 1
        if np.abs(ref(name, m)[t][1]).max() == 0:          # tet, normal consistency: the gradient is 0 by symmetry, the vertices are of size 1
            assert np.abs(g).max() <= TOL["grad_nc"]
    if name == "torus_iso":
        assert not _single(name, "uniform", "lap")[1][-1].any()        # degree 0: no residual, no gradient


@gpu
def test_gpu_tetrahedron_known_answers():
    for m in ("uniform", "cot"):
        assert _single("tet", m, "lap")[0] == pytest.approx(4 / 3, rel=TOL["term"])
    assert _single("tet", "uniform", "nc")[0] == pytest.approx(4 / 3, rel=TOL["term"])


@gpu
def test_gpu_zero_area_face():
    """One zero-area face between two coincident vertices: everything finite; uniform, normal consistency and the edge term within
    the bound (the clamped pair normals are exactly 0 in both precisions); cot and cotcurv finite only -- the area clamp makes them
    ill-conditioned and the condition on the inputs excludes them."""
    for m, t in runs("zero"):
        val, g, _ = _single("zero", m, t)
        assert np.isfinite(val) and np.isfinite(g).all(), (m, t)
        if m == "uniform":
            e = measure("zero", m, t, val, g)
            _report(f"zero {m} {t}", e)
            assert _within(e), (m, t, e)


@gpu
@pytest.mark.parametrize("target", (0.0, 0.07))
def test_gpu_edge_term_is_the_facades(target):
    from followmyhold_amd import facade, ops
    v, f = R.mesh("ico3")
    x64 = torch.tensor(np.array(v), dtype=torch.float64).requires_grad_(True)
    want = facade.mesh_edge_loss(facade.Meshes([x64], [torch.tensor(f)]), target)
    want.backward()
    vd, topo = _device_mesh("ico3")
    x = vd.clone().requires_grad_(True)
    total, terms = ops.mesh_regularizers(x, topo, w_edge=1.0, target_length=target)
    total.backward()
    e = {"term": R.err_term(total.item(), want.item()), "grad_edge": R.err_grad(x.grad.cpu().numpy(), x64.grad.numpy())}
    _report(f"edge term, target {target}", e)
    assert _within(e)


@gpu
def test_gpu_weights():
    """The fused call is the weighted sum of the single-term calls; a zero weight reports 0 and adds nothing to the gradient."""
    from followmyhold_amd import ops
    v, topo = _device_mesh("ico3")
    w = {"lap": 0.7, "nc": 0.2, "edge": 3.0}
    single = {t: _single("ico3", "cot", t) for t in R.TERMS}

    def fused(**kw):
        x = v.clone().requires_grad_(True)
        total, terms = ops.mesh_regularizers(x, topo, lap_method="cot", target_length=TARGET, **kw)
        total.backward()
        return total.item(), terms.tolist(), x.grad.cpu().numpy().astype(np.float64)

    total, terms, g = fused(w_lap=w["lap"], w_nc=w["nc"], w_edge=w["edge"])
    assert terms == [single[t][0] for t in R.TERMS]          # the same kernels on the same data
    assert R.err_term(total, sum(w[t] * np.float64(single[t][0]) for t in R.TERMS)) <= TOL["term"]
    want = sum(w[t] * single[t][1].astype(np.float64) for t in R.TERMS)
    # both sides are the kernel's float32 gradients: they differ by the roundings of three scalings and two additions (at most
    # 6 x 2^-24 = 3.6e-7 of the largest entry), so the tightest of the bounds serves
    assert R.err_grad(g, want) <= TOL["grad_edge"]
    total, terms, g = fused(w_lap=w["lap"], w_nc=0.0, w_edge=w["edge"])
    assert terms[1] == 0.0 and terms[0] == single["lap"][0] and terms[2] == single["edge"][0]
    assert R.err_grad(g, w["lap"] * single["lap"][1].astype(np.float64) + w["edge"] * single["edge"][1]) <= TOL["grad_edge"]
    total, terms, g = fused()
    assert total == 0.0 and terms == [0.0, 0.0, 0.0] and not g.any()


@gpu
def test_gpu_cotangent_dtypes_and_strides():
    from followmyhold_amd import ops
    v, topo = _device_mesh("torus_iso")
    kw = dict(w_lap=1.0, lap_method="cotcurv", w_nc=0.5, w_edge=2.0, target_length=TARGET)
    x = v.clone().requires_grad_(True)
    total, terms = ops.mesh_regularizers(x, topo, **kw)
    assert total.dtype == torch.float32 and total.shape == () and tuple(terms.shape) == (3,) and not terms.requires_grad
    (g1,) = torch.autograd.grad(total, x, retain_graph=True)
    (g2,) = torch.autograd.grad(total, x, retain_graph=True)
    (g3,) = torch.autograd.grad(3 * total, x)
    assert torch.equal(g1, g2) and torch.equal(g3, 3 * g1)
    # float64 and non-contiguous vertices: converted, the gradient in their dtype and shape
    x64 = v.double().requires_grad_(True)
    t64, _ = ops.mesh_regularizers(x64, topo, **kw)
    t64.backward()
    assert x64.grad.dtype == torch.float64 and torch.equal(x64.grad.float(), g1) and t64.item() == total.item()
    wide = torch.zeros(v.shape[0], 5, device=v.device)
    wide[:, 1:4] = v
    wide.requires_grad_(True)
    ts, _ = ops.mesh_regularizers(wide[:, 1:4], topo, **kw)
    ts.backward()
    assert torch.equal(wide.grad[:, 1:4], g1) and not wide.grad[:, 0].any() and not wide.grad[:, 4].any()
    with torch.no_grad():                                     # no gradient wanted: the library's null grad
        tn, termsn = ops.mesh_regularizers(v, topo, **kw)
    assert tn.item() == total.item() and torch.equal(termsn, terms)


@gpu
def test_gpu_empty_meshes():
    from followmyhold_amd import ops
    for V in (0, 5):
        x = torch.rand(V, 3, device="cuda").requires_grad_(True)
        topo = ops.MeshTopology(torch.zeros(0, 3, dtype=torch.int64, device="cuda"), V)
        total, terms = ops.mesh_regularizers(x, topo, w_lap=1.0, lap_method="cot", w_nc=1.0, w_edge=1.0)
        total.backward()
        assert total.item() == 0.0 and terms.tolist() == [0.0] * 3 and not x.grad.any() and tuple(x.grad.shape) == (V, 3)


@gpu
def test_gpu_repeatable_bit_for_bit():
    """The 10 242-vertex object (41 workgroups in the ordered sums): two calls and a call on another stream agree in every bit."""
    from followmyhold_amd import ops
    v, topo = _device_mesh("ico5")
    assert topo.V == 10242 and topo.F == 20480

    def once(method):
        x = v.clone().requires_grad_(True)
        total, terms = ops.mesh_regularizers(x, topo, w_lap=1.0, lap_method=method, w_nc=0.5, w_edge=2.0, target_length=1e-3)
        total.backward()
        return total.detach(), terms, x.grad

    for method in R.METHODS:
        a, b = once(method), once(method)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c = once(method)
        side.synchronize()
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) and torch.equal(p, r) for p, q, r in zip(a, b, c)), method
        assert torch.isfinite(a[2]).all() and a[0].item() > 0 and all(t > 0 for t in a[1].tolist())


@gpu
def test_gpu_facade():
    from followmyhold_amd import facade, ops
    v, f = R.mesh("ico3")
    vd = torch.tensor(v).cuda()
    m = facade.Meshes([vd], [torch.tensor(f).cuda()])
    topo = m.topology()
    assert topo is m.topology() and (topo.V, topo.F) == (len(v), len(f))
    for method in R.METHODS:
        assert facade.mesh_laplacian_smoothing(m, method).item() == ops.mesh_regularizers(vd, topo, w_lap=1.0, lap_method=method)[0].item()
    assert facade.mesh_normal_consistency(m).item() == ops.mesh_regularizers(vd, topo, w_nc=1.0)[0].item()
    total, terms = facade.mesh_regularizers(m, w_lap=1.0, w_nc=1.0, w_edge=1.0, target_length=TARGET)
    assert terms[2].item() == pytest.approx(facade.mesh_edge_loss(m, TARGET).item(), rel=TOL["term"])
    moved = m.update_padded((vd * 1.5).unsqueeze(0).requires_grad_(True))
    assert moved.topology() is topo
    loss = facade.mesh_laplacian_smoothing(moved)
    loss.backward()
    assert loss.item() == pytest.approx(1.5 * facade.mesh_laplacian_smoothing(m).item(), rel=TOL["term"])
