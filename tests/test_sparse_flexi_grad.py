"""The differentiable sparse FlexiCubes (sparse_flexi.flexicubes_sparse_grad, foho_sflexi_bwd): the mesh of ops.flexicubes bit for bit, and
dL/ds against the float64 closed-form referee of tests/flexi_grad_ref.py, bitwise repeatable.

Inputs.  The fields are flexi_grad_ref's: the ten fuzz fields, `allcases`, `tiny`, both chain variants and the four smooth fields, plus
the analytic torus at res 128.  The referee's jittered grid is not separable, so the grid is a new one: per case a (3, res+1) axis
table spanning 2.2 units with every interior entry moved by a seeded +-0.3 of a cell -- monotone, no two cells of equal width, so a
kernel that assumes uniform spacing or mixes up the axes fails -- and x = its "ij" meshgrid.  The chain fields keep the chain grid: the
table linspace(-0.5, 0.5, G) * 0.24 meshes to it bit for bit (asserted).  The reference is flexi_grad_ref.grad(x, s, res, gv) on that x.

Tolerance.  TOL_F32_S is the worst error of the referee's own float32 evaluation against its float64 one over THIS file's inputs, in
flexi_grad_ref.measure with the scale arrays (err = max |got - ref| / max(scale, 1e-4 scale.max())), measured on the CPU:
  fuzz0 1.77e-7   fuzz1 1.37e-7   fuzz2 2.23e-7   fuzz3 1.79e-7   fuzz4 2.20e-7   fuzz5 1.74e-7   fuzz6 2.21e-7   fuzz7 1.26e-7
  fuzz8 2.26e-7   fuzz9 1.45e-7   allcases 2.32e-7   tiny 6.0e-8   chain_multi 1.91e-7   chain_multi_b 1.66e-7   sphere 2.13e-7
  torus 2.5002e-7   two_spheres 1.58e-7   bumpy 1.86e-7   torus128 2.26e-7                                 ->  TOL_F32_S = 2.51e-7
(test_flexi_grad.py's 1.75e-6 is fuzz1 on the referee's non-separable jittered grid, where all three axes enter every dot product.)
TOL_S, the kernel's bound, is 4 x TOL_F32_S rounded up to one significant digit, 2e-6: the project's margin for "the same <= 24 terms in
another order of addition" (test_flexi_grad.py).  Neither number comes from what the kernel achieves; a kernel that needs more is a
finding.  The fp16 bound is test_flexi_grad.py's 2^-10 (half a unit of fp16 and TOL), for its reason.

CPU: the yardstick, the conditions on the inputs, argument validation of foho_sflexi_bwd through the binding, the pipeline switch's
validation.  GPU: every case (forward torch.equal to the dense extractor, dL/ds within TOL_S, exact zeros where the referee's scale is
0), `tiny`, repeatability, shape and dtype, empty and refused inputs, res 128 with the peak memory of both routes, and the pipeline
switch."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import flexi_grad_ref as G  # noqa: E402
from followmyhold_amd import _lib, ops, pipeline as PLN, sparse_flexi as SF, standins  # noqa: E402
from followmyhold_amd.facade import generate_dense_grid_points  # noqa: E402

SF.flexicubes_sparse_grad      # the operator this file tests: without it, nothing here is collected

gpu = pytest.mark.gpu
vp = ctypes.c_void_p
TOL_F32_S = 2.51e-7            # the referee's own float32 evaluation against its float64 one (measured, see above)
TOL_S = 2e-6                   # the kernel against the referee: 4 x TOL_F32_S, rounded up to one significant digit
SMALL = G.FUZZ + ("allcases", "tiny") + G.CHAIN + G.SMOOTH
BIG = "torus128"
ALL = SMALL + (BIG,)
EXTENT = 2.2


def axis_table(res, seed):
    """(3, res+1) float32 over [-1.1, 1.1]: every interior entry moved by uniform +-0.3 of a cell."""
    n = res + 1
    t = np.repeat(np.linspace(-EXTENT / 2, EXTENT / 2, n)[None], 3, 0)
    t[:, 1:-1] += np.random.default_rng(seed).uniform(-0.3, 0.3, size=(3, n - 2)) * (EXTENT / res)
    return torch.from_numpy(t.astype(np.float32))


def mesh_of(axes):
    """The "ij" meshgrid of the tables, (G^3, 3)."""
    return torch.stack(torch.meshgrid(axes[0], axes[1], axes[2], indexing="ij"), -1).reshape(-1, 3)


class Case:
    """A field on its axis tables, the cotangent and the float64 reference: computed once, shared, never changed."""

    def __init__(self, name):
        self.name = name
        if name == BIG:
            self.res = 128
            self.axes = axis_table(self.res, 1300)
            self.x = mesh_of(self.axes)
            self.s = torch.stack([torch.sqrt(self.x[:, 0] ** 2 + self.x[:, 1] ** 2) - 0.6, self.x[:, 2]], 1).norm(dim=1) - 0.25
        else:
            x0, self.s, self.res = G.field(name)
            if name in G.CHAIN:
                lin = torch.linspace(-0.5, 0.5, self.res + 1) * 0.24
                self.axes = torch.stack([lin, lin, lin])
            else:
                self.axes = axis_table(self.res, 1200 + SMALL.index(name))
            self.x = mesh_of(self.axes)
            self.x0 = x0
        self.code = G.cube_codes(self.s.numpy(), self.res)
        self.nv = int(G.N_PATCH[self.code].sum())
        self.gv = G.cotangent(self.nv)
        self.ref = G.grad(self.x.numpy(), self.s.numpy(), self.res, self.gv.numpy())


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def _err(gs, ref):
    return G.measure(gs.reshape(-1), ref[0], ref[2])[0]


# ---------------------------------------------------------------- CPU
def test_tolerance_follows_from_the_yardstick():
    lead = 10.0 ** np.floor(np.log10(4 * TOL_F32_S))
    assert TOL_S == pytest.approx(np.ceil(4 * TOL_F32_S / lead - 1e-9) * lead, rel=1e-12)


def test_float32_yardstick():
    """The referee in float32 against itself in float64 on this file's inputs: no field exceeds TOL_F32_S, and the worst one reaches it
    (a stale header is a failure, not a bound that grows unseen)."""
    worst = 0.0
    for name in ALL:
        c = case(name)
        r32 = G.grad(c.x.numpy(), c.s.numpy(), c.res, c.gv.numpy(), dtype=np.float32)
        assert bool(torch.isfinite(r32[0]).all())
        e = _err(r32[0], c.ref)
        print(f"{name}: float32 referee against float64  dL/ds {e:.3e}")
        assert e <= TOL_F32_S, (name, e)
        worst = max(worst, e)
    print(f"worst {worst:.3e} (TOL_F32_S {TOL_F32_S:.2e}, TOL_S {TOL_S:.0e})")
    assert worst >= 0.9 * TOL_F32_S, worst


def test_inputs_reach_what_they_were_built_for():
    """Conditions on the inputs (if one breaks, change the seed, never the condition)."""
    c = case("allcases")
    assert set(c.code.reshape(16, 16, 16)[::2, ::2, ::2].reshape(-1).tolist()) == set(range(1, 255))
    for name in G.FUZZ + G.CHAIN:
        assert int((G.N_PATCH[case(name).code] > 1).sum()) > 0, name
    six = []
    for name in G.FUZZ:
        f = case(name)
        cross = f.ref[2].reshape((f.res + 1,) * 3) > 0          # grid points that end a crossing edge
        six.append(all(bool(side.any()) for side in (cross[0], cross[-1], cross[:, 0], cross[:, -1], cross[:, :, 0], cross[:, :, -1])))
    assert any(six), six
    assert any(int((case(name).s == 0).sum()) > 0 for name in G.FUZZ)
    t = case("tiny")
    assert t.nv == 8 and bool(torch.isfinite(t.ref[0]).all()) and float(t.ref[0].abs().max()) < 3e38
    for name in ALL:
        f = case(name)
        w = np.diff(f.axes.numpy(), axis=1)
        assert f.axes.shape == (3, f.res + 1) and f.axes.dtype == torch.float32 and (w > 0).all(), name
        assert torch.equal(f.x.reshape(f.res + 1, f.res + 1, f.res + 1, 3)[3 % f.res, 1, 2 % f.res],
                           torch.stack([f.axes[0, 3 % f.res], f.axes[1, 1], f.axes[2, 2 % f.res]]))
        if name in G.CHAIN:
            assert torch.equal(f.x, f.x0), name                   # the chain grid, bit for bit
        else:
            assert len(np.unique(w)) == w.size, name              # no two cells of equal width, on or across the axes
            assert float(f.axes[:, 0].max()) == float(np.float32(-1.1)) == -float(f.axes[:, -1].min())      # spans 2.2 units
            assert float(np.abs(w / (EXTENT / f.res) - 1).max()) <= 0.6 + 1e-5


def test_bwd_validates_arguments_without_a_gpu():
    L = SF.lib()
    assert L.foho_sflexi_version() == SF.VERSION == 100
    one = vp(256)                  # a non-null pointer that is never dereferenced: every call below is refused before any launch
    big = ctypes.c_size_t(1 << 40)

    def bwd(axes=one, s=one, res=8, marks=one, mb=big, cap=10, gv=one, nv=40, gs=one, ws=one, wb=big):
        return L.foho_sflexi_bwd(axes, s, res, marks, mb, cap, gv, nv, gs, ws, wb, None)

    def refused(status, *words):
        msg = L.foho_sflexi_last_error().decode()
        assert status < 0 and "foho_sflexi_bwd" in msg and all(w in msg for w in words), (status, msg)

    for name in ("axes", "s", "marks", "gv", "gs", "ws"):
        refused(bwd(**{name: None}), "null")
    for res in (0, -3, SF.MAX_RES + 1):
        refused(bwd(res=res), "resolution")
    for cap in (-1, SF.MAX_CUBES + 1):
        refused(bwd(cap=cap), "capacity")
    refused(bwd(nv=-1), "vertex count")
    refused(bwd(mb=L.foho_sflexi_mark_bytes(8) - 1), "mark buffer too small")
    refused(bwd(wb=L.foho_sflexi_cube_bytes(10) - 1), "workspace too small")
    # nothing to do is success without a launch (the pointers are never read)
    assert bwd(cap=0) == 0 and bwd(nv=0) == 0


def test_guidance_extract_switch_is_validated(monkeypatch):
    monkeypatch.delenv("FOHO_GUIDANCE_EXTRACT", raising=False)
    assert PLN.guidance_extract_mode() == "dense" and PLN.guidance_extract_mode("sparse") == "sparse"
    with pytest.raises(_lib.FohoError):
        PLN.guidance_extract_mode("nonsense")
    monkeypatch.setenv("FOHO_GUIDANCE_EXTRACT", "sparse")
    assert PLN.guidance_extract_mode() == "sparse" and PLN.guidance_extract_mode("dense") == "dense"      # the kwarg overrides the environment
    monkeypatch.setenv("FOHO_GUIDANCE_EXTRACT", "nonsense")
    assert PLN.guidance_extract_mode("sparse") == "sparse"
    with pytest.raises(_lib.FohoError, match="nonsense"):
        PLN.guidance_extract_mode()
    pipe = standins.make_standin_pipeline(device="cpu", dtype=torch.float32, seed=1)

    def no_work(*a, **k):
        raise AssertionError("a network ran before the switch was validated")

    monkeypatch.setattr(pipe, "prepare_image", no_work)
    monkeypatch.setattr(pipe, "encode_cond", no_work)
    with pytest.raises(_lib.FohoError, match="nonsense"):          # from the environment
        pipe(image=None, final_octree_resolution=32)
    monkeypatch.delenv("FOHO_GUIDANCE_EXTRACT")
    with pytest.raises(_lib.FohoError, match="nonsense"):          # from the argument
        pipe(image=None, final_octree_resolution=32, guidance_extract="nonsense")


# ---------------------------------------------------------------- GPU
def _run(c, s=None, gv=None):
    """flexicubes_sparse_grad on the case's tables -> (verts, faces, l_dev, the leaf field with its gradient)."""
    sg = (c.s if s is None else s).cuda().requires_grad_(True)
    v, f, l = ops.flexicubes_sparse_grad(c.axes.cuda(), sg, c.res)
    (v * (c.gv if gv is None else gv).cuda()).sum().backward()
    return v, f, l, sg


def _dense(c):
    """ops.flexicubes on the meshed grid with the same cotangent -> (verts, faces, l_dev, its dL/ds)."""
    sd = c.s.cuda().requires_grad_(True)
    v, f, l = ops.flexicubes(c.x.cuda(), sd, c.res)
    (v * c.gv.cuda()).sum().backward()
    return v, f, l, sd.grad


@gpu
@pytest.mark.parametrize("name", SMALL)
def test_forward_equals_dense_and_gradient_matches_the_referee(name):
    c = case(name)
    v, f, l, sg = _run(c)
    v0, f0, l0, gd = _dense(c)
    assert len(v) == c.nv and f.dtype == torch.int64
    assert torch.equal(v.detach(), v0.detach()) and torch.equal(f, f0) and torch.equal(l, l0)
    assert not f.requires_grad and not l.requires_grad
    e, ed = _err(sg.grad, c.ref), _err(gd, c.ref)
    print(f"{name}: sparse dL/ds {e:.3e}  (ops.flexicubes {ed:.3e}; TOL_S {TOL_S:.0e}, {c.nv} vertices)")
    assert bool(torch.isfinite(sg.grad).all())
    assert e <= TOL_S, e
    assert not bool(sg.grad.cpu()[c.ref[2] == 0].any())


@gpu
def test_gradient_is_finite_where_d_squared_underflows():
    """`tiny`: D = 1e-30 on the six crossing edges; (s / D) / D stays finite where 1 / (D * D) is infinite."""
    c = case("tiny")
    assert np.float32(1e-30) * np.float32(1e-30) == 0
    _, _, _, sg = _run(c)
    gs = sg.grad.cpu()
    print(f"tiny: dL/ds {gs.tolist()}  largest reference {float(c.ref[0].abs().max()):.3e}")
    assert bool(torch.isfinite(gs).all()) and float(gs.abs().max()) > 1e20
    assert _err(gs, c.ref) <= TOL_S


@gpu
def test_gradient_is_bitwise_repeatable():
    c = case("allcases")
    ax = c.axes.cuda()
    first = _run(c)[3].grad.clone()
    again = _run(c)[3].grad
    # one graph, two backward passes
    sg = c.s.cuda().requires_grad_(True)
    v, _, _ = ops.flexicubes_sparse_grad(ax, sg, c.res)
    loss = (v * c.gv.cuda()).sum()
    loss.backward(retain_graph=True)
    g1 = sg.grad.clone()
    sg.grad = None
    # an unrelated extraction at another resolution between the forward and the second backward
    o = case("fuzz1")
    ops.flexicubes_sparse_grad(o.axes.cuda(), o.s.cuda().requires_grad_(True), o.res)[0].sum().backward()
    loss.backward()
    g2 = sg.grad.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g3 = _run(c)[3].grad
    side.synchronize()
    assert int(torch.count_nonzero(first)) > 1000
    for other in (again, g1, g2, g3):
        assert torch.equal(first, other)
    d1, d2 = _dense(c)[3], _dense(c)[3]
    print(f"allcases: two runs of ops.flexicubes' backward differ by {float((d1 - d2).abs().max()):.3e} at most "
          f"({int((d1 != d2).sum())} of {int(torch.count_nonzero(d1))} entries); the sparse gradient by 0")


@gpu
@pytest.mark.parametrize("name", ["fuzz0", "allcases"])
def test_gradient_keeps_shape_and_dtype(name):
    """A (G,G,G) half-precision field gets a (G,G,G) half-precision gradient within 2^-10 of the referee on the fp16-rounded values."""
    c = case(name)
    n = c.res + 1
    sh = c.s.half()
    nv = G.n_verts(sh.float().numpy(), c.res)
    gv = G.cotangent(nv, seed=12)
    ref = G.grad(c.x.numpy(), sh.float().numpy(), c.res, gv.numpy())
    assert float(ref[0].abs().max()) < 6e4                     # representable in fp16
    s3 = sh.reshape(n, n, n).cuda().requires_grad_(True)
    v, _, _ = ops.flexicubes_sparse_grad(c.axes.cuda(), s3, c.res)
    assert len(v) == nv and v.dtype == torch.float32
    (v * gv.cuda()).sum().backward()
    assert s3.grad.shape == (n, n, n) and s3.grad.dtype == torch.float16
    e = _err(s3.grad, ref)
    print(f"{name}: fp16 dL/ds {e:.3e} (bound {2.0 ** -10:.3e})")
    assert e <= 2.0 ** -10


@gpu
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_one_sign_fields_are_empty_with_a_zero_gradient(sign):
    res = 20
    s = torch.full(((res + 1) ** 3,), 0.25 * sign, device="cuda").requires_grad_(True)
    v, f, l, st = ops.flexicubes_sparse_grad(axis_table(res, 7), s, res, return_stats=True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and l.shape == (0,) and f.dtype == torch.int64
    assert st["cubes"] == 0 and st["vertices"] == 0 and st["faces"] == 0
    (v.sum() + 0.0).backward()
    assert s.grad.shape == s.shape and not bool(s.grad.any())


@gpu
def test_axes_that_require_grad_are_refused_and_stats_are_the_forward_ones():
    c = case("fuzz2")
    with pytest.raises(_lib.FohoError, match="axis tables"):
        ops.flexicubes_sparse_grad(c.axes.cuda().requires_grad_(True), c.s.cuda().requires_grad_(True), c.res)
    with pytest.raises(_lib.FohoError, match="forward only"):          # the forward-only operator stays what it is
        ops.flexicubes_sparse(c.axes.cuda(), c.s.cuda().requires_grad_(True), c.res)
    a = SF.flexicubes_sparse(c.axes, c.s.cuda(), c.res, return_stats=True)
    b = SF.flexicubes_sparse_grad(c.axes, c.s.cuda(), c.res, return_stats=True)      # a field without grad is legal
    assert a[3] == b[3] and all(torch.equal(p, q) for p, q in zip(a[:3], b[:3])) and not b[0].requires_grad


@gpu
def test_torus_at_128_with_less_memory_than_the_dense_route():
    c = case(BIG)
    ax, x, gv = c.axes.cuda(), c.x.cuda(), c.gv.cuda()

    def peak(route):
        s = c.s.cuda().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        v, f, l = route(s)
        (v * gv).sum().backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - held, v.detach(), f, l, s.grad

    pd, v0, f0, l0, gd = peak(lambda s: ops.flexicubes(x, s, c.res))
    ps, v, f, l, gs = peak(lambda s: ops.flexicubes_sparse_grad(ax, s, c.res))
    assert len(v) == c.nv > 20000
    assert torch.equal(v, v0) and torch.equal(f, f0) and torch.equal(l, l0)
    e, ed = _err(gs, c.ref), _err(gd, c.ref)
    print(f"torus128: sparse dL/ds {e:.3e}  (ops.flexicubes {ed:.3e}; TOL_S {TOL_S:.0e}, {c.nv} vertices); "
          f"peak above the held baseline: sparse {ps / 2 ** 20:.1f} MiB, dense {pd / 2 ** 20:.1f} MiB")
    assert e <= TOL_S and not bool(gs.cpu()[c.ref[2] == 0].any())
    assert ps < pd


@gpu
def test_pipeline_guidance_extract_switch(tmp_path, monkeypatch):
    from PIL import Image
    from followmyhold_amd import geo_decode
    from test_pipeline import _renderer, _scene_for_pipeline, _short_config, _write
    sc = _scene_for_pipeline()
    paths = _write(tmp_path, sc)
    img = Image.open(paths["cropped_obj_img_path"])
    cfg = _short_config()
    for name in ("phase1_hand_lrs", "phase2_hand_lrs", "obj_lrs", "obj_2half_lrs"):
        setattr(cfg, name, {k: v / 500.0 for k, v in getattr(cfg, name).items()})
    cfg.noise_obj_lr1, cfg.noise_obj_lr2 = cfg.noise_obj_lr1 / 500.0, cfg.noise_obj_lr2 / 500.0
    pipe = standins.make_standin_pipeline(device="cuda", dtype=torch.float32, seed=1, num_latents=128, embed_dim=8, width=128, heads=2,
                                          layers=1, num_freqs=8)
    geo_decode.install(pipe.vae)
    kw = dict(config=cfg, renderer=_renderer(sc["fov"]), J_regressor=sc["J_regressor"], guidance_octree_resolution=16,
              final_octree_resolution=32)
    monkeypatch.setenv("FOHO_EXACT_SIZE_OBJECTIVE", "1")
    monkeypatch.delenv("FOHO_GUIDANCE_EXTRACT", raising=False)
    checked = []
    orig = ops.flexicubes_sparse_grad

    def spy(axes, s, res, return_stats=False):
        out = orig(axes, s, res, return_stats=return_stats)
        xyz, _, _ = generate_dense_grid_points(np.full(3, -1.10), np.full(3, 1.10), octree_depth=5, octree_resolution=res, indexing="ij")
        v0, f0, l0 = ops.flexicubes(torch.as_tensor(xyz, dtype=torch.float32, device=s.device), s.detach(), res)
        checked.append(res)
        assert s.requires_grad and out[0].requires_grad
        assert v0.shape[0] > 100 and torch.equal(v0, out[0].detach()) and torch.equal(f0, out[1]) and torch.equal(l0, out[2])
        return out

    monkeypatch.setattr(ops, "flexicubes_sparse_grad", spy)

    def run(**extra):
        checked.clear()
        out = pipe(image=[img], mc_algo="mc", generator=torch.manual_seed(2), sil_renderer=None, **kw, **extra, **paths)
        return out, list(checked), dict(pipe.stats)

    out, calls, st = run(guidance_extract="sparse")
    assert len(calls) >= 1 and set(calls) == {16}
    assert st["guidance_extract"]["calls"] == st["exact_size_iterations"] == len(calls)
    assert st["guidance_extract"]["vertices"] > 100 * len(calls) and st["guidance_extract"]["cubes"] > 0 and st["guidance_extract"]["faces"] > 0
    assert st["inner_iterations"] > 0 and out[0].verts_packed().shape[0] > 100
    out, calls, st = run()
    assert calls == [] and "guidance_extract" not in st and st["exact_size_iterations"] > 0
    monkeypatch.setenv("FOHO_GUIDANCE_EXTRACT", "sparse")
    out, calls, st = run(guidance_extract="dense")           # the kwarg overrides the environment
    assert calls == [] and "guidance_extract" not in st
