"""Band decode of the guidance grid (pipeline.latent2sdf_band, geo_decode._GeoBandFn, volume.hierarchical_grid_logits_batch): the 65^3
decodes of the guidance loop queried near the surface only, with gradient.  Contract: decoded values are the dense decode's, the
FlexiCubes mesh is the dense mesh index for index, and the gradient to the latent tokens is bitwise the dense route's for the same
incoming gradient.  CPU: the switch and its validation.  GPU: query points, forward, backward, the batch form and the pipeline switch."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from followmyhold_amd import _lib, pipeline as PLN, standins, volume  # noqa: E402
from followmyhold_amd.facade import generate_dense_grid_points  # noqa: E402

gpu = pytest.mark.gpu
BMIN, BMAX = np.full(3, -1.10), np.full(3, 1.10)


# ---------------------------------------------------------------- CPU
def test_guidance_decode_mode_and_env(monkeypatch):
    monkeypatch.delenv("FOHO_GUIDANCE_DECODE", raising=False)
    assert PLN.guidance_decode_mode() == "dense" and PLN.guidance_decode_mode("hierarchical") == "hierarchical"
    with pytest.raises(_lib.FohoError):
        PLN.guidance_decode_mode("sparse")
    monkeypatch.setenv("FOHO_GUIDANCE_DECODE", "hierarchical")
    assert PLN.guidance_decode_mode() == "hierarchical" and PLN.guidance_decode_mode("dense") == "dense"
    monkeypatch.setenv("FOHO_GUIDANCE_DECODE", "octree")
    with pytest.raises(_lib.FohoError):
        PLN.guidance_decode_mode()
    monkeypatch.setenv("FOHO_FINAL_DECODE", "hierarchical")          # the two switches are independent
    monkeypatch.delenv("FOHO_GUIDANCE_DECODE")
    assert PLN.guidance_decode_mode() == "dense"


def test_guidance_min_res_is_validated():
    assert PLN.guidance_levels(64) == (64, 32) and PLN.guidance_levels(64, 16) == (64, 16) and PLN.guidance_levels(64, 8) == (64, 8)
    assert PLN.guidance_levels(24) == (24, 12)
    for res, mr in [(64, 24), (64, 4), (64, 128), (24, 6), (24, 8), (24, 16)]:
        with pytest.raises(_lib.FohoError):
            PLN.guidance_levels(res, mr)


def _cpu_pipe():
    return standins.make_standin_pipeline(device="cpu", dtype=torch.float32, seed=1)


def test_pipeline_refuses_bad_guidance_decode_before_any_work(monkeypatch):
    monkeypatch.delenv("FOHO_GUIDANCE_DECODE", raising=False)
    pipe = _cpu_pipe()
    assert getattr(pipe.vae, "hip_geo", None) is None
    for kw, what in [(dict(guidance_decode="sparse"), "sparse"), (dict(guidance_decode="hierarchical"), "hip_geo"),
                     (dict(guidance_decode="hierarchical", guidance_decode_min_res=6), "power of two")]:
        with pytest.raises(_lib.FohoError, match=what):
            pipe(image=None, guidance_octree_resolution=24, **kw)
        with pytest.raises(_lib.FohoError, match=what):
            pipe.call_batch([None], [{}], guidance_octree_resolution=24, **kw)
    monkeypatch.setenv("FOHO_GUIDANCE_DECODE", "hierarchical")
    with pytest.raises(_lib.FohoError, match="hip_geo"):
        pipe(image=None, guidance_octree_resolution=24)


def test_missing_hip_geo_is_refused():
    pipe = _cpu_pipe()
    xyz = torch.zeros(25 ** 3, 3)
    with pytest.raises(_lib.FohoError, match="hip_geo"):
        PLN.latent2sdf_band(torch.zeros(1, 64, 8), xyz, [25] * 3, pipe.vae, "cpu", BMIN, BMAX)
    with pytest.raises(_lib.FohoError, match="power of two"):
        PLN.latent2sdf_band(torch.zeros(1, 64, 8), xyz, [25] * 3, pipe.vae, "cpu", BMIN, BMAX, min_res=6)


def test_keep_backward_mode_is_refused():
    pipe = _cpu_pipe()
    pipe.vae.hip_geo = types.SimpleNamespace(backward_mode="keep")
    with pytest.raises(_lib.FohoError, match="keep"):
        PLN.latent2sdf_band(torch.zeros(1, 64, 8), torch.zeros(25 ** 3, 3), [25] * 3, pipe.vae, "cpu", BMIN, BMAX)
    with pytest.raises(_lib.FohoError, match="keep"):
        pipe(image=None, guidance_octree_resolution=24, guidance_decode="hierarchical")
    with pytest.raises(_lib.FohoError, match="keep"):
        pipe.call_batch([None], [{}], guidance_octree_resolution=24, guidance_decode="hierarchical")


# ---------------------------------------------------------------- GPU
def _dense_points(res, dev="cuda"):
    xyz_np, gsz, _ = generate_dense_grid_points(BMIN, BMAX, octree_depth=5, octree_resolution=res, indexing="ij")
    return torch.as_tensor(xyz_np, dtype=torch.float32, device=dev), gsz


def _mesh(xyz, sdf, res):
    from followmyhold_amd import ops
    v, f, _ = ops.flexicubes(xyz, sdf.reshape(-1), res)
    return v, f


def _same_mesh(xyz, a, b, res, min_verts=100):
    v0, f0 = _mesh(xyz, a, res)
    v1, f1 = _mesh(xyz, b, res)
    assert v0.shape[0] > min_verts and torch.equal(v0, v1) and torch.equal(f0, f1)


def _standin_vae(width=128):
    from followmyhold_amd import geo_decode
    torch.manual_seed(0)
    if width == 128:      # a smooth field: the smoke test's decoder shape with few Fourier frequencies
        kw = dict(num_latents=128, embed_dim=8, width=128, heads=2, layers=1, num_freqs=2)
    else:                 # the Hunyuan decoder shape
        kw = dict(num_latents=3072, embed_dim=64, width=1024, heads=16, layers=1, num_freqs=8)
    vae = standins.StandInShapeVAE(**kw).cuda().eval().requires_grad_(False)
    if width != 128:
        vae = vae.half()
    geo_decode.install(vae)
    return vae, kw


def _surface_corners(sdf, res):
    """Point mask of the 8 corners of every cube whose corners differ in sign (what FlexiCubes reads values at)."""
    G = res + 1
    s = (sdf.reshape(G, G, G) < 0).to(torch.int8)
    n = sum(s[i:i + res, j:j + res, k:k + res] for i in (0, 1) for j in (0, 1) for k in (0, 1))
    mixed = ((n > 0) & (n < 8)).to(torch.int8)
    out = torch.zeros(G, G, G, dtype=torch.int8, device=sdf.device)
    for i in (0, 1):
        for j in (0, 1):
            for k in (0, 1):
                out[i:i + res, j:j + res, k:k + res] |= mixed
    return out.reshape(-1).bool()


@gpu
@pytest.mark.parametrize("res", [64, 24])
def test_band_query_points_are_the_dense_query_points(res):
    """Every level's emitted xyz (the full mask at each level of the guidance grid) equals the rows of grid_queries(xyz_samples)
    at those grid points, bit for bit."""
    vae, _ = _standin_vae()
    hip = vae.hip_geo
    xyz, _ = _dense_points(res)
    q = hip.grid_queries(xyz).reshape(res + 1, res + 1, res + 1, 3)
    emit = volume._Compactor(volume.axis_tables(BMIN, BMAX, res).cuda(), res, 1, torch.device("cuda"))
    _, min_res = PLN.guidance_levels(res)
    r = min_res
    while r <= res:
        idx, pts = emit({0: volume._mask((r + 1) ** 3, "cuda", -1)}, r)[0]
        s = res // r
        assert torch.equal(idx.long().cpu(), torch.arange((r + 1) ** 3))
        assert torch.equal(pts, q[::s, ::s, ::s].reshape(-1, 3)), (res, r)
        r *= 2


@gpu
@pytest.mark.parametrize("min_res", [16, 32])
def test_band_forward_is_the_dense_field_where_flexicubes_reads_it(min_res):
    """65^3 with a smooth stand-in field, without and with gradient: signs everywhere and every decoded value equal the dense decode's,
    every corner of a sign-changing cube is decoded, the FlexiCubes mesh is identical, and far fewer rows are decoded."""
    vae, kw = _standin_vae()
    res = 64
    xyz, gsz = _dense_points(res)
    lat = torch.randn(1, kw["num_latents"], kw["embed_dim"], device="cuda")
    for grad in (False, True):
        with torch.set_grad_enabled(grad):
            p = lat.clone().requires_grad_(grad)
            dense = PLN.latent2sdf(p, xyz, gsz, vae, "cuda").detach()
            band, st = PLN.latent2sdf_band(p, xyz, gsz, vae, "cuda", BMIN, BMAX, min_res=min_res)
            assert band.requires_grad == grad
            band = band.detach()
        assert band.shape == dense.shape == (1, res + 1, res + 1, res + 1) and band.dtype == torch.float32
        assert st["levels"] == [min_res] + ([32] if min_res == 16 else []) + [64] and not st["fallback"], st
        assert torch.equal(band < 0, dense < 0)
        same = band.reshape(-1) == dense.reshape(-1)
        assert int(same.sum()) >= st["decoded"]
        assert same[_surface_corners(dense, res)].all()
        _same_mesh(xyz, dense, band, res, min_verts=500)
        assert st["decoded_fraction"] < (0.35 if min_res == 16 else 0.45), st


def _grads(hip, tok, xyz, res, g, band_fn=None):
    band_fn = band_fn or PLN.sdf_band_from_tokens
    t1 = tok.detach().clone().requires_grad_(True)
    band, _, _ = band_fn([t1], xyz, res, hip, BMIN, BMAX)
    t2 = tok.detach().clone().requires_grad_(True)
    dense = -hip(hip.grid_queries(xyz), t2).reshape(-1).float()
    assert torch.equal(band[0][_surface_corners(dense.detach(), res)], dense.detach()[_surface_corners(dense.detach(), res)])
    gb, = torch.autograd.grad(band[0], t1, g)
    gd, = torch.autograd.grad(dense, t2, g)
    return gb, gd, dense.detach()


@gpu
@pytest.mark.parametrize("width", [128, 1024])
def test_band_backward_is_bitwise_the_dense_backward(width):
    """torch.autograd.grad w.r.t. the latent tokens, band vs dense, for one incoming gradient on the corners of sign-changing cubes and
    one non-zero everywhere (points the band only filled included), in "rows" and "recompute" modes: bitwise equal."""
    vae, kw = _standin_vae(width)
    hip = vae.hip_geo
    res = 64
    xyz, _ = _dense_points(res)
    dt = torch.float16 if width == 1024 else torch.float32
    tok = torch.randn(1, kw["num_latents"], kw["width"], device="cuda").to(dt)
    gen = torch.Generator(device="cuda").manual_seed(3)
    for mode in ("rows", "recompute"):
        hip.backward_mode = mode
        with torch.no_grad():
            dense0 = -hip(hip.grid_queries(xyz), tok).reshape(-1).float()
        corners = _surface_corners(dense0, res)
        g_all = torch.randn((res + 1) ** 3, device="cuda", generator=gen)
        for g in (g_all * corners, g_all):
            gb, gd, _ = _grads(hip, tok, xyz, res, g)
            assert gd.abs().max().item() > 0 and torch.isfinite(gd).all()
            assert torch.equal(gb, gd), (mode, (gb.float() - gd.float()).abs().max().item())
    hip.backward_mode = "keep"
    with pytest.raises(_lib.FohoError, match="keep"):
        PLN.sdf_band_from_tokens([tok.clone().requires_grad_(True)], xyz, res, hip, BMIN, BMAX)
    hip.backward_mode = "rows"


@gpu
def test_batch_band_equals_per_image_band_with_one_host_read_per_level():
    """Three images with different fields through sdf_band_from_tokens at once: each image's field, stats and token gradient equal its
    own single-image band decode bitwise, and the levels and closure rounds of all images share one host read each."""
    vae, kw = _standin_vae()
    hip = vae.hip_geo
    res = 64
    xyz, _ = _dense_points(res)
    toks = [torch.randn(1, kw["num_latents"], kw["width"], device="cuda") * s for s in (1.0, 0.7, 1.3)]
    gen = torch.Generator(device="cuda").manual_seed(5)
    g = torch.randn(3, (res + 1) ** 3, device="cuda", generator=gen)
    one = []
    reads_single = 0
    for b, t in enumerate(toks):
        tb = t.clone().requires_grad_(True)
        f, (st,), reads = PLN.sdf_band_from_tokens([tb], xyz, res, hip, BMIN, BMAX)
        assert reads == len(st["levels"]) + st["closure_rounds"] + 1 and not st["fallback"]
        gr, = torch.autograd.grad(f[0], tb, g[b])
        one.append((f.detach()[0], st, gr))
        reads_single += reads
    assert len({o[1]["decoded"] for o in one}) == 3            # three different fields
    tb = [t.clone().requires_grad_(True) for t in toks]
    f, sts, reads = PLN.sdf_band_from_tokens(tb, xyz, res, hip, BMIN, BMAX)
    grads = torch.autograd.grad(f, tb, g)
    for b in range(3):
        assert torch.equal(f[b].detach(), one[b][0]) and sts[b] == one[b][1] and torch.equal(grads[b], one[b][2]), b
    assert reads == len(sts[0]["levels"]) + max(s["closure_rounds"] for s in sts) + 1 < reads_single
    with torch.no_grad():                                        # the no-gradient route (the per-step decodes) as well
        f_ng, sts_ng, _ = PLN.sdf_band_from_tokens(toks, xyz, res, hip, BMIN, BMAX)
        for b, t in enumerate(toks):
            f1, st1, _ = PLN.sdf_band_from_tokens([t], xyz, res, hip, BMIN, BMAX)
            assert torch.equal(f_ng[b], f1[0]) and sts_ng[b] == st1[0]
            _same_mesh(xyz, -hip(hip.grid_queries(xyz), t).reshape(-1).float(), f1[0], res)


@gpu
def test_pipeline_guidance_decode_switch(tmp_path, monkeypatch):
    """The short stand-in schedule, guidance grid 24 (levels 12 -> 24): with guidance_decode="hierarchical" (kwarg, call_batch argument,
    FOHO_GUIDANCE_DECODE) every band decode is checked inside the run against the dense decode of the same latent -- identical mesh,
    and, in the loop, the identical token gradient for the same incoming gradient (two whole runs are not bitwise repeatable, DESIGN.md
    section 11) -- stats["guidance_decode"] is filled in, and the results match the default run's as closely as in the final-decode test."""
    from PIL import Image
    from followmyhold_amd import geo_decode
    from test_pipeline import _renderer, _scene_for_pipeline, _short_config, _write
    monkeypatch.delenv("FOHO_GUIDANCE_DECODE", raising=False)
    monkeypatch.delenv("FOHO_FINAL_DECODE", raising=False)
    sc = _scene_for_pipeline()
    paths = _write(tmp_path, sc)
    img = Image.open(paths["cropped_obj_img_path"])
    cfg = _short_config()
    for name in ("phase1_hand_lrs", "phase2_hand_lrs", "obj_lrs", "obj_2half_lrs"):
        setattr(cfg, name, {k: v / 500.0 for k, v in getattr(cfg, name).items()})
    cfg.noise_obj_lr1, cfg.noise_obj_lr2 = cfg.noise_obj_lr1 / 500.0, cfg.noise_obj_lr2 / 500.0
    pipe = standins.make_standin_pipeline(device="cuda", dtype=torch.float32, seed=1, num_latents=128, embed_dim=8, width=128, heads=2,
                                          layers=1, num_freqs=8)
    hip = geo_decode.install(pipe.vae)
    res = 24
    kw = dict(config=cfg, renderer=_renderer(sc["fov"]), J_regressor=sc["J_regressor"], guidance_octree_resolution=res, final_octree_resolution=40)
    xyz, gsz = _dense_points(res)
    checked = {"grad": 0, "nograd": 0}
    orig_tok = PLN.sdf_band_from_tokens
    gen = torch.Generator(device="cuda").manual_seed(7)          # the spies leave the global RNG alone

    def check_tokens(tok, sdf):
        """sdf: the band field the pipeline got for these tokens; the dense decode's mesh, and with gradient the dense token gradient."""
        grad = torch.is_grad_enabled() and tok.requires_grad
        with torch.no_grad():
            dense = -hip(hip.grid_queries(xyz), tok.detach()).reshape(-1).float()
        if not grad:
            _same_mesh(xyz, dense, sdf.detach(), res, min_verts=20)
            checked["nograd"] += 1
            return
        cap, hip.row_cap = hip.row_cap, None            # the loop's active-row bound belongs to its own backward
        try:
            g = torch.randn((res + 1) ** 3, device="cuda", generator=gen)
            gb, gd, dense_g = _grads(hip, tok, xyz, res, g, band_fn=orig_tok)
            assert torch.equal(gb, gd)
            _same_mesh(xyz, dense_g, sdf.detach(), res, min_verts=20)
        finally:
            hip.row_cap = cap
        checked["grad"] += 1

    def spy_tok(tokens, xyz_, res_, hip_, bmin, bmax, min_res=None, band=1):
        """Both drivers' route: every image's band field against the dense decode of its tokens."""
        out = orig_tok(tokens, xyz_, res_, hip_, bmin, bmax, min_res=min_res, band=band)
        for t, f in zip(tokens, out[0]):
            check_tokens(t.detach().requires_grad_(t.requires_grad), f)
        return out

    monkeypatch.setattr(PLN, "sdf_band_from_tokens", spy_tok)

    # latent2sdf_band itself (the drivers decode at the level of its tokens): its tokens go through sdf_band_from_tokens (checked there)
    torch.manual_seed(11)
    for with_grad in (True, False):
        lat = torch.randn(1, *pipe.vae.latent_shape, device="cuda").requires_grad_(with_grad)
        n = checked["grad"] + checked["nograd"]
        with (torch.enable_grad() if with_grad else torch.no_grad()):
            sdf, st = PLN.latent2sdf_band(lat, xyz, gsz, pipe.vae, "cuda", BMIN, BMAX)
        assert st["levels"] == [12, 24] and not st["fallback"] and sdf.shape == (1, res + 1, res + 1, res + 1)
        assert checked["grad"] + checked["nograd"] == n + 1 and sdf.requires_grad == with_grad
    assert checked == {"grad": 1, "nograd": 1}
    checked.update(grad=0, nograd=0)

    def run(**extra):
        return pipe(image=[img], mc_algo="mc", generator=torch.manual_seed(2), sil_renderer=None, **kw, **paths, **extra)

    def same(a, b):
        (o1, h1), (o2, h2) = a, b
        assert torch.allclose(h1.verts_packed(), h2.verts_packed(), atol=5e-5)
        assert o1.faces_packed().shape == o2.faces_packed().shape and torch.allclose(o1.verts_packed(), o2.verts_packed(), atol=2e-4)

    none = {"grad": 0, "nograd": 0}

    def used():
        # phase B 3 iterations + phase C 2 x 2 with gradient; the per-step decodes of steps 0-3 without
        assert checked == {"grad": 7, "nograd": 4}, checked
        checked.update(none)

    base = run()
    assert "guidance_decode" not in pipe.stats and checked == none
    band = run(guidance_decode="hierarchical")
    st = pipe.stats["guidance_decode"]
    assert st["decodes"] == checked["grad"] + checked["nograd"] and st["levels"] == [12, 24] and st["fallbacks"] == 0
    assert 0 < st["mean_decoded_fraction"] <= st["max_decoded_fraction"] < 1 and st["max_closure_rounds"] >= 0
    used()
    same(base, band)
    monkeypatch.setenv("FOHO_GUIDANCE_DECODE", "hierarchical")
    env = run()
    used()
    assert pipe.stats["guidance_decode"]["decodes"] == 11
    same(base, env)
    monkeypatch.delenv("FOHO_GUIDANCE_DECODE")
    both = pipe.call_batch([img], [paths], **kw)
    assert "guidance_decode" not in pipe.stats and checked == none
    got = pipe.call_batch([img], [paths], guidance_decode="hierarchical", **kw)
    used()
    st = pipe.stats["guidance_decode"]
    assert isinstance(st, list) and len(st) == 1 and st[0]["decodes"] == 11 and st[0]["levels"] == [12, 24]
    same(both[0], got[0])
    same(base, got[0])
