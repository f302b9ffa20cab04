"""Hierarchical final decode (followmyhold_amd/volume.py, libfoho_vol.so): the (res+1)^3 grid of the last latent2sdf queried near the
surface only, with the dense path's mesh as the contract.  CPU: the library, its exports, argument validation, and the numpy
restatement (tests/vol_ref.py) on analytic fields.  GPU: decoder row independence (what the contract rests on), kernels against
vol_ref index for index, mesh identity with the dense path, the work saved, and the pipeline switch."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vol_ref as V  # noqa: E402
from test_cabi import declared_functions as _declared  # noqa: E402

from followmyhold_amd import _lib, pipeline as PLN, standins, volume  # noqa: E402
from followmyhold_amd.facade import generate_dense_grid_points  # noqa: E402

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BMIN, BMAX = np.full(3, -1.10), np.full(3, 1.10)
f32 = np.float32


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = sorted(l.split()[-1] for l in out.splitlines() if len(l.split()) >= 3 and l.split()[-2] in ("T", "t", "W", "V", "B", "D"))
    return [n for n in names if not n.startswith(("_init", "_fini", "__bss_start", "_edata", "_end", "__hip_"))]


# ---------------------------------------------------------------- analytic fields (numpy and torch, the same elementwise ops)
def np_field(name, res):
    def dec(p):
        x, y, z = (p[:, k].astype(f32) for k in range(3))
        if name == "sphere":
            v = f32(0.25) - ((x * x + y * y) + z * z)
        elif name == "torus":
            q = np.sqrt(x * x + y * y) - f32(0.5)
            v = f32(0.2) - np.sqrt(q * q + z * z)
        elif name == "slabs":
            h = f32(2.2 / res)
            u = x + f32(0.07) * y
            c1 = f32(-0.2)
            c2 = c1 + f32(0.04) + f32(1.5) * h
            v = np.maximum(f32(0.02) - np.abs(u - c1), f32(0.02) - np.abs(u - c2))
        else:
            v = f32(0.003) - np.abs(x + f32(0.31) * y + f32(0.17) * z * z - f32(0.05))
        return v.astype(f32)
    return dec


def torch_field(name, res):
    def dec(p):
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        if name == "sphere":
            return 0.25 - ((x * x + y * y) + z * z)
        if name == "torus":
            q = torch.sqrt(x * x + y * y) - 0.5
            return 0.2 - torch.sqrt(q * q + z * z)
        if name == "slabs":
            h = float(np.float32(2.2 / res))
            u = x + 0.07 * y
            c1 = -0.2
            c2 = c1 + 0.04 + 1.5 * h
            return torch.maximum(0.02 - (u - c1).abs(), 0.02 - (u - c2).abs())
        return 0.003 - (x + 0.31 * y + 0.17 * z * z - 0.05).abs()
    return dec


# ---------------------------------------------------------------- CPU
def test_vol_library_builds_and_exports_exactly_its_header():
    _lib.build()
    assert os.path.exists(volume.SO_PATH)
    want = _declared(os.path.join(ROOT, "followmyhold_amd", "csrc", "foho_vol.h"))
    assert "foho_vol_version" in want and "foho_vol_last_error" in want and len(want) == 10, want
    assert _exported(volume.SO_PATH) == want
    hip = _exported(_lib.SO_PATH)                       # libfoho_hip.so keeps its own 58 entry points and gets none of these
    assert len(hip) == 58 and not [n for n in hip if n.startswith("foho_vol_")]


def test_binding_loads_and_validates_arguments_without_a_gpu():
    _lib.build()
    L = volume.lib()
    assert L.foho_vol_version() == volume.VERSION
    assert L.foho_vol_mark(None, 8, 1, None, None, None) == -1 and b"null" in L.foho_vol_last_error()
    assert L.foho_vol_emit(None, 7, 384, None, None, None, None, None) == -1
    assert L.foho_vol_count_blocks(385 ** 3) == ((385 ** 3 + 63) // 64 + 255) // 256


def test_level_arguments_are_validated():
    assert volume.check_levels(384) == (384, 96) and volume.check_levels(384, 48) == (384, 48) and volume.check_levels(40) == (40, 10)
    for res, mr in [(384, 128), (384, 100), (384, 72), (48, 6), (40, 5), (32, 64)]:
        with pytest.raises(_lib.FohoError):
            volume.check_levels(res, mr)
    with pytest.raises(_lib.FohoError):
        volume.hierarchical_grid_logits(lambda q: q[:, 0], BMIN, BMAX, 384, min_res=128)
    with pytest.raises(_lib.FohoError):
        volume.hierarchical_grid_logits(lambda q: q[:, 0], BMIN, BMAX, 48, min_res=6)


def test_final_decode_switch_is_validated(monkeypatch):
    assert PLN.final_decode_mode() == "dense" and PLN.final_decode_mode("hierarchical") == "hierarchical"
    with pytest.raises(_lib.FohoError):
        PLN.final_decode_mode("sparse")
    monkeypatch.setenv("FOHO_FINAL_DECODE", "hierarchical")
    assert PLN.final_decode_mode() == "hierarchical" and PLN.final_decode_mode("dense") == "dense"
    monkeypatch.setenv("FOHO_FINAL_DECODE", "octree")
    with pytest.raises(_lib.FohoError):
        PLN.final_decode_mode()
    monkeypatch.delenv("FOHO_FINAL_DECODE")
    pipe = standins.make_standin_pipeline(device="cpu", dtype=torch.float32, seed=1)
    assert getattr(pipe.vae, "hip_geo", None) is None
    # refused before any work: an unknown mode, a bad level ratio, and hierarchical without the HIP decoder
    for kw, what in [(dict(final_decode="sparse"), "sparse"), (dict(final_decode="hierarchical"), "hip_geo"),
                     (dict(final_decode="hierarchical", final_decode_min_res=48), "power of two")]:
        kw = dict(kw, final_octree_resolution=40)
        with pytest.raises(_lib.FohoError, match=what):
            pipe(image=None, **kw)
        with pytest.raises(_lib.FohoError, match=what):
            pipe.call_batch([None], [{}], final_octree_resolution=40,
                            **{k: v for k, v in kw.items() if k.startswith("final_decode")})
    with pytest.raises(_lib.FohoError, match="hip_geo"):
        PLN.latent2sdf_hierarchical(torch.zeros(1, 64, 8), BMIN, BMAX, 40, pipe.vae, "cpu")


@pytest.mark.parametrize("name", ["sphere", "torus", "slabs", "sheet"])
def test_reference_reproduces_the_dense_sign_field(name):
    """vol_ref on analytic fields, 12 -> 48 and 24 -> 96: the dense sign everywhere, the dense value at every decoded point, every
    corner of every sign-changing cube decoded; the slabs need a closure round, the sheet settles only in the fall-back, which
    decodes everything."""
    for res, mr in [(48, 12), (96, 24)]:
        max_rounds = 1 if name == "sheet" else 8
        dec_fn = np_field(name, res)
        f, dec, st, lists = V.hierarchical(dec_fn, BMIN, BMAX, res, mr, max_rounds=max_rounds)
        d = V.dense(dec_fn, BMIN, BMAX, res)
        assert np.array_equal(V.inside(f), V.inside(d)), (name, res)
        assert np.array_equal(f[dec], d[dec])
        assert not (V._cells_to_points(V.mixed_cells(d), False) & ~dec).any()
        assert st["levels"] == [mr, 2 * mr, res] and st["decoded"] == sum(l[1].size for l in lists) == int(dec.sum())
        assert all(np.all(np.diff(l[1]) > 0) for l in lists)
        if name == "sheet":
            assert st["fallback"] and np.array_equal(f, d) and dec.all()
        else:
            assert not st["fallback"] and st["decoded_fraction"] < 0.6
        if name == "slabs" and res == 96:
            assert st["closure_rounds"] >= 1


def test_reference_fill_is_the_midpoint_mean_in_a_fixed_order():
    c = np.arange(27, dtype=f32).reshape(3, 3, 3) * f32(0.1) - f32(1.0)
    f = V.fill(c)
    assert f.shape == (5, 5, 5) and np.array_equal(f[::2, ::2, ::2], c)
    assert f[1, 0, 0] == (c[0, 0, 0] + c[1, 0, 0]) * f32(0.5)
    assert f[0, 1, 3] == (((c[0, 0, 1] + c[0, 0, 2]) + c[0, 1, 1]) + c[0, 1, 2]) * f32(0.25)
    s = c[1, 1, 1]
    for a, b, d in [(1, 1, 2), (1, 2, 1), (1, 2, 2), (2, 1, 1), (2, 1, 2), (2, 2, 1), (2, 2, 2)]:
        s = f32(s + c[a, b, d])
    assert f[3, 3, 3] == s * f32(0.125)


# ---------------------------------------------------------------- GPU
def _dense_points(res, dev):
    xyz_np, gsz, _ = generate_dense_grid_points(BMIN, BMAX, octree_depth=5, octree_resolution=res, indexing="ij")
    return torch.as_tensor(xyz_np, dtype=torch.float32, device=dev), gsz


@gpu
@pytest.mark.parametrize("shape", ["small", "full"])
def test_decoder_rows_are_independent_of_the_batch(shape):
    """What the exactness contract rests on: the HIP decoder's logits of a gathered, shuffled subset of a grid equal the dense
    decode's at those indices, bit for bit, for subset sizes around chunk_rows and the 192- / 256-row tile choices."""
    from followmyhold_amd import geo_decode
    torch.manual_seed(0)
    if shape == "small":
        kw, chunk, res = dict(num_latents=128, embed_dim=8, width=128, heads=2, layers=1, num_freqs=8), 512, 40
        sizes = [1, 63, 64, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1025, 5000]
    else:
        kw, chunk, res = dict(num_latents=3072, embed_dim=64, width=1024, heads=16, layers=1, num_freqs=8), None, 64
        sizes = [1, 191, 192, 193, 256, 257, 24576 + 192, 49151, 49152, 49153, 100000]
    vae = standins.StandInShapeVAE(**kw).cuda().half().eval().requires_grad_(False)
    hip = geo_decode.install(vae, chunk_rows=chunk)
    tok = torch.randn(1, kw["num_latents"], kw["width"], device="cuda").half()
    xyz, _ = _dense_points(res, "cuda")
    with torch.no_grad():
        dense = hip(hip.grid_queries(xyz), tok).reshape(-1)
        q = xyz.half().float()
        g = torch.Generator().manual_seed(1)
        for n in sizes:
            sub = torch.randperm(q.shape[0], generator=g)[:n].cuda()
            got = hip(q[sub].reshape(1, -1, 3).contiguous(), tok).reshape(-1)
            assert torch.equal(got, dense[sub]), (shape, n, (got.float() - dense[sub].float()).abs().max().item())


class _Recorder:
    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, p):
        self.calls.append(p.clone())
        return self.fn(p)


@gpu
@pytest.mark.parametrize("name", ["sphere", "torus", "slabs", "sheet"])
def test_kernels_match_the_reference_index_for_index(name):
    """48 -> 192: the points every decode receives (ascending indices, fp16-rounded coordinates), the filled field and the stats
    equal vol_ref's exactly; the sheet with max_rounds=1 takes the fall-back and gives the dense field."""
    res, mr = 192, 48
    max_rounds = 1 if name == "sheet" else 8
    fn = torch_field(name, res)
    rec = _Recorder(fn)
    logits, st = volume.hierarchical_grid_logits(rec, BMIN, BMAX, res, min_res=mr, max_rounds=max_rounds)
    ref_fn = lambda p: fn(torch.from_numpy(p).cuda()).cpu().numpy()      # the same elementwise values on both sides
    f, dec, rst, lists = V.hierarchical(ref_fn, BMIN, BMAX, res, mr, max_rounds=max_rounds)
    tab = V.axis_tables(BMIN, BMAX, res)
    assert len(rec.calls) == len([l for l in lists if l[1].size]), (len(rec.calls), [l[1].size for l in lists])
    for got, (r, idx) in zip(rec.calls, [l for l in lists if l[1].size]):
        assert np.array_equal(got.cpu().numpy(), V.coords(idx, r, tab))
    assert np.array_equal(logits.cpu().numpy(), f.reshape(-1))
    for k in ("levels", "decoded_per_level", "closure_rounds", "closure_decoded", "decoded", "fallback"):
        assert st[k] == rst[k], (k, st[k], rst[k])
    if name == "sheet":
        assert st["fallback"] and torch.equal(logits, fn(_dense_points(res, "cuda")[0].half().float()))
    if name == "slabs":
        assert st["closure_rounds"] >= 1


def _mesh(xyz, sdf, res):
    from followmyhold_amd import ops
    v, f, _ = ops.flexicubes(xyz, sdf.reshape(-1), res)
    return v, f


@gpu
@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_analytic_mesh_is_the_dense_mesh_at_384(name):
    res = 384
    fn = torch_field(name, res)
    xyz, _ = _dense_points(res, "cuda")
    logits, st = volume.hierarchical_grid_logits(fn, BMIN, BMAX, res, min_res=96)
    dense = fn(xyz.half().float())
    v0, f0 = _mesh(xyz, -dense, res)
    v1, f1 = _mesh(xyz, -logits, res)
    assert not st["fallback"] and v0.shape[0] > 1000
    assert torch.equal(v0, v1) and torch.equal(f0, f1)


@gpu
def test_sphere_decodes_under_eight_percent_of_the_grid():
    logits, st = volume.hierarchical_grid_logits(torch_field("sphere", 384), BMIN, BMAX, 384, min_res=96)
    # pinned from vol_ref (the field's arithmetic is exact elementwise float32 on both sides): 97^3 at level 0, then the bands
    assert st["decoded_per_level"] == [912673, 213822, 861750] and st["closure_decoded"] == [] and st["decoded"] == 1988245
    assert st["decoded_fraction"] <= 0.08 and not st["fallback"]


@gpu
def test_standin_decoder_mesh_is_the_dense_mesh():
    """A stand-in ShapeVAE with a smooth field (the smoke test's decoder shape, few Fourier frequencies) on the HIP decoder, 32 -> 128:
    latent2sdf_hierarchical + FlexiCubes gives latent2sdf's mesh index for index."""
    from followmyhold_amd import geo_decode
    torch.manual_seed(0)
    vae = standins.StandInShapeVAE(num_latents=128, embed_dim=8, width=128, heads=2, layers=1, num_freqs=2).cuda().eval().requires_grad_(False)
    geo_decode.install(vae)
    lat = torch.randn(1, 128, 8, device="cuda")
    res = 128
    xyz, gsz = _dense_points(res, "cuda")
    with torch.no_grad():
        dense = PLN.latent2sdf(lat, xyz, gsz, vae, "cuda")
        hier, st = PLN.latent2sdf_hierarchical(lat, BMIN, BMAX, res, vae, "cuda", min_res=32)
    assert hier.shape == dense.shape == (1, res + 1, res + 1, res + 1) and hier.dtype == torch.float32
    assert not st["fallback"] and st["decoded_fraction"] < 0.5, st
    assert torch.equal(hier < 0, dense < 0)
    v0, f0 = _mesh(xyz, dense, res)
    v1, f1 = _mesh(xyz, hier, res)
    assert v0.shape[0] > 1000 and torch.equal(v0, v1) and torch.equal(f0, f1)


@gpu
def test_pipeline_final_decode_switch(tmp_path, monkeypatch):
    """The short stand-in schedule with the HIP decoder, final grid 40 from 10: with final_decode="hierarchical" (kwarg, call_batch
    argument, FOHO_FINAL_DECODE) the final decode's FlexiCubes mesh equals the dense decode's of the same latent, index for index
    (checked inside the run: two whole runs are not bitwise repeatable), stats["final_decode"] is filled in,
    and the results match the default run's as closely as two default runs match each other (tame learning rates)."""
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
    kw = dict(config=cfg, renderer=_renderer(sc["fov"]), J_regressor=sc["J_regressor"], guidance_octree_resolution=24, final_octree_resolution=40)
    checked = []
    res = 40
    xyz, _ = _dense_points(res, "cuda")
    orig_tok = PLN.sdf_hierarchical_from_tokens

    def spy_tok(tokens, bmin, bmax, res_, hip, min_res=None, band=1):
        sdf, st = orig_tok(tokens, bmin, bmax, res_, hip, min_res=min_res, band=band)
        dense = -hip(hip.grid_queries(xyz), tokens).reshape(-1).float()
        checked.append((res_, st, _mesh(xyz, sdf, res_), _mesh(xyz, dense, res_)))
        return sdf, st

    monkeypatch.setattr(PLN, "sdf_hierarchical_from_tokens", spy_tok)

    def run(**extra):
        return pipe(image=[img], mc_algo="mc", generator=torch.manual_seed(2), sil_renderer=None, **kw, **paths, **extra)

    def same(a, b):
        (o1, h1), (o2, h2) = a, b
        assert torch.allclose(h1.verts_packed(), h2.verts_packed(), atol=5e-5)
        assert o1.faces_packed().shape == o2.faces_packed().shape and torch.allclose(o1.verts_packed(), o2.verts_packed(), atol=2e-4)

    def exact(n_images=1):
        assert len(checked) == n_images, len(checked)
        for res_, st, (v1, f1), (v0, f0) in checked:
            assert res_ == res and st["levels"] == [10, 20, 40] and not st["fallback"]
            assert v0.shape[0] > 100 and torch.equal(v0, v1) and torch.equal(f0, f1)
        checked.clear()

    base = run()
    assert "final_decode" not in pipe.stats and not checked
    hier = run(final_decode="hierarchical")
    exact(1)                  # the one final decode, at the level of its tokens (both drivers decode through sdf_hierarchical_from_tokens)
    st = pipe.stats["final_decode"]
    assert st["levels"] == [10, 20, 40] and 0 < st["decoded_fraction"] < 1 and st["decoded"] == sum(st["decoded_per_level"]) + sum(st["closure_decoded"])
    same(base, hier)
    monkeypatch.setenv("FOHO_FINAL_DECODE", "hierarchical")
    env = run()
    exact(1)
    assert pipe.stats["final_decode"]["levels"] == [10, 20, 40]
    same(base, env)
    monkeypatch.delenv("FOHO_FINAL_DECODE")
    both = pipe.call_batch([img], [paths], **kw)
    assert "final_decode" not in pipe.stats and not checked
    got = pipe.call_batch([img], [paths], final_decode="hierarchical", **kw)
    exact()
    assert isinstance(pipe.stats["final_decode"], list) and pipe.stats["final_decode"][0]["levels"] == [10, 20, 40]
    same(both[0], got[0])
    same(base, got[0])
