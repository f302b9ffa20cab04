"""The guided flow-matching pipeline (followmyhold_amd/pipeline.py) = the patched
`Hunyuan3DDiTFlowMatchingPipeline_main.__call__` (third_party_patches/hy3dgen/shapegen/pipelines.py:1041-1679) with the
guidance arithmetic on HIP.  The DiT / ShapeVAE are random-initialised stand-ins (followmyhold_amd/standins.py): what is
tested is the loop, the interfaces and the latent -> SDF -> FlexiCubes -> loss -> gradient chain, not a trained model."""
import inspect
import os

import numpy as np
import pytest
import torch

from followmyhold_amd import inputs, pipeline as PLN, standins, synthetic
from followmyhold_amd.scheduler import FlowMatchEulerDiscreteScheduler

gpu = pytest.mark.gpu


def test_call_signature_is_the_reference_one():
    """PL:1044-1072: parameter names, order and defaults."""
    want = [("image", None), ("num_inference_steps", 30), ("timesteps", None), ("sigmas", None), ("eta", 0.0),
            ("guidance_scale", 7.5), ("generator", None), ("box_v", 1.10), ("octree_resolution", 64), ("mc_level", 0.0),
            ("mc_algo", "mc"), ("num_chunks", 8000), ("output_type", "trimesh"), ("enable_pbar", True), ("config", None),
            ("renderer", None), ("sil_renderer", None), ("cropped_obj_img_path", None), ("hamer_for_guid_path", None),
            ("aligned_mano_mesh_path", None), ("obj_mask_path", None), ("hand_mask_path", None), ("moge_mesh_path", None),
            ("h2m_rt_path", None), ("hunyuan_hoi_mesh_path", None)]
    sig = inspect.signature(PLN.GuidedShapePipeline.__call__)
    got = [(n, p.default) for n, p in sig.parameters.items() if n not in ("self", "kwargs")]
    assert got == want
    assert list(sig.parameters)[-1] == "kwargs" and sig.parameters["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    init = list(inspect.signature(PLN.GuidedShapePipeline.__init__).parameters)
    assert init[1:8] == ["vae", "model", "scheduler", "conditioner", "image_processor", "device", "dtype"]   # PL:563-573


def test_latent2sdf_chunking_sign_and_layout():
    """PL:292-313: latent rescaled by 1/scale_factor, fp16 queries in chunks, logits negated, (1,G,G,G) x-major float32."""
    torch.manual_seed(0)
    vae = standins.StandInShapeVAE(scale_factor=0.5)
    xyz, gsz, _ = PLN.generate_dense_grid_points(np.full(3, -1.1), np.full(3, 1.1), 5, octree_resolution=6)
    xyz = torch.as_tensor(xyz)
    lat = torch.randn(1, *vae.latent_shape)
    a = PLN.latent2sdf(lat, xyz, gsz, vae, "cpu", num_chunks=50)
    b = PLN.latent2sdf(lat, xyz, gsz, vae, "cpu", num_chunks=8000)
    assert a.shape == (1, 7, 7, 7) and a.dtype == torch.float32 and torch.allclose(a, b, atol=1e-6)
    direct = -vae.geo_decoder(xyz[None].half(), vae(lat / 0.5)).reshape(7, 7, 7)      # queries are fp16 (PL:303)
    assert torch.allclose(a[0], direct, atol=1e-6)
    assert a[0, 3, 3, 3] < 0 < a[0, 0, 0, 0]                 # negative inside (box centre), positive at the corner
    lat.requires_grad_(True)
    PLN.latent2sdf(lat, xyz, gsz, vae, "cpu").sum().backward()
    assert lat.grad.abs().sum() > 0


def test_encode_cond_prepare_latents_and_image(tmp_path):
    pipe = standins.make_standin_pipeline(device="cpu")
    from PIL import Image
    rgba = np.zeros((40, 40, 4), np.uint8)
    rgba[10:30, 10:30] = 255
    img = Image.fromarray(rgba, "RGBA")
    im, mk = pipe.prepare_image([img])
    assert im.shape == (1, 3, 32, 32) and mk.shape == (1, 1, 32, 32)
    c = pipe.encode_cond(image=im, mask=mk, do_classifier_free_guidance=True, dual_guidance=False)
    assert c["main"].shape[0] == 2 and torch.equal(c["main"][1], torch.zeros_like(c["main"][1]))   # [cond, uncond]
    c1 = pipe.encode_cond(image=im, mask=mk, do_classifier_free_guidance=False, dual_guidance=False)
    assert c1["main"].shape[0] == 1 and torch.allclose(c1["main"][0], c["main"][0])
    l1 = pipe.prepare_latents(1, torch.float32, "cpu", torch.Generator().manual_seed(2))
    l2 = pipe.prepare_latents(1, torch.float32, "cpu", torch.Generator().manual_seed(2))
    assert l1.shape == (1, *pipe.vae.latent_shape) and torch.equal(l1, l2)
    with pytest.raises(ValueError):
        pipe.prepare_latents(2, torch.float32, "cpu", [torch.Generator()])
    with pytest.raises(FileNotFoundError):
        pipe.prepare_image(str(tmp_path / "missing.png"))


def test_similarity_about_center_matches_reference_formula():
    """PL:108-118 with a quaternion rotation (PL:1322-1325)."""
    v = torch.randn(50, 3)
    q = torch.tensor([0.9, 0.1, -0.2, 0.3])
    out = PLN.similarity_about_center(v, torch.tensor([1.3]), q, torch.tensor([0.1, 0.2, -0.3]))
    c = (v.min(0)[0] + v.max(0)[0]) / 2
    w, x, y, z = (q / q.norm()).tolist()
    R = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    assert torch.allclose(out, (1.3 * (v - c)) @ R.T + c + torch.tensor([0.1, 0.2, -0.3]), atol=1e-5)


class _DecoderStandIn:
    """row_cap, rows_dropped_total and take_rows_dropped as geo_decode.HipGeoDecoder defines them."""

    def __init__(self):
        self.row_cap = None
        self.rows_dropped_total = None

    def take_rows_dropped(self):
        if self.rows_dropped_total is None:
            return 0
        n = int(self.rows_dropped_total.item())
        self.rows_dropped_total.zero_()
        return n


@pytest.mark.parametrize("ending", ["exception", "normal"])
def test_latent_phase_scope_leaves_nothing_on_the_shared_decoder(ending):
    """However a latent phase ends, neither its active-row bound nor its dropped-row count outlives it; without a HIP decoder the scope
    does nothing."""
    hip = _DecoderStandIn()

    def phase(h):
        with PLN._latent_phase_scope(h):
            if h is not None:
                h.row_cap = 7
                h.rows_dropped_total = torch.tensor([3], dtype=torch.int32)
            if ending == "exception":
                raise KeyError("inside the phase")
            return "done"

    for h in (hip, None):
        if ending == "exception":
            with pytest.raises(KeyError, match="inside the phase"):
                phase(h)
        else:
            assert phase(h) == "done"
    assert hip.row_cap is None and hip.take_rows_dropped() == 0 and int(hip.rows_dropped_total) == 0
    # the success path's own check still raises inside the scope, and the scope clears up behind it
    with pytest.raises(PLN.E.L.FohoError, match="3 active rows exceeded row_cap"):
        with PLN._latent_phase_scope(hip):
            hip.row_cap, hip.rows_dropped_total = 7, torch.tensor([3], dtype=torch.int32)
            PLN._check_rows_dropped(hip)
    assert hip.row_cap is None and hip.take_rows_dropped() == 0


@pytest.mark.parametrize("fn, env, choices", [("final_decode_mode", "FOHO_FINAL_DECODE", ("dense", "hierarchical")),
                                              ("final_extract_mode", "FOHO_FINAL_EXTRACT", ("dense", "sparse")),
                                              ("guidance_extract_mode", "FOHO_GUIDANCE_EXTRACT", ("dense", "sparse")),
                                              ("guidance_decode_mode", "FOHO_GUIDANCE_DECODE", ("dense", "hierarchical"))])
def test_option_switches_argument_environment_default(monkeypatch, fn, env, choices):
    mode = getattr(PLN, fn)
    other = choices[1]
    for name in ("FOHO_FINAL_DECODE", "FOHO_FINAL_EXTRACT", "FOHO_GUIDANCE_EXTRACT", "FOHO_GUIDANCE_DECODE"):
        monkeypatch.delenv(name, raising=False)
    assert mode() == "dense" and mode(None) == "dense" and mode(other) == other
    monkeypatch.setenv(env, other)
    assert mode() == other and mode("dense") == "dense"              # the environment wins over the default, the argument over both
    monkeypatch.setenv(env, "")
    assert mode() == "dense"
    for bad_arg, bad_env in (("octree", "dense"), (None, "octree")):
        monkeypatch.setenv(env, bad_env)
        with pytest.raises(PLN.E.L.FohoError) as err:
            mode(bad_arg)
        assert "'octree'" in str(err.value) and all(c in str(err.value) for c in choices) and fn[:-5] in str(err.value)


# ---------------------------------------------------------------------------------------------------------- GPU
def _scene_for_pipeline(H=128, W=128, radius=0.8):
    """A synthetic image whose object fills the Hunyuan box like a real decode does: the Hunyuan -> MoGe similarity is
    rescaled so that a Hunyuan-space radius of `radius` becomes the scene's 5 cm object."""
    from followmyhold_amd import engine as E
    sc = synthetic.build_scene(E.hip_render_fn("cuda"), obj_kind="ico4", H=H, W=W, seed=5)
    T = sc["T_h2m"].astype(np.float64)
    ov_moge = sc["obj_verts"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    s_old = np.cbrt(np.linalg.det(T[:3, :3]))
    T2 = T.copy()
    T2[:3, :3] *= (0.05 / radius) / s_old
    sc["T_h2m"] = T2.astype(np.float32)
    sc["obj_verts"] = ((ov_moge - T2[:3, 3]) @ np.linalg.inv(T2[:3, :3]).T).astype(np.float32)
    return sc


def _write(tmp_path, sc, index="7"):
    names = ["cropped_obj_img_dir", "mask_dir", "moge_out_dir", "hunyuan_hoi_mesh_dir", "hamer_out_dir", "h2m_rt_dir",
             "aligned_mano_dir"]
    d = {n: os.path.join(str(tmp_path), n) for n in names}
    T = sc["T_h2m"].astype(np.float64)
    ov = sc["obj_verts"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    mv = np.concatenate([sc["gt_hand_verts"], ov.astype(np.float32)], 0)
    mf = np.concatenate([sc["hand_faces"], sc["obj_faces"] + len(sc["gt_hand_verts"])], 0)
    inputs.save_scene_files(sc, mv, mf, d, index)
    from PIL import Image
    rgba = np.zeros((sc["H"], sc["W"], 4), np.uint8)
    rgba[sc["obj_mask"]] = 255
    img_path = os.path.join(d["cropped_obj_img_dir"], f"{index}_cropped_hoi_1.png")
    Image.fromarray(rgba, "RGBA").save(img_path)
    return dict(cropped_obj_img_path=img_path,
                hamer_for_guid_path=os.path.join(d["hamer_out_dir"], f"{index}_kps_for_guidance.npy"),
                aligned_mano_mesh_path=os.path.join(d["aligned_mano_dir"], f"{index}_hamer_aligned_mano.ply"),
                obj_mask_path=os.path.join(d["mask_dir"], f"{index}_cropped_obj_mask.png"),
                hand_mask_path=os.path.join(d["mask_dir"], f"{index}_cropped_hand_mask.png"),
                moge_mesh_path=os.path.join(d["moge_out_dir"], f"{index}_cropped_hoi", "mesh.glb"),
                h2m_rt_path=os.path.join(d["h2m_rt_dir"], f"{index}_hoi_mesh.npy"),
                hunyuan_hoi_mesh_path=os.path.join(d["hunyuan_hoi_mesh_dir"], f"{index}_hoi_mesh.ply"))


def _short_config(noise_lr=None):
    from followmyhold_amd import engine as E
    c = E.OptimizationConfig()
    c.num_inference_steps, c.guidance_start_step, c.handopt_start_step, c.guidance_end_step = 5, 2, 1, 5
    c.optimization_steps_hand, c.optimization_steps_scale, c.optimization_steps_joint = 10, 3, 2
    if noise_lr is not None:
        c.noise_obj_lr1 = c.noise_obj_lr2 = noise_lr
    return c


def _renderer(fov):
    from followmyhold_amd import facade as p3d
    cams = p3d.FoVPerspectiveCameras(device="cuda", fov=fov)
    return p3d.MeshRenderer(rasterizer=p3d.MeshRasterizer(cameras=cams, raster_settings=p3d.RasterizationSettings(image_size=128)),
                            shader=p3d.PhongNormalShader(cameras=cams))


@gpu
def test_guided_pipeline_end_to_end_on_files(tmp_path, monkeypatch):
    """All five denoising steps of a short schedule: phase A at step 1, B at step 2, C at steps 3-4, final decode on a
    finer grid; returns (object Meshes, hand Meshes) in the MoGe world."""
    from PIL import Image
    from followmyhold_amd import facade as p3d
    sc = _scene_for_pipeline()
    paths = _write(tmp_path, sc)
    monkeypatch.setenv("FOHO_DEBUG_DIR", str(tmp_path / "debug"))
    pipe = standins.make_standin_pipeline(device="cuda", dtype=torch.float32, seed=1)
    img = Image.open(paths["cropped_obj_img_path"])

    def run(cfg):
        return pipe(image=[img], mc_algo="mc", generator=torch.manual_seed(2), config=cfg, renderer=_renderer(sc["fov"]),
                    sil_renderer=None, J_regressor=sc["J_regressor"], guidance_octree_resolution=24,
                    final_octree_resolution=40, callback=lambda *a: None, callback_steps=1, **paths)

    obj, hand = run(_short_config())
    assert isinstance(obj, p3d.Meshes) and isinstance(hand, p3d.Meshes)
    assert pipe.stats == {"inner_iterations": 10 + 3 + 2 * 2, "skipped_empty": 0}
    ov, of = obj.verts_packed(), obj.faces_packed()
    hv, hf = hand.verts_packed(), hand.faces_packed()
    assert ov.shape[0] > 1000 and of.shape[0] == 2 * ov.shape[0] - 4            # closed genus-0 surface from the fine grid
    assert torch.isfinite(ov).all() and torch.isfinite(hv).all()
    assert hv.shape == (778, 3) and np.array_equal(hf.cpu().numpy(), sc["hand_faces"])
    # the object sits where the Hunyuan -> MoGe transform and the optimised similarity put it: near the scene's object
    T = sc["T_h2m"].astype(np.float64)
    centre = (sc["obj_verts"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).mean(0)
    assert np.abs(ov.mean(0).cpu().numpy() - centre).max() < 0.12     # 7 AdamW steps of lr 1e-2 may move it by 7 cm
    # the hand is the MoGe-space MANO mesh under the optimised similarity (PL:1614-1618)
    gb = pipe.guidance_batch
    p = gb.params[0]
    want = PLN.similarity_about_center(torch.as_tensor(sc["hand_verts"], device="cuda"), p[0], p[4:8], p[1:4])
    assert torch.allclose(hv, want, atol=1e-5)
    assert not torch.allclose(p[:8].cpu(), torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0]))      # phase A moved the hand
    assert not torch.allclose(p[8:].cpu(), torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0]))      # phases B / C moved the object
    # debug artefacts (PL:1076-1091, 1664-1675)
    dbg = [os.path.join(r, f) for r, _, fs in os.walk(str(tmp_path / "debug")) for f in fs]
    assert any(f.endswith("params.json") for f in dbg) and any(f.endswith("final_obj_mesh.ply") for f in dbg)
    assert "Joint optimization step 4" in open([f for f in dbg if f.endswith("losses.txt")][0]).read()
    # the grids of rendered against target normals (plot_in_grid, PL:189-201, 1331-1333, 1417-1419, 1664-1667), as PNG files:
    # phase A every 10 iterations (10 iterations here -> opt0), phase B at k = 0, one per denoising step
    names = sorted(os.path.basename(f) for f in dbg if f.endswith(".png"))
    assert names == ["rendered_normal_hand_t1_opt0.png", "rendered_normal_t0.png", "rendered_normal_t1.png", "rendered_normal_t2.png",
                     "rendered_normal_t3.png", "rendered_normal_t4.png", "rendered_obj_normal_t2_opt0.png"], names
    g = np.asarray(Image.open([f for f in dbg if f.endswith("rendered_normal_t4.png")][0]))
    Hs = sc["H"]
    assert g.shape == (Hs, 2 * sc["W"] + 8, 3) and (g[:, :sc["W"]] > 0).any() and (g[:, sc["W"] + 8:] > 0).any()
    # capacity mode's escape hatch: with an object capacity that is far too small the first latent iteration is redone on the
    # exact-size path, the capacity grows, and the run completes (the two runs are not comparable vertex by vertex: phase A's
    # learning rate of 0.5 makes the trajectory chaotic)
    monkeypatch.delenv("FOHO_DEBUG_DIR")
    monkeypatch.setenv("FOHO_OBJ_CAPACITY", "64,128")
    obj_c, hand_c = run(_short_config())
    monkeypatch.delenv("FOHO_OBJ_CAPACITY")
    assert pipe.stats.get("capacity_grown", 0) >= 1 and pipe.stats.get("exact_size_iterations", 0) >= 1
    assert pipe.stats["inner_iterations"] == 10 + 3 + 2 * 2
    oc = obj_c.verts_packed()
    assert oc.shape[0] > 1000 and torch.isfinite(oc).all() and torch.isfinite(hand_c.verts_packed()).all()
    assert np.abs(oc.mean(0).cpu().numpy() - centre).max() < 0.12
    # the gradient reaches the latent: with the latent's learning rates at zero the decoded object differs
    obj0, _ = run(_short_config(noise_lr=0.0))
    v0 = obj0.verts_packed()
    assert v0.shape != ov.shape or not torch.allclose(v0, ov, atol=1e-6)


@gpu
def test_hand_of_the_last_step_is_returned_after_an_empty_final_decode(tmp_path, monkeypatch):
    """The reference builds a step's hand (PL:1615-1619) before its empty-mesh `continue` (PL:1644-1646) and returns it (PL:1679): when the
    final decode gives no surface, the result is the object of the last step that had one with the hand of the LAST step -- from
    `__call__` and from call_batch.  The end-to-end test's configuration; the final grid's extraction (res 40) is made empty."""
    from PIL import Image
    from followmyhold_amd import ops
    sc = _scene_for_pipeline()
    paths = _write(tmp_path, sc)
    img = Image.open(paths["cropped_obj_img_path"])
    pipe = standins.make_standin_pipeline(device="cuda", dtype=torch.float32, seed=1)
    real, counts = ops.flexicubes, []

    def flexicubes(x, s, res, *a, **kw):
        out = real(x, s, res, *a, **kw)
        if res == 40:
            return tuple(o[:0] for o in out)
        if not torch.is_grad_enabled() and out[0].shape[0] > 0:
            counts.append(out[0].shape[0])
        return out

    monkeypatch.setattr(ops, "flexicubes", flexicubes)
    kw = dict(config=_short_config(), renderer=_renderer(sc["fov"]), J_regressor=sc["J_regressor"], guidance_octree_resolution=24,
              final_octree_resolution=40)
    hand_verts = torch.as_tensor(sc["hand_verts"], device="cuda")

    def check(obj, hand):
        p = pipe.guidance_batch.params[0]
        want = PLN.similarity_about_center(hand_verts, p[0], p[4:8], p[1:4])
        assert torch.allclose(hand.verts_packed(), want, atol=1e-5), float((hand.verts_packed() - want).abs().max())
        assert obj.verts_packed().shape[0] == counts[-1]          # the last non-empty one, from the guidance grid: step 4 gave nothing

    obj, hand = pipe(image=[img], mc_algo="mc", generator=torch.manual_seed(2), sil_renderer=None, **kw, **paths)
    # the last phase C moved the hand: a hand kept from the step before would show
    assert (pipe.param_log[-1][2][:8] - pipe.param_log[-2][2][:8]).abs().max().item() > 1e-6
    check(obj, hand)
    counts.clear()
    (obj, hand), = pipe.call_batch([img], [paths], **kw)
    check(obj, hand)


@gpu
def test_guided_pipeline_with_the_hip_geometry_decoder_in_the_loop(tmp_path):
    """The short schedule again with a ShapeVAE whose decoder the matrix-core kernels take (width 128, 2 heads, 128 latent tokens),
    `geo_decode.install`-ed: every decode of the loop -- with autograd in phases B / C (foho_geo_decode_fwd_cached / _bwd_rows), without for
    the per-step and final grids -- goes through the HIP decoder and the run completes like the one on the torch module: same
    iteration counts, finite closed surfaces, the object where the similarity puts it, and the latent's gradient doing something."""
    from PIL import Image
    from followmyhold_amd import facade as p3d, geo_decode
    sc = _scene_for_pipeline()
    paths = _write(tmp_path, sc)
    img = Image.open(paths["cropped_obj_img_path"])
    kw = dict(num_latents=128, embed_dim=8, width=128, heads=2, layers=1, num_freqs=8)
    T = sc["T_h2m"].astype(np.float64)
    centre = (sc["obj_verts"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).mean(0)
    out = {}
    for name in ("torch", "hip"):
        pipe = standins.make_standin_pipeline(device="cuda", dtype=torch.float32, seed=1, **kw)
        if name == "hip":
            dec = geo_decode.install(pipe.vae)
            calls = {"keep": 0, "fwd": 0, "bwd": 0, "rows": 0}
            for attr, key in (("decode_keep", "keep"), ("decode", "fwd"), ("decode_bwd", "bwd"), ("decode_bwd_rows", "rows")):
                fn = getattr(dec, attr)
                setattr(dec, attr, (lambda f, k: (lambda *a, **b: (calls.__setitem__(k, calls[k] + 1), f(*a, **b))[1]))(fn, key))

        def run(cfg):
            return pipe(image=[img], mc_algo="mc", generator=torch.manual_seed(2), config=cfg, renderer=_renderer(sc["fov"]), sil_renderer=None,
                        J_regressor=sc["J_regressor"], guidance_octree_resolution=24, final_octree_resolution=40, callback=lambda *a: None,
                        callback_steps=1, **paths)

        obj, hand = run(_short_config())
        assert isinstance(obj, p3d.Meshes) and pipe.stats == {"inner_iterations": 10 + 3 + 2 * 2, "skipped_empty": 0}
        ov, of = obj.verts_packed(), obj.faces_packed()
        # closed surface(s): V - F / 2 = 2 per component (this random decoder adds a small second blob to the sphere)
        assert ov.shape[0] > 1000 and (2 * ov.shape[0] - of.shape[0]) in (4, 8, 12) and torch.isfinite(ov).all() and torch.isfinite(hand.verts_packed()).all()
        assert np.abs(ov.mean(0).cpu().numpy() - centre).max() < 0.12
        obj0, _ = run(_short_config(noise_lr=0.0))
        v0 = obj0.verts_packed()
        assert v0.shape != ov.shape or not torch.allclose(v0, ov, atol=1e-6)           # the gradient reached the latent
        out[name] = ov
    # 3 + 2 x 2 latent iterations under autograd per run (two runs), each one plain forward (cached query side) + one backward over the
    # rows FlexiCubes sent a gradient to (the default route; nothing kept, no dense backward); the no-gradient decodes besides
    assert calls["keep"] == calls["bwd"] == 0 and calls["rows"] >= 7 and calls["fwd"] >= calls["rows"] + 5, calls
    assert dec._qcache is not None                                  # the guidance grid's query side was cached
    # same decoded object as with the torch decoder up to what a chaotic 17-iteration trajectory does to it
    assert abs(out["hip"].shape[0] - out["torch"].shape[0]) <= 0.2 * out["torch"].shape[0]
    assert (out["hip"].mean(0) - out["torch"].mean(0)).abs().max().item() < 0.05


@gpu
def test_latent_to_loss_chain_matches_the_oracle_chain():
    """One phase-C iteration exactly as the pipeline runs it (PL:1505-1601): noise prediction -> step_final -> VAE ->
    SDF grid -> FlexiCubes -> joint loss, and dL/d(noise prediction).  HIP chain vs the CPU chain through the oracle
    (same VAE weights on the CPU -> oracle/flexi_ref -> oracle/step_ref)."""
    from followmyhold_amd import engine as E, ops
    from helpers import make_scene
    from oracle import flexi_ref as FR, ref_ops as R, step_ref as S
    res = 12
    sc = make_scene("ico2", 64, 64, seed=0)
    # Hunyuan -> MoGe similarity rescaled so that the stand-in decoder's r = 0.8 sphere is the scene's object
    T = sc["T_h2m"].double()
    s_old = float(torch.linalg.det(T[:3, :3])) ** (1 / 3)
    T2 = T.clone()
    T2[:3, :3] *= (float(sc["obj_verts"].norm(dim=1).mean()) * s_old / 0.8) / s_old
    sc["T_h2m"] = T2.float()
    torch.manual_seed(3)
    vae = standins.StandInShapeVAE(gain=0.4)
    sch = FlowMatchEulerDiscreteScheduler()
    sch.set_timesteps(sigmas=np.linspace(0, 1, 20), device="cpu")
    t = sch.timesteps[12]
    latents = torch.randn(1, *vae.latent_shape)
    noise0 = torch.randn(1, *vae.latent_shape)
    xyz, gsz, _ = PLN.generate_dense_grid_points(np.full(3, -1.1), np.full(3, 1.1), 5, octree_resolution=res)
    xyz = torch.as_tensor(xyz)
    # oracle chain (CPU)
    n_o = noise0.clone().requires_grad_(True)
    sdf_o = PLN.latent2sdf(sch.step_final(n_o, t, latents), xyz, gsz, vae, "cpu")
    V, F, _ = FR.flexicubes(xyz, sdf_o[0].flatten(), res)
    assert len(V) > 100
    p = S.make_params()
    total, terms, aux = S.phase_c_loss(dict(sc, obj_faces=F), p, V, R.unique_edges(F), denoise_i=19, grid_res=16)
    total.backward()
    # HIP chain
    sch_g = FlowMatchEulerDiscreteScheduler()
    sch_g.set_timesteps(sigmas=np.linspace(0, 1, 20), device="cuda")
    vae_g = vae.to("cuda")
    n_g = noise0.cuda().requires_grad_(True)
    sdf_g = PLN.latent2sdf(sch_g.step_final(n_g, sch_g.timesteps[12], latents.cuda()), xyz.cuda(), gsz, vae_g, "cuda")
    assert torch.equal(sdf_g.cpu() < 0, sdf_o.detach() < 0)            # same inside/outside pattern on both devices
    v, f, _ = ops.flexicubes(xyz.cuda(), sdf_g[0].flatten(), res)
    assert torch.equal(f.cpu(), F)
    npsc = {k: (v_.numpy() if isinstance(v_, torch.Tensor) else v_) for k, v_ in sc.items()}
    gb = E.GuidanceBatch([npsc], grid_res=16)
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=False)
    loss = gb.objective(v, f, cfg)
    loss.backward()
    torch.cuda.synchronize()
    gb.raise_on_flags()
    assert abs(float(loss) - float(total)) <= 1e-4 * abs(float(total))
    g, go = n_g.grad.cpu().numpy(), n_o.grad.numpy()
    assert np.linalg.norm(go) > 0 and np.linalg.norm(g - go) <= 5e-3 * np.linalg.norm(go), (np.linalg.norm(g - go), np.linalg.norm(go))


@gpu
def test_guidance_stage_driver_with_standin_networks(tmp_path, monkeypatch):
    """`foho.guidance.run.run` (RUN:188-261) end to end through GuidedShapePipeline: image -> RGBA with white made
    transparent, pipeline call with the reference's keyword arguments, {idx}_obj.ply / {idx}_hand.ply written."""
    from foho.guidance import run as G
    from followmyhold_amd import meshio
    sc = _scene_for_pipeline()
    paths = _write(tmp_path, sc, index="31")
    jr = str(tmp_path / "J.npy")
    np.save(jr, sc["J_regressor"])
    monkeypatch.setenv("FOHO_J_REGRESSOR", jr)
    monkeypatch.setenv("FOHO_STANDIN_NETWORKS", "1")
    monkeypatch.setattr(G, "_PIPELINE", None)
    monkeypatch.setattr(G, "OptimizationConfig", lambda: _short_config())
    img = G._load_object_image(paths["cropped_obj_img_path"])[0]
    assert img.mode == "RGBA"
    d = {k: os.path.join(str(tmp_path), k) for k in ["cropped_obj_img_dir", "mask_dir", "moge_out_dir", "hunyuan_hoi_mesh_dir",
                                                     "hamer_out_dir", "h2m_rt_dir", "aligned_mano_dir", "guidance_out_dir"]}
    G.run(project_root=str(tmp_path), task_list_file=None, **d)
    ov, of = meshio.load_ply(os.path.join(d["guidance_out_dir"], "31_obj.ply"))
    hv, hf = meshio.load_ply(os.path.join(d["guidance_out_dir"], "31_hand.ply"))
    assert len(ov) > 1000 and len(of) == 2 * len(ov) - 4 and np.isfinite(ov).all()
    assert hv.shape == (778, 3) and np.array_equal(hf, sc["hand_faces"])


@gpu
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_replay_of_the_reference_loop_trajectory(tmp_path, variant):
    """tests/golden/ref_pipeline*.npz hold what the REFERENCE's own `__call__` (PL:1044-1679) returned and printed when it
    was executed in the build container on these scenes with the CPU restatement standing in for pytorch3d / kaolin
    (tests/golden/make_pipeline_golden.py; variant 1 has two joint denoising steps and the intersection term off).  The
    same inputs through GuidedShapePipeline on the GPU must give the same first-iteration losses of every phase (they
    depend on everything before them: DiT call, CFG mix, scheduler, latent -> SDF -> FlexiCubes, the optimisation of the
    earlier phases, scheduler.step), the same per-phase parameters, the same final hand and the same final object.
    Variant 3 ("_hd64") has a ShapeVAE of width 128 with two heads of 64 over 128 latent tokens: here BOTH `vae_transformer.install` and
    `geo_decode.install` are applied, so `vae(pred)` (PL:295) runs on foho_vae_fwd / _bwd and every decode on foho_geo_decode_* INSIDE
    the compared trajectory -- fp16 kernels against the reference's float32 torch: tolerances x `F16`."""
    import json
    import re
    import sys
    from PIL import Image
    from followmyhold_amd import engine as E
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    sys.path.insert(0, gdir)
    import make_pipeline_golden as MPG
    var = MPG.VARIANTS[variant]
    ref = np.load(os.path.join(gdir, f"ref_pipeline{var['tag']}.npz"))
    meta = json.load(open(os.path.join(gdir, f"ref_pipeline{var['tag']}.json")))
    sc, paths = MPG.build_inputs(tmp_path, var["scene"])
    chk = np.array([float(np.abs(sc[k].astype(np.float64)).sum()) for k in ("hand_verts", "obj_verts", "moge_normal", "moge_disp", "kps_2d", "T_h2m")])
    assert np.allclose(chk, ref["scene_checksum"], rtol=1e-6), "the synthetic scene differs from the one the fixture was made on"
    pipe = standins.make_standin_pipeline(device="cuda", dtype=torch.float32, seed=1, **var.get("vae_kw", MPG.VAE_KW))
    F16 = 1.0
    if var["tag"] == "_hd64":
        from followmyhold_amd import geo_decode, vae_transformer
        geo_decode.install(pipe.vae)
        tr = vae_transformer.install(pipe.vae)
        F16 = 8.0
    wchk = np.array([float(sum(p.detach().double().abs().sum() for p in m.parameters())) for m in (pipe.vae, pipe.model, pipe.conditioner)])
    assert np.allclose(wchk, ref["weights_checksum"], rtol=1e-6), "stand-in network initialisation differs"
    cfg = E.OptimizationConfig()
    for k, v in {**var["schedule"], **var["config"]}.items():
        setattr(cfg, k, v)
    # Phase A takes a few Adam steps with a quaternion learning rate of 0.5 on a small render: its result agrees with the
    # reference's to a few 1e-3 (Adam with eps = 1e-4 turns a 1e-6 difference in a small gradient component into a 1e-3
    # step), and a difference of that size moves enough pixels between faces to change the later (much smaller) phase-C
    # hand gradients.  To compare the later phases like for like, they are started from the reference's own phase-A result.
    after_a = {}

    def align(phase, i, gb):
        if phase == "A":
            after_a["params"] = gb.params[0, :8].clone()
            gb.params[0, :8] = torch.as_tensor(ref["opt0_small"], device=gb.params.device)

    obj, hand = pipe(image=[Image.open(paths["cropped_obj_img_path"])], mc_algo="mc", generator=torch.manual_seed(2), config=cfg,
                     renderer=_renderer(sc["fov"]), sil_renderer=None, J_regressor=sc["J_regressor"], enable_pbar=False,
                     on_phase_end=align, **paths)
    sch = var["schedule"]
    n_joint = sch["num_inference_steps"] - sch["handopt_start_step"] - 2
    assert pipe.stats == {"inner_iterations": sch["optimization_steps_hand"] + sch["optimization_steps_scale"]
                          + n_joint * sch["optimization_steps_joint"], "skipped_empty": 0}
    # variant 2 runs phase A at 1 / 500 of the reference's learning rates, where the trajectory itself is comparable
    d_a = np.abs(after_a["params"].cpu().numpy() - ref["opt0_small"]).max()
    assert d_a < (2e-5 if var["tag"] in ("_tame", "_hd64") else 6e-3), d_a
    if var["tag"] in ("_tame", "_hd64"):
        assert np.abs(ref["opt0_small"] - np.array([1, 0, 0, 0, 1, 0, 0, 0], np.float32)).max() > 1e-4      # it did move
    # first-iteration losses the reference printed (PL:1351-1355, 1446-1450, 1594-1598)
    num = lambda line: dict((k.strip(), float(v)) for k, v in re.findall(r"([A-Za-z_ 0-9]+): ([-+0-9.eE]+)", line.split(",", 1)[1]))
    opt = [num(l) for l in meta["log"] if l.startswith("Opt step 0")]
    assert [(p_, k_) for p_, _, k_, _ in pipe.loss_log] == [("A", 0), ("B", 0)] + [("C", 0)] * n_joint and len(opt) == 2 + n_joint
    close = lambda a, b, tol: abs(a - b) <= tol * abs(b) + 1e-12
    la, lb = pipe.loss_log[0][3], pipe.loss_log[1][3]
    assert close(la["kps"], opt[0]["loss_2d_kps"], 1e-4) and close(la["normal0"], opt[0]["loss_normal_hand"], 1e-4)
    assert close(la["disp0"], opt[0]["loss_disp_hand"], 1e-4)
    assert close(lb["edge"], opt[1]["object loss"], 1e-4 * F16 ** 2) and close(lb["normal0"], opt[1]["loss_normal_obj"], 1e-4 * F16 ** 2), (lb, opt[1])
    assert close(lb["disp0"], opt[1]["loss_disp"], 1e-4 * F16 ** 2)
    for j in range(n_joint):
        lc, rc = pipe.loss_log[2 + j][3], opt[2 + j]
        tol = 2e-3 * (1 + 4 * j) * F16    # each further joint step inherits the differences of the one before
        assert close(lc["edge"], rc["object loss"], tol) and close(lc["normal1"], rc["loss_normal_hoi"], tol), (j, lc, rc)
        assert close(lc["disp1"], rc["loss_disp"], tol)
        if cfg.use_intersection_loss:
            assert close(lc["n_intersect"] / 1000.0, rc["loss_intersection"], 2e-2 * (F16 / 2 if F16 > 1 else 1))
        else:
            assert rc["loss_intersection"] == 0.0
    # parameters each phase ended with (the reference's per-phase leaf tensors, PL:1300-1318, 1366-1384, 1461-1478)
    assert len(pipe.param_log) == 2 + n_joint and meta["optimizers"] == ["Adam"] + ["AdamW"] * (1 + n_joint)
    _, _, pb_, nb = pipe.param_log[1]
    assert np.allclose(pb_[8:].cpu().numpy(), ref["opt1_small"], atol=2e-4 * F16) and np.allclose(nb.cpu().numpy(), ref["opt1_noise"], atol=2e-4 * F16), \
        (np.abs(pb_[8:].cpu().numpy() - ref["opt1_small"]).max(), np.abs(nb.cpu().numpy() - ref["opt1_noise"]).max())
    # The first joint phase starts from matched states and is compared tightly.  A later one inherits 1e-4-level differences,
    # and where a gradient component is near zero Adam (eps 1e-4) turns those into a different step of size lr (1e-2 for the
    # object translation / rotation): only the hand (lr 1e-4 / 1e-2, well-conditioned) stays tight there.
    for j in range(n_joint):
        _, _, pc_, nc = pipe.param_log[2 + j]
        # (fp16 kernels in the loop, variant 3: the object's near-zero gradient components get the Adam treatment from the first joint step on)
        atol = np.full(16, 5e-4) if (j == 0 and F16 == 1.0) else np.concatenate([np.full(8, 2e-3 * min(F16, 2.0)), np.full(8, 2.5e-2)])
        diff = np.abs(pc_.cpu().numpy() - ref[f"opt{2 + j}_small"])
        assert (diff <= atol).all(), (j, pc_.cpu().numpy(), ref[f"opt{2 + j}_small"])
        assert np.allclose(nc.cpu().numpy(), ref[f"opt{2 + j}_noise"], atol=(5e-3 if j == 0 else 5e-2) * min(F16, 2.0))
    # final hand: the MoGe-space MANO under the optimised similarity; final object: res-384 decode under its similarity
    tol_v = 2e-4 * (1 + 10 * (n_joint - 1)) * F16
    if var["tag"] == "_hd64":      # the kernels were in the loop: every latent iteration went through foho_vae_fwd (+ _bwd), none through torch
        assert tr.calls >= sch["optimization_steps_scale"] + n_joint * sch["optimization_steps_joint"] + sch["num_inference_steps"], tr.calls
    hv = hand.verts_packed().cpu().numpy()
    assert np.array_equal(hand.faces_packed().cpu().numpy(), ref["hand_faces"])
    assert np.abs(hv - ref["hand_verts"]).max() < tol_v, np.abs(hv - ref["hand_verts"]).max()
    ov, of = obj.verts_packed().cpu().numpy(), obj.faces_packed().cpu().numpy()
    assert abs(len(ov) - ref["obj_counts"][0]) <= 0.002 * F16 * ref["obj_counts"][0]
    st, want = MPG.object_stats(ov, of), ref["obj_stats"]
    assert np.abs(st[:9] - want[:9]).max() < (1e-3 if n_joint == 1 else 2.5e-2) * min(F16, 3.0)      # centroid and bounding box (metres)
    assert np.allclose(st[9:], want[9:], rtol=(2e-2 if n_joint == 1 else 0.15) * min(F16, 2.0))        # radius mean / std, area, volume


@gpu
def test_call_batch_equals_two_single_image_calls(tmp_path):
    """GuidedShapePipeline.call_batch: two images through ONE pass of the schedule (DiT / VAE on two latents, one two-slot
    capacity-mode GuidanceBatch, one AdamW over both noise predictions) against two `__call__` runs -- the reference's way,
    one image after the other (RUN:208-259) -- at tame learning rates (1/500: at the reference's own rates two executions
    of ONE image already separate)."""
    from PIL import Image
    scs = [_scene_for_pipeline(), _scene_for_pipeline(radius=0.7)]
    scs[1]["kps_2d"] = scs[1]["kps_2d"] + 1.5
    paths = [_write(tmp_path / f"img{b}", sc, index=str(7 + b)) for b, sc in enumerate(scs)]
    cfg = _short_config()
    for name in ("phase1_hand_lrs", "phase2_hand_lrs", "obj_lrs", "obj_2half_lrs"):
        setattr(cfg, name, {k: v / 500.0 for k, v in getattr(cfg, name).items()})
    cfg.noise_obj_lr1, cfg.noise_obj_lr2 = cfg.noise_obj_lr1 / 500.0, cfg.noise_obj_lr2 / 500.0
    pipe = standins.make_standin_pipeline(device="cuda", dtype=torch.float32, seed=1)
    imgs = [Image.open(p["cropped_obj_img_path"]) for p in paths]
    kw = dict(config=cfg, renderer=_renderer(scs[0]["fov"]), J_regressor=scs[0]["J_regressor"], guidance_octree_resolution=24,
              final_octree_resolution=40)
    singles, params = [], []
    for b in range(2):
        singles.append(pipe(image=[imgs[b]], mc_algo="mc", generator=torch.Generator().manual_seed(2), sil_renderer=None, **kw, **paths[b]))
        params.append(pipe.guidance_batch.params[0].clone())
    both = pipe.call_batch(imgs, paths, **kw)
    assert pipe.stats["inner_iterations"] == 10 + 3 + 2 * 2 and len(both) == 2
    for b in range(2):
        assert torch.allclose(pipe.guidance_batch.params[b], params[b], atol=2e-5), (b, pipe.guidance_batch.params[b], params[b])
        (o1, h1), (o2, h2) = singles[b], both[b]
        assert torch.allclose(h1.verts_packed(), h2.verts_packed(), atol=5e-5)
        assert o1.faces_packed().shape == o2.faces_packed().shape and torch.allclose(o1.verts_packed(), o2.verts_packed(), atol=2e-4)
    ext = [(m[0].verts_packed().max(0)[0] - m[0].verts_packed().min(0)[0]).max().item() for m in both]
    assert abs(ext[0] - ext[1]) > 5e-3, ext                                              # two different images (object sizes)
    # an iso-surface beyond the capacity is the one-image path's business: the image LEAVES the batch (its result says why) instead of
    # being approximated -- here both do, at the first iteration that decodes an object
    gone = pipe.call_batch(imgs, paths, obj_capacity=(64, 128), **kw)
    assert all(isinstance(r, PLN.BatchLeftFastPath) and r.phase == "B" and r.iteration == 0 and r.flags & 16 for r in gone), gone
    assert pipe.stats["left_batch"] == [0, 1]


@gpu
def test_call_batch_handles_events_per_image(tmp_path, monkeypatch):
    """One image of a batch meets what the reference handles per image; the other must not notice.  (a) An EMPTY iso-surface at one
    iteration (PL:1394-1397, 1511-1513: `continue` -- no optimiser step for that image at that iteration): the other image's result
    is its result from an undisturbed batch (tame learning rates as in the test above: at the reference's own rates two runs of ONE
    image separate), the skip is counted and nobody leaves.  (b) A NaN loss (PL:1442-1444, 1590-1592): that image leaves the batch
    -- its entry says so, with phase and iteration --, the other one's result is again the undisturbed one."""
    from PIL import Image
    from followmyhold_amd import engine as E
    scs = [_scene_for_pipeline(), _scene_for_pipeline(radius=0.7)]
    paths = [_write(tmp_path / f"img{b}", sc, index=str(7 + b)) for b, sc in enumerate(scs)]
    cfg = _short_config()
    for name in ("phase1_hand_lrs", "phase2_hand_lrs", "obj_lrs", "obj_2half_lrs"):
        setattr(cfg, name, {k: v / 500.0 for k, v in getattr(cfg, name).items()})
    cfg.noise_obj_lr1, cfg.noise_obj_lr2 = cfg.noise_obj_lr1 / 500.0, cfg.noise_obj_lr2 / 500.0
    pipe = standins.make_standin_pipeline(device="cuda", dtype=torch.float32, seed=1)
    imgs = [Image.open(p["cropped_obj_img_path"]) for p in paths]
    kw = dict(config=cfg, renderer=_renderer(scs[0]["fov"]), J_regressor=scs[0]["J_regressor"], guidance_octree_resolution=24, final_octree_resolution=40)
    clean = pipe.call_batch(imgs, paths, **kw)
    assert pipe.stats["skipped_empty"] == 0 and pipe.stats["left_batch"] == []
    orig = E.SdfObjective.run
    for event in ("empty", "nan"):
        n = {"calls": 0}

        def run(self, sdf, cfg_, use_graph=True):
            n["calls"] += 1
            hit = n["calls"] == 2                        # the second latent iteration of phase B, image 1 only
            if hit and event == "empty":
                sdf = sdf.detach().clone()
                sdf[1] = 1.0                             # positive everywhere: no surface
            out = orig(self, sdf, cfg_, use_graph)
            if hit and event == "nan":
                self.gb.flags[1] |= 1                    # what the step reports for a NaN total loss (k_final.inc; tested on its own)
            return out

        monkeypatch.setattr(E.SdfObjective, "run", run)
        got = pipe.call_batch(imgs, paths, **kw)
        monkeypatch.setattr(E.SdfObjective, "run", orig)
        (o0, h0), (c0, ch0) = got[0], clean[0]
        assert o0.faces_packed().shape == c0.faces_packed().shape and torch.allclose(o0.verts_packed(), c0.verts_packed(), atol=2e-4)
        assert torch.allclose(h0.verts_packed(), ch0.verts_packed(), atol=5e-5)
        if event == "empty":
            assert pipe.stats["skipped_empty"] == 1 and pipe.stats["left_batch"] == []
            assert pipe.stats["inner_iterations"] == 10 + 3 + 2 * 2
            o1, h1 = got[1]
            assert torch.isfinite(o1.verts_packed()).all() and torch.isfinite(h1.verts_packed()).all()
        else:
            assert isinstance(got[1], PLN.BatchLeftFastPath) and got[1].phase == "B" and got[1].iteration == 1 and pipe.stats["left_batch"] == [1]


@gpu
def test_guidance_stage_driver_batches_images_with_the_networks_in_the_loop(tmp_path, monkeypatch, capsys):
    """`foho.guidance.run.run` over three images with FOHO_PIPELINE_BATCH=2: two go through ONE pass of the schedule
    (GuidedShapePipeline.call_batch), the third on its own; the reference's messages per image, six PLY files, metrics of
    three images.  Images that leave the batch (here: all, forced by a tiny object capacity) are redone one at a time."""
    from foho.guidance import run as G
    from followmyhold_amd import meshio, pipeline as PL_
    scs = [_scene_for_pipeline(), _scene_for_pipeline(radius=0.7), _scene_for_pipeline(radius=0.75)]
    for b, sc in enumerate(scs):
        _write(tmp_path, sc, index=str(41 + b))
    jr = str(tmp_path / "J.npy")
    np.save(jr, scs[0]["J_regressor"])
    monkeypatch.setenv("FOHO_J_REGRESSOR", jr)
    monkeypatch.setenv("FOHO_STANDIN_NETWORKS", "1")
    monkeypatch.setenv("FOHO_PIPELINE_BATCH", "2")
    monkeypatch.setattr(G, "_PIPELINE", None)
    monkeypatch.setattr(G, "OptimizationConfig", lambda: _short_config())
    calls = []
    orig = PL_.GuidedShapePipeline.call_batch
    monkeypatch.setattr(PL_.GuidedShapePipeline, "call_batch", lambda self, images, paths, **kw: (calls.append(len(images)), orig(self, images, paths, **kw))[1])
    d = {k: os.path.join(str(tmp_path), k) for k in ["cropped_obj_img_dir", "mask_dir", "moge_out_dir", "hunyuan_hoi_mesh_dir",
                                                     "hamer_out_dir", "h2m_rt_dir", "aligned_mano_dir", "guidance_out_dir"]}
    tot = G.run(project_root=str(tmp_path), task_list_file=None, **d)
    out = capsys.readouterr().out
    assert calls == [2] and tot["n_images"] == 3 and tot["n_failed"] == 0
    for idx in ("41", "42", "43"):
        assert f"Processing {idx}" in out and f"Reconstructed object {idx}" in out
        ov, of = meshio.load_ply(os.path.join(d["guidance_out_dir"], f"{idx}_obj.ply"))
        hv, _ = meshio.load_ply(os.path.join(d["guidance_out_dir"], f"{idx}_hand.ply"))
        assert len(ov) > 1000 and len(of) == 2 * len(ov) - 4 and np.isfinite(ov).all() and hv.shape == (778, 3)
    # the fall-back: a batch whose surfaces exceed the capacity is redone image by image
    import shutil
    shutil.rmtree(d["guidance_out_dir"])
    monkeypatch.setattr(PL_.GuidedShapePipeline, "call_batch", lambda self, images, paths, **kw: orig(self, images, paths, obj_capacity=(64, 128), **kw))
    tot = G.run(project_root=str(tmp_path), task_list_file=None, **d)
    out = capsys.readouterr().out
    assert "left the batched path" in out and tot["n_failed"] == 0 and len(os.listdir(d["guidance_out_dir"])) == 6
