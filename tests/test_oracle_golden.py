"""Pin the oracle (and the host-side mirrors) to golden vectors produced by the REFERENCE's own helpers.

tests/golden/ref_helpers.npz + ref_meta.json were generated in the build container by
tests/golden/make_golden.py, which imports /root/reference's pipelines.py / schedulers.py / code_utils.py /
guid_config.py with stub modules for the un-vendored dependencies (fixtures F1-F9).
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import ref_ops as R

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "ref_helpers.npz"))
META = json.load(open(os.path.join(HERE, "golden", "ref_meta.json")))


def t(name):
    return torch.from_numpy(G[name])


def test_f1_normal_alignment_loss():
    a, b, m = t("f1_a"), t("f1_b"), t("f1_mask")
    assert abs(float(R.normal_alignment_loss(a, b, m)) - float(G["f1_loss_mask"])) < 1e-6
    assert abs(float(R.normal_alignment_loss(a, b)) - float(G["f1_loss_nomask"])) < 1e-6


def test_f2_honerf_intersection_is_a_count_without_gradient():
    sh, so = t("f2_sdf_hand"), t("f2_sdf_obj")
    assert float(R.honerf_intersection_loss(sh, so)) == pytest.approx(float(G["f2_honerf"]), abs=0)
    assert META["f2_honerf_requires_grad"] is False
    assert not R.honerf_intersection_loss(sh.clone().requires_grad_(True), so).requires_grad
    # the engine consumes it as count/1000 of points inside both meshes
    n = int(((sh < 0) & (so < 0)).sum())
    assert n / 1000 == pytest.approx(float(G["f2_honerf"]))


def test_f3_dense_grid_points():
    xyz = R.dense_grid_points(np.array([-1.1] * 3), np.array([1.1] * 3), 64)
    assert list(xyz.shape) == list(G["f3_shape"])
    assert np.array_equal(xyz[:70], G["f3_first"]) and np.array_equal(xyz[-70:], G["f3_last"])
    cs = np.array([xyz.astype(np.float64).sum(), (xyz.astype(np.float64) ** 2).sum()])
    assert np.allclose(cs, G["f3_checksum"], rtol=0, atol=1e-9)
    small = R.dense_grid_points(np.array([-0.3, 0.1, -0.7], np.float32), np.array([0.4, 0.35, -0.2], np.float32), 8)
    assert np.array_equal(small, G["f3_small"])  # x-major order, float64 linspace cast to float32


def test_f4_render_normal_and_disparity():
    rgba, z = t("f4_rgba")[0], t("f4_zbuf")[0, ..., 0]
    nn, dd = R.render_normal_and_disparity(rgba, z)
    assert np.abs(nn.numpy() - G["f4_normal"][0]).max() < 1e-6
    assert np.abs(dd.numpy() - G["f4_disp"][0]).max() < 1e-6


def test_f5_transforms_and_keypoints():
    v, T, s, jr = t("f5_verts"), t("f5_T"), t("f5_scale"), t("f5_jreg")
    out = R.transform_around_center_w_scale(v, T[:3, :3], T[:3, 3], s)
    assert np.abs(out.numpy() - G["f5_center_scale"]).max() < 1e-6
    out1 = R.transform_around_center_w_scale(v, T[:3, :3], T[:3, 3], torch.tensor([1.0]))
    assert np.abs(out1.numpy() - G["f5_center"]).max() < 1e-6
    assert np.abs(R.transform_hunyuan2moge(v, T).numpy() - G["f5_h2m"]).max() < 1e-6
    assert np.abs(R.mano_vert_to_3dkps(v, jr).numpy() - G["f5_kps"]).max() < 1e-6


def test_f6_get_guidance_params():
    from followmyhold_amd.engine import OptimizationConfig
    from followmyhold_amd.guidance_params import get_guidance_params
    cfg = OptimizationConfig()
    names = ["noise_pred_obj", "scale_hand", "trans_hand", "rotation_hand", "scale_obj", "trans_obj", "rotation_obj"]
    base = dict(noise_pred_obj=torch.randn(1, 8, 4).half(), scale_hand=torch.tensor([1.0]), trans_hand=torch.zeros(3),
                rotation_hand=torch.tensor([1.0, 0, 0, 0]), device="cpu", phase1_hand_lrs=cfg.phase1_hand_lrs,
                phase2_hand_lrs=cfg.phase2_hand_lrs, noise_obj_lr1=cfg.noise_obj_lr1, noise_obj_lr2=cfg.noise_obj_lr2,
                obj_lrs=cfg.obj_lrs, obj_2half_lrs=cfg.obj_2half_lrs, scale_obj=torch.tensor([1.0]),
                trans_obj=torch.zeros(3), rotation_obj=torch.tensor([1.0, 0, 0, 0]))
    for phase in (1, 1.5, 2):
        ref = META["f6"][str(phase)]
        res = get_guidance_params(phase, **base)
        groups = res[0]
        assert [g["lr"] for g in groups] == ref["lrs"]
        assert [list(g["params"][0].shape) for g in groups] == ref["shapes"]
        assert [str(g["params"][0].dtype) for g in groups] == ref["dtypes"]
        for n, tt in zip(names, res[1:]):
            assert bool(tt.requires_grad) == ref["requires_grad"][n], (phase, n)
            assert bool(tt is base[n]) == ref["is_same_object"][n], (phase, n)
    with pytest.raises(ValueError):
        get_guidance_params(3, **base)
    assert META["f6"]["bad_phase_raises"] is True


def test_f7_optimization_config():
    from foho.configs import OptimizationConfig
    cfg = OptimizationConfig()
    assert {k: v for k, v in vars(cfg).items()} == META["f7"]
    assert cfg() is cfg and META["f7_call_returns_self"]


def test_f8_scheduler_step_and_step_final():
    from followmyhold_amd.scheduler import FlowMatchEulerDiscreteScheduler, retrieve_timesteps
    s = FlowMatchEulerDiscreteScheduler()
    assert vars(s.config) == META["f8_config"]
    ts, n = retrieve_timesteps(s, 20, "cpu", sigmas=np.linspace(0, 1, 20))
    assert n == 20 and np.array_equal(ts.numpy(), G["f8_timesteps"]) and np.array_equal(s.sigmas.numpy(), G["f8_sigmas"])
    x, vel = t("f8_lat0"), t("f8_vel")
    for k in range(3):
        before = s.step_final(vel[k], ts[k], x)             # inner loops (pipelines.py:1391, :1507) read sigma_k
        x = s.step(vel[k], ts[k], x).prev_sample             # pipelines.py:1612
        after = s.step_final(vel[k], ts[k], x)               # the decode after step (pipelines.py:1621) reads sigma_{k+1}
        assert np.array_equal(before.numpy(), G["f8_final_before"][k])
        assert np.array_equal(x.numpy(), G["f8_prev"][k])
        assert np.array_equal(after.numpy(), G["f8_final_after"][k])
        assert x.dtype == torch.float16
    with pytest.raises(ValueError):
        s.step(vel[0], 3, x)


def test_f9_task_list_and_path_contract(tmp_path, monkeypatch):
    from foho.guidance.run import _load_task_list, derive_paths
    d = tmp_path / "imgs"
    d.mkdir()
    for n in ["12_cropped_hoi_1.png", "3_cropped_hoi_0.png", "7_cropped_hoi_1.png"]:
        (d / n).write_bytes(b"")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    assert _load_task_list(None, str(d)) == sorted(os.listdir(d))
    tl = tmp_path / "tasks.json"
    tl.write_text(json.dumps([["a_1.png"], ["b_1.png", "c_0.png"]]))
    monkeypatch.setenv("SLURM_ARRAY_TASK_ID", "1")
    assert _load_task_list(str(tl), str(d)) == ["b_1.png", "c_0.png"]
    monkeypatch.delenv("SLURM_ARRAY_TASK_ID")
    assert _load_task_list(str(tl), str(d)) == ["a_1.png"]
    p = derive_paths("12_cropped_hoi_1.png", "I", "M", "G", "H", "A", "T", "L", "O")
    assert p["index"] == "12" and p["is_right"] == "1"
    assert p["cropped_hand_mask_path"] == "M/12_cropped_hand_mask.png"
    assert p["moge_mesh_path"] == "G/12_cropped_hoi/mesh.glb" and p["moge_fov_path"] == "G/12_cropped_hoi/fov.json"
    assert p["T_h2m_path"] == "T/12_hoi_mesh.npy" and p["aligned_mano_mesh_path"] == "L/12_hamer_aligned_mano.ply"
    assert p["hunyuan_hoi_mesh_path"] == "H/12_hoi_mesh.ply" and p["hamer_for_guid_path"] == "A/12_kps_for_guidance.npy"
    assert p["save_path_obj"] == "O/12_obj.ply" and p["save_path_hand"] == "O/12_hand.ply"


def test_f11_latent2sdf_matches_the_reference():
    """pipeline.latent2sdf against the reference's latent2sdf (PL:292-313) run on an arithmetic stand-in VAE: latent
    rescaling, fp16 queries, 8000-point chunks, (1,G,G,G) layout, negation."""
    from followmyhold_amd import pipeline as PLN

    class FakeVAE:
        scale_factor = 0.7

        def __init__(self, w):
            self.w = w

        def __call__(self, x):
            return x * 2 + 1

        def geo_decoder(self, queries, latents):
            assert queries.dtype == torch.float16 and queries.shape[1] <= 8000
            return (queries.float() @ self.w + latents.float().mean())[..., :1].to(latents.dtype)

    w = torch.from_numpy(G["f11_w"])
    lat = torch.from_numpy(G["f11_latent"])
    xyz, gs, _ = PLN.generate_dense_grid_points(np.array([-1.1] * 3), np.array([1.1] * 3), 5, "ij", 24)
    got = PLN.latent2sdf(lat, torch.as_tensor(xyz), gs, FakeVAE(w), "cpu")
    assert got.dtype == torch.float32 and tuple(got.shape) == G["f11_sdf"].shape == (1, 25, 25, 25)
    assert np.array_equal(got.numpy(), G["f11_sdf"])


def test_f12_encode_cond_matches_the_reference():
    """GuidedShapePipeline.encode_cond against Hunyuan3DDiTPipeline.encode_cond (PL:599-639): batch order and dtype of the
    classifier-free-guidance conditioning, nested dictionaries included."""
    from followmyhold_amd import pipeline as PLN

    class FakeCond:
        def __call__(self, image=None, mask=None):
            return {"main": image.mean(dim=(2, 3)).unsqueeze(1).float(), "additional": {"x": mask.float().sum(dim=(1, 2, 3)).reshape(-1, 1)}}

        def unconditional_embedding(self, bsz):
            return {"main": torch.zeros(bsz, 1, 3), "additional": {"x": -torch.ones(bsz, 1)}}

    pipe = object.__new__(PLN.GuidedShapePipeline)
    pipe.conditioner, pipe.dtype = FakeCond(), torch.float16
    img, msk = torch.from_numpy(G["f12_image"]), torch.from_numpy(G["f12_mask"])
    plain, cfg, dual = pipe.encode_cond(img, msk, False, False), pipe.encode_cond(img, msk, True, False), pipe.encode_cond(img, msk, True, True)
    assert np.array_equal(plain["main"].numpy(), G["f12_plain_main"])
    assert np.array_equal(cfg["main"].numpy(), G["f12_cfg_main"]) and np.array_equal(cfg["additional"]["x"].numpy(), G["f12_cfg_add"])
    assert np.array_equal(dual["main"].numpy(), G["f12_dual_main"]) and np.array_equal(dual["additional"]["x"].numpy(), G["f12_dual_add"])
    assert {k: str(v) for k, v in dict(plain=plain["main"].dtype, cfg=cfg["main"].dtype, dual=dual["additional"]["x"].dtype).items()} == META["f12_dtypes"]


def test_f13_alignment_drivers_pair_files_like_the_reference(tmp_path, monkeypatch):
    """foho.alignment.h2m.run / mano.run (h2m.py:12-55, mano.py:12-44): same source / target / output pairing -- incl. the
    mesh.ply > pointcloud.ply > mesh.glb preference and the skip of images without MoGe geometry -- and the same
    align_meshes_impl arguments as the reference produced on this directory tree."""
    from foho.alignment import h2m, mano
    f13 = META["f13"]
    root = str(tmp_path)
    for rel in f13["tree"]:
        os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
        open(os.path.join(root, rel), "w").close()
    calls = []
    rel_ = lambda v: os.path.relpath(v, root) if isinstance(v, str) else v
    for mod in (h2m, mano):
        monkeypatch.setattr(mod, "align_meshes_impl", lambda **kw: calls.append({k: rel_(v) for k, v in kw.items()}))
    h2m.run(os.path.join(root, "hy"), os.path.join(root, "moge"), os.path.join(root, "rt"))
    assert sorted(calls, key=lambda c: c["source_mesh_path"]) == f13["h2m"]
    calls.clear()
    mano.run(os.path.join(root, "hamer"), os.path.join(root, "hy"), os.path.join(root, "aligned"))
    assert sorted(calls, key=lambda c: c["source_mesh_path"]) == f13["mano"]


def test_f14_mesh_align_command_line_matches_the_reference(monkeypatch):
    """foho.alignment.mesh_align.main (ICP:219-262): the same option names, short forms, types and defaults reach
    align_meshes_impl as through the reference's click command."""
    from foho.alignment import mesh_align as MA
    got = []
    monkeypatch.setattr(MA, "align_meshes_impl", lambda *a: got.append(list(a)))
    for argv in META["f14"]["argv"]:
        MA.main(list(argv))
    assert got == META["f14"]["args"]


def test_f15_guidance_driver_matches_the_reference(tmp_path, monkeypatch):
    """foho.guidance.run.run (RUN:188-261) on the directory tree the reference's own run() was executed on: the same images
    reach run_hunyuan_w_guid with the same keyword arguments (file names, fov), the same ones are skipped (outputs
    exist, empty mask, missing fov.json -> per-image exception), a (None, None) result moves on, and the task list is
    chunked by SLURM_ARRAY_TASK_ID."""
    from PIL import Image
    from foho.guidance import run as G
    f15 = META["f15"]
    root = str(tmp_path)
    d = {k: os.path.join(root, k) for k in ["cropped_obj_img_dir", "mask_dir", "moge_out_dir", "hunyuan_hoi_mesh_dir",
                                            "hamer_out_dir", "h2m_rt_dir", "aligned_mano_dir", "guidance_out_dir"]}
    for v in d.values():
        os.makedirs(v)
    for name in f15["images"]:
        idx = name.split("_")[0]
        Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(os.path.join(d["cropped_obj_img_dir"], name))
        os.makedirs(os.path.join(d["moge_out_dir"], f"{idx}_cropped_hoi"))
        if idx != "21":
            with open(os.path.join(d["moge_out_dir"], f"{idx}_cropped_hoi", "fov.json"), "w") as f:
                json.dump({"fov_x": 40.0 + int(idx)}, f)
        hand = np.full((4, 4), 255, np.uint8) if idx != "7" else np.zeros((4, 4), np.uint8)
        Image.fromarray(hand).save(os.path.join(d["mask_dir"], f"{idx}_cropped_hand_mask.png"))
        Image.fromarray(np.full((4, 4), 255, np.uint8)).save(os.path.join(d["mask_dir"], f"{idx}_cropped_obj_mask.png"))
    for tag in ("obj", "hand"):
        open(os.path.join(d["guidance_out_dir"], f"3_{tag}.ply"), "w").close()
    seen = []
    rel_ = lambda v: os.path.relpath(v, root) if isinstance(v, str) else v

    def fake_guid(**kw):
        seen.append({k: rel_(v) for k, v in kw.items() if k != "config"})
        return (None, None) if "9_" in kw["cropped_obj_img_path"] else (1, 1)

    monkeypatch.setattr(G, "run_hunyuan_w_guid", fake_guid)
    for k in ("SLURM_ARRAY_TASK_ID", "WORLD_SIZE", "RANK"):
        monkeypatch.delenv(k, raising=False)
    G.run(project_root=root, task_list_file=None, **d)
    assert len(seen) == f15["n_calls"] and sorted(seen, key=lambda c: c["cropped_obj_img_path"]) == f15["calls"]
    tl = os.path.join(root, "tasks.json")
    with open(tl, "w") as f:
        json.dump([["12_cropped_hoi_1.png"], ["9_cropped_hoi_1.png", "3_cropped_hoi_0.png"]], f)
    monkeypatch.setenv("SLURM_ARRAY_TASK_ID", "1")
    n0 = len(seen)
    G.run(project_root=root, task_list_file=tl, **d)
    assert [c["cropped_obj_img_path"] for c in seen[n0:]] == f15["task_list_calls"]
    monkeypatch.delenv("SLURM_ARRAY_TASK_ID")
    assert G._load_task_list(None, d["cropped_obj_img_dir"]) == f15["listing_set"]


def test_f16_run_hunyuan_w_guid_matches_the_reference(tmp_path, monkeypatch):
    """foho.guidance.run.run_hunyuan_w_guid against a recording of the reference's (RUN:65-175): camera, blend and raster
    settings of the two renderers, the RGBA image (pure white -> transparent), the pipeline's keyword arguments and seed,
    post-processing + export of both meshes."""
    from PIL import Image
    from foho.guidance import run as Gd
    from followmyhold_amd import facade as p3d, meshio, postprocess
    f16 = META["f16"]
    rec = {}
    for name, kw in f16["log"]:
        rec.setdefault(name, []).append(kw)
    root = str(tmp_path)
    img_path, hm = os.path.join(root, "12_cropped_hoi_1.png"), os.path.join(root, "hand.png")
    Image.fromarray(G["f16_rgb"]).save(img_path)
    Image.fromarray(np.full((6, 5), 255, np.uint8)).save(hm)
    calls, order = [], []

    class FakePipe:
        def __call__(self, **kw):
            calls.append(kw)
            return (p3d.Meshes(verts=[torch.rand(5, 3)], faces=[torch.tensor([[0, 1, 2]])]),
                    p3d.Meshes(verts=[torch.rand(4, 3)], faces=[torch.tensor([[0, 1, 3]])]))

    monkeypatch.setattr(Gd, "_build_pipeline", lambda device: FakePipe())
    for cls in ("FloaterRemover", "DegenerateFaceRemover", "FaceReducer"):
        orig = getattr(postprocess, cls).__call__
        monkeypatch.setattr(getattr(postprocess, cls), "__call__",
                            (lambda o, c: lambda self, mesh, *a, **k: (order.append(c), o(self, mesh, *a, **k))[1])(orig, cls))
    res = Gd.run_hunyuan_w_guid(
        cropped_obj_img_path=img_path, fovx=41.5, hamer_for_guid_path="K", aligned_mano_mesh_path="MANO",
        cropped_obj_mask_path="OM", cropped_hand_mask_path=hm, moge_mesh_path="MOGE", T_h2m_path="T",
        hunyuan_hoi_mesh_path="HY", save_path_obj=os.path.join(root, "o.ply"), save_path_hand=os.path.join(root, "h.ply"),
        config="CFG", device="cpu")
    assert isinstance(res, tuple) and len(res) == 2 and f16["returns_pair"]
    kw = calls[0]
    assert sorted(kw.keys()) == f16["pipeline_kwarg_names"]
    rel_ = lambda v: os.path.relpath(v, root) if isinstance(v, str) and v.startswith(root) else v
    assert {k: rel_(v) for k, v in kw.items() if k not in ("image", "generator", "renderer", "sil_renderer")} == f16["pipeline_kwargs"]
    assert len(kw["image"]) == f16["n_images"] and kw["image"][0].mode == f16["image_mode"]
    assert np.array_equal(np.array(kw["image"][0]), G["f16_image"])
    assert int(kw["generator"].initial_seed()) == f16["generator_seed"]
    # renderers
    cam_ref, blend_ref = rec["FoVPerspectiveCameras"][0], rec["BlendParams"][0]
    rs_ref, rs_sil_ref = rec["RasterizationSettings"]
    for rend, rs_want, shader in ((kw["renderer"], rs_ref, p3d.PhongNormalShader), (kw["sil_renderer"], rs_sil_ref, p3d.SoftSilhouetteShader)):
        cam, rs = rend.rasterizer.cameras, rend.rasterizer.raster_settings
        assert isinstance(rend.shader, shader)
        assert cam.R.tolist() == cam_ref["R"] and cam.T.tolist() == cam_ref["T"]
        assert (cam.fov, cam.znear, cam.zfar) == (cam_ref["fov"], cam_ref["znear"], cam_ref["zfar"])
        assert list(rs.image_size) == rs_want["image_size"] and rs.faces_per_pixel == rs_want["faces_per_pixel"]
        assert rs.bin_size == rs_want["bin_size"] and rs.max_faces_per_bin == rs_want["max_faces_per_bin"]
        assert np.float32(rs.blur_radius) == np.float32(rs_want["blur_radius"])
        bp = rend.shader.blend_params
        assert np.float32(bp.sigma) == np.float32(blend_ref["sigma"]) and np.float32(bp.gamma) == np.float32(blend_ref["gamma"])
    # post-processing order and outputs
    assert order == [n for n, _ in f16["log"] if n in ("FloaterRemover", "DegenerateFaceRemover", "FaceReducer")]
    ov, of = meshio.load_ply(os.path.join(root, rec["export"][0]["path"]))
    hv, hf = meshio.load_ply(os.path.join(root, rec["IO.save_mesh"][0]["path"]))
    assert len(hv) == 4 and len(hf) == 1 and len(of) == 1
