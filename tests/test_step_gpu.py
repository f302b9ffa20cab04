"""GPU parity of the HIP guidance step (through the C ABI) against the CPU oracle on the same seeded inputs.

Bar (BASELINE.json north_star): face indices bit-exact; vertex positions, losses and gradients within
1e-4 relative in fp32.
"""
import numpy as np
import pytest
import torch

from helpers import make_scene
from oracle import ref_ops as R
from oracle import step_ref as S

gpu = pytest.mark.gpu
RTOL = 1e-4


def _np_scene(sc):
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in sc.items()}


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def small():
    """64x64 image, MANO-sized hand + icosphere(2) object, grid 16^3; oracle forward/backward of phase C."""
    sc = make_scene("ico2", 64, 64, seed=0)
    p = S.make_params(
        scale_hand=torch.tensor([1.02]), trans_hand=torch.tensor([0.004, -0.003, 0.002]),
        rot_hand=torch.tensor([0.999, 0.02, -0.01, 0.03]), scale_obj=torch.tensor([0.97]),
        trans_obj=torch.tensor([-0.002, 0.003, 0.001]), rot_obj=torch.tensor([0.998, -0.03, 0.02, 0.01]))
    st = S.JointStepper(sc, p, denoise_i=19, grid_res=16)
    total, terms, aux, grads = st.step(update=True)
    after = {k: v.detach().clone() for k, v in st.p.items()}
    return dict(scene=sc, params=p, total=total, terms=terms, aux=aux, grads=grads, after=after)


def _engine(sc, p, grid_res=16):
    from followmyhold_amd import engine as E
    gb = E.GuidanceBatch([_np_scene(sc)], grid_res=grid_res)
    gb.set_params(0, **{k: v.numpy() for k, v in p.items()})
    return E, gb


@gpu
def test_vertex_stage_bit_exact(small):
    """Similarity transform + projection: identical op order as the oracle -> identical bits."""
    E, gb = _engine(small["scene"], small["params"])
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=False)
    gb.step(cfg, stages=E.L.STAGE_VERTEX)
    torch.cuda.synchronize()
    aux = small["aux"]
    world_ref = torch.cat([aux["hand"]["verts"], aux["obj_verts_t"]], 0).detach().numpy()
    world = gb.region("world", torch.float32, (-1, 3)).cpu().numpy()
    assert rel_err(world, world_ref) < 1e-6
    cam = R.Camera(small["scene"]["fov"], 64, 64)
    ndc_ref = R.world_to_ndc(torch.from_numpy(world_ref), cam).numpy()
    ndc = gb.region("ndc", torch.float32, (-1, 3)).cpu().numpy()
    assert np.array_equal(world, world_ref), f"world differs, max abs {np.abs(world - world_ref).max()}"
    assert np.array_equal(ndc, ndc_ref), f"ndc differs, max abs {np.abs(ndc - ndc_ref).max()}"
    vn_ref = torch.cat([R.vertex_normals(aux["hand"]["verts"].detach(), small["scene"]["hand_faces"]),
                        R.vertex_normals(aux["obj_verts_t"].detach(), small["scene"]["obj_faces"])], 0).numpy()
    vn = gb.region("vn", torch.float32, (-1, 3)).cpu().numpy()
    assert np.abs(vn - vn_ref).max() < 1e-6
    idx = gb.region("knn_idx", torch.int32)[:778].cpu().numpy()
    assert np.array_equal(idx, aux["knn_idx"].numpy())


@gpu
def test_raster_face_indices_bit_exact(small):
    E, gb = _engine(small["scene"], small["params"])
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=False)
    gb.step(cfg, stages=E.L.STAGE_VERTEX | E.L.STAGE_RASTER)
    torch.cuda.synchronize()
    gb.raise_on_flags()
    P = 64 * 64
    p2f = gb.region("p2f", torch.int32, (2, P)).cpu().numpy()
    zb = gb.region("zbuf", torch.float32, (2, P)).cpu().numpy()
    sd = gb.region("sdist", torch.float32, (2, P)).cpu().numpy()
    prod = gb.region("prod", torch.float32, (2, P)).cpu().numpy()
    aux = small["aux"]
    for r, ren in enumerate([aux["hand"]["render"], aux["render"]]):
        sel = ren["sel"]
        ref = sel["pix_to_face"].reshape(-1)
        assert (p2f[r] >= 0).sum() > 20
        mism = int((p2f[r] != ref).sum())
        assert mism == 0, f"render {r}: {mism} face-index mismatches"
        hit = ref >= 0                                       # z / dist / product planes are defined for hit pixels only
        assert np.array_equal(zb[r][hit], sel["zbuf"].reshape(-1)[hit])
        assert np.array_equal(sd[r][hit], sel["dists"].reshape(-1)[hit])
    sil_ref = aux["render"]["sil"].detach().numpy().reshape(-1)
    hit = aux["render"]["sel"]["pix_to_face"].reshape(-1) >= 0
    assert np.abs((1.0 - prod[1][hit]) - sil_ref[hit]).max() < 1e-6 and np.abs(sil_ref[~hit]).max() == 0.0


@gpu
def test_losses_and_gradients(small):
    E, gb = _engine(small["scene"], small["params"])
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=True)
    gb.step(cfg)
    torch.cuda.synchronize()
    gb.raise_on_flags()
    l = gb.loss_dict(0)
    t = {k: float(v) for k, v in small["terms"].items()}
    assert int(l["n_intersect"]) == small["aux"]["n_int"]
    pairs = [("contact", "contact"), ("kps", "kps"), ("trans_hand", "trans_hand"), ("trans_obj", "trans_obj"),
             ("verts_obj", "verts_obj"), ("edge", "edge"), ("normal0", "normal_hand"), ("disp0", "disp_hand"),
             ("normal1", "normal_hoi"), ("disp1", "disp_hoi"), ("sil1", "sil_hoi")]
    for a, b in pairs:
        assert abs(l[a] - t[b]) <= RTOL * max(abs(t[b]), 1e-6), (a, l[a], t[b])
    assert abs(l["total"] - float(small["total"])) <= RTOL * abs(float(small["total"]))
    g = gb.grad_params[0].cpu().numpy()
    gref = np.concatenate([small["grads"][k].numpy().reshape(-1) for k in E.PARAM_NAMES])
    for k, sl in E.PARAM_SLICES.items():
        assert rel_err(g[sl], gref[sl]) < 5 * RTOL, (k, g[sl], gref[sl])
    gv = gb.grad_obj_verts(0).cpu().numpy()
    assert rel_err(gv, small["grads"]["obj_verts"].numpy()) < 5 * RTOL
    # AdamW update (PL:1478, 1601)
    p_after = gb.get_params(0)
    for k in E.PARAM_NAMES:
        ref = small["after"][k].numpy()
        assert np.abs(p_after[k].numpy() - ref).max() <= 2e-6 + RTOL * np.abs(ref).max() * 1e-2, (k, p_after[k], ref)


def _perturbed():
    return S.make_params(
        scale_hand=torch.tensor([1.02]), trans_hand=torch.tensor([0.004, -0.003, 0.002]),
        rot_hand=torch.tensor([0.999, 0.02, -0.01, 0.03]), scale_obj=torch.tensor([0.97]),
        trans_obj=torch.tensor([-0.002, 0.003, 0.001]), rot_obj=torch.tensor([0.998, -0.03, 0.02, 0.01]))


@gpu
@pytest.mark.parametrize("phase", ["A", "B"])
def test_phase_a_and_b(phase):
    """Hand-only (Adam) and object-only (AdamW) phases run on the same kernels with other recipes."""
    from followmyhold_amd import engine as E
    sc = make_scene("ico2", 64, 64, seed=1)
    p = _perturbed()
    st = S.PhaseStepper(phase, sc, p)
    total, terms, aux, grads = st.step(update=True)
    gb = E.GuidanceBatch([_np_scene(sc)], grid_res=16, n_renders=1)
    gb.set_params(0, **{k: v.numpy() for k, v in p.items()})
    cfg, nr = E.phase_cfg(phase, do_update=True)
    assert nr == 1
    gb.step(cfg)
    torch.cuda.synchronize()
    gb.raise_on_flags()
    l = gb.loss_dict(0)
    assert abs(l["total"] - float(total)) <= RTOL * abs(float(total)), (l, {k: float(v) for k, v in terms.items()})
    sel = aux["render"]["sel"]
    p2f = gb.region("p2f", torch.int32, (1, 64 * 64)).cpu().numpy()
    assert np.array_equal(p2f[0], sel["pix_to_face"].reshape(-1))
    g = gb.grad_params[0].cpu().numpy()
    for k, gr in grads.items():
        if k == "obj_verts":
            assert rel_err(gb.grad_obj_verts(0).cpu().numpy(), gr.numpy()) < 5 * RTOL
        else:
            assert rel_err(g[E.PARAM_SLICES[k]], gr.numpy()) < 5 * RTOL, (k, g[E.PARAM_SLICES[k]], gr)
    after = gb.get_params(0)
    for k in E.PARAM_NAMES:
        ref = st.p[k].detach().numpy()
        assert np.abs(after[k].numpy() - ref).max() <= 2e-6 + 1e-6 * np.abs(ref).max(), (k, after[k], ref)


@gpu
def test_ragged_batch_matches_single_image_runs():
    """B=2 with different object sizes: every image of a batch gets the result of its own single-image run."""
    from followmyhold_amd import engine as E
    scs = [_np_scene(make_scene("ico2", 64, 64, seed=3)), _np_scene(make_scene("ico4", 64, 64, seed=4))]
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=True)
    singles = []
    for s in scs:
        gb = E.GuidanceBatch([s], grid_res=16)
        for _ in range(2):      # two iterations: the second one runs on updated parameters (longer runs let atomic-sum noise reach
                                # the discontinuities of the silhouette BCE, see test_fullsize_gpu._clamp_flips)
            gb.step(cfg)
        torch.cuda.synchronize()
        singles.append((gb.losses[0].cpu().numpy(), gb.params[0].cpu().numpy(), gb.region("p2f", torch.int32).cpu().numpy()))
    gb = E.GuidanceBatch(scs, grid_res=16)
    for _ in range(2):      # two iterations: the second one runs on updated parameters (longer runs let atomic-sum noise reach
                                # the discontinuities of the silhouette BCE, see test_fullsize_gpu._clamp_flips)
        gb.step(cfg)
    torch.cuda.synchronize()
    gb.raise_on_flags()
    p2f = gb.region("p2f", torch.int32, (2, 2, 64 * 64)).cpu().numpy()
    for b in range(2):
        assert np.allclose(gb.losses[b].cpu().numpy(), singles[b][0], rtol=1e-5, atol=1e-7)
        assert np.allclose(gb.params[b].cpu().numpy(), singles[b][1], rtol=1e-5, atol=1e-7)
        assert np.array_equal(p2f[:, b].reshape(-1), singles[b][2])


@gpu
def test_short_trajectory_tracks_the_oracle():
    """5 consecutive AdamW steps (no teacher forcing): losses stay within 1e-3 of the oracle's trajectory."""
    from followmyhold_amd import engine as E
    sc = make_scene("ico2", 64, 64, seed=0)
    st = S.JointStepper(sc, S.make_params(), denoise_i=19, grid_res=16)
    gb = E.GuidanceBatch([_np_scene(sc)], grid_res=16)
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=True)
    for k in range(5):
        total, _, _, _ = st.step(update=True)
        gb.step(cfg)
        torch.cuda.synchronize()
        assert abs(gb.loss_dict(0)["total"] - float(total)) <= 1e-3 * abs(float(total)), k


@gpu
def test_standalone_raster_and_knn_ops():
    """foho_raster_fwd / foho_raster_bwd / foho_knn1_fwd against the C oracle and torch autograd."""
    import ctypes
    from followmyhold_amd import _lib as L
    from oracle import clib
    lib = L.lib()
    H, W = 48, 64                                     # non-square
    v, f = __import__("followmyhold_amd.synthetic", fromlist=["x"]).icosphere(2, 0.4)
    vt = torch.from_numpy(v) + torch.tensor([0.05, -0.02, -2.0])
    cam = R.Camera(50.0, H, W)
    ndc = R.world_to_ndc(vt, cam).contiguous()
    blur = R.blur_radius_from_sigma()
    ref = clib.render_pass(ndc[torch.from_numpy(f)].numpy(), H, W, blur)
    dv = ndc.cuda()
    df = torch.from_numpy(f).int().cuda()
    nws = lib.foho_raster_workspace_bytes(len(v), len(f), H, W)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda")
    p2f = torch.empty(H * W, dtype=torch.int64, device="cuda")
    zb, di, pr = (torch.empty(H * W, device="cuda") for _ in range(3))
    ba = torch.empty(H * W, 3, device="cuda")
    ov = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = ctypes.c_void_p
    L.check(lib.foho_raster_fwd(P(dv.data_ptr()), P(df.data_ptr()), len(v), len(f), H, W, ctypes.c_float(blur),
                                ctypes.c_float(1e-8), P(p2f.data_ptr()), P(zb.data_ptr()), P(ba.data_ptr()),
                                P(di.data_ptr()), P(pr.data_ptr()), P(ov.data_ptr()), P(ws.data_ptr()),
                                ctypes.c_size_t(nws), stream), "foho_raster_fwd")
    torch.cuda.synchronize()
    assert np.array_equal(p2f.cpu().numpy(), ref["pix_to_face"].reshape(-1))
    assert np.array_equal(zb.cpu().numpy(), ref["zbuf"].reshape(-1))
    assert np.array_equal(ba.cpu().numpy(), ref["bary"].reshape(-1, 3))
    assert np.array_equal(di.cpu().numpy(), ref["dists"].reshape(-1))
    # backward vs autograd of the oracle's differentiable re-evaluation
    gz, gd = torch.randn(H * W), torch.randn(H * W) * 1e3
    gb_ = torch.randn(H * W, 3)
    n2 = ndc.clone().requires_grad_(True)
    hit = (torch.from_numpy(ref["pix_to_face"]).reshape(-1) >= 0).nonzero(as_tuple=True)[0]
    pz, bary, sd, _ = R.eval_fragments(n2, torch.from_numpy(f), hit, torch.from_numpy(ref["pix_to_face"]).reshape(-1)[hit], H, W)
    ((pz * gz[hit]).sum() + (bary * gb_[hit]).sum() + (sd * gd[hit]).sum()).backward()
    gout = torch.zeros(len(v), 3, device="cuda")
    dgz, dgb, dgd = gz.cuda(), gb_.cuda(), gd.cuda()          # keep the device copies alive across the call
    L.check(lib.foho_raster_bwd(P(dv.data_ptr()), P(df.data_ptr()), len(v), len(f), H, W, P(p2f.data_ptr()),
                                P(dgz.data_ptr()), P(dgb.data_ptr()), P(dgd.data_ptr()),
                                P(gout.data_ptr()), ctypes.c_float(blur), stream), "foho_raster_bwd")
    torch.cuda.synchronize()
    assert rel_err(gout.cpu().numpy(), n2.grad.numpy()) < 2e-4
    # knn
    a, b = torch.randn(300, 3), torch.randn(1000, 3)
    d2 = torch.empty(300, device="cuda")
    idx = torch.empty(300, dtype=torch.int64, device="cuda")
    da, db = a.cuda(), b.cuda()
    L.check(lib.foho_knn1_fwd(P(da.data_ptr()), 300, P(db.data_ptr()), 1000, P(d2.data_ptr()),
                              P(idx.data_ptr()), stream), "foho_knn1_fwd")
    torch.cuda.synchronize()
    rd2, ridx = clib.knn1(a.numpy(), b.numpy())
    assert np.array_equal(idx.cpu().numpy(), ridx) and np.allclose(d2.cpu().numpy(), rd2, rtol=1e-6)


@gpu
def test_two_hand_scene_config4_shape_regime():
    """BASELINE config 4 shape regime (two hands = 1556 hand vertices, keypoints regress from the first 778)."""
    from followmyhold_amd import engine as E
    sc = make_scene("ico2", 64, 64, seed=6, two_hands=True)
    assert sc["hand_verts"].shape[0] == 1556
    p = _perturbed()
    st = S.JointStepper(sc, p, denoise_i=19, grid_res=16)
    total, terms, aux, grads = st.step(update=False)
    gb = E.GuidanceBatch([_np_scene(sc)], grid_res=16)
    gb.set_params(0, **{k: v.numpy() for k, v in p.items()})
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=False)
    gb.step(cfg)
    torch.cuda.synchronize()
    gb.raise_on_flags()
    p2f = gb.region("p2f", torch.int32, (2, 64 * 64)).cpu().numpy()
    assert np.array_equal(p2f[1], aux["render"]["sel"]["pix_to_face"].reshape(-1))
    assert abs(gb.loss_dict(0)["total"] - float(total)) <= RTOL * abs(float(total))
    g = gb.grad_params[0].cpu().numpy()
    gref = np.concatenate([grads[k].numpy().reshape(-1) for k in E.PARAM_NAMES])
    assert rel_err(g, gref) < 5 * RTOL


@gpu
def test_graph_replay_equals_eager_launches():
    """A captured hipGraph of the step must behave like eager launches (regression: a hipMemsetAsync node inside the
    captured graph was not ordered with the kernel nodes, so accumulators were cleared mid-step after a few replays;
    they are now cleared by a kernel).  Trajectories are compared over 3 steps only: beyond that Adam amplifies
    float-atomic rounding noise in degenerate directions (e.g. the quaternion's radial component, whose exact
    gradient is zero) into full learning-rate steps, in the reference as well."""
    from followmyhold_amd import engine as E
    sc = _np_scene(make_scene("ico4", 128, 128, seed=7))
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=True)
    ga, gb_ = E.GuidanceBatch([sc], grid_res=32), E.GuidanceBatch([sc], grid_res=32)
    for _ in range(3):
        ga.step(cfg)
    graph = gb_.capture(cfg)
    ident = dict(scale_hand=[1.0], trans_hand=[0, 0, 0], rot_hand=[1, 0, 0, 0], scale_obj=[1.0], trans_obj=[0, 0, 0],
                 rot_obj=[1, 0, 0, 0])
    gb_.set_params(0, **ident)
    gb_.reset_optimizer()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert np.allclose(ga.params.cpu().numpy(), gb_.params.cpu().numpy(), rtol=0, atol=2e-4)
    assert abs(ga.loss_dict(0)["total"] - gb_.loss_dict(0)["total"]) <= 1e-3 * abs(ga.loss_dict(0)["total"])
    # many replays: counters stay sane (the broken memset node showed up as garbage counters / overflow flags)
    for _ in range(40):
        graph.replay()
    torch.cuda.synchronize()
    gb_.raise_on_flags()
    fc = gb_.region("frac_count", torch.int32).cpu().numpy()          # overflow list of the fragment segments: unused here
    sg = gb_.region("seg_count", torch.int32).reshape(2, -1).cpu().numpy()
    assert (fc == 0).all() and sg[0].sum() == 0 and 0 < sg[1].sum() < 20000 and sg.max() <= 256   # only the hand+object render carries the silhouette
    assert int(gb_.adam_t[0]) == 43 and np.isfinite(gb_.loss_dict(0)["total"])


@gpu
def test_multi_iteration_graph_and_stream_groups_equal_plain_stepping():
    """A slice of the inner loop captured as ONE hipGraph, and images split over several streams (GuidanceGroup), give
    what plain eager stepping of one batch gives (2 iterations: beyond that Adam amplifies the atomic-sum noise)."""
    from followmyhold_amd import engine as E
    scenes = [_np_scene(make_scene("ico2", 64, 64, seed=s)) for s in (11, 12, 13)]
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=True)
    ref = E.GuidanceBatch(scenes, grid_res=16)
    for _ in range(2):
        ref.step(cfg)
    torch.cuda.synchronize()
    ref_p, ref_l = ref.params.cpu().numpy(), ref.losses[:, 0].cpu().numpy()
    # (a) two iterations in one graph
    ga = E.GuidanceBatch(scenes, grid_res=16)
    g2 = ga.capture(cfg, steps_per_graph=2)
    assert int(ga.adam_t[0]) == 0                        # capture leaves the optimiser state untouched
    g2.replay()
    torch.cuda.synchronize()
    assert int(ga.adam_t[0]) == 2
    assert np.allclose(ga.params.cpu().numpy(), ref_p, atol=2e-4)
    assert np.allclose(ga.losses[:, 0].cpu().numpy(), ref_l, rtol=1e-3)
    # (b) three images on two streams (batches of 2 + 1), separate graphs and the joint graph
    for joint in (False, True):
        grp = E.GuidanceGroup(scenes, n_streams=2, grid_res=16)
        assert [b.B for b in grp.batches] == [2, 1] and grp.B == 3
        grp.capture(cfg, joint=joint, steps_per_graph=1 if joint else 2)
        grp.run(cfg, 2)
        grp.synchronize()
        torch.cuda.synchronize()
        p = np.concatenate([b.params.cpu().numpy() for b in grp.batches])
        l = np.concatenate([b.losses[:, 0].cpu().numpy() for b in grp.batches])
        assert np.allclose(p, ref_p, atol=2e-4), joint
        assert np.allclose(l, ref_l, rtol=1e-3), joint
        for b in grp.batches:
            b.raise_on_flags()


@gpu
@pytest.mark.parametrize("seed,size,obj", [(11, (48, 80), "ico2"), (12, (96, 96), "ico3"), (13, (80, 48), "ico2"), (14, (128, 128), "ico3"),
                                           (15, (72, 72), "ico1"), (16, (64, 64), "ico3")])
def test_fused_step_face_indices_over_random_scenes(seed, size, obj):
    """The scatter rasteriser inside the fused step (all three renders of phase C) over other scenes, image shapes, object
    tessellations and random similarity parameters: face ids, depths and signed distances of both K=1 renders equal the
    oracle's bit for bit, the loss to 1e-5, all gradients to the 1e-4 class."""
    from followmyhold_amd import engine as E
    H, W = size
    sc = make_scene(obj, H, W, seed=seed)
    rng = np.random.default_rng(seed)
    q = lambda: torch.tensor(np.concatenate([[1.0], rng.normal(size=3) * 0.05]), dtype=torch.float32)
    p = S.make_params(scale_hand=torch.tensor([1.0 + 0.05 * rng.normal()], dtype=torch.float32),
                      trans_hand=torch.tensor(rng.normal(size=3) * 0.004, dtype=torch.float32), rot_hand=q(),
                      scale_obj=torch.tensor([1.0 + 0.05 * rng.normal()], dtype=torch.float32),
                      trans_obj=torch.tensor(rng.normal(size=3) * 0.004, dtype=torch.float32), rot_obj=q())
    st = S.JointStepper(sc, p, denoise_i=19, grid_res=16)
    total, terms, aux, grads = st.step(update=False)
    gb = E.GuidanceBatch([_np_scene(sc)], grid_res=16)
    gb.set_params(0, **{k: v.numpy() for k, v in p.items()})
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=False)
    gb.step(cfg)
    torch.cuda.synchronize()
    gb.raise_on_flags()
    P = H * W
    p2f = gb.region("p2f", torch.int32, (2, P)).cpu().numpy()
    zb = gb.region("zbuf", torch.float32, (2, P)).cpu().numpy()
    sd = gb.region("sdist", torch.float32, (2, P)).cpu().numpy()
    for r, ren in enumerate([aux["hand"]["render"], aux["render"]]):
        ref = ren["sel"]["pix_to_face"].reshape(-1)
        hit = ref >= 0
        assert hit.sum() > 20 and np.array_equal(p2f[r], ref)
        assert np.array_equal(zb[r][hit], ren["sel"]["zbuf"].reshape(-1)[hit]) and np.array_equal(sd[r][hit], ren["sel"]["dists"].reshape(-1)[hit])
    l = gb.loss_dict(0)
    assert int(l["n_intersect"]) == aux["n_int"]
    assert abs(l["total"] - float(total)) <= 1e-5 * abs(float(total))
    # gradients of the 16 similarity parameters and of the object vertices (1e-4 relative, north-star tolerance x 5 on
    # the small parameter blocks whose gradient is a sum of cancelling terms)
    g = gb.grad_params[0].cpu().numpy()
    gref = np.concatenate([grads[k].numpy().reshape(-1) for k in E.PARAM_NAMES])
    assert rel_err(g, gref) < RTOL
    for k, sl in E.PARAM_SLICES.items():
        assert rel_err(g[sl], gref[sl]) < 5 * RTOL, (k, g[sl], gref[sl])
    assert rel_err(gb.grad_obj_verts(0).cpu().numpy(), grads["obj_verts"].numpy()) < 5 * RTOL


@gpu
@pytest.mark.parametrize("n", [3, 4])
def test_deferred_update_graph_replays_equal_plain_stepping(n, monkeypatch):
    """A captured slice of n > 1 iterations leaves each iteration's final stage (loss assembly, parameter gradients, Adam)
    to the prologue of the next k_xform and closes with foho_step_finalize; the partial sums are double buffered by
    iteration parity.  Odd and even n, two replays in a row (the second starts from what the first left in both
    buffers): step count, parameters, moments and losses follow plain eager stepping, and the same graph captured with
    the deferred update switched off."""
    from followmyhold_amd import engine as E
    scenes = [_np_scene(make_scene("ico2", 64, 64, seed=s)) for s in (21, 22)]
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=True)
    for q in range(16):
        cfg.lr[q] *= 0.05          # short Adam steps: atomic-sum noise cannot grow into visible differences over 2 n iterations
    # ... and no silhouette term: its BCE is discontinuous where 1 - alpha rounds to 0 (a jump of 84 in one pixel's loss and of
    # 6e4 x in its gradient, tests/test_fullsize_gpu.py::_clamp_flips), so 1e-7 of atomic-sum noise in the parameters can move a
    # whole trajectory -- this test is about the plumbing of the deferred update, not about that term
    cfg.render[1].w_sil = 0.0
    ref = E.GuidanceBatch(scenes, grid_res=16)
    for _ in range(2 * n):
        ref.step(cfg)
    torch.cuda.synchronize()
    outs = {}
    for mode in ("deferred", "plain"):
        if mode == "plain":
            monkeypatch.setenv("FOHO_NO_DEFERRED_UPDATE", "1")
        gb = E.GuidanceBatch(scenes, grid_res=16)
        g = gb.capture(cfg, steps_per_graph=n)
        assert int(gb.adam_t[0]) == 0
        g.replay()
        g.replay()
        torch.cuda.synchronize()
        gb.raise_on_flags()
        assert gb.adam_t.cpu().tolist() == [2 * n, 2 * n]
        outs[mode] = gb
        for a, b_, tol in ((gb.params, ref.params, 2e-4), (gb.adam_m, ref.adam_m, 1e-3), (gb.losses[:, 0], ref.losses[:, 0], None)):
            a, b_ = a.cpu().numpy(), b_.cpu().numpy()
            assert np.allclose(a, b_, atol=tol) if tol else np.allclose(a, b_, rtol=2e-3), (mode, a, b_)
        # gradients of the last iteration, incl. the six arg-min / arg-max vertices the final stage completes
        # (free-running trajectories of 2 n iterations: the atomic-sum noise of the earlier iterations shows up here at the
        # per-cent level -- 2.03 % was seen once in ~20 runs; a plumbing error moves these by O(1))
        assert rel_err(gb.grad_params.cpu().numpy(), ref.grad_params.cpu().numpy()) < 5e-2
        assert rel_err(gb.grad_verts_in.cpu().numpy(), ref.grad_verts_in.cpu().numpy()) < 5e-2
    # nothing is left pending: a plain eager step on the deferred batch continues the same trajectory
    gd = outs["deferred"]
    gd.step(cfg)
    ref.step(cfg)
    torch.cuda.synchronize()
    assert gd.adam_t.cpu().tolist() == [2 * n + 1] * 2 and np.allclose(gd.params.cpu().numpy(), ref.params.cpu().numpy(), atol=3e-4)


@gpu
@pytest.mark.parametrize("layout", ["concatenated", "interleaved", "reversed"])
def test_knn_role_ties_keep_lowest_index(layout):
    """Duplicated object vertices make every nearest neighbour a tie (knn_points keeps the first minimum, PL:1529-1532):
    the duplicates sit in different chunks / waves (concatenated, reversed) or in the same selection group (interleaved).
    Checked for both homes of the key decode: k_knn_decode (vertex stage alone) and the passengers of k_resolve, and for
    any content of the pruning bound."""
    from followmyhold_amd import engine as E
    sc = _np_scene(make_scene("ico3", 64, 64, seed=3))
    ov, of = sc["obj_verts"], sc["obj_faces"]
    N = ov.shape[0]
    if layout == "concatenated":
        src = np.concatenate([np.arange(N), np.arange(N)])
    elif layout == "reversed":
        src = np.concatenate([np.arange(N), np.arange(N)[::-1]])
    else:
        src = np.repeat(np.arange(N), 2)
    first = np.full(N, -1)
    for j in range(2 * N - 1, -1, -1):
        first[src[j]] = j                                  # lowest index holding each base vertex
    second = np.array([np.nonzero(src == i)[0][1] for i in range(N)])
    sc["obj_verts"] = np.ascontiguousarray(ov[src])
    sc["obj_faces"] = np.concatenate([first[of], second[of]], 0).astype(of.dtype)
    gb = E.GuidanceBatch([sc], grid_res=16)
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=False)
    out = {}
    rng = np.random.default_rng(11)
    # The role prunes with the distance to whatever index knn_idx holds from the iteration before (k_vertex.inc): the answer
    # must not depend on it -- cleared (first round), the true answer (second), garbage incl. negative and out-of-range
    # entries, and the LATER copy of the true answer (a bound that ties with the winner from a higher index).
    for name, stages in (("decode kernel", E.L.STAGE_VERTEX), ("k_resolve", None), ("garbage bound", E.L.STAGE_VERTEX),
                         ("later copy as bound", None)):
        kreg = gb.region("knn_idx", torch.int32)
        if name == "garbage bound":
            kreg.copy_(torch.from_numpy(rng.integers(-5, 4 * N, kreg.numel()).astype(np.int32)))
        elif name == "later copy as bound":
            kreg[:gb.meta[0]["Vh"]].copy_(torch.from_numpy(second[src[out["k_resolve"]]].astype(np.int32)))
        gb.step(cfg) if stages is None else gb.step(cfg, stages=stages)
        torch.cuda.synchronize()
        world = gb.region("world", torch.float32, (-1, 3)).cpu().numpy()
        Vh = gb.meta[0]["Vh"]
        h, o = world[:Vh], world[Vh:Vh + 2 * N]
        d = h[:, None, :] - o[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]   # fp32, the kernel's order
        ref = d2.argmin(1)                                  # first minimum
        idx = gb.region("knn_idx", torch.int32)[:Vh].cpu().numpy()
        kd2 = gb.region("knn_d2", torch.float32)[:Vh].cpu().numpy()
        assert np.array_equal(idx, ref), f"{layout} / {name}: {np.count_nonzero(idx != ref)} indices differ"
        assert np.array_equal(kd2, d2[np.arange(Vh), ref])
        assert np.array_equal(idx, first[src[idx]])         # never the later copy
        out[name] = idx
    assert all(np.array_equal(out["decode kernel"], v) for v in out.values())


@gpu
def test_a_batch_refuses_images_with_different_joint_regressors():
    """foho_step_desc.J_regressor is ONE regressor per batch: an image that brings another one is refused when the batch is built
    (it would silently be regressed with the first image's) -- and again when a capacity-mode batch is re-loaded."""
    from followmyhold_amd import _lib as L, engine as E
    from helpers import make_scene
    a = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in make_scene("ico2", 64, 64, seed=0).items()}
    b = dict(a)
    b["J_regressor"] = np.asarray(a["J_regressor"]).copy()
    b["J_regressor"][3, 10] += 0.25
    E.GuidanceBatch([a, dict(a)], grid_res=16)                          # equal regressors: fine
    with pytest.raises(L.FohoError):
        E.GuidanceBatch([a, b], grid_res=16)
    gb = E.GuidanceBatch([a, dict(a)], grid_res=16, obj_capacity=(4096, 8192))
    if gb.fits([a, b]):
        with pytest.raises(L.FohoError):
            gb.load_scenes([a, b])


@gpu
def test_both_entry_points_pack_a_scene_the_same_way():
    """One scene through GuidanceBatch(...) at its exact size, and through load_scenes() into a capacity-mode batch that was built from
    ANOTHER scene: what the two leave on the device is the same, byte for byte -- the image record (once foho_object_update has written
    Vo, Fo and n_edges = 3 Fo / 2 into the capacity batch's; one image, so both start at vertex / face 0), mask, key points, regressor,
    parameters, hand-order table, the vertices up to the object's last one and the hand's faces.  Nothing differs legitimately."""
    from followmyhold_amd import engine as E
    scene, other = (_np_scene(make_scene("ico2", 64, 64, seed=s)) for s in (0, 1))
    Vh, Fh, Vo, Fo = (len(scene[k]) for k in ("hand_verts", "hand_faces", "obj_verts", "obj_faces"))
    exact = E.GuidanceBatch([scene], grid_res=16)
    cap = E.GuidanceBatch([other], grid_res=16, obj_capacity=(Vo + 38, Fo + 80))
    cap.set_params(0, scale_hand=[1.5], rot_obj=[0.0, 1.0, 0.0, 0.0])            # load_scenes returns them to the identity
    assert cap.fits([scene])
    cap.load_scenes([scene])
    cap.raise_on_flags()
    assert int(cap.load_flags.cpu()[0]) == 0
    rec = E.L.FohoImage.from_buffer_copy(bytes(exact.images.cpu().numpy()))
    assert (rec.Vh, rec.Vo, rec.Fh, rec.Fo, rec.n_edges) == (Vh, Vo, Fh, Fo, 3 * Fo // 2) and exact.images.numel() == 144
    for name in ("images", "mask", "kps_2d", "J", "params"):
        a, b = getattr(exact, name).cpu().numpy(), getattr(cap, name).cpu().numpy()
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    order = [gb.region("hand_order", torch.int32, (1, Vh)).cpu().numpy() for gb in (exact, cap)]
    assert np.array_equal(order[0], order[1]) and np.array_equal(order[0][0], E.morton_order(scene["hand_verts"]) - np.arange(Vh))
    assert exact.verts_in[:Vh + Vo].cpu().numpy().tobytes() == cap.verts_in[:Vh + Vo].cpu().numpy().tobytes()
    assert exact.faces.dtype == cap.faces.dtype == torch.int32 and torch.equal(exact.faces[:Fh].cpu(), cap.faces[:Fh].cpu())
    assert np.array_equal(exact.params.cpu().numpy()[0], E.IDENTITY_PARAMS)
