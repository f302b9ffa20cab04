"""Shading and blending of K-fragment planes, fused (ops.blend_k / blend_k_alpha, libfoho_rastk.so) against the facade's torch route
(interpolate_face_attributes + softmax_rgb_blend; the torch.prod of SoftSilhouetteShader), one JSON document.

Scene: followmyhold_amd.synthetic.build_scene at 512 x 512 (778-vertex hand + the 20k object, about 22 k faces) at its start pose, the
blur radius of scripts/raster_k_bench.py, BlendParams' default sigma = gamma = 1e-4, the mesh's vertex normals as (F,3,3) face attributes
weighted by the barycentrics.  For K = 8 and 100 and for each route:
  fwd_ms        the blend alone on planes rasterised beforehand, without autograd
  fwd_bwd_ms    ops.raster_k -> blend -> backward to the NDC vertices under a random grad_out (the rasteriser's forward and backward are
                in both routes' figure; raster_fwd_bwd_ms is that part alone)
  peak_bytes    torch.cuda.max_memory_allocated over one fwd_bwd, and what was allocated before it
and the same for the silhouette alpha.  The two routes run interleaved in one process; each figure is the median of --repeats after one
untimed warm-up, host clock around a call that ends in a device synchronise.  No timing target: the comparison is the torch route in the
same run.

    python scripts/blend_k_bench.py [--out profiles/r10_blend_k_bench.json] [--size 512] [--repeats 5] [--ks 8,100]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_blend_k_bench.json"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ks", default="8,100")
    a = ap.parse_args()
    import numpy as np
    import torch
    from followmyhold_amd import engine as E, facade, ops, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("blend_k_bench.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    H = W = a.size
    sc = synthetic.build_scene(E.hip_render_fn(dev), obj_kind="20k", H=H, W=W, seed=0)
    T = sc["T_h2m"]
    world = torch.from_numpy(np.concatenate([sc["hand_verts"], sc["obj_verts"] @ T[:3, :3].T + T[:3, 3]], 0).astype(np.float32)).to(dev)
    faces = torch.from_numpy(np.concatenate([sc["hand_faces"], sc["obj_faces"] + len(sc["hand_verts"])], 0)).to(dev)
    Rm = torch.tensor([[-1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0]], device=dev).unsqueeze(0)
    cams = facade.FoVPerspectiveCameras(device=dev, R=Rm, T=torch.zeros(1, 3, device=dev), znear=0.01, zfar=100.0, fov=sc["fov"])
    ndc0 = cams.transform_points_ndc(world).contiguous()
    attr = facade.Meshes([world], [faces]).verts_normals_packed()[faces].contiguous()
    blur = float(np.float32(np.log(1.0 / 1e-4 - 1.0) * np.float32(1e-8)))
    bp = facade.BlendParams()
    zn, zf = cams.znear, cams.zfar
    gen = torch.Generator().manual_seed(0)

    def lap(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    def interleaved(fns):
        """{name: median ms}: one untimed warm-up of each, then --repeats rounds that run every route once, in turn"""
        for fn in fns.values():
            fn()
        torch.cuda.synchronize(dev)
        laps = {n: [] for n in fns}
        for _ in range(a.repeats):
            for n, fn in fns.items():
                laps[n].append(lap(fn))
        return {n: statistics.median(v) for n, v in laps.items()}

    def peak(fn):
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        fn()
        torch.cuda.synchronize(dev)
        return {"allocated_before": int(before), "peak_bytes": int(torch.cuda.max_memory_allocated(dev))}

    rec = {"frame": [H, W], "vertices": int(ndc0.shape[0]), "faces": int(faces.shape[0]), "blur_radius": blur, "sigma": bp.sigma, "gamma": bp.gamma,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(dev),
           "timing": "median of repeats after one untimed warm-up, routes interleaved; host clock around one call that ends in a device synchronise",
           "k": {}}
    for K in [int(k) for k in a.ks.split(",")]:
        p2f, z, b, d, _ = [t.detach() for t in ops.raster_k(ndc0, faces, H, W, K, blur)]
        frag = facade.Fragments(p2f[None], z[None], b[None], d[None], None, k_planes=True)
        g_rgb = torch.randn(H, W, 4, generator=gen).to(dev)
        g_a = torch.randn(H, W, generator=gen).to(dev)

        def torch_blend(fr):
            return facade.softmax_rgb_blend(facade.interpolate_face_attributes(fr.pix_to_face, fr.bary_coords, attr), fr, bp, znear=zn, zfar=zf)[0]

        def torch_alpha(fr):
            return 1.0 - torch.prod(1.0 - torch.sigmoid(-fr.dists / bp.sigma) * (fr.pix_to_face >= 0), dim=-1)[0]

        def through(blend, g):
            """raster_k -> blend -> backward to the NDC vertices; blend=None: the rasteriser's part alone, a random gradient into its planes"""
            def run():
                v = ndc0.clone().requires_grad_(True)
                q = ops.raster_k(v, faces, H, W, K, blur)
                out = blend(q) if blend is not None else q[1]
                out.backward(g if blend is not None else g_planes)
                return v.grad
            return run

        g_planes = torch.randn(H, W, K, generator=gen).to(dev)
        as_frag = lambda q: facade.Fragments(q[0][None], q[1][None], q[2][None], q[3][None], None, k_planes=True)
        with torch.no_grad():
            fwd = interleaved({
                "fused": lambda: ops.blend_k_fwd(p2f, z, b, d, attr, bp.sigma, bp.gamma, zn, zf, bp.background_color),
                "torch": lambda: torch_blend(frag),
                "fused_alpha": lambda: ops.blend_k_fwd(p2f, None, None, d, None, bp.sigma, 1.0, 0.0, 1.0, None, alpha_only=True),
                "torch_alpha": lambda: torch_alpha(frag)})
        routes = {
            "fused": through(lambda q: ops.blend_k(q[0], q[1], q[2], q[3], attr, bp.sigma, bp.gamma, zn, zf, bp.background_color), g_rgb),
            "torch": through(lambda q: torch_blend(as_frag(q)), g_rgb),
            "fused_alpha": through(lambda q: ops.blend_k_alpha(q[0], q[3], bp.sigma), g_a),
            "torch_alpha": through(lambda q: torch_alpha(as_frag(q)), g_a),
            "raster": through(None, None)}
        both = interleaved(routes)
        mem = {n: peak(fn) for n, fn in routes.items()}
        gv = {n: fn() for n, fn in routes.items() if n != "raster"}
        scale = float(gv["torch"].abs().max())
        rec["k"][str(K)] = {
            "fragments": int((p2f >= 0).sum()), "plane_bytes": int(sum(t.numel() * t.element_size() for t in (p2f, z, b, d))),
            "fwd_ms": fwd, "fwd_bwd_ms": both, "raster_fwd_bwd_ms": both["raster"], "memory": mem,
            "vertex_grad_fused_vs_torch_rel": float((gv["fused"] - gv["torch"]).abs().max()) / scale,
            "vertex_grad_alpha_fused_vs_torch_rel": float((gv["fused_alpha"] - gv["torch_alpha"]).abs().max()) / float(gv["torch_alpha"].abs().max())}
        print(json.dumps({f"K={K}": rec["k"][str(K)]}), flush=True)
    doc = json.dumps(rec, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
