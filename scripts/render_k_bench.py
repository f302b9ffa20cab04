"""The fused K-fragment render (ops.render_k / render_k_alpha: mesh -> image in one operator, no (H,W,K) planes in memory) against the
composed route ops.raster_k -> ops.blend_k / blend_k_alpha, one JSON document.  All of it is libfoho_rastk.so.

Scene: scripts/blend_k_bench.py's -- followmyhold_amd.synthetic.build_scene at 512 x 512 (778-vertex hand + the 20k object, about 22 k
faces) at its start pose, the blur radius of scripts/raster_k_bench.py, BlendParams' default sigma = gamma = 1e-4, the mesh's vertex
normals as (F,3,3) face attributes weighted by the barycentrics.  For K = 8 and 100, for Phong attributes and for the alpha alone, and
for each route:
  fwd_ms        mesh -> image without autograd
  fwd_bwd_ms    mesh -> image -> backward to the NDC vertices and the attributes under a random grad_out
  peak_bytes    torch.cuda.max_memory_allocated over one fwd_bwd, above what was allocated before it
The two routes run interleaved in one process; each figure is the median of --repeats after one untimed warm-up, host clock around a
call that ends in a device synchronise.  No timing target: the composed route in the same run is the yardstick.

    python scripts/render_k_bench.py [--out profiles/r11_render_k_bench.json] [--size 512] [--repeats 5] [--ks 8,100]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_render_k_bench.json"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ks", default="8,100")
    a = ap.parse_args()
    import numpy as np
    import torch
    from followmyhold_amd import engine as E, facade, ops, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("render_k_bench.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    H = W = a.size
    sc = synthetic.build_scene(E.hip_render_fn(dev), obj_kind="20k", H=H, W=W, seed=0)
    T = sc["T_h2m"]
    world = torch.from_numpy(np.concatenate([sc["hand_verts"], sc["obj_verts"] @ T[:3, :3].T + T[:3, 3]], 0).astype(np.float32)).to(dev)
    faces = torch.from_numpy(np.concatenate([sc["hand_faces"], sc["obj_faces"] + len(sc["hand_verts"])], 0)).to(dev)
    Rm = torch.tensor([[-1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0]], device=dev).unsqueeze(0)
    cams = facade.FoVPerspectiveCameras(device=dev, R=Rm, T=torch.zeros(1, 3, device=dev), znear=0.01, zfar=100.0, fov=sc["fov"])
    ndc0 = cams.transform_points_ndc(world).contiguous()
    attr0 = facade.Meshes([world], [faces]).verts_normals_packed()[faces].contiguous()
    blur = float(np.float32(np.log(1.0 / 1e-4 - 1.0) * np.float32(1e-8)))
    bp = facade.BlendParams()
    zn, zf = cams.znear, cams.zfar
    blend = (bp.sigma, bp.gamma, zn, zf, bp.background_color)
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
        return {"allocated_before": int(before), "peak_bytes_above": int(torch.cuda.max_memory_allocated(dev) - before)}

    rec = {"frame": [H, W], "vertices": int(ndc0.shape[0]), "faces": int(faces.shape[0]), "blur_radius": blur, "sigma": bp.sigma, "gamma": bp.gamma,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(dev),
           "timing": "median of repeats after one untimed warm-up, routes interleaved; host clock around one call that ends in a device synchronise",
           "routes": {"render_k": "ops.render_k / render_k_alpha", "composed": "ops.raster_k -> ops.blend_k / blend_k_alpha"}, "k": {}}
    for K in [int(k) for k in a.ks.split(",")]:
        g_rgb = torch.randn(H, W, 4, generator=gen).to(dev)
        g_a = torch.randn(H, W, generator=gen).to(dev)

        def image(route, v, attr):
            if route == "render_k":
                return ops.render_k(v, faces, H, W, K, blur, attr, *blend)
            p2f, z, b, d, _ = ops.raster_k(v, faces, H, W, K, blur)
            return ops.blend_k(p2f, z, b, d, attr, *blend)

        def alpha(route, v):
            if route == "render_k":
                return ops.render_k_alpha(v, faces, H, W, K, blur, bp.sigma)
            p2f, _, _, d, _ = ops.raster_k(v, faces, H, W, K, blur)
            return ops.blend_k_alpha(p2f, d, bp.sigma)

        def through(route, phong):
            def run():
                v = ndc0.clone().requires_grad_(True)
                at = attr0.clone().requires_grad_(True)
                (image(route, v, at) if phong else alpha(route, v)).backward(g_rgb if phong else g_a)
                return v.grad
            return run

        names = [(r, p) for p in (True, False) for r in ("render_k", "composed")]
        label = lambda r, p: r + ("" if p else "_alpha")
        with torch.no_grad():
            fwd = interleaved({label(r, p): (lambda r=r, p=p: image(r, ndc0, attr0) if p else alpha(r, ndc0)) for r, p in names})
            same = {"image": bool(torch.equal(image("render_k", ndc0, attr0), image("composed", ndc0, attr0))),
                    "alpha": bool(torch.equal(alpha("render_k", ndc0), alpha("composed", ndc0)))}
            planes = ops.raster_k_fwd(ndc0, faces, H, W, K, blur)
            fragments = int((planes["pix_to_face"] >= 0).sum())
            plane_bytes = int(sum(planes[n].numel() * planes[n].element_size() for n in ("pix_to_face", "zbuf", "bary", "dists")))
            del planes
        routes = {label(r, p): through(r, p) for r, p in names}
        both = interleaved(routes)
        mem = {n: peak(fn) for n, fn in routes.items()}
        gv = {n: fn() for n, fn in routes.items()}
        rel = lambda x, y: float((x - y).abs().max()) / float(y.abs().max())
        rec["k"][str(K)] = {
            "fragments": fragments, "plane_bytes": plane_bytes, "forward_bitwise_equal": same, "fwd_ms": fwd, "fwd_bwd_ms": both, "memory": mem,
            "vertex_grad_render_k_vs_composed_rel": rel(gv["render_k"], gv["composed"]),
            "vertex_grad_alpha_render_k_vs_composed_rel": rel(gv["render_k_alpha"], gv["composed_alpha"])}
        print(json.dumps({f"K={K}": rec["k"][str(K)]}), flush=True)
    doc = json.dumps(rec, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
