"""The K-fragment rasteriser (ops.raster_k_fwd / raster_k_bwd, libfoho_rastk.so) on the synthetic hand and object scene, one JSON document.

Scene: followmyhold_amd.synthetic.build_scene at 512 x 512 (778-vertex hand + the 20k object, about 21.5 k faces) at its start pose,
the reference's blur radius.  For K = 1, 8 and 100: forward and backward milliseconds, median of --repeats after one untimed warm-up,
each call ending in a device synchronise (the forward includes its one host read of the overflow word and its allocations); the
workspace bytes; fragments per pixel.  For information only: ops.raster_fwd (one fragment per pixel plus the silhouette product) and
ops.raster_bwd on the same scene.  No timing target: nothing existing is replaced.

    python scripts/raster_k_bench.py [--out profiles/r09_raster_k_bench.json] [--size 512] [--repeats 5] [--ks 1,8,100]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_raster_k_bench.json"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ks", default="1,8,100")
    a = ap.parse_args()
    import numpy as np
    import torch
    from followmyhold_amd import engine as E, facade, ops, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("raster_k_bench.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    H = W = a.size
    sc = synthetic.build_scene(E.hip_render_fn(dev), obj_kind="20k", H=H, W=W, seed=0)
    T = sc["T_h2m"]
    world = np.concatenate([sc["hand_verts"], sc["obj_verts"] @ T[:3, :3].T + T[:3, 3]], 0).astype(np.float32)
    faces = torch.from_numpy(np.concatenate([sc["hand_faces"], sc["obj_faces"] + len(sc["hand_verts"])], 0)).to(dev)
    Rm = torch.tensor([[-1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0]], device=dev).unsqueeze(0)
    cams = facade.FoVPerspectiveCameras(device=dev, R=Rm, T=torch.zeros(1, 3, device=dev), znear=0.01, zfar=100.0, fov=sc["fov"])
    ndc = cams.transform_points_ndc(torch.from_numpy(world).to(dev)).contiguous()
    blur = float(np.float32(np.log(1.0 / 1e-4 - 1.0) * np.float32(1e-8)))

    def timed(fn):
        fn()                                            # warm-up: kernels, allocator
        torch.cuda.synchronize(dev)
        laps = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            laps.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(laps)

    rec = {"frame": [H, W], "vertices": int(ndc.shape[0]), "faces": int(faces.shape[0]), "blur_radius": blur, "repeats": a.repeats,
           "timing": "median of repeats after one untimed warm-up; host clock around one call that ends in a device synchronise",
           "device": torch.cuda.get_device_name(dev), "k": {}}
    gen = torch.Generator().manual_seed(0)
    for K in [int(k) for k in a.ks.split(",")]:
        out = ops.raster_k_fwd(ndc, faces, H, W, K, blur)
        cap = out["list_cap"]
        p2f = out["pix_to_face"]
        gz = torch.randn(H, W, K, generator=gen).to(dev)
        gb = torch.randn(H, W, K, 3, generator=gen).to(dev)
        gd = torch.randn(H, W, K, generator=gen).to(dev)
        rec["k"][str(K)] = {
            "fwd_ms": timed(lambda: ops.raster_k_fwd(ndc, faces, H, W, K, blur, list_cap=cap)),
            "bwd_ms": timed(lambda: ops.raster_k_bwd(ndc, faces, p2f, gz, gb, gd, blur_radius=blur)),
            "workspace_bytes": out["workspace_bytes"], "list_entries": cap, "retried_at_default_cap": bool(out["retried"]),
            "fragments": int((p2f >= 0).sum()), "max_fragments_per_pixel": int(out["counts"].max()),
            "output_bytes": int(sum(out[k].numel() * out[k].element_size() for k in ("pix_to_face", "zbuf", "bary", "dists", "counts")))}
        print(json.dumps({f"K={K}": rec["k"][str(K)]}), flush=True)
    one = ops.raster_fwd(ndc, faces, H, W, blur)
    g1 = [torch.randn(H, W, generator=gen).to(dev), torch.randn(H, W, 3, generator=gen).to(dev), torch.randn(H, W, generator=gen).to(dev)]
    rec["raster_fwd_for_information"] = {
        "fwd_ms": timed(lambda: ops.raster_fwd(ndc, faces, H, W, blur)),
        "bwd_ms": timed(lambda: ops.raster_bwd(ndc, faces, one["pix_to_face"], g1[0], g1[1], g1[2], blur_radius=blur)),
        "workspace_bytes": int(one["_keep"][2].numel())}
    doc = json.dumps(rec, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
