"""Dense vs hierarchical final decode (followmyhold_amd/volume.py) at octree resolution 384 (385^3 grid), one JSON document.

(a) noisy field: the Hunyuan3D-2-shape stand-in ShapeVAE of bench.py's final_decode_record (random weights, random latent) on the
    HIP geometry decoder -- latent2sdf vs latent2sdf_hierarchical, wall time, decoded fraction, closure rounds, mesh identity.
(b) compact field, COST MODEL: the band is selected by an analytic torus (what a trained decoder's compact object looks like), and the
    decode callable ALSO runs the same Hunyuan-shape HIP decoder on exactly the selected points and discards its output, so the time
    carries the real decoder cost of the points decoded.  The dense side of (b) is the same model on every grid point.

    python scripts/volume_decode_bench.py [--out profiles/volume_decode_bench.json] [--res 384] [--min-res 96] [--repeats 2]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--res", type=int, default=384)
    ap.add_argument("--min-res", type=int, default=96)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--cases", default="a,b")
    a = ap.parse_args()
    import numpy as np
    import torch
    from followmyhold_amd import geo_decode, ops, pipeline as PLN, standins, volume
    from followmyhold_amd.facade import generate_dense_grid_points
    if not torch.cuda.is_available():
        raise SystemExit("volume_decode_bench.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    vae = standins.StandInShapeVAE(num_latents=3072, embed_dim=64, width=1024, heads=16, layers=16, num_freqs=8).to(dev).half().eval()
    vae.requires_grad_(False)
    hip = geo_decode.install(vae)
    lat = torch.randn(1, 3072, 64, device=dev).half()
    res, mr = a.res, a.min_res
    bmin, bmax = np.full(3, -1.10), np.full(3, 1.10)
    xyz_np, gsz, _ = generate_dense_grid_points(bmin, bmax, octree_depth=5, octree_resolution=res, indexing="ij")
    xyz = torch.as_tensor(xyz_np, dtype=torch.float32, device=dev)
    n = int(xyz.shape[0])

    def timed(fn):
        best, out = None, None
        for _ in range(a.repeats):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            with torch.no_grad():
                out = fn()
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best * 1e3, out

    def mesh(sdf):
        v, f, _ = ops.flexicubes(xyz, sdf.reshape(-1), res)
        return v, f

    rec = {"grid": f"{res + 1}^3", "query_points": n, "min_res": mr, "band": 1, "repeats": a.repeats, "timing": "best of repeats, host clock "
           "around work that ends in a device synchronise"}
    if "a" in a.cases:
        dense_ms, dense = timed(lambda: PLN.latent2sdf(lat, xyz, gsz, vae, dev))
        hier_ms, (hier, st) = timed(lambda: PLN.latent2sdf_hierarchical(lat, bmin, bmax, res, vae, dev, min_res=mr))
        v0, f0 = mesh(dense)
        v1, f1 = mesh(hier)
        sign_diff = (dense.reshape(-1) < 0) != (hier.reshape(-1) < 0)
        rec["a_noisy_standin"] = {"what": "Hunyuan-shape stand-in ShapeVAE (random weights): latent2sdf vs latent2sdf_hierarchical",
                                  "dense_ms": dense_ms, "hierarchical_ms": hier_ms, "speedup": dense_ms / hier_ms, "stats": st,
                                  "vertices_dense": int(v0.shape[0]), "vertices_hierarchical": int(v1.shape[0]),
                                  "sign_mismatch_points": int(sign_diff.sum()),
                                  "meshes_identical": bool(torch.equal(v0, v1) and torch.equal(f0, f1))}
        del dense, hier
        print(json.dumps(rec["a_noisy_standin"]), flush=True)
    if "b" in a.cases:
        with torch.no_grad():
            tok = PLN.vae_tokens(vae, 1 / vae.scale_factor * lat)

        def torus(p):
            x, y, z = p[:, 0], p[:, 1], p[:, 2]
            q = torch.sqrt(x * x + y * y) - 0.5
            return 0.2 - torch.sqrt(q * q + z * z)

        def modelled(p):
            hip(p.reshape(1, -1, 3), tok)                # the decoder's cost on exactly these points; output discarded
            return torus(p)

        def dense_b():
            q = xyz.half().float()
            hip(q.reshape(1, -1, 3), tok)
            return torus(q)

        dense_ms, dense = timed(dense_b)
        hier_ms, (hier, st) = timed(lambda: volume.hierarchical_grid_logits(modelled, bmin, bmax, res, min_res=mr, device=dev))
        v0, f0 = mesh(-dense)
        v1, f1 = mesh(-hier)
        rec["b_compact_cost_model"] = {"what": "COST MODEL: band selected by an analytic torus (R 0.5, r 0.2); the Hunyuan-shape HIP decoder "
                                       "runs on exactly the selected points (output discarded); dense = the same on all points",
                                       "dense_ms": dense_ms, "hierarchical_ms": hier_ms, "speedup": dense_ms / hier_ms, "stats": st,
                                       "vertices_dense": int(v0.shape[0]), "meshes_identical": bool(torch.equal(v0, v1) and torch.equal(f0, f1))}
        print(json.dumps(rec["b_compact_cost_model"]), flush=True)
    rec["device"] = torch.cuda.get_device_name(dev)
    out = json.dumps(rec, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out + "\n")
    print(out)


if __name__ == "__main__":
    main()
