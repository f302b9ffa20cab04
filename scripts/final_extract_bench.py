"""The final step from VAE tokens to mesh at octree resolution 384 (385^3 grid) with the dense and the sparse extractor, one JSON document.

Three configurations, interleaved in one process, median of --repeats:
  hier_dense    hierarchical decode + ops.flexicubes on the dense point grid (the route before the sparse extractor existed)
  hier_sparse   hierarchical decode + sparse_flexi.flexicubes_sparse on axis tables: no dense point grid at all
  dense_sparse  dense decode (needs the point grid for its queries) + flexicubes_sparse
each split into: host grid build (generate_dense_grid_points, or grid_axes), host-to-device copy, decode, extraction; plus the peak of
torch.cuda.max_memory_allocated over the run and whether the meshes are identical.

Two fields, those of scripts/volume_decode_bench.py:
(a) noisy field: the Hunyuan3D-2-shape stand-in ShapeVAE (random weights, random latent) on the HIP geometry decoder.
(b) compact field, COST MODEL: values from an analytic torus, while the same HIP decoder also runs on exactly the decoded points (output
    discarded), so the decode time carries the real decoder cost.

    python scripts/final_extract_bench.py [--out profiles/r08_final_extract_bench.json] [--res 384] [--min-res 96] [--repeats 5] [--cases a,b]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ("hier_dense", "hier_sparse", "dense_sparse")
PARTS = ("grid_build_ms", "h2d_ms", "decode_ms", "extract_ms", "total_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_final_extract_bench.json"))
    ap.add_argument("--res", type=int, default=384)
    ap.add_argument("--min-res", type=int, default=96)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", default="a,b")
    a = ap.parse_args()
    import numpy as np
    import torch
    from followmyhold_amd import geo_decode, ops, pipeline as PLN, standins, volume
    from followmyhold_amd.facade import generate_dense_grid_points
    if not torch.cuda.is_available():
        raise SystemExit("final_extract_bench.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    vae = standins.StandInShapeVAE(num_latents=3072, embed_dim=64, width=1024, heads=16, layers=16, num_freqs=8).to(dev).half().eval()
    vae.requires_grad_(False)
    hip = geo_decode.install(vae)
    lat = torch.randn(1, 3072, 64, device=dev).half()
    res, mr = a.res, a.min_res
    G = res + 1
    bmin, bmax = np.full(3, -1.10), np.full(3, 1.10)
    with torch.no_grad():
        tok = PLN.vae_tokens(vae, 1 / vae.scale_factor * lat)

    def torus(p):
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        q = torch.sqrt(x * x + y * y) - 0.5
        return 0.2 - torch.sqrt(q * q + z * z)

    def modelled(p):
        hip(p.reshape(1, -1, 3), tok)                # the decoder's cost on exactly these points; output discarded
        return torus(p)

    def decode_dense(case, xyz):
        if case == "a":
            return -hip(hip.grid_queries(xyz), tok).reshape(-1).float(), None
        q = hip.grid_queries(xyz)
        hip(q, tok)
        return -torus(q.reshape(-1, 3)), None

    def decode_hier(case):
        if case == "a":
            sdf, st = PLN.sdf_hierarchical_from_tokens(tok, bmin, bmax, res, hip, min_res=mr)
            return sdf.reshape(-1), st
        logits, st = volume.hierarchical_grid_logits(modelled, bmin, bmax, res, min_res=mr, device=dev)
        return -logits, st

    def run(case, config):
        """One final step, tokens -> mesh; every part ends in a device synchronise."""
        torch.cuda.synchronize(dev)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        t = {}
        clock = [time.perf_counter()]

        def lap(name):
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            t[name] = (now - clock[0]) * 1e3
            clock[0] = now

        dense_grid = config != "hier_sparse"
        sparse = config != "hier_dense"
        xyz = axes = None
        with torch.no_grad():
            if dense_grid:
                xyz_np, _, _ = generate_dense_grid_points(bmin, bmax, octree_depth=5, octree_resolution=res, indexing="ij")
            if sparse:
                axes_host = ops.grid_axes(bmin, bmax, res)
            lap("grid_build_ms")
            if dense_grid:
                xyz = torch.as_tensor(xyz_np, dtype=torch.float32, device=dev)       # pageable host memory, as the pipeline copies it
            if sparse:
                axes = axes_host.to(dev)
            lap("h2d_ms")
            sdf, st = decode_dense(case, xyz) if config == "dense_sparse" else decode_hier(case)
            lap("decode_ms")
            if sparse:
                v, f, _, est = ops.flexicubes_sparse(axes, sdf, res, return_stats=True)
            else:
                v, f, _ = ops.flexicubes(xyz, sdf, res)
                est = None
            lap("extract_ms")
        t["total_ms"] = sum(t.values())
        t["peak_bytes"] = int(torch.cuda.max_memory_allocated(dev))
        hip.drop_grid_cache()           # the decoder's per-grid query cache does not outlive the run it belongs to
        return t, (v, f), st, est

    rec = {"grid": f"{G}^3", "query_points": G ** 3, "min_res": mr, "repeats": a.repeats, "configs": list(CONFIGS),
           "timing": "median of repeats, the configurations interleaved in one process; host clock around parts that each end in a device "
                     "synchronise; one untimed warm-up round first"}
    names = {"a": "a_noisy_standin", "b": "b_compact_cost_model"}
    for case in [c for c in a.cases.split(",") if c in names]:
        laps = {c: [] for c in CONFIGS}
        meshes, extra = {}, {}
        for rep in range(a.repeats + 1):
            for config in CONFIGS:
                t, mesh, st, est = run(case, config)
                if rep:                 # round 0 warms up allocator, kernels and caches
                    laps[config].append(t)
                meshes[config], extra[config] = mesh, (st, est)
        out = {}
        for config in CONFIGS:
            out[config] = {p: statistics.median(l[p] for l in laps[config]) for p in PARTS}
            out[config]["peak_bytes"] = max(l["peak_bytes"] for l in laps[config])
            st, est = extra[config]
            if st is not None:
                out[config]["decoded_fraction"] = st["decoded_fraction"]
            if est is not None:
                out[config]["extract_stats"] = est
        v0, f0 = meshes["hier_dense"]
        out["vertices"], out["faces"] = int(v0.shape[0]), int(f0.shape[0])
        out["hier_sparse_mesh_identical_to_hier_dense"] = bool(torch.equal(v0, meshes["hier_sparse"][0]) and torch.equal(f0, meshes["hier_sparse"][1]))
        # the dense decode's field can differ from the hierarchical one's (volume.py's known limit): reported, not assumed
        out["dense_sparse_mesh_identical_to_hier_dense"] = bool(v0.shape == meshes["dense_sparse"][0].shape and torch.equal(v0, meshes["dense_sparse"][0])
                                                                 and torch.equal(f0, meshes["dense_sparse"][1]))
        out["hier_sparse_over_hier_dense_total"] = out["hier_sparse"]["total_ms"] / out["hier_dense"]["total_ms"]
        rec[names[case]] = out
        print(json.dumps({names[case]: out}), flush=True)
        del meshes
    rec["device"] = torch.cuda.get_device_name(dev)
    doc = json.dumps(rec, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
