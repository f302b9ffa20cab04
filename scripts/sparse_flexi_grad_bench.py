"""Extraction plus backward to the field, dense route (ops.flexicubes on the dense point grid) against sparse route
(sparse_flexi.flexicubes_sparse_grad on axis tables), one JSON document.

Per field and resolution, both routes interleaved in one process, median of --repeats after one untimed warm-up round:
  extract_ms    the forward (field on the device -> vertices, faces, l_dev); the sparse route's two host reads are inside
  backward_ms   (verts * g).sum().backward() for a seeded cotangent g, down to dL/ds
each ending in a device synchronise, plus the peak of torch.cuda.max_memory_allocated above what was held before the forward (the
field, the cotangent, and for the dense route its (res+1)^3 x 3 point grid, which is reported separately as held_grid_bytes), whether
the meshes are identical, and the largest difference of the two gradients.  The grid and the tables are on the device before the clock
starts, as in the guidance loop, which builds them once.

Two fields at each of --res (64, 128, 256):
  torus   analytic
  noisy   the Hunyuan3D-2-shape stand-in ShapeVAE (random weights, random latent) on the HIP geometry decoder, as
          scripts/final_extract_bench.py's case (a)

    python scripts/sparse_flexi_grad_bench.py [--out profiles/r12_sparse_flexi_grad_bench.json] [--res 64,128,256] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = ("dense", "sparse")
PARTS = ("extract_ms", "backward_ms", "total_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_sparse_flexi_grad_bench.json"))
    ap.add_argument("--res", default="64,128,256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fields", default="torus,noisy")
    a = ap.parse_args()
    import numpy as np
    import torch
    from followmyhold_amd import geo_decode, ops, pipeline as PLN, standins
    from followmyhold_amd.facade import generate_dense_grid_points
    if not torch.cuda.is_available():
        raise SystemExit("sparse_flexi_grad_bench.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    bmin, bmax = np.full(3, -1.10), np.full(3, 1.10)
    fields = [f for f in a.fields.split(",") if f in ("torus", "noisy")]
    hip = tok = None
    if "noisy" in fields:
        torch.manual_seed(0)
        vae = standins.StandInShapeVAE(num_latents=3072, embed_dim=64, width=1024, heads=16, layers=16, num_freqs=8).to(dev).half().eval()
        vae.requires_grad_(False)
        hip = geo_decode.install(vae)
        lat = torch.randn(1, 3072, 64, device=dev).half()
        with torch.no_grad():
            tok = PLN.vae_tokens(vae, 1 / vae.scale_factor * lat)

    def field(name, xyz):
        with torch.no_grad():
            if name == "torus":
                q = torch.sqrt(xyz[:, 0] ** 2 + xyz[:, 1] ** 2) - 0.5
                return torch.sqrt(q * q + xyz[:, 2] ** 2) - 0.2
            s = -hip(hip.grid_queries(xyz), tok).reshape(-1).float()
            hip.drop_grid_cache()
            return s

    def run(route, xyz, axes, s0, gv, caps):
        """One extraction and its backward; `gv` None: the cotangent is not known yet (the warm-up round sizes it).  `caps`: the dense
        route's capacities, the mesh's own size once it is known, so that no timed dense extraction runs twice for an overflow."""
        s = s0.clone().requires_grad_(True)
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        held = torch.cuda.memory_allocated(dev)
        t0 = time.perf_counter()
        if route == "sparse":
            v, f, _, est = ops.flexicubes_sparse_grad(axes, s, res, return_stats=True)
        else:
            v, f, _ = ops.flexicubes(xyz, s, res, *caps)
            est = None
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        g = gv if gv is not None else torch.ones_like(v)
        (v * g).sum().backward()
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        t = {"extract_ms": (t1 - t0) * 1e3, "backward_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3,
             "peak_bytes_above_held": int(torch.cuda.max_memory_allocated(dev) - held)}
        return t, v.detach(), f, s.grad, est

    rec = {"routes": list(ROUTES), "repeats": a.repeats,
           "timing": "median of repeats, the routes interleaved in one process; host clock around parts that each end in a device "
                     "synchronise; one untimed warm-up round first; grid and axis tables on the device before the clock starts"}
    for res in [int(r) for r in a.res.split(",")]:
        G = res + 1
        xyz_np, _, _ = generate_dense_grid_points(bmin, bmax, octree_depth=5, octree_resolution=res, indexing="ij")
        xyz = torch.as_tensor(xyz_np, dtype=torch.float32, device=dev)
        axes = ops.grid_axes(bmin, bmax, res).to(dev)
        for name in fields:
            s0 = field(name, xyz)
            laps = {r: [] for r in ROUTES}
            last, gv, caps = {}, None, ()
            for rep in range(a.repeats + 1):
                for route in ROUTES:
                    t, v, f, gs, est = run(route, xyz, axes, s0, gv, caps)
                    if gv is None:          # round 0, first route: the vertex count is known now
                        gv = torch.randn(v.shape, generator=torch.Generator().manual_seed(11)).to(dev)
                        caps = (max(int(v.shape[0]), 1), max(int(f.shape[0]), 1))
                    if rep:                 # round 0 warms up allocator and kernels
                        laps[route].append(t)
                    last[route] = (v, f, gs, est)
            out = {"grid": f"{G}^3", "held_grid_bytes": int(xyz.numel() * 4), "held_axes_bytes": int(axes.numel() * 4)}
            for route in ROUTES:
                out[route] = {p: statistics.median(l[p] for l in laps[route]) for p in PARTS}
                out[route]["peak_bytes_above_held"] = max(l["peak_bytes_above_held"] for l in laps[route])
            (v0, f0, g0, _), (v1, f1, g1, est) = last["dense"], last["sparse"]
            out["extract_stats"] = est
            out["vertices"], out["faces"] = int(v0.shape[0]), int(f0.shape[0])
            out["meshes_identical"] = bool(v0.shape == v1.shape and torch.equal(v0, v1) and torch.equal(f0, f1))
            out["max_abs_gradient_difference"] = float((g0 - g1).abs().max())
            out["max_abs_gradient"] = float(g0.abs().max())
            out["sparse_over_dense_total"] = out["sparse"]["total_ms"] / out["dense"]["total_ms"]
            rec[f"{name}_{res}"] = out
            print(json.dumps({f"{name}_{res}": out}), flush=True)
            del last, s0
        del xyz
        torch.cuda.empty_cache()
    rec["device"] = torch.cuda.get_device_name(dev)
    doc = json.dumps(rec, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
