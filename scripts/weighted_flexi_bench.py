"""Weighted FlexiCubes (ops.flexicubes_weighted, libfoho_wflexi.so): forward and forward + backward, one JSON document.

One field (the analytic torus) at each of --res (64, 128), five routes interleaved in one process, median of --repeats after one untimed
warm-up round:
  flexicubes          ops.flexicubes, gradient to s and x (float atomics)                  -- the default-weight operator
  unit                ops.flexicubes_weighted without weights, gradient to s and x        -- the same mesh, bit for bit (checked)
  weighted            seeded random alpha, beta, gamma; gradient to s, x, alpha, beta
  weighted_training   the same with training=True (centres, four triangles a quad); gradient to gamma too
  weighted_s_only     as `weighted`, gradient to s alone
each measured as
  forward_ms    inputs on the device -> vertices, faces, l_dev (the host read of the counts is inside)
  backward_ms   ((verts * g).sum() + (l_dev * h).sum()).backward() for seeded cotangents g, h (ops.flexicubes: l_dev carries no gradient)
each ending in a device synchronise (a host clock around synchronised work: a launch returns before its kernel ends).  The capacities are
the mesh's own sizes, known from the warm-up round, so that no timed extraction runs twice for an overflow.  Nothing is asserted about
the ratios.

    python scripts/weighted_flexi_bench.py [--out profiles/weighted_flexi_bench.json] [--res 64,128] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = ("flexicubes", "unit", "weighted", "weighted_training", "weighted_s_only")
PARTS = ("forward_ms", "backward_ms", "total_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weighted_flexi_bench.json"))
    ap.add_argument("--res", default="64,128")
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch
    from followmyhold_amd import ops
    from followmyhold_amd.facade import generate_dense_grid_points
    if not torch.cuda.is_available():
        raise SystemExit("weighted_flexi_bench.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    bmin, bmax = np.full(3, -1.10), np.full(3, 1.10)

    def run(route, res, xyz, s0, w, cot, caps):
        need = {"flexicubes": "sx", "unit": "sx", "weighted": "sxab", "weighted_training": "sxabg", "weighted_s_only": "s"}[route]
        s = s0.clone().requires_grad_(True)
        x = xyz.clone().requires_grad_("x" in need)
        al, be, ga = (t.clone().requires_grad_(k in need) for t, k in zip(w, "abg"))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if route == "flexicubes":
            v, f, l = ops.flexicubes(x, s, res, *caps)
        elif route == "unit":
            v, f, l = ops.flexicubes_weighted(x, s, res, verts_cap=caps[0], faces_cap=caps[1])
        else:
            v, f, l = ops.flexicubes_weighted(x, s, res, al, be, ga, training=(route == "weighted_training"), verts_cap=caps[0], faces_cap=caps[1])
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        gv, gl = cot if cot is not None else (torch.ones_like(v), torch.ones_like(l))
        loss = (v * gv).sum() + ((l * gl).sum() if l.requires_grad else 0.0)
        loss.backward()
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        return {"forward_ms": (t1 - t0) * 1e3, "backward_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3}, v.detach(), f, l.detach()

    rec = {"routes": list(ROUTES), "repeats": a.repeats,
           "timing": "median of repeats, the routes interleaved in one process; host clock around parts that each end in a device "
                     "synchronise; one untimed warm-up round first; every input on the device before the clock starts"}
    for res in [int(r) for r in a.res.split(",")]:
        xyz_np, _, _ = generate_dense_grid_points(bmin, bmax, octree_depth=5, octree_resolution=res, indexing="ij")
        xyz = torch.as_tensor(xyz_np, dtype=torch.float32, device=dev)
        q = torch.sqrt(xyz[:, 0] ** 2 + xyz[:, 1] ** 2) - 0.5
        s0 = torch.sqrt(q * q + xyz[:, 2] ** 2) - 0.2
        g = torch.Generator().manual_seed(5)
        C = res ** 3
        w = tuple(t.to(dev) for t in (0.01 + 1.98 * torch.rand(C, 8, generator=g), 0.01 + 1.98 * torch.rand(C, 12, generator=g),
                                      0.005 + 0.99 * torch.rand(C, generator=g)))
        laps = {r: [] for r in ROUTES}
        cots, caps, last = {}, {}, {}
        for rep in range(a.repeats + 1):
            for route in ROUTES:
                t, v, f, l = run(route, res, xyz, s0, w, cots.get(route), caps.get(route, (None, None)))
                if rep == 0:            # the warm-up round sizes the cotangents and the capacities
                    gg = torch.Generator().manual_seed(11)
                    cots[route] = (torch.randn(v.shape, generator=gg).to(dev), torch.randn(l.shape, generator=gg).to(dev))
                    caps[route] = (max(int(v.shape[0]), 1), max(int(f.shape[0]), 1))
                else:
                    laps[route].append(t)
                last[route] = (v, f, l)
        out = {"grid": f"{res + 1}^3", "surface": {r: {"vertices": int(last[r][0].shape[0]), "faces": int(last[r][1].shape[0])} for r in ROUTES}}
        for route in ROUTES:
            out[route] = {p: statistics.median(l[p] for l in laps[route]) for p in PARTS}
        out["unit_mesh_identical"] = bool(all(torch.equal(p, q) for p, q in zip(last["flexicubes"], last["unit"])))
        rec[f"torus_{res}"] = out
        print(json.dumps({f"torus_{res}": out}), flush=True)
        del xyz, s0, w, last, cots
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
