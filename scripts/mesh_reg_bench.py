"""Mesh regularisers (ops.mesh_regularizers, libfoho_mreg.so) against the same formulas in float32 torch on the device: one JSON document.

Meshes: icosphere(3) (642 V / 1280 F), the workload's object (10 242 V / 20 480 F), the 40 k-face object (20 160 V / 40 320 F).
Cases, each forward + gradient to the vertices: uniform, cot, cotcurv (Laplacian alone), nc (normal consistency alone), fused (cot +
normal consistency + edge length in one call).  Routes:
  hip     ops.mesh_regularizers(...)[0].backward(): one foho_mreg_run (three launches at most) and the scaling by the cotangent
  torch   the formulas of csrc/foho_mreg.h in float32 torch ops through autograd (index_add over the directed edges, a (P, 4) gather
          for the pairs), the index tensors built once outside the clock -- what a user writes without the operator
The two routes alternate in one process; a measurement is the host clock around --inner calls that end in one device synchronise,
divided by --inner; the median over --repeats after one untimed warm-up round.  build_ms is MeshTopology(faces, V) on device faces,
timed on its own (median, each ending in a synchronise).  algorithmic_bytes is what one hip call has to move, counted from the shapes:
every table and the vertices once per kernel that reads them, every record written once and read once, the gradient once;
share_of_hbm_peak is algorithmic_bytes / hip time over 8 TB/s -- an end-to-end figure of the whole call, launches included, not a
kernel's share of peak.  Nothing is asserted about the ratios; the routes' totals are compared (relative difference reported).

    python scripts/mesh_reg_bench.py [--out profiles/mesh_reg_bench.json] [--repeats 7] [--inner 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"uniform": dict(w_lap=1.0, lap_method="uniform"), "cot": dict(w_lap=1.0, lap_method="cot"),
         "cotcurv": dict(w_lap=1.0, lap_method="cotcurv"), "nc": dict(w_nc=1.0),
         "fused": dict(w_lap=1.0, lap_method="cot", w_nc=0.5, w_edge=2.0, target_length=0.0)}
HBM_PEAK = 8.0e12


def algorithmic_bytes(t, w_lap=0.0, lap_method="uniform", w_nc=0.0, w_edge=0.0, **_):
    """Bytes one foho_mreg_run with a gradient has to move (csrc/foho_mreg.hip's three kernels), from the table sizes."""
    V, F, E, P = t.V, t.F, t.E, t.P
    cot, lap, nc, edge = bool(w_lap) and lap_method != "uniform", bool(w_lap), bool(w_nc) and P > 0, bool(w_edge)
    nbr = 4 * (V + 1) + 4 * 2 * E + (4 * 2 * E if cot else 0)       # offsets, neighbours, edge ids
    b = 0
    if cot:                                                         # k_mreg_items, edges: lists, faces, vertices; W and area out
        b += 4 * (E + 1) + 4 * 3 * F + 12 * F + 12 * V + 8 * E
    if nc:                                                          # k_mreg_items, pairs: table, vertices; four records out
        b += 16 * P + 12 * V + 64 * P
    if lap or edge:                                                 # k_mreg_rows: lists, vertices, W; two records out
        b += nbr + 12 * V + (8 * E if cot else 0) + (32 * V if lap else 0)
        b += nbr + 12 * V + (8 * E if cot else 0) + (32 * V if lap else 0)      # k_mreg_gather reads the same back
    if nc:                                                          # k_mreg_gather: the (pair, slot) lists and the records
        b += 4 * (V + 1) + 16 * P + 64 * P
    return b + 12 * V                                               # the gradient


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_reg_bench.json"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    a = ap.parse_args()
    import torch
    from followmyhold_amd import ops, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("mesh_reg_bench.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)

    def torch_tables(t):
        """The index tensors of the torch route (int64, cached outside the clock)."""
        f, e = t.faces.long(), t.edges.long()
        src, dst = torch.cat([e[:, 0], e[:, 1]]), torch.cat([e[:, 1], e[:, 0]])
        deg = torch.zeros(t.V, device=dev).index_add_(0, src, torch.ones(src.shape[0], device=dev))
        return dict(f=f, e=e, src=src, dst=dst, deg=deg, pairs=t.pairs.long())

    def torch_lap(v, T, method):
        V = v.shape[0]
        if method == "uniform":
            s = torch.zeros_like(v).index_add(0, T["src"], v[T["dst"]])
            inv = torch.where(T["deg"] > 0, 1.0 / T["deg"].clamp(min=1.0), T["deg"])
            return ((s * inv[:, None] - v) * (T["deg"] > 0)[:, None]).norm(dim=1).sum() / V
        f = T["f"]
        with torch.no_grad():
            p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
            A, B, C = (p1 - p2).norm(dim=1), (p0 - p2).norm(dim=1), (p0 - p1).norm(dim=1)
            s = 0.5 * (A + B + C)
            area = (s * (s - A) * (s - B) * (s - C)).clamp(min=1e-12).sqrt()
            A2, B2, C2 = A * A, B * B, C * C
            cot = torch.stack([B2 + C2 - A2, A2 + C2 - B2, A2 + B2 - C2], 1) / area[:, None] / 4.0
            ii = torch.cat([f[:, 1], f[:, 2], f[:, 0], f[:, 2], f[:, 0], f[:, 1]])       # both directions of the side opposite corner c
            jj = torch.cat([f[:, 2], f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 0]])
            w = torch.cat([cot[:, 0], cot[:, 1], cot[:, 2]]).repeat(2)
            S = torch.zeros(V, device=dev).index_add_(0, ii, w)
            ar = torch.zeros(V, device=dev).index_add_(0, f.reshape(-1), area.repeat_interleave(3))
        Lv = torch.zeros_like(v).index_add(0, ii, v[jj] * w[:, None])
        if method == "cot":
            n = torch.where(S > 0, 1.0 / S, S)
            return (Lv * n[:, None] - v).norm(dim=1).sum() / V
        q = torch.where(ar > 0, 1.0 / ar, ar)
        return ((Lv - S[:, None] * v) * (0.25 * q)[:, None]).norm(dim=1).sum() / V

    def torch_nc(v, T):
        p = T["pairs"]
        v0, e = v[p[:, 0]], v[p[:, 1]] - v[p[:, 0]]
        n0, n1 = torch.cross(e, v[p[:, 2]] - v0, dim=1), -torch.cross(e, v[p[:, 3]] - v0, dim=1)
        return (1.0 - (n0 * n1).sum(1) / (n0.norm(dim=1).clamp(min=1e-8) * n1.norm(dim=1).clamp(min=1e-8))).mean()

    def torch_edge(v, T, target):
        return (((v[T["e"][:, 0]] - v[T["e"][:, 1]]).norm(dim=1) - target) ** 2).mean()

    def torch_total(v, T, w_lap=0.0, lap_method="uniform", w_nc=0.0, w_edge=0.0, target_length=0.0):
        total = 0.0
        if w_edge:
            total = total + w_edge * torch_edge(v, T, target_length)
        if w_lap:
            total = total + w_lap * torch_lap(v, T, lap_method)
        if w_nc:
            total = total + w_nc * torch_nc(v, T)
        return total

    def timed(fn, x):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(a.inner):
            x.grad = None
            fn(x).backward()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 / a.inner

    meshes = {"icosphere3": synthetic.icosphere(3, 0.05), "object_20k": synthetic.make_object("20k"), "object_40k": synthetic.make_object("40k")}
    rec = {"cases": list(CASES), "repeats": a.repeats, "inner": a.inner,
           "timing": "ms per forward + backward: host clock around `inner` calls ending in one device synchronise, median of `repeats`, "
                     "the routes alternating in one process, one untimed warm-up round first; every input on the device before the clock starts"}
    for name, (v_np, f_np) in meshes.items():
        v = torch.as_tensor(v_np, dtype=torch.float32, device=dev)
        f = torch.as_tensor(f_np, dtype=torch.int64, device=dev)
        builds = []
        for rep in range(a.repeats + 1):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            topo = ops.MeshTopology(f, v.shape[0])
            torch.cuda.synchronize(dev)
            if rep:
                builds.append((time.perf_counter() - t0) * 1e3)
        T = torch_tables(topo)
        out = {"V": topo.V, "F": topo.F, "E": topo.E, "P": topo.P, "build_ms": statistics.median(builds), "table_bytes": topo.table_bytes()}
        x = v.clone().requires_grad_(True)
        routes = {c: {"hip": (lambda y, kw=kw: ops.mesh_regularizers(y, topo, **kw)[0]), "torch": (lambda y, kw=kw: torch_total(y, T, **kw))}
                  for c, kw in CASES.items()}
        laps = {c: {"hip": [], "torch": []} for c in CASES}
        for rep in range(a.repeats + 1):
            for c in CASES:
                for r in ("hip", "torch"):
                    t = timed(routes[c][r], x)
                    if rep:
                        laps[c][r].append(t)
        for c, kw in CASES.items():
            hip, tor = statistics.median(laps[c]["hip"]), statistics.median(laps[c]["torch"])
            th, tt = routes[c]["hip"](x).item(), routes[c]["torch"](x).item()
            nbytes = algorithmic_bytes(topo, **kw)
            out[c] = {"hip_ms": hip, "torch_ms": tor, "torch_over_hip": tor / hip, "total_rel_diff": abs(th - tt) / abs(tt),
                      "algorithmic_bytes": nbytes, "share_of_hbm_peak": nbytes / (hip * 1e-3) / HBM_PEAK}
        rec[name] = out
        print(json.dumps({name: out}), flush=True)
    rec["device"] = torch.cuda.get_device_name(dev)
    doc = json.dumps(rec, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
