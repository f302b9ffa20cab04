"""Dense vs band decode of the guidance grid (pipeline.latent2sdf_band) at octree resolution 64 (65^3 grid), per
inner iteration, min_res 16 and 32, one JSON document.  The Hunyuan3D-2-shape stand-in ShapeVAE (3072 x 64 latents, width 1024, 16
heads, fp16, random weights) on the HIP geometry decoder.

(a) COST MODEL: the band of an analytic compact field (torus R 0.5, r 0.2) -- what a trained decoder's object looks like -- with the
    HIP decoder run on exactly the selected rows (its output discarded); dense = the same decoder on every row.  Timed: the forward
    (set_kv + decodes), and the forward plus the rows backward (foho_geo_decode_bwd_rows on the full grid) under a FlexiCubes-shaped
    gradient (non-zero on the corners of the torus's sign-changing cubes).  The backward is the same call on both routes.
(b) pipeline iteration, stand-in networks (noisy random field: the band is wide, closure rounds are many): one inner iteration as
    the pipeline's latent_phase runs it -- latent2sdf[_band] -> SdfObjective (FlexiCubes, fused step) -> backward to the noise
    prediction -- for B = 1, and the call_batch form for B = 4.  Decoded fraction, closure rounds, host reads per iteration.

    python scripts/guidance_decode_bench.py [--out profiles/guidance_decode_bench.json] [--iters 5] [--cases a,b] [--min-res 16,32]
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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--min-res", default="16,32")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--band-only", action="store_true", help="case b: band iterations only, B = 1 (the kernel-trace run)")
    a = ap.parse_args()
    import numpy as np
    import torch
    from followmyhold_amd import engine as E, geo_decode, pipeline as PLN, standins, synthetic, vae_transformer, volume
    if not torch.cuda.is_available():
        raise SystemExit("guidance_decode_bench.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    vae = standins.StandInShapeVAE(num_latents=3072, embed_dim=64, width=1024, heads=16, layers=16, num_freqs=8).to(dev).half().eval()
    vae.requires_grad_(False)
    hip = geo_decode.install(vae, device=dev)
    vae_transformer.install(vae, device=dev)
    res = 64
    bmin, bmax = np.full(3, -1.10), np.full(3, 1.10)
    xyz_np, gsz, _ = PLN.generate_dense_grid_points(bmin, bmax, octree_depth=5, octree_resolution=res, indexing="ij")
    xyz = torch.as_tensor(xyz_np, dtype=torch.float32, device=dev)
    q = hip.grid_queries(xyz)
    min_res = [int(m) for m in a.min_res.split(",")]
    sync = lambda: torch.cuda.synchronize(dev)

    def median_ms(fn, n):
        fn()
        ts = []
        for _ in range(n):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), [round(t, 3) for t in ts]

    rec = {"grid": f"{res + 1}^3", "query_points": int(xyz.shape[0]), "iters": a.iters, "band": 1,
           "timing": "median of iters, host clock around work that ends in a device synchronise", "device": torch.cuda.get_device_name(dev)}

    def corners_of(field):
        G = res + 1
        s = (field.reshape(G, G, G) < 0).to(torch.int8)
        n = sum(s[i:i + res, j:j + res, k:k + res] for i in (0, 1) for j in (0, 1) for k in (0, 1))
        mixed = ((n > 0) & (n < 8)).to(torch.int8)
        out = torch.zeros(G, G, G, dtype=torch.int8, device=dev)
        for i in (0, 1):
            for j in (0, 1):
                for k in (0, 1):
                    out[i:i + res, j:j + res, k:k + res] |= mixed
        return out.reshape(-1).bool()

    if "a" in a.cases:
        tok = torch.randn(1, 3072, 1024, device=dev).half()
        kv = hip.kv_of(tok)

        def torus(p):
            x, y, z = p[:, 0], p[:, 1], p[:, 2]
            r = torch.sqrt(x * x + y * y) - 0.5
            return 0.2 - torch.sqrt(r * r + z * z)

        g = torch.randn(xyz.shape[0], device=dev) * corners_of(-torus(q.reshape(-1, 3)))
        g = g.contiguous()

        def modelled(p):
            hip.decode(p)                  # the decoder's cost on exactly these rows; output discarded
            return torus(p)

        def dense_fwd():
            hip.set_kv(kv)
            hip.decode(q)

        def band_fwd(mr):
            hip.set_kv(kv)
            return volume.hierarchical_grid_logits(modelled, bmin, bmax, res, min_res=mr, device=dev)

        def bwd():
            hip.decode_bwd_rows(q, g)

        out = {"what": "COST MODEL: band selected by an analytic torus (R 0.5, r 0.2); the Hunyuan-shape HIP decoder runs on exactly the "
                       "selected rows (output discarded); dense = the same decoder on all rows; backward = foho_geo_decode_bwd_rows on the "
                       "full grid under a gradient on the corners of sign-changing cubes", "gradient_rows": int((g != 0).sum())}
        out["dense_fwd_ms"], _ = median_ms(dense_fwd, a.iters)
        out["dense_fwd_bwd_ms"], _ = median_ms(lambda: (dense_fwd(), bwd()), a.iters)
        for mr in min_res:
            _, st = band_fwd(mr)
            f_ms, _ = median_ms(lambda: band_fwd(mr), a.iters)
            fb_ms, _ = median_ms(lambda: (band_fwd(mr), bwd()), a.iters)
            out[f"band_min_res_{mr}"] = {"fwd_ms": f_ms, "fwd_bwd_ms": fb_ms, "fwd_saving_ms": out["dense_fwd_ms"] - f_ms,
                                         "fwd_bwd_saving_ms": out["dense_fwd_bwd_ms"] - fb_ms, "decoded_fraction": st["decoded_fraction"],
                                         "decoded_per_level": st["decoded_per_level"], "closure_rounds": st["closure_rounds"],
                                         "closure_decoded": st["closure_decoded"], "fallback": st["fallback"]}
        rec["a_cost_model"] = out
        print(json.dumps(out), flush=True)

    if "b" in a.cases:
        render_fn = E.hip_render_fn(dev)
        scene = synthetic.build_scene(render_fn, obj_kind="20k", H=512, W=512, seed=100)
        T = np.array(scene["T_h2m"], np.float32)
        T[:3, :3] *= 0.9 * 0.06
        scene = dict(scene, T_h2m=T)
        cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=True)
        reads = {"n": 0}
        orig_batch = volume.hierarchical_grid_logits_batch

        def counted(*args, **kw):
            fields, sts, n = orig_batch(*args, **kw)
            reads["n"] += n
            return fields, sts, n

        volume.hierarchical_grid_logits_batch = counted
        out = {"what": "one inner iteration as the pipeline's loop runs it (latent2sdf[_band] -> SdfObjective -> backward to the noise "
                       "prediction), stand-in networks with random weights: a noisy field, NOT a trained decoder's"}
        for B in ((1,) if a.band_only else (1, a.batch)):
            gb = E.GuidanceBatch([scene] * B, device=dev, obj_capacity=(32768, 65536))
            obj = E.SdfObjective(gb, xyz, res)
            lat = torch.randn(B, 3072, 64, device=dev, dtype=torch.float16)
            noise = torch.zeros_like(lat).requires_grad_(True)
            per = {}
            for mode in ([] if a.band_only else ["dense"]) + [f"band_min_res_{mr}" for mr in min_res]:
                mr = int(mode.rsplit("_", 1)[1]) if mode != "dense" else None
                sts = []

                def one():
                    noise.grad = None
                    x1 = lat + 0.1 * noise
                    if mode == "dense" and B == 1:
                        sdf = PLN.latent2sdf(x1, xyz, gsz, vae, dev).reshape(1, -1)
                    elif mode == "dense":      # the drivers' dense decode (pipeline._StepDecoder): the transformer on all images, the decoder per image
                        tokens = PLN.vae_tokens(vae, 1 / vae.scale_factor * x1)
                        sdf = torch.stack([-hip(q, tokens[b:b + 1]).reshape(-1).float() for b in range(B)], 0)
                    elif B == 1:
                        sdf, st = PLN.latent2sdf_band(x1, xyz, gsz, vae, dev, bmin, bmax, min_res=mr)
                        sdf = sdf.reshape(1, -1)
                        sts.append([st])
                    else:
                        tokens = PLN.vae_tokens(vae, 1 / vae.scale_factor * x1)
                        sdf, st, _ = PLN.sdf_band_from_tokens([tokens[b:b + 1] for b in range(B)], xyz, res, hip, bmin, bmax, min_res=mr)
                        sts.append(st)
                    loss = obj(sdf, cfg)
                    PLN._bound_active_rows(vae, max(obj.active_rows()))
                    loss.sum().backward()

                reads["n"] = 0
                one()
                r1 = reads["n"]
                ms, all_ms = median_ms(one, a.iters)
                hip.row_cap = None
                hip.take_rows_dropped()
                e = {"iteration_ms": ms, "iteration_ms_all": all_ms}
                if mode != "dense":
                    fr = [s["decoded_fraction"] for it in sts for s in it]
                    e.update(host_reads_per_iteration=r1, mean_decoded_fraction=float(np.mean(fr)), max_decoded_fraction=float(np.max(fr)),
                             max_closure_rounds=max(s["closure_rounds"] for it in sts for s in it),
                             fallbacks=sum(int(s["fallback"]) for it in sts for s in it),
                             decoded_per_level=sts[-1][0]["decoded_per_level"], closure_decoded=sts[-1][0]["closure_decoded"])
                    if "dense" in per:
                        e["saving_ms"] = per["dense"]["iteration_ms"] - ms
                per[mode] = e
                print(json.dumps({"B": B, mode: e}), flush=True)
            out[f"B{B}"] = per
        volume.hierarchical_grid_logits_batch = orig_batch
        rec["b_pipeline_iteration"] = out
    doc = json.dumps(rec, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")
    print(doc)


if __name__ == "__main__":
    main()
