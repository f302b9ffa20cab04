#!/usr/bin/env python
"""bench.py -- guidance-steps/sec of the HIP hot path on MI355X (BASELINE.json metric).

A "step" is one iteration of the reference's joint loop (pipelines.py:1480-1601) for one image: transforms,
hand render, hand+object render with silhouette, keypoints, nearest-neighbour contact, edge loss, 65^3
intersection count, all losses, backward and the AdamW update.  Workload at every N: configs[1] of
BASELINE.json -- one synthetic 512x512 frame per GPU, 778-vertex hand + 10 242-vertex / 20 480-face object
(image-sharded: rank r owns its own frame, no data-path collective; one RCCL all-reduce of the metrics
vector at the end of the batch).

    python bench.py --gpus 1 --steps 50 --warmup 5 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times EXACTLY --steps iterations once (`ms_per_step` = that region / steps; the last one
starts from a restart, so that what it computes is the same in every run), writes the outputs of the last timed step if
--dump-outputs is given and prints the line: nothing else runs.  --full adds what the
headline figure does not need: the timed region repeated until it has measured MIN_TIMED_S (the median repeat is
reported), the per-kernel roofline, the side records and the CPU baseline + parity below.

Prints ONE JSON line on rank 0 (stdout): the contract's fields (+ `roofline` + `cpu_baseline` + `parity` with --full), kept under
1 900 characters so that it survives whole in a log tail (`roofline.secondary` carries the headline numbers of the side records).  The DETAIL
record -- everything below -- goes to stderr as one line prefixed `bench-detail: ` and to gpurun_out/bench_detail.json:
  roofline            the dominant kernel: algorithmic bytes per launch / hipEvent-timed duration on the launch stream
  kernels             every launch of the step the same way
  step_roofline_frac  SURVEY 8(d)'s B_step x steps/s / HBM peak;  step_traffic_frac: the MEASURED bytes per step;
                      batched.valu_issue_frac: the share of the chip's vector-ALU issue slots the measured rate needs
                      (rocprofv3 PMC summary under profiles/) x steps/s / HBM peak
  parity              first step of the benchmark scene, HIP vs the CPU oracle: loss_rel_err_vs_oracle,
                      pix_to_face_mismatch (the metric's "loss match vs ref")
  cpu_baseline        the CPU oracle ("port" of the reference path) on this box's host cores, bounded sample;
  cpu_baseline_1t     the same with one thread, the reference's own thread policy (src/foho/main.py:65-68)
  batched             configs[2]'s per-GPU regime: 8 frames per GPU, 4 streams x 2 frames
  closeup             the reference's real frames: crops around hand + object (meshes fill the frame), 1 and 32 images in flight
  job                 the 750-iteration per-image job through the product entry point's engine at 1 / 8 / 16 images in flight
  driver_on_files     foho.guidance.run.run() on scene folders in the reference's file formats, wall time per image
  topology_changing   the step as the real pipeline sees it: a new FlexiCubes mesh (new topology) every iteration
  geo_decode          the ShapeVAE geometry decoder of latent2sdf (65^3 queries x 3072 tokens) on the matrix cores vs torch
  vae_transformer     `vae(pred)` of latent2sdf (16 layers x 3072 tokens) forward + backward: foho_vae_fwd/_bwd against the torch module
  pipeline_iteration  one inner iteration of the real pipeline (VAE transformer -> geometry decoder -> FlexiCubes -> step -> backward)
                      with Hunyuan-shaped stand-in networks: torch decoder vs the HIP decoder
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md "HBM3E peak BW")
STEP_KERNELS = ("k_xform", "k_stage2", "k_resolve", "k_loss", "k_pix_bwd", "k_vert_bwd")
MIN_TIMED_S = 0.25     # the timed region of --steps iterations is repeated until this much has been measured
# committed rocprofv3 summaries, by workload (object kind, image size, images per GPU): PMC traffic and kernel trace are only
# attached to a record of the SAME workload (images per LAUNCH: the b8 files are one 8-image batch on one stream) --
# another object / size / batch gets null, never a borrowed number
def _prof(name):
    """Committed rocprofv3 summaries of a workload, newest round first."""
    return [os.path.join("profiles", f"{r}_{name}") for r in ("r06", "r05", "r04", "r03", "r02")]


PMC_CSVS = {("20k", 512, 1): _prof("rocprofv3_pmc_fetch_write_b1.csv"), ("20k", 512, 8): _prof("rocprofv3_pmc_fetch_write_b8.csv")}
KSTATS_CSVS = {("20k", 512, 1): _prof("rocprofv3_kernel_stats_bench_b1.csv"), ("20k", 512, 8): _prof("rocprofv3_kernel_stats_bench_b8_1stream.csv")}
SQ_CSVS = {("20k", 512, 1): _prof("rocprofv3_sq_counters_b1.csv"), ("20k", 512, 8): _prof("rocprofv3_sq_counters_b8_1stream.csv")}
VALU_PEAK_CYCLES_PER_S = 1024 * 2.4e9     # 256 CUs x 4 SIMDs at the 2.4 GHz peak clock: busy SIMD cycles the chip can offer per second


def algorithmic_bytes(H, W, Vh, Vo, Fh, Fo):
    """B_step = 206*H*W + 96*(Vh+Vo) + 48*(Fh+Fo) + 12*Fo bytes per guidance step."""
    return 206 * H * W + 96 * (Vh + Vo) + 48 * (Fh + Fo) + 12 * Fo


def kernel_bytes(name, H, W, Vh, Vo, Fh, Fo, hits=None, grid_res=64):
    """Compulsory HBM bytes of each launch of the step for the data structures this build uses:
    every buffer a kernel must read or write counted once.  The G-buffer is HIT-ONLY: face ids exist for every pixel
    (4 B), depth / edge distance / silhouette product / colour (24 B) only where a face was hit, and the backward pass
    only opens tiles with a hit.  `hits` = dict(px=[hit pixels of render 0, 1], tile_px=[pixels in hit tiles]) measured
    on the benchmark scene; without it every pixel is charged.  P pixels, V vertices, F faces; hand faces feed both
    renders."""
    P, V, F = H * W, Vh + Vo, Fh + Fo
    px = hits["px"] if hits else [P, P]
    tpx = hits["tile_px"] if hits else [P, P]
    G1 = grid_res + 1
    zeroed = 36 * V + 2 * G1 * G1 * 16                                 # per-step accumulators cleared by k_xform's extra columns
    table = {
        "k_xform": 36 * V + zeroed,                                     # verts_in -> world, ndc
        # normals (faces via CSR + positions -> raw + unit normals), KNN, keypoints, edge loss; scatter rasteriser (face
        # ids + NDC gather of every face, hand faces twice; 8-B key per fragment ~ hit pixel); inside test (ids + vertices)
        "k_stage2": 48 * V + 12 * F + 12 * Fo + 48 * (Fh + F) + 8 * (px[0] + px[1]) + 24 * F,
        # key plane read + cleared and face id written where a tile was opened; 24 B of planes per hit pixel; normals
        "k_resolve": (8 + 8 + 4) * (tpx[0] + tpx[1]) + 24 * (px[0] + px[1]) + 12 * V,
        # hit tiles only (everything else comes from static sums of the targets): face ids + targets (12 + 4 + 1 B) per tile
        # pixel, planes of the hit pixels
        "k_loss": (4 + 17) * (tpx[0] + tpx[1]) + 24 * (px[0] + px[1]),
        # hit tiles only: face ids + targets per tile pixel, planes per hit pixel, 24 B of vertex-gradient atomics per
        # (face, corner) reached
        "k_pix_bwd": (4 + 17) * (tpx[0] + tpx[1]) + 24 * (px[0] + px[1]) + 24 * (Fh + F),
        # per vertex: NDC / normal / direct gradients in, world gradient + grad_verts_in out, positions; per (vertex, face)
        # pair of the normal backward: the pair record
        "k_vert_bwd": 108 * V + 8 * 3 * F,
        "k_final": 0,
    }
    return table.get(name)


def pmc_table(workload):
    """({kernel: HBM bytes per launch}, file) from the committed rocprofv3 PMC passes of THIS workload (FETCH_SIZE /
    WRITE_SIZE are in KiB and FETCH_SIZE reads half of a wide coalesced stream on gfx950 -- MI355X_MICROARCH.md
    "HBM" -- hence 2 x FETCH + WRITE); ({}, None) when no summary of this workload is committed."""
    for rel in PMC_CSVS.get(workload, []):
        path = os.path.join(ROOT, rel)
        if not os.path.exists(path):
            continue
        vals = {}
        for line in open(path).read().splitlines()[1:]:
            k, cn, _, mean = line.split(",")
            vals.setdefault(k, {})[cn] = float(mean)
        out = {k: (2.0 * v["FETCH_SIZE"] + v["WRITE_SIZE"]) * 1024.0 for k, v in vals.items()
               if "FETCH_SIZE" in v and "WRITE_SIZE" in v}
        return out, rel
    return {}, None


EA_CSVS = {("20k", 512, 1): _prof("rocprofv3_ea_requests_b1.csv"), ("20k", 512, 8): _prof("rocprofv3_ea_requests_b8.csv")}


def sq_table(workload):
    """({kernel: {counter: mean per launch}}, file) from the committed SQ-counter passes of THIS workload."""
    import csv
    for rel in SQ_CSVS.get(workload, []):
        path = os.path.join(ROOT, rel)
        if not os.path.exists(path):
            continue
        out = {}
        for r in csv.DictReader(open(path)):
            out.setdefault(r["kernel"], {})[r["counter"]] = float(r["mean_per_launch"])
        return out, rel
    return {}, None


def geo_pipe_busy():
    """Matrix / vector / LDS pipe occupancy of the geometry decoder's kernels from the committed counter passes
    (profiles/r0N_rocprofv3_counters_geo_decode.csv, scripts/profile_r04.sh): SQ_VALU_MFMA_BUSY_CYCLES (cycles, summed over the
    SIMDs) and 4 x SQ_ACTIVE_INST_VALU (quad-cycles) over 1024 SIMDs x the launch's cycles (GRBM_GUI_ACTIVE is summed over the 8
    XCDs), LDS_IDX_ACTIVE over 256 CUs x the same."""
    import csv
    for rel in _prof("rocprofv3_counters_geo_decode.csv"):
        path = os.path.join(ROOT, rel)
        if not os.path.exists(path):
            continue
        tab = {}
        for r in csv.DictReader(open(path)):
            tab.setdefault(r["kernel"], {})[r["counter"]] = float(r["mean_per_launch"])
        out = {}
        for k, c in tab.items():
            if "GRBM_GUI_ACTIVE" not in c or not c.get("SQ_INSTS_MFMA"):
                continue
            cyc = c["GRBM_GUI_ACTIVE"] / 8.0
            # _ZN3geo13k_geo_gemm256ILi9EEEvPK... -> k_geo_gemm256<9>
            name = "k_geo" + k.split("k_geo", 1)[1].split("EPK")[0].split("ILi")[0] + (("<" + k.split("ILi")[1].split("E")[0] + ">") if "ILi" in k else "")
            out[name] = {"mfma_busy_frac": round(c.get("SQ_VALU_MFMA_BUSY_CYCLES", 0.0) / (1024 * cyc), 3),
                         "valu_busy_frac": round(4 * c.get("SQ_ACTIVE_INST_VALU", 0.0) / (1024 * cyc), 3),
                         "lds_busy_frac": round(c.get("SQ_LDS_IDX_ACTIVE", 0.0) / (256 * cyc), 3),
                         "wait_frac": round(c["SQ_WAIT_ANY"] / c["SQ_WAVE_CYCLES"], 3) if c.get("SQ_WAVE_CYCLES") else None}
        return out, rel
    return {}, None


def valu_roofline(sq, kernel_ms, images):
    """The vector-ALU side of the roofline, per kernel: busy SIMD cycles of one launch (SQ_ACTIVE_INST_VALU counts quad-cycles
    in which a VALU instruction issues, x 4) over the SIMD cycles the chip offers during the launch's LIVE duration (1024
    SIMDs at the 2.4 GHz peak clock), and the wave-instruction counts behind them.  The counters come from the committed
    profile of the same workload (a profiled launch runs the same instructions), the durations from this run."""
    out = {}
    for k, ms in kernel_ms.items():
        c = sq.get(k)
        if not c or "SQ_ACTIVE_INST_VALU" not in c or ms <= 0:
            continue
        busy = 4.0 * c["SQ_ACTIVE_INST_VALU"]
        out[k] = {"valu_wave_instructions": round(c.get("SQ_INSTS_VALU", 0.0)), "valu_busy_simd_cycles": round(busy),
                  "valu_frac": busy / (ms * 1e-3 * VALU_PEAK_CYCLES_PER_S), "wait_frac": (c["SQ_WAIT_ANY"] / c["SQ_WAVE_CYCLES"]) if c.get("SQ_WAVE_CYCLES") else None}
    return out


def ea_table(workload):
    """({kernel: HBM bytes per launch}, file) from the L2's memory-side request counters BY SIZE CLASS -- 32 x RDREQ_32B +
    64 x RDREQ_64B + 128 x RDREQ_128B read, 64 x WRREQ_64B + 32 x (WRREQ - WRREQ_64B) written (atomics are 32-byte write
    requests) -- of the committed passes of THIS workload; ({}, None) without one.  The derived FETCH_SIZE tallies gfx950's
    128-byte requests at 64 (hence the guide's factor 2, which over-charges the 64-byte ones); the size classes need no
    correction: `scripts/micro/ea_calib.hip` reads / writes 1 GiB in five access shapes and the classes add up to the byte
    count to 0.003 % (profiles/r03_ea_calibration.csv).  Reported BESIDE the guide's figure, never instead of it."""
    for rel in EA_CSVS.get(workload, []):
        path = os.path.join(ROOT, rel)
        if not os.path.exists(path):
            continue
        vals = {}
        for line in open(path).read().splitlines()[1:]:
            k, cn, _, mean = line.split(",")
            vals.setdefault(k, {})[cn] = float(mean)
        need = ("TCC_EA0_RDREQ_32B_sum", "TCC_EA0_RDREQ_64B_sum", "TCC_EA0_RDREQ_128B_sum", "TCC_EA0_WRREQ_sum", "TCC_EA0_WRREQ_64B_sum")
        out = {}
        for k, v in vals.items():
            if all(n in v for n in need):
                out[k] = (32.0 * v["TCC_EA0_RDREQ_32B_sum"] + 64.0 * v["TCC_EA0_RDREQ_64B_sum"] + 128.0 * v["TCC_EA0_RDREQ_128B_sum"]
                          + 64.0 * v["TCC_EA0_WRREQ_64B_sum"] + 32.0 * (v["TCC_EA0_WRREQ_sum"] - v["TCC_EA0_WRREQ_64B_sum"]))
        return out, rel
    return {}, None


def dominant_from_kernel_stats(names, workload):
    """(longest step kernel by mean duration, file) in the committed rocprofv3 kernel trace of this workload, (None, None)
    without one.  Reported BESIDE the live choice (`dominant_by_trace`), it never replaces it."""
    import csv
    for rel in KSTATS_CSVS.get(workload, []):
        path = os.path.join(ROOT, rel)
        if not os.path.exists(path):
            continue
        best, best_ns = None, 0.0
        for row in csv.DictReader(open(path)):
            k = row["Name"].replace("void ", "").split("(")[0].split("<")[0]
            if k in names and float(row["AverageNs"]) > best_ns:
                best, best_ns = k, float(row["AverageNs"])
        return best, rel
    return None, None


def pick_spg(steps, cap=0):
    spg = 1
    for cand in (50, 25, 20, 10, 5):
        if steps % cand == 0:
            spg = cand
            break
    return min(spg, cap) if cap > 0 else spg


def make_runner(E, torch, scenes, n_streams, dev, cfg, spg, graph=True, joint=False, tail=0, **kw):
    """tail > 1: one more hipGraph per stream of `tail` iterations, replayed for a chunk whose last `tail` iterations do not
    fill a graph of `spg` (instead of `tail` single-iteration replays)."""
    group = E.GuidanceGroup(scenes, n_streams, device=dev, **kw)
    tails = []
    if graph:
        group.capture(cfg, joint=joint, steps_per_graph=spg)
        if not joint and spg > 1 and tail > 1:
            for gb, st in zip(group.batches, group.streams):
                with torch.cuda.stream(st):
                    tails.append(gb.capture(cfg, steps_per_graph=tail))
            torch.cuda.synchronize(dev)
    ident = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0] * 2, dtype=torch.float32, device=dev)  # PL:1207-1215

    state = {"it": 0}
    window = max(spg, 1) * max(1, round(50 / max(spg, 1)))     # 50 iterations, or the multiple of the graph length next to it

    def run_steps(n):
        """Every CFG.joint_iters = 50 iterations the reference starts a new denoising step with a fresh AdamW
        (PL:1478).  The pose parameters are put back to the scene's start point as well, so that the measured
        workload stays the configs[1] scene instead of whatever the synthetic optimisation drifts to (with the
        reference's learning rates the synthetic object shrinks away after ~150 iterations, which would make the
        rasteriser's job easier than the benchmark claims).  The windows (50 iterations, 40 when the graphs hold 20) run
        across calls: a timed region of 20 iterations holds a restart in every second repeat, not in every one."""
        done = 0
        while done < n:
            if state["it"] % window == 0:
                group.restart(ident)
            k = min(window - state["it"] % window, n - done)
            if tails and k % spg == tail:
                group.run(cfg, k - tail)
                for g, st in zip(tails, group.streams):
                    with torch.cuda.stream(st):
                        g.replay()
            else:
                group.run(cfg, k)
            done += k
            state["it"] += k

    run_steps.realign = lambda: state.update(it=0)     # the next call starts a window (with a restart)
    run_steps.window = window
    return group, run_steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--images-per-gpu", type=int, default=1)
    ap.add_argument("--streams", type=int, default=0, help="independent image groups, one HIP stream + hipGraph each "
                    "(0 = auto: min(4, images per GPU))")
    ap.add_argument("--obj", default="20k", choices=["ico4", "20k", "40k"])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--joint-graph", action="store_true", help="one hipGraph with a branch per stream instead of one graph "
                    "per stream (measured slower on ROCm 7.2)")
    ap.add_argument("--steps-per-graph", type=int, default=0, help="cap on the iterations captured per hipGraph (0 = auto)")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the batched / topology_changing sub-records")
    ap.add_argument("--cpu-steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=None, help="repeats of the timed region (0 = as many as it takes to measure "
                    f"{MIN_TIMED_S} s; the median repeat is reported).  Default: 1, with --full 0")
    ap.add_argument("--gbuf-f16", action="store_true", help="depth / colour planes of the G-buffer in fp16 (configs[4])")
    ap.add_argument("--full", action="store_true", help="measure beyond the headline figure: repeated timed regions, per-kernel "
                    "roofline, side records (unless --no-extras), CPU baseline and parity (unless --no-cpu-baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step left for its caller (rank 0's images) "
                    "as DIR/<name>.npy, float32 / float64")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 0 if args.full else 1

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))          # plain `python bench.py --gpus N`: this process becomes the launcher

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    if world != args.gpus:
        # a line that says n_gpus = world while the caller asked for --gpus N would be a mislabelled measurement
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU "
                         f"(`python bench.py --gpus {args.gpus}` does it by itself)")
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    # FOHO_BENCH_BACKEND=gloo lets the N>1 code path be exercised with several ranks on ONE GPU (development aid);
    # the driver's multi-GPU runs use RCCL ("nccl") with one rank per GPU.
    backend = os.environ.get("FOHO_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank %= torch.cuda.device_count()
    elif local_rank >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: rank {rank} wants GPU {local_rank} but this node shows {torch.cuda.device_count()} "
                         "(one rank per GPU over RCCL; FOHO_BENCH_BACKEND=gloo shares GPUs for plumbing tests)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    # FOHO_BENCH_FORCE_DIST=1: join a process group even as the only rank, so that the RCCL branch of this file (init with
    # a device id, barriers, device-side all-reduces) runs on a one-GPU box too (tests/test_bench_gpu.py)
    if world > 1 or os.environ.get("FOHO_BENCH_FORCE_DIST") == "1":
        import torch.distributed as dist_
        dist = dist_
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    from followmyhold_amd import engine as E
    from followmyhold_amd import synthetic
    from followmyhold_amd import sharding

    H = W = args.size
    ipg = args.images_per_gpu
    render_fn = E.hip_render_fn(dev)
    # image-sharded: global image index = rank * ipg + j (seed per image)
    scenes = [synthetic.build_scene(render_fn, obj_kind=args.obj, H=H, W=W, seed=rank * ipg + j) for j in range(ipg)]
    # measured (8 images: 1 / 2 / 4 / 8 streams = 38 / 48 / 58 / 40 k steps/s): up to four independent groups overlap well
    n_streams = args.streams if args.streams > 0 else min(4, ipg)
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=True)
    # iterations per hipGraph: the reference's inner loop is 50 iterations per denoising step, and nothing in the step
    # needs the host, so a slice of that loop is ONE graph replay (no host work between iterations)
    spg = 1 if (args.no_graph or args.joint_graph) else pick_spg(args.steps, args.steps_per_graph)
    # the timed path ends with a restart and ONE iteration (run_timed): the K - 1 before it leave (K - 1) % spg iterations
    # after their last full graph, replayed as one graph of their own
    group, run_steps = make_runner(E, torch, scenes, n_streams, dev, cfg, spg, graph=not args.no_graph, joint=args.joint_graph,
                                   tail=(args.steps - 1) % spg if spg > 1 else 0, gbuf_f16=args.gbuf_f16)
    gb = group.batches[0]

    run_steps(50)            # setup: let clocks / caches settle before the counted warm-up
    torch.cuda.synchronize(dev)

    run_steps(args.warmup)
    torch.cuda.synchronize(dev)

    def run_timed(n):
        """The timed path: n iterations in the 50-iteration windows of the workload, each window starting with a restart
        (scene start point, fresh AdamW), the LAST iteration in a window of its own.  Its inputs are then the same in every
        run: the float atomics of k_pix_bwd leave ~1e-7 of run-to-run noise per iteration, which the
        optimisation at the reference's learning rates amplifies to O(1) within ~10 iterations of a restart, so what the
        last iteration of a longer window computes would differ from run to run."""
        run_steps.realign()
        run_steps(n - 1)
        run_steps.realign()
        run_steps(1)

    def timed_region():
        """EXACTLY args.steps iterations between barrier + synchronize on both sides; max over ranks."""
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        run_timed(args.steps)
        torch.cuda.synchronize(dev)
        if dist is not None:
            dist.barrier()
        dt_ = time.perf_counter() - t0
        tm = torch.tensor([dt_], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        if dist is not None:
            dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        return float(tm.item())

    # A plain run times the region once: --steps is the number of timed iterations.  With --full (or --repeats 0), a short
    # --steps (the driver's 20) is a ~1 ms region -- two graph replays, at the mercy of one scheduling hiccup -- so the
    # region is repeated until MIN_TIMED_S has been measured and the MEDIAN repeat is reported; every repeat is the
    # contract's region (K steps, barriers, max over ranks), `steps` stays K.  The repeat count follows from the first
    # repeat's all-reduced time, so every rank arrives at the same number.
    times = [timed_region()]
    n_rep = int(min(200, max(1, -(-MIN_TIMED_S // max(times[0], 1e-6))))) if args.repeats <= 0 else args.repeats
    while len(times) < n_rep:
        times.append(timed_region())
    dt = float(np.median(times))
    # end-of-batch metrics all-reduce (the only collective of the path)
    metrics = sum(sharding.local_metrics(g, n_steps=args.steps * len(times), wall_ms=sum(times) * 1e3 if i == 0 else 0.0)
                  for i, g in enumerate(group.batches))
    if dist is not None:
        if backend != "nccl":
            metrics = metrics.cpu()
        metrics = sharding.all_reduce_metrics(metrics, dist)
    for g in group.batches:
        g.raise_on_flags()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, group, np)      # before anything below runs another step

    m0 = gb.meta[0]
    value = world * ipg * args.steps / dt
    out = {
        "metric": "guidance-steps/sec (512x512, 778+20k verts)", "value": value, "unit": "guidance-steps/s",
        "n_gpus": world, "rccl_ranks": (dist.get_world_size() if dist is not None else 1), "collective_backend": backend if dist is not None else None,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt * 1e3 / args.steps,
        "repeats": len(times), "ms_per_step_min_max": [min(times) * 1e3 / args.steps, max(times) * 1e3 / args.steps],
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32" if not args.gbuf_f16 else "f32 (G-buffer f16)",
        "data": "synthetic",
        "config": {"workload": f"configs[1]: single {H}x{W} synthetic frame per GPU, {m0['Vh']}-vert hand + "
                               f"{m0['Vo']}-vert/{m0['Fo']}-face object, joint guidance step (phase C)",
                   "images_per_gpu": ipg, "global_images": world * ipg, "parallelism": f"image-sharded x{world}",
                   "hip_graph": not args.no_graph, "steps_per_graph": spg, "streams": len(group.batches),
                   "restart_every": run_steps.window},
        "final_loss_mean": float(metrics[2] / max(metrics[0], 1.0)), "nan_images": int(metrics[sharding.IDX["n_nan"]]),
        "metrics": {k: float(v) for k, v in zip(sharding.METRIC_NAMES, metrics.tolist())},
    }

    if rank == 0:
        if args.full:
            sizes = (H, W, m0["Vh"], m0["Vo"], m0["Fh"], m0["Fo"])
            # ---- roofline of the dominant kernel: hipEvents around every launch, averaged over the timed step count
            acc, samples = {}, {}
            nprof = 100
            run_steps(25)            # profile in the middle of a 50-iteration window
            torch.cuda.synchronize(dev)
            cfg_frozen, _ = E.phase_cfg("C", denoise_i=19, do_update=False)
            for _ in range(nprof):      # timed the way the iterations run inside the multi-iteration graphs (deferred final stage)
                for k, v in gb.step_profiled(cfg_frozen, deferred=spg > 1).items():
                    acc[k] = acc.get(k, 0.0) + v / nprof
                    samples.setdefault(k, []).append(v)
            # hit statistics of the profiled scene (the G-buffer is hit-only): hit pixels and pixels of 32x8 tiles with a hit
            P = H * W
            p2f = gb.region("p2f", torch.int32, (2, gb.B, H, W))[:, 0]
            hits = {"px": [int((p2f[r] >= 0).sum()) for r in range(2)], "tile_px": []}
            for r in range(2):
                t = (p2f[r] >= 0)[: H // 8 * 8, : W // 32 * 32].reshape(H // 8, 8, W // 32, 32).any(3).any(1)
                hits["tile_px"].append(int(t.sum()) * 256)
            # the dominant kernel is picked LIVE, by the MEDIAN of the profiled launches (one disturbed launch in the sample must
            # not change which kernel the record is about); the roofline figures use the mean, as the contract asks.  What the
            # committed rocprofv3 kernel trace of the same workload says is reported beside it (`dominant_by_trace`): event
            # timing adds ~3 us per launch and reads k_pix_bwd high in about one process out of six, so the two can differ -- the
            # record says so instead of hiding it.
            med = {k: float(np.median(v)) for k, v in samples.items()}
            dom = max(med, key=lambda k: med[k])
            workload = (args.obj, args.size, gb.B)       # object, image size, images per LAUNCH (the profiled batch)
            prof_dom, prof_src = dominant_from_kernel_stats(set(acc), workload)
            kb = kernel_bytes(dom, *sizes, hits=hits)
            bstep = algorithmic_bytes(*sizes)
            if kb is None:
                kb = bstep
            ipb = gb.B               # images in the profiled batch (the first stream's)
            achieved = kb * ipb / (acc[dom] * 1e-3) / 1e9
            pmc, pmc_src = pmc_table(workload)
            ea, ea_src = ea_table(workload)
            out["roofline"] = {"bound": "hbm", "roof": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": achieved / HBM_PEAK_GBS, "traffic": pmc.get(dom),
                               "traffic_source": f"{pmc_src} (2*FETCH_SIZE+WRITE_SIZE, KiB)" if pmc_src else None,
                               "traffic_by_request_size": ea.get(dom), "traffic_by_request_size_source": ea_src,
                               "kernel_ms": acc[dom], "kernel_ms_median": med[dom], "algorithmic_bytes_per_launch": kb * ipb,
                               "dominant_by_trace": prof_dom, "trace_source": prof_src}
            sq, sq_src = sq_table(workload)
            vr = valu_roofline(sq, acc, ipb)
            if vr:
                tot_busy = sum(v["valu_busy_simd_cycles"] for v in vr.values())
                out["roofline_valu"] = {"bound": "valu-issue", "kernel": dom, "frac": vr.get(dom, {}).get("valu_frac"), "kernels": vr,
                                        "step_valu_wave_instructions": sum(v["valu_wave_instructions"] for v in vr.values()),
                                        "step_valu_frac": tot_busy / ipb * value / world / VALU_PEAK_CYCLES_PER_S, "source": sq_src,
                                        "peak": "1024 SIMDs x 2.4 GHz busy cycles/s (SQ_ACTIVE_INST_VALU x 4 per launch / live duration)"}
                hb, vf = out["roofline"]["frac"], vr.get(dom, {}).get("valu_frac") or 0.0
                # what binds: neither roof is near at one image per launch -- the kernels wait (wait_frac) on chains of dependent
                # round trips; the record says so instead of letting "bound": "hbm" stand alone
                # `bound` names what binds: at one image per launch neither roof does (the HBM figures are quoted against `roof`)
                if hb < 0.25 and vf < 0.5:
                    out["roofline"]["bound"] = "latency"
                elif vf >= 0.5:
                    out["roofline"]["bound"] = "valu-issue"
                out["roofline"]["binding"] = (f"latency: {dom} uses {hb:.3f} of the HBM roof and {vf:.3f} of the VALU-issue roof, "
                                              f"its waves wait {vr.get(dom, {}).get('wait_frac') or 0:.2f} of their life (SQ_WAIT_ANY)")
            out["kernel_ms"] = {k: round(v, 5) for k, v in acc.items()}
            out["kernel_ms_median"] = {k: round(v, 5) for k, v in med.items()}
            out["hit_pixels"] = hits
            out["kernels"] = {}
            for k, v in acc.items():           # every launch of the step against the HBM roofline (algorithmic bytes / duration)
                kbk = kernel_bytes(k, *sizes, hits=hits) or 0
                gbs = kbk * ipb / (v * 1e-3) / 1e9
                out["kernels"][k] = {"ms": round(v, 5), "algorithmic_MB": round(kbk * ipb / 1e6, 3), "GBs": round(gbs, 1),
                                     "frac": round(gbs / HBM_PEAK_GBS, 4),
                                     "traffic_MB": round(pmc[k] / 1e6, 3) if k in pmc else None,
                                     "traffic_by_request_size_MB": round(ea[k] / 1e6, 3) if k in ea else None}
            out["step_hbm_GBs"] = bstep * value / world / 1e9  # whole-step algorithmic bytes x steps/s per GPU
            out["step_roofline_frac"] = out["step_hbm_GBs"] / HBM_PEAK_GBS
            if pmc:
                step_traffic = sum(pmc.get(k, 0.0) for k in acc)
                out["step_traffic_MB"] = round(step_traffic / 1e6, 3)
                out["step_traffic_frac"] = step_traffic * value / world / 1e9 / HBM_PEAK_GBS

            if world == 1 and not args.no_extras:
                # side records: a failure in one of them (a raised step flag, say) is reported in its place and must not cost
                # the headline line above
                for key, fn in (("batched", lambda: batched_record(E, torch, synthetic, render_fn, args, dev, cfg)),
                                ("batched_f16_gbuffer", lambda: batched_record(E, torch, synthetic, render_fn, args, dev, cfg, gbuf_f16=True)),
                                ("topology_changing", lambda: topology_record(E, torch, scenes[0], dev)),
                                ("closeup", lambda: closeup_record(E, torch, np, synthetic, render_fn, args, dev, cfg)),
                                ("obj_40k", lambda: obj40k_record(E, torch, synthetic, render_fn, args, dev, cfg)),
                                ("geo_decode", lambda: geo_decode_record(torch, dev)),
                                ("vae_attention", lambda: vae_attention_record(torch, dev)),
                                ("vae_transformer", lambda: vae_transformer_record(torch, dev)),
                                ("icp", lambda: icp_record(torch, np, dev)),
                                ("lbs", lambda: lbs_record(torch, np, synthetic, dev)),
                                ("pipeline_iteration", lambda: pipeline_iteration_record(E, torch, scenes[0], dev)),
                                ("final_decode", lambda: final_decode_record(torch, np, dev)),
                                ("job", lambda: job_record(E, torch, synthetic, render_fn, args, dev)),
                                ("driver_on_files", lambda: driver_record(E, torch, np, synthetic, render_fn, args))):
                    try:
                        out[key] = fn()
                    except Exception as e:  # noqa: BLE001
                        out[key] = {"error": f"{type(e).__name__}: {e}"}
            if world == 1 and not args.no_cpu_baseline:
                base, first = cpu_baseline(scenes[0], args.cpu_steps)
                out["cpu_baseline"] = base
                out["parity"] = parity_record(E, torch, np, scenes[0], dev, first)
                out["cpu_baseline_1t"] = cpu_baseline(scenes[0], 5, threads=1, budget_s=20.0)[0]
        emit(out)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(d, group, np):
    """--dump-outputs: what the last timed step left for the caller of the step, per image of this rank in batch order --
    pose parameters (B, 16), loss terms (B, N_LOSS), parameter gradient (B, 16), AdamW moments and step count, flag words
    and the gradient of every input vertex (Vtot, 3) -- as d/<name>.npy, float32 (integers as float64, exact).  The inputs
    are the seeded synthetic scenes and the last timed iteration starts from a restart (run_timed), so two runs with the
    same arguments write the same arrays up to the ~1e-7 float-atomic noise of one backward.  Past DUMP_MAX_BYTES in all,
    grad_verts_in keeps a fixed, seeded sample of its rows (their indices in grad_verts_rows)."""
    def cat(name):
        return np.concatenate([getattr(gb, name).detach().cpu().numpy() for gb in group.batches], 0)
    arrays = {"params": cat("params"), "losses": cat("losses"), "grad_params": cat("grad_params"), "adam_m": cat("adam_m"),
              "adam_v": cat("adam_v"), "adam_t": cat("adam_t").astype(np.float64), "flags": cat("flags").astype(np.float64),
              "grad_verts_in": cat("grad_verts_in")}
    g = arrays["grad_verts_in"]
    room = DUMP_MAX_BYTES - sum(a.nbytes for k, a in arrays.items() if k != "grad_verts_in")
    if g.nbytes > room:
        rows = np.sort(np.random.default_rng(0).choice(len(g), room // (g[0].nbytes + 8), replace=False))
        arrays["grad_verts_in"], arrays["grad_verts_rows"] = g[rows], rows.astype(np.float64)
    os.makedirs(d, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(d, k + ".npy"), a)


def _r(x, nd=4):
    return None if x is None else float(f"{float(x):.{nd}g}")


def headline(out):
    """The ONE stdout line: the contract's fields, `roofline` (the dominant kernel + `secondary`: the side records' headline numbers),
    `cpu_baseline`, `parity` -- short enough (< 1 900 characters) to survive in a 2 000-character log tail."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
    line = {k: out[k] for k in keep if k in out}
    line["value"], line["ms_per_step"] = _r(out["value"], 6), _r(out["ms_per_step"], 5)
    c = out["config"]
    line["config"] = {"workload": "configs[1]: 512x512 frame/GPU, 778-vert hand + 10242-vert/20480-face object, joint step (phase C)"
                      if "10242-vert/20480-face" in c["workload"] and "512x512" in c["workload"] else c["workload"],
                      "images_per_gpu": c["images_per_gpu"], "global_images": c["global_images"], "parallelism": c["parallelism"],
                      "steps_per_graph": c["steps_per_graph"]}
    line["repeats"], line["rccl_ranks"] = out.get("repeats"), out.get("rccl_ranks")
    rf = out.get("roofline")
    if rf:
        r2 = {k: rf.get(k) for k in ("bound", "roof", "kernel", "unit")}
        r2.update(achieved=_r(rf["achieved"]), peak=rf["peak"], frac=_r(rf["frac"]), traffic=rf.get("traffic"), kernel_us=_r(rf["kernel_ms"] * 1e3),
                  alg_bytes=rf.get("algorithmic_bytes_per_launch"))
        if "roofline_valu" in out:
            r2["valu_frac"] = _r(out["roofline_valu"].get("frac"), 3)
        sec = {}
        def get(d, *path):
            for k in path:
                d = d.get(k) if isinstance(d, dict) else None
            return d
        g = out.get("geo_decode") or {}
        if "fwd_ms" in g:
            sec["geo_decode"] = {"fwd_ms": _r(g["fwd_ms"]), "mfma_frac": _r(get(g, "roofline", "frac"), 3), "fwd_bwd_rows_ms": _r(g.get("fwd_bwd_rows_ms")),
                                 "fwd_bwd_dense_ms": _r(g.get("fwd_bwd_ms"))}
        pi = out.get("pipeline_iteration") or {}
        if "hip_transformer" in pi:
            sec["pipeline_iteration"] = {"ms": _r(get(pi, "hip_transformer", "iteration_ms")), "bwd_ms": _r(get(pi, "hip_transformer", "backward_ms")),
                                         "torch_vae_ms": _r(get(pi, "hip_decoder", "iteration_ms")), "torch_ms": _r(get(pi, "torch_decoder", "iteration_ms")),
                                         "active_rows": _r(pi.get("active_row_frac"), 3), "b4_ms": _r(get(pi, "batch_of_4", "iteration_ms"))}
        vt = out.get("vae_transformer") or {}
        if "fwd_ms" in vt:
            sec["vae_transformer"] = {k: _r(vt.get(k), 3) for k in ("fwd_ms", "bwd_ms", "mfma_frac", "torch_fwd_bwd_ms", "b4_fwd_bwd_ms")}
        fd0 = out.get("final_decode") or {}
        if "hip_transformer" in pi and "latent2sdf_ms" in fd0 and "phase_a_step_ms" in pi:
            # what ONE IMAGE costs on the path (CFG:12-18, PL:1269-1662; stand-in networks; the DiT's 20 forwards are not part of it): 550 inner
            # iterations through latent2sdf (100 of phase B + 9 x 50 of phase C), 200 of phase A, 19 no-gradient decodes on the 65^3 grid, the last
            # decode on 385^3 -- every term measured in this run
            sec["image_s"] = _r((550 * pi["hip_transformer"]["iteration_ms"] + 200 * pi["phase_a_step_ms"] + 19 * pi["step_decode_nograd_ms"]
                                 + fd0["latent2sdf_ms"] + fd0["flexicubes_ms"]) / 1e3, 4)
        cu = out.get("closeup") or {}
        if "one_image" in cu:
            sec["closeup"] = {"b1": _r(get(cu, "one_image", "value")), "b32": _r(get(cu, "in_flight_32", "value"))}
        if "value" in (out.get("batched") or {}):
            sec["batched_b8"] = _r(out["batched"]["value"])
        if "value" in (out.get("obj_40k") or {}):
            sec["obj_40k"] = _r(out["obj_40k"]["value"])
        if "ms_per_step" in (out.get("topology_changing") or {}):
            sec["topology_ms"] = _r(out["topology_changing"]["ms_per_step"])
        jb = out.get("job") or {}
        if "in_flight_16" in jb:
            sec["job_img_s"] = {k.replace("in_flight_", "f"): _r(v["images_per_s"], 3) for k, v in jb.items() if k.startswith("in_flight_")}
        if "images_per_s" in (out.get("driver_on_files") or {}):
            sec["driver_img_s"] = _r(out["driver_on_files"]["images_per_s"], 3)
        fd = out.get("final_decode") or {}
        if "latent2sdf_ms" in fd:
            sec["final_decode_ms"] = _r(fd["latent2sdf_ms"] + fd["flexicubes_ms"])
        ic = out.get("icp") or {}
        if "hip_ms" in ic:
            sec["icp"] = {"ms": _r(ic["hip_ms"]), "cpu_ms": _r(ic.get("cpu_ms_extrapolated"))}
        va = out.get("vae_attention") or {}
        if "torch_efficient" in va:
            sec["vae_attn_fb_us"] = {k.replace("torch_", ""): _r(get(va, k, "forward_backward_us"), 3) for k in ("torch_default", "torch_efficient", "hip")}
        lb = out.get("lbs") or {}
        if "b8192" in lb:
            sec["lbs"] = {"b1_us": _r(get(lb, "b1", "fwd_bwd_us")), "b8192_frac": _r(get(lb, "b8192", "poseblend_frac_of_fp32_matrix_peak"), 3)}
        for k in ("geo_decode", "vae_transformer", "pipeline_iteration", "final_decode", "closeup", "batched", "obj_40k", "topology_changing", "job", "driver_on_files", "icp", "lbs", "vae_attention"):
            if isinstance(out.get(k), dict) and "error" in out[k]:
                sec[k] = {"error": out[k]["error"][:60]}
        if sec:
            r2["secondary"] = sec
        line["roofline"] = r2
    cb = out.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {"value": _r(cb["value"]), "unit": cb["unit"], "cores": cb["cores"], "kind": cb["kind"],
                                "sample": cb["sample"].split(" of the same")[0] + " of the same scene, oracle/step_ref.py"}
        if "cpu_baseline_1t" in out:
            line["cpu_baseline"]["value_1_thread"] = _r(out["cpu_baseline_1t"]["value"])
    pr = out.get("parity")
    if pr:
        line["parity"] = {"loss_rel_err": _r(pr["loss_rel_err_vs_oracle"], 2), "p2f_mismatch": pr["pix_to_face_mismatch"]}
    return line


def emit(out):
    """Detail record -> stderr (one line) and gpurun_out/bench_detail.json; headline -> stdout, the contract's ONE JSON line."""
    detail = json.dumps(out)
    print("bench-detail: " + detail, file=sys.stderr, flush=True)
    try:
        d = os.path.join(ROOT, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "bench_detail.json"), "w") as f:
            f.write(detail + "\n")
    except OSError:
        pass
    line = json.dumps(headline(out), separators=(",", ":"))
    print(line, flush=True)


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: re-run this command as N ranks, one per GPU, under
    torch.distributed.run (rendezvous on 127.0.0.1, a free port) and return its exit status.  The reference's analogue is
    one SLURM array task per chunk of the image list (src/foho/guidance/run.py:178-185)."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # RCCL needs dmabuf IPC on this stack
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def valu_record(args, image_steps_per_s):
    """Share of the chip's vector-ALU issue slots a rate of image-steps/s needs: SQ counters of ONE 8-image launch sequence
    (SQ_ACTIVE_INST_VALU x 4 = busy SIMD cycles, committed under profiles/) against 1024 SIMDs at the 2.4 GHz peak clock."""
    if (args.obj, args.size) != ("20k", 512):
        return {}
    sq, rel = sq_table((args.obj, args.size, 8))
    busy = sum(4.0 * sq[k].get("SQ_ACTIVE_INST_VALU", 0.0) for k in STEP_KERNELS if k in sq)
    insts = sum(sq[k].get("SQ_INSTS_VALU", 0.0) for k in STEP_KERNELS if k in sq)
    if busy <= 0:
        return {}
    per_kernel = {k: round(sq[k].get("SQ_INSTS_VALU", 0.0) / 8.0) for k in STEP_KERNELS if k in sq}
    return {"valu_instructions_per_image_step": round(insts / 8.0), "valu_issue_frac": busy / 8.0 * image_steps_per_s / VALU_PEAK_CYCLES_PER_S,
            "valu_instructions_per_image_step_by_kernel": per_kernel,
            "roofline_valu": {"bound": "valu-issue", "frac": busy / 8.0 * image_steps_per_s / VALU_PEAK_CYCLES_PER_S,
                              "peak": "1024 SIMDs x 2.4 GHz busy cycles/s"},
            "valu_source": f"{rel} (SQ_ACTIVE_INST_VALU x 4 busy SIMD cycles per 8-image step)"}


def batched_record(E, torch, synthetic, render_fn, args, dev, cfg, n_img=8, steps=200, gbuf_f16=False):
    """configs[2]'s per-GPU regime (64 frames image-sharded over 8 GPUs = 8 frames per GPU): 4 streams x 2 frames,
    one hipGraph of 50 iterations per stream.  gbuf_f16: configs[4]'s numeric regime (8-image batch, fp16 G-buffer planes,
    fp32 accumulation)."""
    H = W = args.size
    scenes = [synthetic.build_scene(render_fn, obj_kind=args.obj, H=H, W=W, seed=100 + j) for j in range(n_img)]
    group, run_steps = make_runner(E, torch, scenes, 4, dev, cfg, 50, gbuf_f16=gbuf_f16)
    run_steps(100)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    run_steps(steps)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    for g in group.batches:
        g.raise_on_flags()
    m = group.batches[0].meta[0]
    bstep = algorithmic_bytes(H, W, m["Vh"], m["Vo"], m["Fh"], m["Fo"])
    v = n_img * steps / dt
    rec = {"images_per_gpu": n_img, "streams": 4, "steps": steps, "gbuf_f16": bool(gbuf_f16), "value": v, "unit": "guidance-steps/s",
           "ms_per_batch_step": dt * 1e3 / steps, "step_roofline_frac": bstep * v / 1e9 / HBM_PEAK_GBS}
    # bytes actually moved per image and step in the batch regime: rocprofv3 PMC passes over ONE 8-image batch on one stream
    pmc, src = pmc_table((args.obj, args.size, 8))
    if pmc and not gbuf_f16:
        per_image = sum(pmc.get(k, 0.0) for k in STEP_KERNELS) / 8.0
        rec.update(step_traffic_MB_per_image=round(per_image / 1e6, 3), step_traffic_frac=per_image * v / 1e9 / HBM_PEAK_GBS,
                   traffic_source=src)
    # ... and the vector-ALU issue slots the step needs (the batch regime's nearer roof)
    if not gbuf_f16:
        rec.update(valu_record(args, v))
    return rec


def closeup_record(E, torch, np, synthetic, render_fn, args, dev, cfg, steps=500):
    """The reference's real input regime: its frames are 512 x 512 CROPS around hand + object (union box + 10 px, squared,
    x 1.25; src/foho/preprocess/segment_hoi_sam2.py:108-124, 180-196 -> synthetic.hoi_crop), so the meshes fill the frame: a
    ~25 degree field of view, six times the hit pixels and five times the hit tiles of the 60-degree scene SURVEY 8(d)
    prescribes for the headline.  Same meshes, same joint step; one image (50-iteration graphs) and 32 in flight (4 streams x 8
    images, listed k_resolve); per-kernel durations of the one-image step (hipEvents, as in the headline's `kernels`)."""
    H = W = args.size
    scenes = [synthetic.build_scene(render_fn, obj_kind=args.obj, H=H, W=W, seed=400 + j, crop="hoi") for j in range(32)]
    rec = {"workload": f"{H}x{W} crop around hand + object (hoi_crop), fov {scenes[0]['fov']:.1f} deg, {args.obj} object, joint guidance step",
           "unit": "guidance-steps/s"}
    for n_img, n_streams, key in ((1, 1, "one_image"), (32, 4, "in_flight_32")):
        group, run_steps = make_runner(E, torch, scenes[:n_img], n_streams, dev, cfg, 50)
        run_steps(100)
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(3):
            run_steps.realign()
            t0 = time.perf_counter()
            run_steps(steps if n_img == 1 else 200)
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) / (steps if n_img == 1 else 200))
        for g in group.batches:
            g.raise_on_flags()
        dt = float(np.median(ts))
        rec[key] = {"value": n_img / dt, "ms_per_step": dt * 1e3, "images": n_img, "streams": n_streams}
        if n_img == 1:
            gb = group.batches[0]
            cfg_frozen, _ = E.phase_cfg("C", denoise_i=19, do_update=False)
            acc = {}
            for _ in range(50):
                for k, v in gb.step_profiled(cfg_frozen, deferred=True).items():
                    acc[k] = acc.get(k, 0.0) + v / 50
            p2f = gb.region("p2f", torch.int32, (2, gb.B, H, W))[:, 0]
            rec["hit_pixels"] = [int((p2f[r] >= 0).sum()) for r in range(2)]
            rec["hit_tiles"] = [int((p2f[r] >= 0)[: H // 8 * 8, : W // 32 * 32].reshape(H // 8, 8, W // 32, 32).any(3).any(1).sum()) for r in range(2)]
            rec["kernel_us"] = {k: round(v * 1e3, 2) for k, v in acc.items()}
        del group
    return rec


def geo_decode_record(torch, dev, res=64, reps=5):
    """SURVEY 8(f) rank 1, first half: the geometry decoder of latent2sdf (PL:292-313) at the Hunyuan3D-2 shape -- 3072 x 1024
    latent tokens, 16 heads, hidden 4096, (res+1)^3 = 274 625 query points -- forward, fp16: `foho_geo_decode_fwd` (one call,
    hand-written MFMA kernels) beside the torch module run the reference's way (35 chunks of 8000 queries through hipBLASLt /
    SDPA).  Random-initialised stand-in of that shape (no Hunyuan weights on this box); bound: the fp16 matrix peak."""
    import math
    from followmyhold_amd import standins
    from followmyhold_amd.geo_decode import HipGeoDecoder
    W, NH, NL, F = 1024, 16, 3072, 4096
    torch.manual_seed(0)
    vae = standins.StandInShapeVAE(num_latents=NL, embed_dim=64, width=W, heads=NH, layers=1, num_freqs=8)
    dec = vae.geo_decoder.to(dev).eval()
    n = (res + 1) ** 3
    axes = torch.linspace(-1.1, 1.1, res + 1)
    xyz = torch.stack(torch.meshgrid(axes, axes, axes, indexing="ij"), -1).reshape(-1, 3).to(dev)
    lat = torch.randn(1, NL, W, device=dev).half()
    flop_q = 2 * 64 * W + 2 * W * W + 4 * NL * W + 2 * W * W + 4 * W * F + 2 * W
    flops = n * flop_q + NL * (2 * W * 2 * W)
    hip = HipGeoDecoder.from_module(dec, device=dev)
    q_plain = xyz.half().float().unsqueeze(0)

    def time_fwd(q):
        out_ = hip(q, lat)
        torch.cuda.synchronize(dev)
        ts_ = []
        for _ in range(reps):
            hip._prepared = None                   # K / V projection of the tokens is part of every decode
            t0_ = time.perf_counter()
            out_ = hip(q, lat)
            torch.cuda.synchronize(dev)
            ts_.append(time.perf_counter() - t0_)
        return min(ts_), out_

    t_plain, out_plain = time_fwd(q_plain)         # foho_geo_decode_fwd: the whole chain
    # what latent2sdf runs: the grid's latent-independent half (embedding -> query_proj -> ln_1 -> c_q) cached once per grid
    # (foho_geo_prepare_queries, PL:1125-1143: the same 65^3 points for every decode) -- same kernels, logits bitwise equal
    q32 = hip.grid_queries(xyz)
    t_hip, out = time_fwd(q32)
    cached_equal = bool(torch.equal(out, out_plain))
    flops_cached = flops - n * (2 * 64 * W + 2 * W * W)
    dech = vae.geo_decoder.half()
    def torch_decode():
        outs = []
        with torch.no_grad():
            for s0 in range(0, n, 8000):
                outs.append(dech(xyz[s0:s0 + 8000].half().unsqueeze(0), lat))
        return torch.cat(outs, 1)
    ref = torch_decode()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref = torch_decode()
        torch.cuda.synchronize(dev)
        ts.append(time.perf_counter() - t0)
    t_torch = min(ts)
    err = (out.float() - ref.float()).abs().max().item()
    # forward + backward to the latent tokens (the decodes of PL:1391-1393 / 1507-1509): foho_geo_decode_fwd + foho_geo_decode_bwd
    # (which recomputes the chain) beside torch autograd through the same 35 chunks
    go = torch.randn(1, n, 1, device=dev)
    hip.backward_mode = "keep"                     # a DENSE gradient's fastest route: activations kept (18 KB per query)
    def hip_fb():
        l = lat.clone().requires_grad_(True)
        (hip(q32, l).float() * go).sum().backward()
        return l.grad
    def torch_fb():
        l = lat.clone().requires_grad_(True)
        outs = [dech(xyz[s0:s0 + 8000].half().unsqueeze(0), l) for s0 in range(0, n, 8000)]
        (torch.cat(outs, 1).float() * go).sum().backward()
        return l.grad
    fb = {}
    for name, fn, r in (("hip", hip_fb, reps), ("torch", torch_fb, 2)):
        g = fn()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(r):
            t0 = time.perf_counter()
            g = fn()
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        fb[name] = (min(ts), g.float())
    # backward flops: dX GEMMs of fc2 / fc1 / c_proj (no weight gradients) + S again, dP, dV, dK of the attention (the forward's
    # activations are kept: nothing else is recomputed)
    flops_bwd = n * (4 * W * F + 2 * W * W + 8 * NL * W)
    gerr = (fb["hip"][1] - fb["torch"][1]).abs().max().item() / fb["torch"][1].abs().max().item()
    # the gradient the guidance loop really sends back (PL:1507-1509, 1600): dL/dSDF out of the FlexiCubes backward, non-zero at the end
    # points of the crossed grid edges only -> foho_geo_decode_bwd_rows (default route): rows compacted on the device, chain recomputed
    # and back-propagated for them alone, nothing kept by the forward
    from followmyhold_amd import ops as _ops
    sdf = (-out.detach().float().reshape(-1)).clone().requires_grad_(True)
    fv, ff, _ = _ops.flexicubes(xyz, sdf, res)
    (fv * torch.randn_like(fv)).sum().backward()
    go_s = (-sdf.grad).reshape(1, n, 1)
    hip.backward_mode = "rows"
    def hip_fb_rows():
        l = lat.clone().requires_grad_(True)
        (hip(q32, l).float() * go_s).sum().backward()
        return l.grad
    g_rows = hip_fb_rows()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        g_rows = hip_fb_rows()
        torch.cuda.synchronize(dev)
        ts.append(time.perf_counter() - t0)
    t_rows = min(ts)
    row_stats = hip.last_row_stats.cpu().tolist()
    hip.backward_mode = "keep"
    l_ = lat.clone().requires_grad_(True)
    (hip(q32, l_).float() * go_s).sum().backward()
    rows_vs_dense = (g_rows.float() - l_.grad.float()).abs().max().item() / max(l_.grad.float().abs().max().item(), 1e-30)
    hip.set_kv(hip.kv_of(lat).detach())
    hip.decode_bwd_rows(q32, go_s)
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        hip.decode_bwd_rows(q32, go_s)
        torch.cuda.synchronize(dev)
        ts.append(time.perf_counter() - t0)
    t_rows_bwd = min(ts)
    # the same decode with the module laid out like hy3dgen's CrossAttentionDecoder as the released ShapeVAE configures it
    # (bias-free c_q / c_kv with K and V interleaved per head, qk_norm: LayerNorm over the head dimension of q and k, no prior)
    torch.manual_seed(1)
    dech3 = standins.Hy3dgenLayoutDecoder(W, NH, qk_norm=True).to(dev).eval()
    hip3 = HipGeoDecoder.from_module(dech3, device=dev)
    hip3.backward_mode = "keep"
    hip3.prepare_queries(q32)
    def hip3_f():
        hip3._prepared = None
        with torch.no_grad():
            return hip3(q32, lat)
    def hip3_fb():
        l = lat.clone().requires_grad_(True)
        (hip3(q32, l).float() * go).sum().backward()
    h3 = {}
    for name, fn in (("fwd_ms", hip3_f), ("fwd_bwd_ms", hip3_fb)):
        fn()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append(time.perf_counter() - t0)
        h3[name] = min(ts) * 1e3
    with torch.no_grad():
        r3 = torch.cat([dech3.half()(xyz[s0:s0 + 8000].half().unsqueeze(0), lat) for s0 in range(0, n, 8000)], 1)
    h3["max_abs_diff_vs_torch_fp16"] = (hip3_f().float() - r3.float()).abs().max().item()
    h3["logit_scale"] = r3.float().abs().max().item()
    del hip3, dech3, r3
    pipes, pipes_src = geo_pipe_busy()
    return {"fwd_uncached_ms": t_plain * 1e3, "cached_logits_bitwise_equal": cached_equal,
            "fwd_bwd_rows_ms": t_rows * 1e3, "bwd_rows_ms": t_rows_bwd * 1e3, "active_rows": row_stats[0], "active_row_frac": row_stats[0] / n,
            "rows_dropped": row_stats[1], "rows_vs_dense_grad_rel_diff": rows_vs_dense, "surface_faces": int(ff.shape[0]),
            "hy3dgen_layout_qk_norm": h3, "pipe_busy_by_kernel": pipes, "pipe_busy_source": pipes_src, "fwd_bwd_ms": fb["hip"][0] * 1e3, "torch_fwd_bwd_ms": fb["torch"][0] * 1e3, "fwd_bwd_speedup_vs_torch": fb["torch"][0] / fb["hip"][0],
            "fwd_bwd_tflops": (flops + flops_bwd) / fb["hip"][0] / 1e12, "grad_rel_diff_vs_torch_fp16": gerr,
            "queries": n, "latent_tokens": NL, "width": W, "heads": NH, "hidden": F, "dtype": "f16 (fp32 accumulate)",
            "fwd_ms": t_hip * 1e3, "torch_fwd_ms": t_torch * 1e3, "speedup_vs_torch": t_torch / t_hip, "tflop": flops_cached / 1e12,
            "tflop_uncached": flops / 1e12, "tflops": flops_cached / t_hip / 1e12, "tflops_uncached": flops / t_plain / 1e12,
            # the flops the cached forward EXECUTES (the query side's 2.3 MFLOP per row are not counted) over its duration
            "roofline": {"bound": "mfma", "achieved": flops_cached / t_hip / 1e12, "peak": 2500.0, "unit": "TFLOP/s", "frac": flops_cached / t_hip / 1e12 / 2500.0},
            "max_abs_diff_vs_torch_fp16": err, "logit_scale": ref.float().abs().max().item(),
            "backward": "fwd_bwd_ms: dense random gradient, foho_geo_decode_fwd_keep + foho_geo_decode_bwd (kept activations, 18 KB per query); "
                        "fwd_bwd_rows_ms: the FlexiCubes gradient, foho_geo_decode_fwd_cached + foho_geo_decode_bwd_rows (active rows only, nothing kept); no atomics"}


def obj40k_record(E, torch, synthetic, render_fn, args, dev, cfg, steps=1000):
    """The literal reading of the metric's "778 + 20k VERTS": the 20 160-vertex / 40 320-face torus (configs[3]'s object) with
    one hand, one image, 50-iteration graphs -- the headline line follows north_star / configs[1]'s "~20k-FACE" object."""
    H = W = args.size
    scene = synthetic.build_scene(render_fn, obj_kind="40k", H=H, W=W, seed=0)
    group, run_steps = make_runner(E, torch, [scene], 1, dev, cfg, 50)
    run_steps(100)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    run_steps(steps)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    group.batches[0].raise_on_flags()
    m = group.batches[0].meta[0]
    bstep = algorithmic_bytes(H, W, m["Vh"], m["Vo"], m["Fh"], m["Fo"])
    v = steps / dt
    return {"workload": f"single {H}x{W} frame, {m['Vh']}-vert hand + {m['Vo']}-vert/{m['Fo']}-face object", "steps": steps,
            "value": v, "unit": "guidance-steps/s", "ms_per_step": dt * 1e3 / steps, "step_roofline_frac": bstep * v / 1e9 / HBM_PEAK_GBS}


def job_record(E, torch, synthetic, render_fn, args, dev):
    """The per-image JOB behind the product entry point (`python -m foho.guidance.run` with FOHO_MESH_LEVEL_GUIDANCE=1 ->
    inputs.MeshGuidanceRunner): the reference's whole schedule -- 200 hand + 100 object + 9 x 50 joint iterations = 750 per
    image (CFG:11-13, PL:1293-1610) -- for images already in host memory, including the upload of every image set, the
    installation of its objects on the device and the export read-back; graphs are captured by a first, untimed image set
    (once per process).  Images per second and GPU at 1, 8, 16 and 32 images in flight."""
    from followmyhold_amd import inputs
    H = W = args.size
    cfg0 = E.OptimizationConfig()
    n_iter = sum(it for _, it, _ in inputs.job_schedule(cfg0))
    rec = {"iterations_per_image": n_iter, "schedule": "200 A + 100 B + 9 x 50 C", "unit": "images/s"}
    scenes = [synthetic.build_scene(render_fn, obj_kind=args.obj, H=H, W=W, seed=200 + j) for j in range(16)]
    scenes = scenes + scenes          # 32 scene dicts (16 distinct images)
    for in_flight, n_img in ((1, 4), (8, 16), (16, 32), (32, 64)):    # 32: eight images per launch, k_resolve in listed mode
        runner = inputs.MeshGuidanceRunner(cfg0, device=dev, in_flight=in_flight)
        res = runner.run(scenes[:in_flight])              # captures (untimed: once per process)
        torch.cuda.synchronize(dev)
        todo = [scenes[j % 32] for j in range(n_img)]
        t0 = time.perf_counter()
        res = runner.run(todo)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        ok = sum(1 for r in res if r["ok"])
        rec[f"in_flight_{in_flight}"] = {"images": n_img, "ok": ok, "images_per_s": n_img / dt, "ms_per_image": dt * 1e3 / n_img,
                                         "guidance_steps_per_s": n_img * n_iter / dt, "streams": runner.n_streams,
                                         "graph_captures": runner.stats["captures"], "slots_built": runner.stats["slots_built"]}
        rec[f"in_flight_{in_flight}"].update({k: v for k, v in valu_record(args, n_img * n_iter / dt).items() if k == "valu_issue_frac"})
    return rec


def pipeline_iteration_record(E, torch, scene, dev, iters=5):
    """One inner iteration of phases B / C as the real pipeline runs it (PL:1478-1601): clean latent -> ShapeVAE transformer ->
    geometry decoder on the 65^3 grid (`latent2sdf`) -> FlexiCubes -> new object installed -> fused guidance step -> backward
    through all of it to the noise prediction.  Stand-in networks of the Hunyuan3D-2 shape (3072 x 64 latents, width 1024, 16
    heads, 16 transformer layers, fp16; random weights -- no checkpoint on this box); the geometry decoder once as the torch
    module in the reference's 35 chunks of 8000 queries, once through `geo_decode.install` (cached query side, foho_geo_decode_fwd_cached;
    backward over the rows FlexiCubes sends a gradient to, foho_geo_decode_bwd_rows)."""
    import numpy as np
    from followmyhold_amd import geo_decode, pipeline as PLN, standins
    res = 64
    g = np.linspace(-1.1, 1.1, res + 1, dtype=np.float32)
    xyz = torch.from_numpy(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)).to(dev)
    scene = dict(scene)
    T = np.array(scene["T_h2m"], np.float32)
    T[:3, :3] *= 0.9 * 0.06
    scene["T_h2m"] = T
    gb = E.GuidanceBatch([scene], device=dev, obj_capacity=(32768, 65536))
    obj = E.SdfObjective(gb, xyz, res)
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=True)
    torch.manual_seed(0)
    vae = standins.StandInShapeVAE(num_latents=3072, embed_dim=64, width=1024, heads=16, layers=16, num_freqs=8).to(dev).half().eval()
    vae.requires_grad_(False)      # as GuidedShapePipeline holds its networks: the guidance optimises no weight
    lat = torch.randn(1, 3072, 64, device=dev, dtype=torch.float16)
    gsz = (res + 1, res + 1, res + 1)
    out, sdfs = {}, {}
    for name in ("torch_decoder", "hip_decoder", "hip_transformer"):
        if name == "hip_decoder":
            geo_decode.install(vae, device=dev)
        if name == "hip_transformer":      # ... and `vae(pred)` itself (PL:295) on foho_vae_fwd / foho_vae_bwd: the product's default route
            from followmyhold_amd import vae_transformer
            vae_transformer.install(vae, device=dev)
        noise = torch.zeros_like(lat).requires_grad_(True)
        def one():
            if noise.grad is not None:
                noise.grad = None
            t = {}
            torch.cuda.synchronize(dev); a = time.perf_counter()
            sdf = PLN.latent2sdf(lat + 0.1 * noise, xyz, gsz, vae, dev)
            torch.cuda.synchronize(dev); t["latent2sdf_fwd_ms"] = (time.perf_counter() - a) * 1e3; a = time.perf_counter()
            sdfs[name] = sdf.detach()
            loss = obj(sdf.reshape(1, -1), cfg)
            if name != "torch_decoder":    # what the pipeline does at its per-iteration read-back: the exact count of rows with a gradient
                PLN._bound_active_rows(vae, obj.active_rows()[0])
            torch.cuda.synchronize(dev); t["flexicubes_step_ms"] = (time.perf_counter() - a) * 1e3; a = time.perf_counter()
            loss.sum().backward()
            torch.cuda.synchronize(dev); t["backward_ms"] = (time.perf_counter() - a) * 1e3
            return t
        one(); one()
        ts = [one() for _ in range(iters)]
        rec = {k: float(np.median([x[k] for x in ts])) for k in ts[0]}
        rec["sections_sum_ms"] = sum(rec.values())       # (three device synchronisations per iteration: the sections' own clock)
        # the iteration as the pipeline's loop runs it (pipeline.latent_phase_body): nothing waits for the device but the read-back of the
        # iteration's flags / active-row count between the objective and the backward
        def loop_body():
            if noise.grad is not None:
                noise.grad = None
            sdf = PLN.latent2sdf(lat + 0.1 * noise, xyz, gsz, vae, dev)
            loss = obj(sdf.reshape(1, -1), cfg)
            rows = obj.active_rows()[0]                  # the loop's one host round trip
            if name != "torch_decoder":
                PLN._bound_active_rows(vae, rows)
            loss.sum().backward()
        loop_body()

        def batch():
            torch.cuda.synchronize(dev); a = time.perf_counter()
            for _ in range(iters):
                loop_body()
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - a) * 1e3 / iters
        # five batches of `iters` iterations, the median batch: one batch is 90 ms of wall clock with a host round trip per iteration, and
        # the same library on the same box gave 17.6 and 18.3 ms in two such batches minutes apart
        batches = [batch() for _ in range(5)]
        rec["iteration_ms"] = float(np.median(batches))
        rec["iteration_ms_batches"] = [round(b, 3) for b in batches]
        rec["grad_finite"] = bool(torch.isfinite(noise.grad).all())     # (fp16 leaf, random networks: its magnitude means nothing)
        out[name] = rec
    # ... and four images through one iteration the way GuidedShapePipeline.call_batch runs them ("batch the rank's images
    # through each kernel launch"): the VAE transformer on four latents, the decoder per image on the shared cached query side, ONE
    # replay of iso-surfacing + object install + fused step + iso-surface backward for all four, backward to the four noise predictions
    try:
        B4 = 4
        gb4 = E.GuidanceBatch([scene] * B4, device=dev, obj_capacity=(32768, 65536))
        obj4 = E.SdfObjective(gb4, xyz, res)
        lat4 = torch.randn(B4, 3072, 64, device=dev, dtype=torch.float16)
        noise4 = torch.zeros_like(lat4).requires_grad_(True)
        hip = vae.hip_geo
        def one4():
            noise4.grad = None
            torch.cuda.synchronize(dev); a = time.perf_counter()
            pred = PLN.vae_tokens(vae, (1 / vae.scale_factor) * (lat4 + 0.1 * noise4))
            sdf4 = torch.stack([-hip(hip.grid_queries(xyz), pred[b:b + 1]).view(-1).float() for b in range(B4)], 0)
            loss = obj4(sdf4, cfg)
            gb4.flags.cpu()
            PLN._bound_active_rows(vae, max(obj4.active_rows()))
            loss.sum().backward()
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - a) * 1e3
        one4(); one4()
        t4 = float(np.median([one4() for _ in range(iters)]))
        out["batch_of_4"] = {"iteration_ms": t4, "ms_per_image": t4 / B4, "vs_one_image": t4 / out["hip_transformer"]["iteration_ms"],
                             "grad_finite": bool(torch.isfinite(noise4.grad).all())}
        del gb4, obj4
    except Exception as e:  # noqa: BLE001
        out["batch_of_4"] = {"error": f"{type(e).__name__}: {e}"}
    # the decode WITHOUT gradients that closes every denoising step (PL:1613-1641: 19 of the 20 on the 65^3 grid, the last one on 385^3 --
    # `final_decode`): latent -> transformer -> decoder -> FlexiCubes, and one iteration of phase A (hand only, PL:1320-1358: no decode)
    from followmyhold_amd import ops
    def nograd():
        with torch.no_grad():
            sdf = PLN.latent2sdf(lat, xyz, gsz, vae, dev)
            ops.flexicubes(xyz, sdf[0].flatten(), res)
    nograd(); nograd()
    torch.cuda.synchronize(dev); a = time.perf_counter()
    for _ in range(3):
        nograd()
    torch.cuda.synchronize(dev)
    out["step_decode_nograd_ms"] = (time.perf_counter() - a) * 1e3 / 3
    cfgA, _ = E.phase_cfg("A", denoise_i=9, do_update=True)
    gbA = E.GuidanceBatch([scene], device=dev)
    gA = gbA.capture(cfgA, steps_per_graph=50)
    gA.replay(); torch.cuda.synchronize(dev); a = time.perf_counter()
    for _ in range(4):
        gA.replay()
    torch.cuda.synchronize(dev)
    out["phase_a_step_ms"] = (time.perf_counter() - a) * 1e3 / 200
    del gA, gbA
    nv, nf, flags = obj.status()[0]
    st_rows = vae.hip_geo.last_row_stats
    if st_rows is not None:
        out["active_rows"], out["rows_dropped"] = st_rows.cpu().tolist()
        out["active_row_frac"] = out["active_rows"] / xyz.shape[0]
    out["hip_decoder_backward_mode"] = vae.hip_geo.backward_mode
    out["faces"] = nf
    out["sdf_max_abs_diff_between_decoders"] = float((sdfs["torch_decoder"] - sdfs["hip_decoder"]).abs().max())
    out["sdf_abs_max"] = float(sdfs["torch_decoder"].abs().max())
    out["speedup"] = out["torch_decoder"]["iteration_ms"] / out["hip_transformer"]["iteration_ms"]
    out["sdf_max_abs_diff_hip_transformer"] = float((sdfs["hip_decoder"] - sdfs["hip_transformer"]).abs().max())
    out["vae_transformer_calls"] = vae.hip_transformer.calls
    out["what"] = ("latent -> 16-layer VAE transformer (torch_decoder / hip_decoder: torch; hip_transformer: foho_vae_fwd/_bwd) -> geometry decoder on 65^3 points -> FlexiCubes -> object install -> fused joint "
                   "step -> backward to the noise prediction; stand-in networks of the Hunyuan3D-2 shape, fp16")
    return out


def vae_transformer_record(torch, dev, reps=10):
    """`pred = vae(pred)` of latent2sdf (PL:295) at the Hunyuan3D-2 shape -- 3072 tokens x 1024, 16 heads of 64, hidden 4096, sixteen layers,
    qk_norm, hy3dgen's module layout (standins.Hy3dgenLayoutShapeVAE) -- forward and backward to the tokens, run in every one of the 550 inner
    iterations per image (PL:1391-1393, 1507-1509): foho_vae_fwd / foho_vae_bwd (followmyhold_amd.vae_transformer) against the torch module
    under `pipeline.vae_attention_backend()` (fp16, this package's attention forward, torch's memory-efficient backward: round 5's route).
    mfma_frac: 1.86 TFLOP forward + 2.78 TFLOP backward (dX only: GEMMs 2 x 77 GFLOP, attention 39 + 97 GFLOP per layer) / time / the
    2.5 PFLOP/s dense fp16 matrix peak."""
    from followmyhold_amd import pipeline as PLN, standins, vae_transformer
    torch.manual_seed(0)
    vae = standins.Hy3dgenLayoutShapeVAE().to(dev).half().eval().requires_grad_(False)
    tr = vae_transformer.HipVaeTransformer.from_module(vae, device=dev)
    L_, W_, F_, nl = 3072, 1024, 4096, 16
    flop_f = nl * (2 * L_ * W_ * (3 * W_ + W_ + 2 * F_) + 4 * L_ * L_ * W_)
    flop_b = nl * (2 * L_ * W_ * (3 * W_ + W_ + 2 * F_) + 10 * L_ * L_ * W_)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / reps
    rec = {"shape": "3072 tokens x 1024, 16 heads, hidden 4096, 16 layers, qk_norm", "flop_fwd": flop_f, "flop_bwd": flop_b}
    for B in (1, 4):
        lat = torch.randn(B, L_, 64, device=dev, dtype=torch.float16)
        x0 = vae.post_kl(lat).detach()
        go = torch.randn_like(x0)
        saved = [None]

        def f_keep():
            saved[0] = tr.forward_raw(x0, keep=True)[1]

        def f_b():
            tr.backward_raw(go, tr.forward_raw(x0, keep=True)[1], tuple(x0.shape))

        def t_fb():
            l = lat.clone().requires_grad_(True)
            with PLN.vae_attention_backend():
                vae(l).backward(go)
        t_f, t_fb_ = timed(f_keep), timed(f_b)
        t_t = timed(t_fb)
        k = "" if B == 1 else f"b{B}_"
        rec.update({f"{k}fwd_ms": t_f, f"{k}bwd_ms": t_fb_ - t_f, f"{k}fwd_bwd_ms": t_fb_, f"{k}torch_fwd_bwd_ms": t_t,
                    f"{k}mfma_frac": B * (flop_f + flop_b) / (t_fb_ * 1e-3) / 2.5e15, f"{k}tflops": B * (flop_f + flop_b) / (t_fb_ * 1e-3) / 1e12})
        if B == 1:
            with torch.no_grad(), PLN.vae_attention_backend():
                ref = vae(lat)
            got = tr(x0)
            rec["max_rel_diff_vs_torch_fp16"] = float((got.float() - ref.float()).abs().max() / ref.float().abs().max())
    return rec


def final_decode_record(torch, np, dev):
    """The pipeline's LAST decode (PL:1623-1642): the final latent through the VAE transformer and the geometry decoder on the dense
    385^3 grid (octree resolution 384: 57 M query points, 208 times the guidance grid, 1.9 PFLOP), then the iso-surface at resolution
    384 -- once per image, stand-in networks of the Hunyuan3D-2 shape.  The query side of a grid this size is not cached (228 GB):
    `foho_geo_decode_fwd` recomputes it per row block."""
    from followmyhold_amd import geo_decode, ops, pipeline as PLN, standins
    from followmyhold_amd.facade import generate_dense_grid_points
    torch.manual_seed(0)
    vae = standins.StandInShapeVAE(num_latents=3072, embed_dim=64, width=1024, heads=16, layers=16, num_freqs=8).to(dev).half().eval()
    vae.requires_grad_(False)
    geo_decode.install(vae)
    lat = torch.randn(1, 3072, 64, device=dev).half()
    res = 384
    b = np.array([1.1] * 3, dtype=np.float32)
    xyz_np, gsz, _ = generate_dense_grid_points(-b, b, octree_depth=5, octree_resolution=res, indexing="ij")
    xyz = torch.as_tensor(xyz_np, dtype=torch.float32, device=dev)
    best = None
    for _ in range(2):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        with torch.no_grad():
            sdf = PLN.latent2sdf(lat, xyz, gsz, vae, dev)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        v, f, _ = ops.flexicubes(xyz, sdf[0].flatten(), res)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        if best is None or t2 - t0 < best[0] + best[1]:
            best = (t1 - t0, t2 - t1)
    n = int(xyz.shape[0])
    flop = n * (4 * 3072 * 1024 + 2 * 1024 * 1024 + 4 * 1024 * 4096 + 2 * 64 * 1024 + 2 * 1024 * 1024)
    return {"grid": f"{res + 1}^3", "query_points": n, "latent2sdf_ms": best[0] * 1e3, "flexicubes_ms": best[1] * 1e3, "decoder_tflops": flop / best[0] / 1e12,
            "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "sdf_finite": bool(torch.isfinite(sdf).all()),
            "what": "VAE transformer + geometry decoder on the dense 385^3 grid + FlexiCubes at resolution 384, once per image"}


def vae_attention_record(torch, dev):
    """The self-attention of the ShapeVAE transformer inside latent2sdf (PL:295: sixteen layers over 3072 tokens, 16 heads of 64, forward
    and backward in every inner iteration) at its shape (1, 16, 3072, 64) fp16: torch's scaled_dot_product_attention on its default
    (flash) backend, on its memory-efficient backend, and this repository's kernels (followmyhold_amd.sdpa) in the two forms of
    `pipeline.vae_attention_backend()`: `hip` = the HIP forward with torch's memory-efficient backward fed from it (the pipeline's
    default), `hip_bwd` = the HIP backward kernels as well (k_geo_attn_bwd + k_geo_attn_dq) -- microseconds per layer.  The operands are
    (B, N, H, 64) tensors viewed as (B, H, N, 64), the layout the transformer's projections leave them in."""
    import torch.nn.functional as F
    from torch.nn.attention import SDPBackend, sdpa_kernel
    from followmyhold_amd import sdpa
    base = [torch.randn(1, 3072, 16, 64, device=dev, dtype=torch.float16, requires_grad=True) for _ in range(3)]
    q, k, v = (t.transpose(1, 2) for t in base)
    go = torch.randn(1, 3072, 16, 64, device=dev, dtype=torch.float16).transpose(1, 2)

    def timed(fn, n=20):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / n * 1e6

    def torch_fn(backend):
        def call():
            if backend is None:
                return F.scaled_dot_product_attention(q, k, v)
            with sdpa_kernel(backend):
                return F.scaled_dot_product_attention(q, k, v)
        return call

    rec = {"shape": "(1, 16, 3072, 64) fp16", "unit": "us per layer", "gflop_forward": 4 * 16 * 3072 * 3072 * 64 / 1e9}
    def hip_fn(route):
        def call():
            sdpa.backward_route = route
            return sdpa.attention(q, k, v)
        return call

    saved_route = sdpa.backward_route
    for name, fn in (("torch_default", torch_fn(None)), ("torch_efficient", torch_fn(SDPBackend.EFFICIENT_ATTENTION)), ("hip", hip_fn("torch")),
                     ("hip_bwd", hip_fn("hip"))):
        def fwd():
            with torch.no_grad():
                return fn()
        def fb():
            for t in base:
                t.grad = None
            fn().backward(go)
        try:
            rec[name] = {"forward_us": timed(fwd), "forward_backward_us": timed(fb)}
        except Exception as e:  # noqa: BLE001
            rec[name] = {"error": f"{type(e).__name__}: {e}"[:200]}
    # ... and a batch of four (call_batch's transformer pass): which backward should follow the HIP forward?
    base4 = [torch.randn(4, 3072, 16, 64, device=dev, dtype=torch.float16, requires_grad=True) for _ in range(3)]
    q4, k4, v4 = (t.transpose(1, 2) for t in base4)
    go4 = torch.randn(4, 3072, 16, 64, device=dev, dtype=torch.float16).transpose(1, 2)
    rec["b4"] = {}
    for name, route in (("hip", "torch"), ("hip_bwd", "hip")):
        def fb4():
            for t in base4:
                t.grad = None
            sdpa.backward_route = route
            sdpa.attention(q4, k4, v4).backward(go4)
        try:
            rec["b4"][name] = {"forward_backward_us": timed(fb4, n=10)}
        except Exception as e:  # noqa: BLE001
            rec["b4"][name] = {"error": f"{type(e).__name__}: {e}"[:200]}
    sdpa.backward_route = saved_route
    rec["hip_backward_by_torch_refused"] = bool(sdpa._torch_route_refused)
    with torch.no_grad():
        ref = torch_fn(SDPBackend.MATH)().float()
        rec["hip_max_abs_diff_vs_torch_math"] = float((sdpa.attention(q, k, v).float() - ref).abs().max())
    return rec


def icp_record(torch, np, dev):
    """the two-stage trimmed ICP with scale of `foho.alignment.h2m` at the reference's sizes (mesh_align.py:56-175,
    h2m.py:12-21: coarse 50 iterations x 1000 source x 5000 target points, fine 100 x 5000 x 10000, 20 % outliers, scale in
    [0.7, 3]) -- `foho_icp_run_batch`, device-resident float64 loop, one enqueue + one synchronisation per stage -- beside the numpy
    restatement (oracle/icp_ref.py) timed on a bounded number of iterations of the same point sets."""
    from followmyhold_amd import ops
    from oracle import icp_ref
    rng = np.random.default_rng(0)
    def cloud(n):
        p = rng.normal(size=(n, 3))
        p /= np.linalg.norm(p, axis=1, keepdims=True)
        return p * np.array([1.0, 0.7, 0.5]) + 0.01 * rng.normal(size=(n, 3))
    ang = 0.3
    Rm = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]])
    stages = {"coarse": (50, 1000, 5000), "fine": (100, 5000, 10000)}
    rec, tot, cpu_tot = {"unit": "ms", "outliers": 0.2, "stages": {}}, 0.0, 0.0
    for name, (n_iter, ns, nt) in stages.items():
        tgt = cloud(nt)
        src = (cloud(ns) * 0.8) @ Rm.T + np.array([0.05, -0.02, 0.03])
        n_out = int(0.2 * ns)
        ops.icp_points(src, tgt, n_iter=n_iter, n_outliers=n_out, min_scale=0.7, max_scale=3.0)
        ts = []
        for _ in range(3):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            T, c = ops.icp_points(src, tgt, n_iter=n_iter, n_outliers=n_out, min_scale=0.7, max_scale=3.0)
            ts.append(time.perf_counter() - t0)
        k = 4 if name == "coarse" else 2                   # bounded CPU sample: k iterations, scaled to the stage's count
        t0 = time.perf_counter()
        icp_ref.icp_points(src, tgt, n_iter=k, outliers=0.2, min_scale=0.7, max_scale=3.0)
        t_cpu = (time.perf_counter() - t0) / k * n_iter
        Tr, cr = icp_ref.icp_points(src, tgt, n_iter=2, outliers=0.2, min_scale=0.7, max_scale=3.0)
        T2, c2 = ops.icp_points(src, tgt, n_iter=2, n_outliers=n_out, min_scale=0.7, max_scale=3.0)
        rec["stages"][name] = {"iterations": n_iter, "source_points": ns, "target_points": nt, "hip_ms": min(ts) * 1e3, "cpu_ms_extrapolated": t_cpu * 1e3,
                               "cpu_iterations_timed": k, "final_cost": float(c), "max_abs_diff_vs_oracle_after_2_iterations": float(np.abs(T2 - Tr).max())}
        tot += min(ts)
        cpu_tot += t_cpu
    rec.update(hip_ms=tot * 1e3, cpu_ms_extrapolated=cpu_tot * 1e3, what="foho_icp_run_batch (float64, device-resident loop incl. upload and read-back) vs oracle/icp_ref.py (numpy, 1 process)")
    return rec


def lbs_record(torch, np, synthetic, dev):
    """MANO linear blend skinning forward + backward (`foho_lbs_fwd/_bwd`) at the batch the pipeline uses (one hand) and
    at batches where the pose-blend contraction (B x 135) . (135 x 2334) runs on `v_mfma_f32_16x16x4_f32`; the contraction's rate is
    quoted against the dense fp32 matrix peak (157.3 TFLOP/s, MI355X_MICROARCH.md) -- negligible work at the pipeline's size, as
    SURVEY 8(d) expects."""
    from followmyhold_amd import ops
    model = ops.LbsModel(synthetic.mano_like_model(1), device=dev)
    rec = {"unit": "us", "verts": model.V}
    for B in (1, 64, 1024, 8192):
        betas = torch.randn(B, 10, device=dev).requires_grad_(True)
        rot = torch.eye(3, device=dev).expand(B, 16, 3, 3).contiguous() + 0.05 * torch.randn(B, 16, 3, 3, device=dev)
        rot.requires_grad_(True)
        gv = torch.randn(B, model.V, 3, device=dev)
        def fwd():
            with torch.no_grad():
                return ops.lbs(betas, rot, model, use_mfma=1 if B >= 16 else 0)
        def fb():
            betas.grad = rot.grad = None
            v, j = ops.lbs(betas, rot, model, use_mfma=1 if B >= 16 else 0)
            (v * gv).sum().backward()
        out = {}
        for name, fn in (("fwd_us", fwd), ("fwd_bwd_us", fb)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(20):
                fn()
            torch.cuda.synchronize(dev)
            out[name] = (time.perf_counter() - t0) / 20 * 1e6
        out["hands_per_s_fwd"] = B / (out["fwd_us"] * 1e-6)
        out["poseblend_tflops_if_forward_were_only_that"] = 2 * B * 136 * 2336 / (out["fwd_us"] * 1e-6) / 1e12
        out["poseblend_frac_of_fp32_matrix_peak"] = out["poseblend_tflops_if_forward_were_only_that"] / 157.3
        rec[f"b{B}"] = out
    rec["note"] = ("fwd_us is the WHOLE forward (shape blend, joints, pose blend, kinematic chain, skinning; host wall clock over 20 calls), so the "
                   "pose-blend rate is a lower bound; the kernel alone reached 59 TFLOP/s = 0.38 at B = 8192 under rocprofv3 (profiles/r01_lbs_mfma.md)")
    return rec


def topology_record(E, torch, scene, dev, steps=200):
    """The iteration the guided pipeline actually runs in phases B and C (PL:1507-1601): the object is re-extracted from the
    SDF every iteration, so its vertex count, face count and connectivity change every time -- FlexiCubes forward, new
    object installed on the device (image records, topology tables, pair table, AABB), fused joint step, backward to the
    SDF; one hipGraph replay per iteration (engine.SdfObjective, capacity mode, counts never leave the device).  The SDF
    is a sphere whose radius wobbles by iteration (res 64, 512 x 512 targets of `scene`)."""
    import numpy as np
    res = 64
    g = np.linspace(-1.1, 1.1, res + 1, dtype=np.float32)
    xyz = torch.from_numpy(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)).to(dev)
    rad = torch.linalg.norm(xyz, dim=1)
    # like a decoded Hunyuan shape the sphere fills the [-1.1, 1.1] box (radius 0.84-0.86 -> ~8 k vertices / 16 k faces at
    # res 64); the Hunyuan -> MoGe transform scales it to the 5 cm object the targets show
    sdfs = [(rad - (0.84 + 0.02 * (k / 7.0))).contiguous() for k in range(7)]
    scene = dict(scene)
    T = np.array(scene["T_h2m"], np.float32)
    T[:3, :3] *= 0.9 * 0.06
    scene["T_h2m"] = T
    gb = E.GuidanceBatch([scene], device=dev, obj_capacity=(24576, 49152))
    obj = E.SdfObjective(gb, xyz, res)
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=True)
    for k in range(14):
        obj.run(sdfs[k % 7], cfg)
    torch.cuda.synchronize(dev)
    sizes = set()
    for k in range(7):
        obj.run(sdfs[k], cfg)
        sizes.add(obj.status()[0][:2])
    ident = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0] * 2, dtype=torch.float32, device=dev)
    gb.params.copy_(ident.expand_as(gb.params))
    gb.reset_optimizer()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for k in range(steps):
        if k % 50 == 0:
            gb.params.copy_(ident.expand_as(gb.params))
            gb.reset_optimizer()
        obj.run(sdfs[k % 7], cfg)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    nv, nf, flags = obj.status()[0]
    gb.raise_on_flags(strict_k=False)
    return {"ms_per_step": dt * 1e3 / steps, "steps": steps, "flexicubes_res": res, "faces": nf, "distinct_meshes": len(sizes),
            "launches_per_step": 18,
            "what": "SDF -> FlexiCubes -> new object installed on the device (records, topology tables, pair table, AABB) -> "
                    "fused joint step -> dL/dSDF; new topology every iteration, one hipGraph replay, no host sync"}


def driver_record(E, torch, np, synthetic, render_fn, args, n_img=64):
    """The product entry point itself, on FILES: `foho.guidance.run.run(...)` (FOHO_MESH_LEVEL_GUIDANCE=1) over n_img scene
    folders in the reference's formats and names -- masks, key points, aligned MANO and Hunyuan meshes, the 4 x 4 transform,
    fov.json and a 522 k-face MoGe image mesh (mesh.glb) per image --, wall time from the call to the last written
    `{idx}_obj.ply` / `{idx}_hand.ply`: file parsing, the target-map render of the image mesh, uploads, the 750-iteration job,
    read-back and PLY export included.  Two calls: the first builds the process's slots, target renderers and hipGraphs
    (`first_call_ms_per_image`), the second finds them ready -- the steady state of a long list."""
    import shutil
    import tempfile
    import contextlib
    import io
    from followmyhold_amd import inputs
    from foho.guidance import run as G
    H = W = args.size
    tmp = tempfile.mkdtemp(prefix="foho_bench_")
    try:
        names = ["cropped_obj_img_dir", "mask_dir", "moge_out_dir", "hunyuan_hoi_mesh_dir", "hamer_out_dir", "h2m_rt_dir", "aligned_mano_dir"]
        d = {k: os.path.join(tmp, k) for k in names}
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")          # MoGe-style image mesh: one vertex per pixel
        t = np.tan(np.radians(60.0) / 2)
        z = 0.5 + 0.1 * np.sin(xs / W * 6.0) * np.cos(ys / H * 5.0)
        mv = np.stack([(xs + 0.5 - W / 2) / (W / 2) * t * z * 0.9, -(ys + 0.5 - H / 2) / (H / 2) * t * z * 0.9, -z], -1).reshape(-1, 3).astype(np.float32)
        i = (ys[:-1, :-1] * W + xs[:-1, :-1]).reshape(-1)
        mf = np.concatenate([np.stack([i, i + W, i + 1], 1), np.stack([i + 1, i + W, i + W + 1], 1)], 0).astype(np.int64)
        sc = None
        for k in range(n_img):
            sc = synthetic.build_scene(render_fn, obj_kind=args.obj, H=H, W=W, seed=300 + k)
            inputs.save_scene_files(sc, mv, mf, d, f"{k:04d}")
        jr = os.path.join(tmp, "J.npy")
        np.save(jr, sc["J_regressor"])
        env = {"FOHO_J_REGRESSOR": jr, "FOHO_MESH_LEVEL_GUIDANCE": "1"}
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            rec, first = {}, None
            for rep in range(2):
                out_dir = os.path.join(tmp, f"out{rep}")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    tot = G.run(project_root=tmp, task_list_file=None, guidance_out_dir=out_dir, **d)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                rec = {"images": n_img, "images_per_s": n_img / dt, "ms_per_image": dt * 1e3 / n_img, "n_images": tot["n_images"],
                       "n_failed": tot["n_failed"], "meshes_written": len(os.listdir(out_dir)), "moge_mesh_faces": int(len(mf)),
                       "in_flight": int(os.environ.get("FOHO_IMAGES_IN_FLIGHT", "16")), "loader_threads": int(os.environ.get("FOHO_LOADER_THREADS", "8"))}
                if first is None:
                    first = rec["ms_per_image"]
            rec["first_call_ms_per_image"] = first
            return rec
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def parity_record(E, torch, np, scene, dev, first):
    """The metric's "loss match vs ref": first joint step of the benchmark scene on the HIP path against the CPU
    oracle's first step (same start point, before any update)."""
    gb = E.GuidanceBatch([scene], device=dev)
    cfg, _ = E.phase_cfg("C", denoise_i=19, do_update=False)
    gb.step(cfg)
    torch.cuda.synchronize(dev)
    gb.raise_on_flags()
    P = scene["H"] * scene["W"]
    p2f = gb.region("p2f", torch.int32, (2, P)).cpu().numpy()
    mism = int((p2f[0] != first["p2f_hand"]).sum() + (p2f[1] != first["p2f_hoi"]).sum())
    tot = gb.loss_dict(0)["total"]
    return {"loss_rel_err_vs_oracle": abs(tot - first["total"]) / abs(first["total"]), "pix_to_face_mismatch": mism,
            "loss_hip": tot, "loss_oracle": first["total"], "pixels_compared": 2 * P}


def cpu_baseline(scene, n_steps, threads=None, budget_s=25.0):
    """The CPU oracle (a port of the reference's PyTorch-CPU path; the reference itself cannot run without
    pytorch3d/kaolin) timed on this box's host cores on the SAME scene: 1 warm-up + n_steps joint steps.
    Returns (record, first-step results for the parity record)."""
    import torch
    from oracle import clib
    from oracle import step_ref as S
    sc = {k: (torch.from_numpy(v) if hasattr(v, "dtype") and not isinstance(v, torch.Tensor) else v) for k, v in scene.items()}
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    cores = threads or max(1, min(avail, 32))  # the oracle stops scaling (and oversubscribes) beyond a few dozen threads
    torch.set_num_threads(cores)
    clib.set_threads(cores)
    st = S.JointStepper(sc, S.make_params(), denoise_i=19)
    t0 = time.perf_counter()
    total, _, aux, _ = st.step()
    warm = time.perf_counter() - t0
    first = {"total": float(total), "p2f_hand": aux["hand"]["render"]["sel"]["pix_to_face"].reshape(-1),
             "p2f_hoi": aux["render"]["sel"]["pix_to_face"].reshape(-1)}
    n_steps = max(1, min(n_steps, int(budget_s / max(warm, 1e-3))))  # bound the sample to ~budget_s of CPU work
    t0 = time.perf_counter()
    for _ in range(n_steps):
        st.step()
    dt = time.perf_counter() - t0
    return {"value": n_steps / dt, "unit": "guidance-steps/s", "cores": cores, "kind": "port",
            "sample": f"{n_steps} joint steps (after 1 warm-up) of the same 512x512 / 20k-face scene, oracle/step_ref.py "
                      f"with OpenMP C rasteriser + torch CPU autograd, {cores} thread(s)"}, first


if __name__ == "__main__":
    main()
