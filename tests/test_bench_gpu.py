"""bench.py as the driver launches it: the N=1 line's contract fields and the N>1 path (one rank per GPU; here two ranks
share the box's one GPU and the collectives go through gloo -- FOHO_BENCH_BACKEND -- instead of RCCL)."""
import json
import math
import os
import subprocess
import sys

import pytest

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, stdout[-3000:]
    return json.loads(lines[0])


def _detail(text):
    """The detail record bench.py writes to stderr beside the headline line."""
    lines = [l for l in text.splitlines() if l.startswith("bench-detail: ")]
    assert len(lines) == 1, text[-3000:]
    return json.loads(lines[0][len("bench-detail: "):])


def _env(**kw):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **kw)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


@gpu
def test_bench_line_n1_and_two_ranks_gloo():
    """`python bench.py --gpus 1 --steps 20 --warmup 5 --full` and the same workload as
    `torch.distributed.run --nproc-per-node 2 bench.py --gpus 2 ...`: one JSON line each, whole-job value, weak scaling
    (every rank brings its own frame), timings max-reduced over the ranks, metrics vector summed over them."""
    flags = ["--steps", "20", "--warmup", "5", "--no-extras", "--no-cpu-baseline", "--full"]
    r1 = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + flags, env=_env(), cwd=ROOT, stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, text=True, timeout=900)
    assert r1.returncode == 0, r1.stderr[-3000:]
    o1 = _line(r1.stdout)
    assert len(r1.stdout.strip().splitlines()[-1]) < 1900          # the ONE line survives whole in a 2000-character log tail
    assert o1["roofline"]["bound"] in ("latency", "hbm", "valu-issue") and o1["roofline"]["roof"] == "hbm" and o1["config"]["global_images"] == 1
    o1 = _detail(r1.stderr)
    assert o1["n_gpus"] == 1 and o1["steps"] == 20 and o1["warmup"] == 5 and o1["scaling"] == "weak"
    assert o1["config"]["global_images"] == 1 and o1["higher_is_better"] is True and o1["vs_baseline"] is None
    assert o1["repeats"] >= 2 and o1["repeats"] * 20 * o1["ms_per_step"] * 1e-3 > 0.1     # short regions are repeated
    assert abs(o1["value"] - 1e3 / o1["ms_per_step"]) <= 1e-6 * o1["value"]
    rf = o1["roofline"]
    assert rf["roof"] == "hbm" and rf["peak"] == 8000.0 and 0 < rf["frac"] < 1 and rf["kernel"] in o1["kernels"]
    assert rf["kernel"] == max(o1["kernel_ms_median"], key=o1["kernel_ms_median"].get)     # chosen live
    assert o1["metrics"]["n_images"] == 1 and o1["nan_images"] == 0

    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29655", "bench.py", "--gpus", "2"] + flags
    r2 = subprocess.run(cmd, env=_env(FOHO_BENCH_BACKEND="gloo"), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                        text=True, timeout=900)
    assert r2.returncode == 0, r2.stdout[-4000:]
    o2 = _line(r2.stdout)
    assert o2["n_gpus"] == 2 and o2["config"]["global_images"] == 2 and o2["rccl_ranks"] == 2
    o2 = _detail(r2.stdout)
    assert o2["n_gpus"] == 2 and o2["config"]["global_images"] == 2 and o2["config"]["images_per_gpu"] == 1
    assert o2["steps"] == 20 and o2["scaling"] == "weak" and o2["metric"] == o1["metric"] and o2["unit"] == o1["unit"]
    assert abs(o2["value"] - 2 * 1e3 / o2["ms_per_step"]) <= 1e-6 * o2["value"]            # whole-job aggregate
    # two ranks time-share one GPU here: anything between one and four single-rank throughputs is plausible, outside that
    # the aggregation (x world, max over ranks) is wrong
    assert o1["value"] <= 2.0 * o2["value"] and o2["value"] <= 4.0 * o1["value"], (o1["value"], o2["value"])
    m1, m2 = o1["metrics"], o2["metrics"]
    assert m2["n_images"] == 2 and m2["n_steps"] == 2 * 20 * o2["repeats"] and m2["n_nan"] == 0
    # the loss terms are summed over the ranks too.  Their values depend on how many repeats the timed region took (the loops
    # keep optimising) and rank 1 works on another frame (seed = rank), so only the order of magnitude is comparable
    assert math.isfinite(m2["sum_total_loss"]) and 0.02 * m1["sum_total_loss"] < m2["sum_total_loss"] < 50.0 * m1["sum_total_loss"]
    assert "roofline" in o2 and "cpu_baseline" not in o2
    assert o2["rccl_ranks"] == 2 and o2["collective_backend"] == "gloo" and o1["rccl_ranks"] == 1

    # the PLAIN form the driver uses at N = 1, with N = 2: bench.py launches its own ranks (one per GPU; gloo lets the two
    # share this box's GPU) and the line says two
    r3 = subprocess.run([sys.executable, "bench.py", "--gpus", "2"] + flags, env=_env(FOHO_BENCH_BACKEND="gloo"), cwd=ROOT,
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r3.returncode == 0, r3.stdout[-4000:]
    o3 = _detail(r3.stdout)
    assert _line(r3.stdout)["n_gpus"] == 2
    assert o3["n_gpus"] == 2 and o3["rccl_ranks"] == 2 and o3["config"]["global_images"] == 2
    assert abs(o3["value"] - 2 * 1e3 / o3["ms_per_step"]) <= 1e-6 * o3["value"]
    assert o1["value"] <= 2.0 * o3["value"] and o3["value"] <= 4.0 * o1["value"], (o1["value"], o3["value"])


def test_bench_refuses_a_rank_count_other_than_gpus():
    """`--gpus N` under a launcher that started another number of ranks is an error, not a line with a different n_gpus
    (checked before anything touches a GPU, so this runs anywhere)."""
    env = _env()
    env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "20"], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stdout and '{"metric"' not in r.stdout
    env.update(WORLD_SIZE="4")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20"], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=4" in r.stdout


def test_bench_plain_form_launches_one_rank_per_gpu():
    """Without a GPU the launched ranks stop at "needs an MI355X" -- what is checked here is that `python bench.py --gpus 2`
    goes through the launcher (a rank reports the refusal; torch elastic tears the other rank down as soon as the first one exits, so
    whether BOTH get to print is a race: one run in two) and that the launcher hands the failure on as its exit status."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("covered by the gpu test")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "20", "--warmup", "5"], env=_env(), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode != 0
    assert 1 <= r.stdout.count("bench.py needs an MI355X") <= 2, r.stdout[-3000:]
    assert "--nproc-per-node" in r.stdout or "torch.distributed" in r.stdout or "ChildFailedError" in r.stdout or "local_rank" in r.stdout, r.stdout[-3000:]


@gpu
def test_bench_rccl_branch_runs_with_one_rank():
    """The box has one GPU, so the N > 1 tests above go through gloo.  FOHO_BENCH_FORCE_DIST=1 makes the single rank join an
    `nccl` (= RCCL) process group all the same: init with the device id, the barriers around the timed region and the
    device-side all-reduces of the timing and the metrics vector all execute on the real backend."""
    flags = ["--steps", "20", "--warmup", "5", "--no-extras", "--no-cpu-baseline"]
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + flags, env=_env(FOHO_BENCH_FORCE_DIST="1"), cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert _line(r.stdout)["rccl_ranks"] == 1
    o = _detail(r.stderr)
    assert o["n_gpus"] == 1 and o["rccl_ranks"] == 1 and o["collective_backend"] == "nccl"
    assert o["metrics"]["n_images"] == 1 and o["nan_images"] == 0 and o["value"] > 0


def test_headline_line_stays_under_the_log_tail_with_every_side_record_present():
    """bench.headline(): the stdout line carries the contract's fields, `roofline` (+ `secondary`: the side records' headline
    numbers), `cpu_baseline` and `parity` in under 1 900 characters whatever the side records hold (no GPU needed)."""
    sys.path.insert(0, ROOT)
    import bench
    big = 123456.789012345
    out = {"metric": "guidance-steps/sec (512x512, 778+20k verts)", "value": big, "unit": "guidance-steps/s", "n_gpus": 8, "steps": 2000, "warmup": 100,
           "ms_per_step": 0.0549312345, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic", "repeats": 200,
           "rccl_ranks": 8,
           "config": {"workload": "configs[1]: single 512x512 synthetic frame per GPU, 778-vert hand + 10242-vert/20480-face object, joint guidance step (phase C)",
                      "images_per_gpu": 1, "global_images": 8, "parallelism": "image-sharded x8", "hip_graph": True, "steps_per_graph": 50, "streams": 1, "restart_every": 50},
           "roofline": {"bound": "latency", "roof": "hbm", "kernel": "k_pix_bwd", "achieved": 245.678912, "peak": 8000.0, "unit": "GB/s", "frac": 0.0307123, "traffic": 7100123.4,
                        "kernel_ms": 0.0115471, "algorithmic_bytes_per_launch": 2836864, "binding": "x" * 300},
           "roofline_valu": {"frac": 0.234567, "kernels": {"k": {"a": 1}}},
           "geo_decode": {"fwd_ms": 9.3123, "roofline": {"frac": 0.39812}, "fwd_bwd_rows_ms": 11.3123, "fwd_bwd_ms": 24.6123},
           "pipeline_iteration": {"hip_decoder": {"iteration_ms": 31.5123, "backward_ms": 14.2123}, "torch_decoder": {"iteration_ms": 116.123}, "active_row_frac": 0.04641,
                                  "batch_of_4": {"iteration_ms": 84.6789}},
           "closeup": {"one_image": {"value": 10712.34}, "in_flight_32": {"value": 43123.4}}, "batched": {"value": 74812.3}, "obj_40k": {"value": 14512.3},
           "topology_changing": {"ms_per_step": 0.14212}, "job": {f"in_flight_{k}": {"images_per_s": 200.123} for k in (1, 8, 16, 32)},
           "driver_on_files": {"images_per_s": 112.345}, "icp": {"hip_ms": 74.123, "cpu_ms_extrapolated": 51234.5},
           "lbs": {"b1": {"fwd_bwd_us": 61.234}, "b8192": {"poseblend_frac_of_fp32_matrix_peak": 0.3812}},
           "vae_attention": {k: {"forward_us": 137.123, "forward_backward_us": 509.123} for k in ("torch_default", "torch_efficient", "hip")},
           "cpu_baseline": {"value": 2.2812345, "unit": "guidance-steps/s", "cores": 32, "kind": "port",
                            "sample": "30 joint steps (after 1 warm-up) of the same 512x512 / 20k-face scene, oracle/step_ref.py with OpenMP C rasteriser + torch CPU autograd, 32 thread(s)"},
           "cpu_baseline_1t": {"value": 0.2012345}, "parity": {"loss_rel_err_vs_oracle": 1.2345e-7, "pix_to_face_mismatch": 0}}
    line = json.dumps(bench.headline(out), separators=(",", ":"))
    assert len(line) < 1900, len(line)
    back = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in back, k
    assert set(back["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic", "secondary"}
    assert set(back["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"}
    # a side record that failed is named, not dropped
    out["closeup"] = {"error": "FohoError: " + "y" * 500}
    line = json.dumps(bench.headline(out), separators=(",", ":"))
    assert len(line) < 1900 and "error" in json.loads(line)["roofline"]["secondary"]["closeup"]


@gpu
def test_bench_plain_run_times_exactly_steps_and_dumps_outputs(tmp_path):
    """The plain form `python bench.py --gpus 1 --steps K --warmup W`: ONE timed region of exactly K iterations, nothing beyond
    the headline (no roofline, side records or CPU baseline), and --dump-outputs writes what the K-th timed step left as
    float32 / float64 arrays.  That step starts from a restart of the seeded scene (bench.run_timed), so two runs with the
    same arguments write the same arrays up to the float-atomic noise of one backward (~1e-7).  K = 30
    takes 10-iteration graphs: the 29 iterations before the last one end in a 9-iteration graph of their own."""
    import numpy as np

    def run(steps, warmup, d):
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(d)],
                           env=_env(), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        line = _line(r.stdout)
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in line, k
        assert line["steps"] == steps and line["warmup"] == warmup and line["repeats"] == 1
        assert "roofline" not in line and "cpu_baseline" not in line and "parity" not in line
        o = _detail(r.stderr)
        assert o["repeats"] == 1 and o["metrics"]["n_steps"] == steps and o["nan_images"] == 0
        assert abs(o["value"] - 1e3 / o["ms_per_step"]) <= 1e-6 * o["value"]
        assert not {"kernels", "batched", "geo_decode", "cpu_baseline"} & set(o)
        arrs = {p.stem: np.load(p) for p in d.iterdir()}
        assert {"params", "losses", "grad_params", "grad_verts_in", "adam_t", "flags"} <= set(arrs)
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert arrs["params"].shape == (1, 16) and arrs["grad_verts_in"].shape[1] == 3
        assert all(np.isfinite(a).all() for a in arrs.values()) and not arrs["flags"].any()
        assert arrs["adam_t"].tolist() == [1]              # the last timed step is the first AdamW step after its restart
        return arrs

    a, b = run(30, 5, tmp_path / "k30a"), run(30, 5, tmp_path / "k30b")
    for k, x in a.items():
        assert np.abs(b[k] - x).max() <= 1e-5 * np.abs(x).max(), k


def test_dump_outputs_stays_under_its_cap(tmp_path, monkeypatch):
    """bench.dump_outputs (no GPU needed): every array a float32 / float64 .npy, and past the cap grad_verts_in keeps a fixed,
    seeded sample of its rows whose indices are written beside it."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench

    class Batch:
        def __init__(self, B, V, seed):
            g = torch.Generator().manual_seed(seed)
            self.params, self.losses, self.grad_params = torch.rand(B, 16, generator=g), torch.rand(B, 24, generator=g), torch.rand(B, 16, generator=g)
            self.adam_m, self.adam_v = torch.rand(B, 16, generator=g), torch.rand(B, 16, generator=g)
            self.adam_t, self.flags = torch.full((B,), 7, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
            self.grad_verts_in = torch.rand(V, 3, generator=g)

    class Group:
        batches = [Batch(2, 30000, 0), Batch(1, 20000, 1)]

    bench.dump_outputs(str(tmp_path / "all"), Group, np)
    a = {p.stem: np.load(p) for p in (tmp_path / "all").iterdir()}
    assert a["params"].shape == (3, 16) and a["grad_verts_in"].shape == (50000, 3) and "grad_verts_rows" not in a
    assert a["adam_t"].dtype == np.float64 and (a["adam_t"] == 7).all()
    np.testing.assert_array_equal(a["grad_verts_in"][30000:], Group.batches[1].grad_verts_in.numpy())
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 200000)
    for run in ("s0", "s1"):
        bench.dump_outputs(str(tmp_path / run), Group, np)
    s0 = {p.stem: np.load(p) for p in (tmp_path / "s0").iterdir()}
    s1 = {p.stem: np.load(p) for p in (tmp_path / "s1").iterdir()}
    assert all(v.dtype in (np.float32, np.float64) for v in s0.values())
    assert sum(v.nbytes for v in s0.values()) <= 200000 and len(s0["grad_verts_in"]) > 1000
    rows = s0["grad_verts_rows"].astype(np.int64)
    np.testing.assert_array_equal(s0["grad_verts_in"], a["grad_verts_in"][rows])
    for k in s0:
        np.testing.assert_array_equal(s0[k], s1[k])
