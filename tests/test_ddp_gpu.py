"""The real multi-GPU path (BASELINE configs[3]): needs >= 2 GPUs on the box, skipped otherwise."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _env():
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    return env


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_two_rank_nccl_lane_sync_matches_global_batch():
    """2 ranks x (lane + GradArena.sync() + RCCL all-reduce started inside backward) == 1 process on the global batch"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "ddp_lane_worker.py")]
    r = subprocess.run(cmd, env=_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "DDP_LANE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_two_ranks_on_one_gpu_lane_sync_matches_global_batch():
    """The same worker on a single-GPU box: two processes share cuda:0 and exchange their gradients through gloo (RCCL
    refuses two ranks on one device).  Everything but the transport is the benched path: lane, contribution counting,
    all-reduces started inside backward on the communication stream, loss-scalar reduction."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "ddp_lane_worker.py")]
    env = _env()
    env["IRR_DDP_BACKEND"] = "gloo"
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "DDP_LANE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_single_rank_rccl_transport_lane_sync():
    """RCCL ITSELF on a one-GPU box (VERDICT r4 missing #1: `init_process_group("nccl")` and the comm-stream / RCCL interaction had
    run zero times): RCCL refuses two ranks on one device, so the worker runs as a process group of ONE rank with every collective of
    the data-parallel step really issued (IRR_DDP_SINGLE_RANK=1, irr_amd.ddp.collectives_on) -- communicator creation with device_id,
    parameter broadcast, the MIN / MAX calibration all-reduces, bucket all-reduces started inside backward on the communication stream
    behind the lane's tail, the loss-scalar all-reduce.  An all-reduce over one rank is the identity; the result must equal the plain
    single-process gradient, and the bucket schedule must be the multi-rank one."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "ddp_lane_worker.py")]
    env = _env()
    env["IRR_DDP_SINGLE_RANK"] = "1"
    env.pop("IRR_DDP_BACKEND", None)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "DDP_LANE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("lane", ["inline", "plain"])
def test_single_rank_rccl_other_gradient_routes_with_branch_streams(lane):
    """with the occlusion branch of the coarse levels on its own stream (the default), a bucket's all-reduce
    must wait for EVERY stream that contributed to it -- the inline lane (bench.py --no-async-wgrad) and the plain autograd hooks
    deliver contributions on both streams.  Same worker, same assertions (gradient == single process, buckets 0 and 1 started
    inside backward), plus: bucket 1 saw two contributing streams."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "ddp_lane_worker.py")]
    env = _env()
    env["IRR_DDP_SINGLE_RANK"] = "1"
    env["IRR_DDP_LANE"] = lane
    env["IRR_BRANCH_STREAMS"] = "1"
    env.pop("IRR_DDP_BACKEND", None)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "DDP_LANE_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_bench_single_rank_over_rccl():
    """bench.py with the same switch: the line says transport rccl and rank 0's buckets 0 and 1 start inside backward"""
    import json
    env = _env()
    env["IRR_DDP_SINGLE_RANK"] = "1"
    env.pop("IRR_DDP_BACKEND", None)
    env["MASTER_PORT"] = str(_free_port())
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "4",
                        "--no-cpu-baseline", "--no-secondary", "--no-extra-legs"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    # stdout is EXACTLY the one JSON line: RCCL's version banner (NCCL_DEBUG=VERSION on the GPU boxes; C stdio, flushed at exit) used to
    # follow it there -- bench.py points file descriptor 1 at stderr and writes the line to a saved duplicate of the real stdout
    assert len(r.stdout.strip().splitlines()) == 1, r.stdout[-2000:]
    assert "RCCL version" in r.stderr or os.environ.get("NCCL_DEBUG", "") == ""
    out = json.loads(r.stdout)
    assert out["n_gpus"] == 1 and out["config"]["transport"] == "rccl" and out["value"] > 0
    log = out["ranks"]["bucket_launches_last_step"]
    assert [b for b, _, _ in log] == [0, 1, 2] and log[0][1] == "backward" and log[1][1] == "backward", log


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_bench_self_launches_two_ranks():
    """`python bench.py --gpus 2` from a cold shell: the script starts its own ranks and prints ONE JSON line"""
    import json
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "4",
                        "--no-cpu-baseline"], env=_env(), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 8 and out["value"] > 0


def test_bench_two_ranks_share_one_gpu_over_gloo():
    """`python bench.py --gpus 2 --full` from a cold shell on a ONE-GPU box: the script starts its own ranks (launch_ranks), both
    share cuda:0 and exchange through gloo (IRR_DDP_BACKEND) -- broadcast_params, reduce_losses, the bucketed gradient all-reduce,
    the MAX-over-ranks timing and the rank-0 relay of bench.py run exactly as in the driver's multi-GPU leg, incl. the secondary
    448x1024 workload; ONE JSON line comes back."""
    import json
    env = _env()
    env["IRR_DDP_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "2", "--batch", "2",
                        "--full", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 4 and out["value"] > 0 and out["config"]["transport"] == "gloo"
    assert out["secondary"]["value"] > 0 and out["secondary"]["roofline"]["achieved"] > 0
    assert out["roofline"]["achieved"] > 0 and "cpu_baseline" not in out
    # the configuration that found round 4's two-rank NaN stays in the suite: the streaming kernel's fp16x2 form is the default now
    assert out["x3s_h2"] is True and out["launches_per_step"].get("fwd_x3s", 0) > 0
    # north_star: "all-reduce of gradients ... overlapped with the backward correlation kernel": bucket 0 (the occlusion upsampler,
    # final after levels 6-5) is enqueued inside backward before the FIRST cost-volume gradient launch (levels 4 .. 0 follow it: it is
    # reduced under all five of them), bucket 1 (the shared decoders, final after the coarsest level) after the level-4 one
    log = out["ranks"]["bucket_launches_last_step"]
    corr = out["ranks"]["corr_backward_launches_ms"]
    assert [tuple(e[:2]) for e in log] == [(0, "backward"), (1, "backward"), (2, "backward")], log
    assert len(corr) == 5 and log[0][2] < corr[0] < log[1][2], (log, corr)


def test_bench_eight_ranks_share_one_gpu_over_gloo():
    """The driver's 8-GPU leg as far as ONE GPU allows: `bench.py --gpus 8` from a cold shell, eight ranks
    sharing cuda:0 over gloo on a small shape -- launch_ranks, broadcast_params, contribution counting + MIN/MAX calibration over
    8 ranks, the three buckets started inside backward on every later step, loss-scalar all-reduce, MAX-over-ranks timing with the
    per-rank spread, rank-0 relay.  Only the RCCL transport itself is not exercised."""
    import json
    env = _env()
    env["IRR_DDP_BACKEND"] = "gloo"
    env["OMP_NUM_THREADS"] = "2"
    # Eight PROCESSES on one GPU are what this test has to make do with; in earlier rounds such a run died in some attempts with
    # "HSA_STATUS_ERROR_ILLEGAL_INSTRUCTION" in one rank's queue (profiles/NOTES.md C.4).  A faulted device is not used again: the run
    # is made once, and a fault is a failure.
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "2", "--batch", "1",
                        "--height", "128", "--width", "192", "--no-secondary", "--no-cpu-baseline", "--prealloc-gb", "0"],
                       env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["config"]["global_batch"] == 8 and out["value"] > 0 and out["config"]["transport"] == "gloo"
    assert len(out["ranks"]["per_rank_ms_per_step"]) == 8 and max(out["ranks"]["per_rank_ms_per_step"]) == pytest.approx(out["ms_per_step"], rel=1e-3)
    log = [tuple(e[:2]) for e in out["ranks"]["bucket_launches_last_step"]]
    assert log == [(0, "backward"), (1, "backward"), (2, "backward")], out["ranks"]
