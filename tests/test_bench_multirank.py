"""bench.py's N > 1 path, end to end: `python bench.py --gpus 2` with no launcher and no environment spawns its two ranks itself
(object k -> rank k mod N, CORE/src/nerf.cu:27-33), trains one object per rank, gathers the final render and prints n_gpus = 2.
On a 1-GPU box both ranks share device 0 and the collective falls back to gloo (RCCL wants one GPU per rank); on an 8-GPU node the
same code path runs one rank per GPU over RCCL with device-resident crops."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _run(args, timeout=900, env=None):
    env = dict({k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MON_BENCH_DIST_BACKEND")},
            **(env or {}))
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)


def _json_line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_two_self_spawned_ranks_report_two_gpus_and_gather_both_crops(pkg):
    assert pkg.device_count() >= 1
    small = ["--steps", "6", "--warmup", "2", "--repeats", "2", "--full", "--no-cpu-baseline", "--objects-per-gpu", "0", "--views", "12", "--no-sustained"]
    r2 = _run(["--gpus", "2"] + small)
    assert r2.returncode == 0, r2.stderr[-3000:]
    j2 = _json_line(r2.stdout)
    assert j2["n_gpus"] == 2 and j2["config"]["objects"] == 2 and j2["config"]["launcher"] == "self-spawned ranks"
    assert len(j2["psnr_db"]) == 2 and all(p > 5.0 for p in j2["psnr_db"])             # both ranks' crops arrived through the gather
    assert j2["render_gather"] == "ok"
    assert len(j2["per_rank_ray_samples_per_s"]) == 2 and all(v > 0 for v in j2["per_rank_ray_samples_per_s"])
    assert j2["scaling"] == "weak" and len(j2["ms_per_step_repeats"]) == 2
    r1 = _run(["--gpus", "1"] + small)
    assert r1.returncode == 0, r1.stderr[-3000:]
    j1 = _json_line(r1.stdout)
    assert j1["n_gpus"] == 1 and len(j1["psnr_db"]) == 1 and j1["config"]["launcher"] == "single process" and j1["render_gather"] is None
    # whole-job value = the ray-samples of ALL ranks over the slowest rank's time (two processes sharing one GPU slow each other down by an amount that varies
    # from run to run, so nothing is claimed against the one-rank value): n_gpus x R x S per step time, and every rank's own rate is at least the slowest rank's
    B = 4096 * 32
    for j, n in ((j1, 1), (j2, 2)):
        assert abs(j["value"] - n * B / (1e-3 * j["ms_per_step"])) < 2e-3 * j["value"], (j["value"], j["ms_per_step"])
    pr = j2["per_rank_ray_samples_per_s"]
    assert min(pr) >= 0.999 * B / (1e-3 * j2["ms_per_step_repeats"][-1]), (pr, j2["ms_per_step_repeats"])
    for j in (j1, j2):
        rf = j["roofline"]
        assert rf["bound"] in ("l2-requests", "hbm") and 0 < rf["frac"] < 1 and rf["avg_launch_ms"] > 0


@pytest.mark.gpu
def test_eight_self_spawned_ranks_run_the_drivers_n8_command_end_to_end(pkg):
    """The command the driver runs on the 8-GPU node, `python bench.py --gpus 8 ...`, end to end on whatever this box has: eight ranks (one process each;
    rank r -> device r mod the visible ones, gloo when they have to share a GPU), eight objects trained, eight crops gathered to rank 0, one JSON line
    whose config says what the collective itself reported -- its world size and backend, and the device every rank trained on."""
    assert pkg.device_count() >= 1
    r = _run(["--gpus", "8", "--steps", "4", "--warmup", "2", "--repeats", "1", "--full", "--no-cpu-baseline", "--objects-per-gpu", "0", "--views", "8",
              "--no-sustained", "--no-stress"], timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    j = _json_line(r.stdout)
    assert j["n_gpus"] == 8 and j["config"]["objects"] == 8 and j["config"]["ranks_in_collective"] == 8
    ndev = pkg.device_count()
    assert j["config"]["collective_backend"] == ("nccl" if ndev >= 8 else "gloo") and j["config"]["visible_devices"] == ndev
    assert j["config"]["rank_devices"] == [k % ndev for k in range(8)]                      # object k -> rank k -> device k mod nGPU (nerf.cu:27-33)
    assert len(j["per_rank_ray_samples_per_s"]) == 8 and all(v > 0 for v in j["per_rank_ray_samples_per_s"])
    assert j["render_gather"] == "ok" and len(j["psnr_db"]) == 8 and all(p > 5.0 for p in j["psnr_db"])
    B = 4096 * 32
    assert abs(j["value"] - 8 * B / (1e-3 * j["ms_per_step"])) < 2e-3 * j["value"]
    assert j["scaling"] == "weak"


@pytest.mark.gpu
def test_the_drivers_launcher_command_runs_two_ranks(pkg):
    """The driver's own N > 1 command -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N
    --steps K --warmup W` -- with N = 2 on this box: the ranks come from the launcher's environment (no self-spawn), rank 0 prints the one JSON line."""
    assert pkg.device_count() >= 1
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MON_BENCH_DIST_BACKEND", "MON_BENCH_SPAWNED")}
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--repeats", "1", "--full", "--no-cpu-baseline", "--objects-per-gpu", "0",
           "--views", "8", "--no-sustained", "--no-stress"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    j = _json_line(r.stdout)
    ndev = pkg.device_count()
    assert j["n_gpus"] == 2 and j["config"]["launcher"] == "torch.distributed.run" and j["config"]["ranks_in_collective"] == 2
    assert j["config"]["collective_backend"] == ("nccl" if ndev >= 2 else "gloo") and j["config"]["rank_devices"] == [0, 1 % ndev]
    assert j["render_gather"] == "ok" and len(j["psnr_db"]) == 2 and len(j["per_rank_ray_samples_per_s"]) == 2
    assert j["steps"] == 4 and j["warmup"] == 2 and j["value"] > 0


def test_gpus_flag_without_a_device_fails_loudly():
    """No CPU fallback: without a HIP device the spawner stops with a message instead of printing a line."""
    import __graft_entry__ as ge
    if ge.load_package().device_count() > 0:
        pytest.skip("a HIP device is visible")
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1"], timeout=300)
    assert r.returncode != 0 and "no HIP device" in (r.stderr + r.stdout)
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_a_gather_that_cannot_finish_does_not_take_the_bench_line_with_it(pkg):
    """The throughput is complete before the final render is gathered; a gather that hangs or fails (here: a deadline of zero seconds) must leave the JSON line,
    with the failure named in it and rank 0's own crop scored."""
    assert pkg.device_count() >= 1
    r = _run(["--gpus", "2", "--steps", "6", "--warmup", "2", "--repeats", "2", "--full", "--no-cpu-baseline", "--objects-per-gpu", "0", "--views", "12"],
            env={"MON_BENCH_GATHER_TIMEOUT": "0"})
    assert r.returncode == 0, r.stderr[-3000:]
    j = _json_line(r.stdout)
    assert j["n_gpus"] == 2 and j["value"] > 0 and j["render_gather"].startswith("FAILED") and len(j["psnr_db"]) == 1
