"""bench.py's plain run and `--dump-outputs DIR`: a plain run prints the headline line only (everything else is behind `--full`), times exactly `--steps`
steps once, and writes the timed path's outputs of its last step as float32 / float64 .npy files, at most 64 MB in all; the same arguments give the same
inputs, hence the same outputs, from run to run."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


class _FakeObject:
    """get_params() of an object with n parameters: fp32 master, fp16 working copy and EMA as raw bits."""

    def __init__(self, n):
        self.master = np.arange(n, dtype=np.float32) * np.float32(1e-3)
        self.half = self.master.astype(np.float16).view(np.uint16)
        self.ema = (self.master * np.float32(0.5)).astype(np.float16).view(np.uint16)

    def get_params(self, which=0):
        return (self.master, self.half, self.ema)[which]


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_writes_every_parameter_below_the_budget(tmp_path):
    b = _bench_module(); o = _FakeObject(1000)
    b.dump_outputs(str(tmp_path), o, 0.25)
    assert sorted(os.listdir(tmp_path)) == ["loss.npy", "params_ema.npy", "params_half.npy", "params_master.npy"]
    assert np.load(tmp_path / "loss.npy").dtype == np.float64 and np.load(tmp_path / "loss.npy")[0] == np.float32(0.25)
    assert np.array_equal(np.load(tmp_path / "params_master.npy"), o.master)
    assert np.array_equal(np.load(tmp_path / "params_half.npy"), o.half.view(np.float16).astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "params_ema.npy"), o.ema.view(np.float16).astype(np.float32))


def test_dump_of_a_large_table_is_a_fixed_sample_inside_64_mb(tmp_path):
    b = _bench_module(); o = _FakeObject(6 * 10 ** 6)              # 72 MB of parameters as three float32 arrays
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), o, 1.0)
        assert _dir_bytes(tmp_path / d) <= 64 * 10 ** 6
        for f in os.listdir(tmp_path / d):
            assert np.load(tmp_path / d / f).dtype in (np.float32, np.float64), f
    idx = np.load(tmp_path / "a" / "params_sample_index.npy")
    assert np.array_equal(idx, np.load(tmp_path / "b" / "params_sample_index.npy")) and len(idx) > 2 * 10 ** 6
    assert np.array_equal(np.load(tmp_path / "a" / "params_master.npy"), o.master[idx.astype(np.int64)])


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_the_same_outputs_twice(pkg, tmp_path):
    assert pkg.device_count() >= 1
    outs = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--views", "8",
                            "--dump-outputs", str(tmp_path / d)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        j = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in j, k
        assert j["steps"] == 7 and j["warmup"] == 3 and len(j["ms_per_step_repeats"]) == 1 and j["ms_per_step"] > 0
        assert abs(j["value"] - 4096 * 32 / (1e-3 * j["ms_per_step"])) < 2e-3 * j["value"]
        for k in ("roofline", "cpu_baseline", "late_training", "offline_job", "multi_object", "stress_T22", "psnr_db"):
            assert k not in j, k
        assert _dir_bytes(tmp_path / d) <= 64 * 10 ** 6
        outs.append({f: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    assert sorted(outs[0]) == ["loss.npy", "params_ema.npy", "params_half.npy", "params_master.npy"]
    assert outs[0]["params_master.npy"].size > 0 and all(np.isfinite(a).all() for a in outs[0].values())
    for f in outs[0]:
        assert np.array_equal(outs[0][f], outs[1][f]), f
