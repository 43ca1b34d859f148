"""The launch schedule of every training path, held to a recorded trace.  The host side is compiled --offload-host-only (no sanitizer) against the stand-in
HIP runtime of the ThreadSanitizer test (tests/tsan/hip_stub.cpp) with its launch trace on, and tests/tsan/trace_driver.cpp walks the C ABI single-threaded:
base.json's shape with lds_encode 0 / 1 / 2 and with option backend 0, shapes outside the fused kernels (S = 32 plain, with the hybrid scatter and the tile
encode, under step_variant; S = 16), a table above 8 M parameters, occupancy skipping past its first refresh, the XORWOW sample stream -- each through
train(3), train_stages(1), (1|2), (4), (2|4); a fused and a hybrid-scatter object also through add_boxes within and past the list's capacity, set_params,
set_pose, set_backend and set_debug_dump, a fused and a chunk-record object through a checkpoint save + load, every one followed by a train call -- and one
online-manager update_dataset between two slices.  Every kernel launch (registered
name, grid, block, dynamic LDS bytes, stream by creation index) and every asynchronous fill / copy (bytes, stream) is one line.  The trace is folded without
loss -- a block of up to 12 lines that repeats back to back is written once, followed by "x N" (fold) -- and must then equal tests/golden/launch_trace.txt line
for line.  No GPU.

NOT covered: the stand-in runtime returns zeros for every read-back and refuses stream capture, so the large-table scatter's hysteresis (big_active), the
choice of the gather chain under occupancy skipping (gathers_preferred) and the hipGraph replay (option use_graph) never change state here; the GPU suite
holds them (test_gpu_parity.py, test_occupancy.py, test_occupancy_oracle.py, test_checkpoint.py).

A change that moves the schedule ON PURPOSE records the new trace: python tests/test_launch_trace.py --record"""
import difflib
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_trace.txt")


def fold(lines, max_period=12):
    """Run-length form of the trace: lines[i:i+p] repeated r >= 2 times back to back -> the p lines once, then 'x r (the p lines above)'.  At each position
    the period that covers the most lines wins (the shortest on a tie); the encoding is a function of the input alone, and lossless."""
    out, i = [], 0
    while i < len(lines):
        best_p, best_r = 0, 1
        for p in range(1, max_period + 1):
            blk = lines[i:i + p]
            if len(blk) < p or any(l.startswith(("==", "--")) for l in blk):
                break
            r = 1
            while lines[i + r * p:i + (r + 1) * p] == blk:
                r += 1
            if r >= 2 and r * p > best_r * best_p:
                best_p, best_r = p, r
        if best_p:
            out += lines[i:i + best_p] + ["x %d (the %d line%s above)" % (best_r, best_p, "" if best_p == 1 else "s")]
            i += best_p * best_r
        else:
            out.append(lines[i]); i += 1
    return out


def build_and_trace(out_dir):
    r = subprocess.run(["bash", os.path.join(ROOT, "tests", "tsan", "build_trace.sh"), str(out_dir)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    with open(os.path.join(str(out_dir), "launch_trace.txt")) as f:
        return "\n".join(fold(f.read().splitlines())) + "\n"


def test_launch_trace_matches_the_recorded_schedule(tmp_path):
    import pytest
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    got = build_and_trace(tmp_path / "trace").splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    if got != want:
        diff = list(difflib.unified_diff(want, got, "tests/golden/launch_trace.txt", "this build", n=3, lineterm=""))
        raise AssertionError("the launch schedule moved (%d lines recorded, %d now):\n%s" % (len(want), len(got), "\n".join(l[:200] for l in diff[:80])))


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_launch_trace.py --record")
    with tempfile.TemporaryDirectory() as d:
        text = build_and_trace(d)
    with open(GOLDEN, "w") as f:
        f.write(text)
    print("recorded %d lines into %s" % (len(text.splitlines()), GOLDEN))
