"""The launch schedule of every training path, held to a recorded trace.  The host side is compiled --offload-host-only (no sanitizer) against the stand-in
HIP runtime of the ThreadSanitizer test (tests/tsan/hip_stub.cpp) with its launch trace on, and tests/tsan/trace_driver.cpp walks the C ABI single-threaded:
base.json's shape with lds_encode 0 / 1 / 2 and with option backend 0, shapes outside the fused kernels (S = 32 plain, with the hybrid scatter and the tile
encode, under step_variant; S = 16), a table above 8 M parameters, occupancy skipping past its first refresh, the XORWOW sample stream -- each through
train(3), train_stages(1), (1|2), (4), (2|4); a fused and a hybrid-scatter object also through add_boxes within and past the list's capacity, set_params,
set_pose, set_backend and set_debug_dump, a fused and a chunk-record object through a checkpoint save + load, every one followed by a train call -- and one
online-manager update_dataset between two slices.  A second part ("== inference routes") walks every scene and object-pose route of the C ABI once on each
side over two trained and published objects (camera and window refinement with and without a coarse-to-fine schedule, a window of two frames, one of them
with two boxes) and every online counterpart on a manager whose two objects have published; then the field queries on each side: the object's and the
scene's point queries and gradients (lists of 5 points, with and without level weights and select), the lattice query, the lattice gradients, the distance
field and the components (region 0 with a table, region 1 with and without its optional outputs) on a lattice of 3 x 2 x 2 and, once per family, on one of
33 x 32 x 16 cells (a pass boundary with a ragged tail of 512), the normals at ray hits, the six online counterparts, and with no side
mon_distance_transform, mon_label_components, mon_lattice_points and mon_camera_rays.  Behind them, in a section of its own ("-- lattice routes": a handle
makes a stream, and the streams above keep their creation indices), the cost fields and the device-resident distance fields: per side
mon_scene_paths_lattice (with a soft cost and every optional output, with neither, on 33 x 32 x 16) and mon_scene_dist_field (both lattices); with no side
mon_shortest_paths (with and without cell_cost and next, both lattices), mon_lattice_path, mon_dist_field_create and, on its handle, _info, _read, _sample
(with and without gradients), _score (way_floats 3 and 16, with and without the optional outputs), _match (with and without the normal equations and the
pivots), mon_register_default, mon_dist_field_register and _destroy; mon_online_paths_lattice and mon_online_dist_field.  The stand-in runtime leaves every
read-back 0, so a cost field settles after its first batch of sweeps and a registration ends in its first round: with status 3 under the default
min_inside, with status 2 (no factorisation of an all-zero row) under min_inside 0; both are called.  On the created handle also mon_trace_default, mon_dist_field_trace (range alone, every optional
output, poses16 NULL with one pose, three poses) and mon_dist_field_beam_score (with and without its counts); with no side mon_signed_distance_transform (with
and without nearest_edge, both lattices); mon_online_signed_distance_lattice and mon_online_signed_dist_field; and behind them, per side ("-- lattice routes,
signed distance": their handles' streams take the creation indices after every handle above), mon_scene_signed_distance_lattice (every optional output,
none, MON_SIGNED_LOG, 33 x 32 x 16) and mon_scene_signed_dist_field (both lattices).  Every kernel launch (registered
name, grid, block, dynamic LDS bytes, stream by creation index) and every asynchronous fill / copy (bytes, stream) is one line.  The trace is folded without
loss -- a block of up to 12 lines that repeats back to back is written once, followed by "x N" (fold) -- and must then equal tests/golden/launch_trace.txt line
for line.  No GPU.

"== inference errors" lists calls of those routes that must fail, one line each: "-- <route>, <the arguments changed> -> <code>: <mon_last_error()>" -- every
NULL pointer, every count at 0 and one past its maximum, bad sides, poses, rays, boxes, windows and schedules, a NULL object, objects of other datasets,
objects outside the fused kernels, unpublished objects and managers, and the pairs of errors whose precedence the ABI tests pin.  (The stand-in runtime gives
real objects, so the errors that need one are reached without a GPU.)  The section was recorded before the routes' checks were written once, and the code
of every line holds as recorded.  Where several wordings of one check became one, the message that is printed now stands, whole line, in
tests/golden/launch_trace_reworded.txt: a line may differ from the recorded one only by being listed there with the same call and the same code.  Five of
the listed lines are not rewordings: there the boundary's order (what needs no object, the objects, what needs them, then a schedule) reports another of two
errors first than the recorded build did --
    scene_pose_loss and scene_pose_loss_batch, a NULL object with n_obs = 0:   "null object 1" -> "no boxes"
    scene_refine_window, a NULL object with a bad schedule:                    the schedule's error -> "null object 1"
    online_relocalise, n_obs = 0 with keep 17:                                 "no boxes" -> "keep 17"
    online_refine_window, a bad schedule with refine_objects and no fixed frame: the schedule's error -> the window's

NOT covered: the stand-in runtime returns zeros for every read-back and refuses stream capture, so the large-table scatter's hysteresis (big_active), the
choice of the gather chain under occupancy skipping (gathers_preferred) and the hipGraph replay (option use_graph) never change state here; the GPU suite
holds them (test_gpu_parity.py, test_occupancy.py, test_occupancy_oracle.py, test_checkpoint.py).

The field queries' lines, routes and refusals, were recorded from the commit before their host chain was written once ("Add connected components over a
lattice of the object map"), with this driver and that commit's product sources; the lines above and between them came out as they stood.  (Their object
lists need no common camera, dataset or sample stream: other_K, other_ds and xorwow are accepted there and their launches are in the trace.)  The
"-- lattice routes" lines and their refusals (every NULL argument, every count at 0 and one past its maximum, connectivity 7, max_cost 0, a seed outside
the lattice, way_floats 4, huber 0, lambda_up 1, a NULL handle beside a bad count) were recorded in the same way from the commit before the lattice routes'
chain was written once ("Add scan matching against a device-resident distance field").  The ray tracing, beam score and signed-field lines and their
refusals (every NULL argument; rays, poses, rays x poses and max_steps at 0 and one past their maxima; t_min above t_max, relax 0 and 1.5, step_min 0, a
NaN march parameter, beam huber 0, two poses without poses16; flags 2, max_dist 0 and +inf, step 0 on an axis of several cells, iso NaN; a NULL handle beside
a bad count) were recorded in the same way from the commit before the handle calls' output plan, the block row and the fill were written once ("Add signed,
sub-cell distance fields from the map's density"); every line recorded before came out as it stood.

A change that moves the schedule ON PURPOSE records the new trace: python tests/test_launch_trace.py --record
A refactor shows that nothing moved by recording from the parent commit's product sources with this driver, and getting the committed file:
    MON_TRACE_SRC=<checkout of the parent commit> python tests/test_launch_trace.py --record
A record from this tree's own sources (no MON_TRACE_SRC) writes the messages it prints into the golden itself and empties launch_trace_reworded.txt, which
holds nothing but the difference between the golden and this tree; a record from another checkout leaves that file alone -- and prints that checkout's
wording of the lines listed there, which go back to the recorded wording before the file is committed (git diff shows nothing else)."""
import difflib
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_trace.txt")
REWORDED = os.path.join(ROOT, "tests", "golden", "launch_trace_reworded.txt")


def call_and_code(line):
    """'-- <call> -> <code>' of an error line, None for any other line"""
    head, sep, rest = line.partition(" -> ")
    return head + sep + rest.partition(":")[0] if line.startswith("-- ") and sep else None


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
    with open(REWORDED) as f:
        reworded = set(f.read().splitlines())
    if len(got) == len(want):       # a reworded message: the listed line, in place of a recorded line with the same call and code
        got = [w if g != w and g in reworded and call_and_code(w) and call_and_code(g) == call_and_code(w) else g for g, w in zip(got, want)]
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
    if not os.environ.get("MON_TRACE_SRC"):      # the golden now holds this tree's own messages: nothing is reworded against it
        open(REWORDED, "w").close()
    print("recorded %d lines into %s" % (len(text.splitlines()), GOLDEN))
