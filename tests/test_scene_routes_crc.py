"""The scene and pose routes' outputs, bit for bit against the build of the commit before their host boundary was written once (scene.cpp's *_check
functions, scene_models, scene_levels, pose_inout).

That refactor touched no kernel and no launch line, and tests/test_launch_trace.py holds every launch, grid, stream and copy size of these routes.  What a
launch trace cannot see is a kernel ARGUMENT: an offset into an output row, a pointer into the level-weight table, the in-out pose that is copied around a
refinement.  So every public scene route and the object's coarse-to-fine refinement is called once on each side, and the CRC32 of every array it returns must
equal the one recorded from the parent commit's build on an MI355X:

    tools/variant_build.sh parent          # in a checkout of the parent commit
    MON_CORE_LIB=<that checkout>/ro-map_amd/build_parent/libmon_core.so python tests/test_scene_routes_crc.py --record

conftest's small_scene (120 x 160, 12 views), two base.json objects on its one object (the second on a box 1.5 times as large) with fixed sample seeds, 60
steps each.  The shapes cross what the host computes offsets for: the full frame is 19 200 pixels (a pass boundary at 16 384), the probe and the cast take
16 384 + 100 items, the batch scores 5 poses x 4000 drawn rays (passes of 4 and 1), the window has 3 frames and refines the objects, relocalisation keeps 2 of
6 candidates.  The field queries (scene_field.cpp) joined when their host chain was written once, recorded in the same way from the commit before that one ("Add
connected components over a lattice of the object map"); the nine routes above came out of that record as they stood.  They take 16 384 + 100 world points
over the larger box (the gradients with a select and level weights that are not all ones), as many unit-cube points on the first object, and one lattice of
33 x 32 x 17 around the objects for the lattice query, the lattice gradients, the distance field (truncated with free_dist, untruncated without) and the
components (region 0, 26-connected, with its table; region 1, 6-connected, with dist, sigma and owner).  sigma_min is the 90th percentile of the lattice
query's own sigma; between 1 % and 99 % of the cells must be occupied before the distance and component calls are made.
The cost fields and the device-resident distance fields (scene_field.cpp, dist_field.cpp) joined before their host chains were written once, recorded in the
same way from the commit before ("Add scan matching against a device-resident distance field"); every CRC above came out of that record as it stood.  On the
same lattice and sigma_min: the cost field, 26-connected with clearance = the largest step, a soft cost of weight 2 within three such steps and every
optional output, from the three traversable cells of lowest flat index; the same 6-connected without a soft cost, cost alone, cut at a quarter of the
lattice's diagonal (between 1 % and 99 % of the cells must have a finite cost in either); the distance field kept on the device, cut at a quarter of the
diagonal, read back with its description; and on that handle its samples with gradients at the first 1 000 world points, the scores of 8 trajectories of 5
matrix waypoints (n_sub 3, two spheres, every output), the match of a scan under 4 pose hypotheses with the normal equations, and their registration
(the defaults with max_evals 6, every output).  The scan is the first 1 000 lattice points whose distance is below one step (there must be 1 000), and at
least one hypothesis must end with a status other than 3.  These kernels use no float atomics.
Side 1 is compared only when render_snapshot reports step 60 for both objects; otherwise the case fails.  The online routes are left out:
what their snapshots hold depends on thread timing.

Bit equality is the condition: there is no tolerance."""
import ctypes as C
import json
import math
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_routes_parent_crc.json")
SCENE = dict(n_views=12, H=120, W=160, f=130.0, seed=0)          # (conftest's small_scene)
KW = (dict(sample_seed=5), dict(sample_seed=7))                  # base.json otherwise
INFLATE = (1.0, 1.5)
STEPS = 60
VIEWS = (3, 4, 5)                                                # the window's frames; VIEWS[0]: the frame of the single-frame routes
N_ITEMS = 16384 + 100                                            # probe queries and cast rays: one pass boundary
ROUTES = ("render_scene", "probe_scene", "cast_scene", "scene_pose_loss", "scene_refine_camera", "scene_pose_loss_batch", "scene_refine_window",
          "scene_relocalise", "refine_pose_c2f",
          "query_scene_points", "query_scene_lattice", "query_scene_gradients", "query_scene_lattice_gradients", "cast_scene_normals",
          "scene_distance_lattice", "scene_distance_lattice_untruncated", "scene_components_lattice", "scene_components_lattice_free",
          "object_query_points", "object_query_gradients",
          "scene_paths_lattice", "scene_paths_lattice_plain", "scene_dist_field", "dist_field_sample", "dist_field_score", "dist_field_match",
          "dist_field_register")
LATTICE = (33, 32, 17)                                           # 17 952 cells: one pass boundary, the field routes' common lattice


def _crc(a):
    return "%08x" % zlib.crc32(np.ascontiguousarray(a).tobytes())


def make_objects(pkg, ss, sc):
    """the dataset and the two objects, trained and published at step STEPS"""
    ds, o0 = ge.make_problem(pkg, sc, KW[0])
    ob = sc.objects[0]
    o1 = pkg.ObjectNeRF(ds, pkg.default_config(**KW[1]), ob["cls"], ss.colmajor(ob["Tow"]), -ob["half"] * INFLATE[1], ob["half"] * INFLATE[1])
    o1.add_boxes(ob["boxes"])
    box = _boxes(sc, VIEWS[:1])[0]
    for o in (o0, o1):
        o.train(STEPS - 1)
        try:                                                     # a viewer asks, so that the next train call publishes whatever the clock says
            o.render_snapshot(box, ss.colmajor(sc.Twc[VIEWS[0]]))
        except Exception:                                        # (nothing published yet: the request stands all the same)
            pass
        o.train(1)
    return ds, [o0, o1]


def _boxes(sc, views):
    return np.array([[q for q in sc.objects[0]["boxes"] if int(q[0]) == v][0] for v in views], np.uint32)


def _field_inputs(sc):
    """world points over the larger object's box, unit-cube points, the lattice around the objects (10 % margin)"""
    ob = sc.objects[0]; rs = np.random.RandomState(23)
    half = np.asarray(ob["half"], np.float64) * max(INFLATE); R, t = ob["Two"][:3, :3], ob["Two"][:3, 3]
    world = (rs.uniform(-1.1, 1.1, (N_ITEMS, 3)) * half) @ R.T + t
    unit = rs.uniform(0.0, 1.0, (N_ITEMS, 3))
    select = rs.randint(-1, 2, N_ITEMS)
    c = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * half @ R.T + t
    lo, hi = c.min(0), c.max(0); pad = 0.1 * (hi - lo); lo -= pad; hi += pad
    return world.astype(np.float32), unit.astype(np.float32), select.astype(np.int32), lo.astype(np.float32), ((hi - lo) / (np.array(LATTICE) - 1)).astype(np.float32)


def _components_arrays(r):
    label, comp, table, n, rows = r
    return [label, comp, table, np.uint32(n)] + [rows[k] for k in sorted(rows)]


def _paths_cost_only(pkg, objs, origin, step, smin, seeds, clearance, max_cost, side):
    """mon_scene_paths_lattice, 6-connected without a soft cost, every output but cost NULL (the binding's call always asks for next)"""
    P = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
    hs = (C.c_void_p * len(objs))(*[o.h for o in objs]); sd = np.ascontiguousarray(seeds, np.int32); cost = np.empty(int(np.prod(LATTICE)), np.float32)
    rc = pkg.lib().mon_scene_paths_lattice(hs, len(objs), side, P(origin), P(step), *LATTICE, smin, clearance, 0.0, 0.0, 6, P(sd), sd.size, max_cost, P(cost),
                                           None, None, None, None)
    assert rc == 0, pkg.lib().mon_last_error()
    return cost


def _rotations(rs, n, max_angle):
    """n rotation matrices by Rodrigues' formula: a random axis, an angle of up to max_angle"""
    out = np.empty((n, 3, 3))
    for k in range(n):
        a = rs.normal(size=3); a /= np.linalg.norm(a); t = rs.uniform(-max_angle, max_angle)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        out[k] = np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)
    return out


def run_lattice_routes(pkg, objs, side, origin, step, smin, dist, world):
    """the cost fields and the device-resident distance field with its sample, score, match and register calls: {route: every array it returns}.
    dist: scene_distance_lattice's untruncated row, which says where a seed may stand and where the scan lies."""
    n = int(np.prod(LATTICE)); h = float(step.max()); diag = float(np.linalg.norm(step * (np.array(LATTICE) - 1)))
    seeds = np.flatnonzero(dist > np.float32(h))[:3].astype(np.int32)
    assert seeds.size == 3, seeds
    out = {}
    cost, nxt, rows = pkg.scene_paths_lattice(objs, origin, step, LATTICE, smin, seeds, clearance=h, soft_radius=3.0 * h, soft_weight=2.0, connectivity=26,
                                              side=side, rows=("dist", "sigma", "owner"))
    out["scene_paths_lattice"] = [cost, nxt, rows["dist"], rows["sigma"], rows["owner"]]
    out["scene_paths_lattice_plain"] = [_paths_cost_only(pkg, objs, origin, step, smin, seeds, h, 0.25 * diag, side)]
    for k in ("scene_paths_lattice", "scene_paths_lattice_plain"):
        n_fin = int(np.isfinite(out[k][0]).sum())
        print("side %d: %s: %d of %d cells have a finite cost" % (side, k, n_fin, n))
        assert n // 100 <= n_fin <= n - n // 100, (k, n_fin, n)
    scan = pkg.lattice_points(origin, step, LATTICE)[np.flatnonzero(dist < np.float32(h))[:1000]]
    assert scan.shape == (1000, 3), scan.shape
    rs = np.random.RandomState(29); centre = scan.mean(0, dtype=np.float64)
    # 4 hypotheses about the identity (the scan is in world coordinates), turned about the scan's centre; row-major for the match calls
    hyp = pkg.pose_hypotheses(np.eye(4, dtype=np.float32).reshape(16), 4, math.radians(2.0), 0.5 * h, pivot=centre, seed=4)
    poses = np.ascontiguousarray(hyp.reshape(4, 4, 4).transpose(0, 2, 1))
    lo = origin.astype(np.float64); ext = step.astype(np.float64) * (np.array(LATTICE) - 1)
    ways = np.zeros((8, 5, 4, 4)); ways[:, :, 3, 3] = 1.0
    ways[:, :, :3, :3] = _rotations(rs, 40, 0.5).reshape(8, 5, 3, 3); ways[:, :, :3, 3] = lo + rs.uniform(0.05, 0.95, (8, 5, 3)) * ext
    spheres = np.array([[0.0, 0.0, 0.0, 0.5 * h], [h, 0.0, 0.5 * h, 0.25 * h]], np.float32)
    with pkg.scene_dist_field(objs, origin, step, LATTICE, smin, 0.25 * diag, side=side) as f:
        d = f.info()
        out["scene_dist_field"] = [f.read(), np.array([d.nx, d.ny, d.nz, d.device, *d.origin, *d.step, d.max_value], np.float32)]
        out["dist_field_sample"] = f.sample(world[:1000], outside=0.25 * diag, grad=True)
        sc_ = f.score(spheres, ways.astype(np.float32), n_sub=3, outside=0.25 * diag, margin=0.5 * h, safe=2.0 * h)
        out["dist_field_score"] = [sc_[k] for k in ("min_clear", "first_hit", "cost", "way_clear", "way_grad")]
        m = f.match(scan, poses, pivots=np.tile(centre, (4, 1)), huber=2.0 * h, outside=0.25 * diag, normal=True)
        out["dist_field_match"] = [m[k] for k in ("cost", "n_inside", "n_inlier", "A", "b")]
        r = f.register(scan, poses, max_evals=6)
        print("side %d: register: status %s, evals %s, best %d" % (side, r["status"], r["evals"], r["best"]))
        assert (r["status"] != 3).any(), r["status"]
        out["dist_field_register"] = [r[k] for k in ("poses", "cost", "n_inside", "n_inlier", "evals", "status")] + [np.int32(r["best"])]
    return out


def run_field_routes(pkg, objs, rays, side, sc):
    """the field queries (scene_field.cpp): {route: every array it returns}"""
    world, unit, select, origin, step = _field_inputs(sc)
    L = max(o.cfg.n_levels for o in objs); lw = np.where(np.arange(L) % 2 == 0, 1.0, 0.5).astype(np.float32)
    out = {}
    out["query_scene_points"] = pkg.query_scene_points(objs, world, side=side)
    out["query_scene_lattice"] = pkg.query_scene_lattice(objs, origin, step, LATTICE, side=side)
    out["query_scene_gradients"] = pkg.query_scene_gradients(objs, world, level_weights=lw, select=select, side=side)
    out["query_scene_lattice_gradients"] = pkg.query_scene_lattice_gradients(objs, origin, step, LATTICE, level_weights=lw, side=side)
    out["cast_scene_normals"] = pkg.cast_scene_normals(objs, rays, side=side)
    sigma = out["query_scene_lattice"][0]; n = sigma.size
    smin = float(np.percentile(sigma, 90.0, method="lower"))          # (tests/test_scene_distance.py::_sigma_min)
    n_occ = int((~(sigma <= np.float32(smin))).sum())
    print("side %d: sigma_min %.5g, %d of %d cells occupied" % (side, smin, n_occ, n))
    assert n // 100 <= n_occ <= n - n // 100, (n_occ, n)
    diag = float(np.linalg.norm(step * (np.array(LATTICE) - 1)))
    out["scene_distance_lattice"] = pkg.scene_distance_lattice(objs, origin, step, LATTICE, smin, max_dist=0.25 * diag, side=side, free=True)
    out["scene_distance_lattice_untruncated"] = [a for a in pkg.scene_distance_lattice(objs, origin, step, LATTICE, smin, side=side, free=False)
                                                 if a is not None]
    out["scene_components_lattice"] = _components_arrays(pkg.scene_components_lattice(objs, origin, step, LATTICE, smin, region=0, connectivity=26, side=side))
    out["scene_components_lattice_free"] = _components_arrays(pkg.scene_components_lattice(
        objs, origin, step, LATTICE, smin, region=1, clearance=float(step.max()), connectivity=6, side=side, rows=("dist", "sigma", "owner")))
    out["object_query_points"] = (pkg.query_object_points(objs[0], unit, side=side),)
    out["object_query_gradients"] = pkg.query_object_gradients(objs[0], unit, level_weights=lw[:objs[0].cfg.n_levels], side=side)
    out.update(run_lattice_routes(pkg, objs, side, origin, step, smin, out["scene_distance_lattice_untruncated"][0], world))
    return out


def run_routes(pkg, ss, sc, objs, side):
    """{route: [CRC32 of every array it returns]} on one side"""
    v0 = VIEWS[0]; T16 = ss.colmajor(sc.Twc[v0]); box = _boxes(sc, VIEWS[:1])
    rs = np.random.RandomState(11)
    q = pkg.scene_queries(rs.randint(0, 2, N_ITEMS), np.arange(N_ITEMS), rs.uniform(0, sc.W - 1, N_ITEMS), rs.uniform(0, sc.H - 1, N_ITEMS))
    Twc2 = np.stack([ss.colmajor(sc.Twc[v]) for v in VIEWS[:2]])
    rays, _ = pkg.camera_rays((sc.fx, sc.fy, sc.cx, sc.cy), Twc2, q)
    off = pkg.pose_hypotheses(T16, 6, math.radians(6.0), 0.03, seed=4)          # candidate 0: the frame's pose, 1..5 around it
    p3 = pkg.pose_refine_default(iters=3, rays_per_iter=512)
    wobs = _boxes(sc, VIEWS); Twc3 = np.stack([off[1], off[2], off[3]]); Tow = np.stack([ss.colmajor(sc.objects[0]["Tow"])] * 2)
    out = {}
    out["render_scene"] = pkg.render_scene(objs, (v0, 0, 0, sc.H, sc.W), T16, side=side)
    out["probe_scene"] = pkg.probe_scene(objs, q, Twc2, side=side)
    out["cast_scene"] = pkg.cast_scene(objs, rays, side=side)
    loss, g = pkg.scene_pose_loss(objs, box, off[1], pkg.pose_refine_default(rays_per_iter=512), side=side, iteration=5)
    out["scene_pose_loss"] = (np.float32(loss), g)
    out["scene_refine_camera"] = pkg.scene_refine_camera(objs, box, off[1], p3, c2f=True, side=side)
    out["scene_pose_loss_batch"] = (pkg.scene_pose_loss_batch(objs, box, off[:5], pkg.pose_refine_default(rays_per_iter=4000), side=side, iteration=5),)
    out["scene_refine_window"] = pkg.scene_refine_window(objs, wobs, Twc3, Tow, p3, window=dict(n_fixed_frames=1, refine_objects=1), side=side)
    pose, res, scores = pkg.scene_relocalise(objs, box, off, p3, reloc=pkg.reloc_default(keep=2, score_rays=256), side=side)
    out["scene_relocalise"] = (pose, np.array([res.best_candidate, res.refined], np.uint32),
                               np.array([res.score_candidate0, res.score_best_candidate, res.score_final], np.float32), scores)
    out["refine_pose_c2f"] = objs[0].refine_pose_c2f(box, Tow[0], p3, side=side)
    out.update(run_field_routes(pkg, objs, rays, side, sc))
    assert set(out) == set(ROUTES)
    return {k: [_crc(a) for a in v] for k, v in out.items()}


def snapshot_steps(ss, sc, objs):
    return [int(o.render_snapshot(_boxes(sc, VIEWS[:1])[0], ss.colmajor(sc.Twc[VIEWS[0]]))[-1]) for o in objs]


@pytest.fixture(scope="module")
def crcs(pkg, ss, small_scene):
    """every route on both sides, once for all cases"""
    assert pkg.device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    ds, objs = make_objects(pkg, ss, small_scene)
    steps = snapshot_steps(ss, small_scene, objs)
    got = {side: run_routes(pkg, ss, small_scene, objs, side) for side in (0, 1)}
    for o in objs:
        o.close()
    ds.close()
    return steps, got


@pytest.mark.gpu
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("route", ROUTES)
def test_route_returns_the_parent_builds_bits(crcs, route, side):
    steps, got = crcs
    with open(GOLDEN) as f:
        want = json.load(f)[str(side)][route]
    print(route, side, got[side][route], want, steps)
    if side == 1:
        assert steps == [STEPS, STEPS], "side 1 does not hold the objects' final step: %s" % (steps,)
    assert got[side][route] == want, (route, side, got[side][route], want)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: MON_CORE_LIB=<library of the parent commit> python tests/test_scene_routes_crc.py --record")
    pkg_, ss_ = ge.load_package(), ge.load_tools()
    sc_ = ss_.make_scene(**SCENE)
    ds_, objs_ = make_objects(pkg_, ss_, sc_)
    assert snapshot_steps(ss_, sc_, objs_) == [STEPS, STEPS]
    rec = {str(side): run_routes(pkg_, ss_, sc_, objs_, side) for side in (0, 1)}
    print(json.dumps(rec))
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=1); f.write("\n")
