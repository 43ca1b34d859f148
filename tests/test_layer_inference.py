"""GPU tests (-m gpu) of the LAYER CHAIN, the one inference route of every network shape the fused kernels do not take (16 neurons, 2 x 128, three and
four hidden layers) and of backend 0 on a fused shape: k_render_rays, k_gen_samples, k_encode, k_mlp_fwd_all in inference mode with k_mlp_forward on a tail
of fewer than 32 samples, k_composite_render, k_grid_points, k_mesh_warp, k_extract_density -- at TRAINED weights against the fp64 references of
tests/render_reference.py (tests/test_layer_inference_reference.py holds those to the CPU oracle first).

One object per instantiation of k_mlp_fwd_all<EPAD, W>, the deepest network each width allows among them, and c2s (64 x 1, a fused shape) under
set_backend(0), where the whole chain runs on k_mlp_forward; 300 steps on the device, 2048 rays per batch, so that the debug read-back (the first R S entries
of pts, tdist, E, O and the first R ray rows) holds a whole pass of R / 2 = 1024 rays.
  (a) one 32 x 32 crop, one pass: ray_flag against the independent slab restatement (rays the restated row cannot decide set aside, <= 1 %); tdist and
      pts of the hit rays bit for bit from the device's own ray rows, zero on a miss; E bit for bit from orc_encode at the device's own pts; every O of
      every hit sample within delta of raw_bounds; the image within the counted bound of composite_render64 of the device's OWN O, tdist, ray rows, the mask
      equal outside the ambiguous rays (<= 1 %), a missed or masked-out pixel exactly white / 0 / 0; on c2s O bit for bit from orc_mlp_forward
  (b) a 160 x 108 rect, 17 280 rays, under a tilted camera that puts the object into its last rows: the buffers then hold the last pass, rays 16 384 and up (the second pass of 16 384 rays on the layer shapes; on c2s
      under backend 0 a pass is R / 2 = 1 024 rays and it is the seventeenth, beginning at the same ray) -- its tdist and pts at the jitter indices
      p0 2S + s, its pixels the composite of its own buffers, the whole image against orc_render on the same weights at the bars of
      test_render_matches_oracle_and_golden
  (c) density_grid on 3 x 3 x 3 (all tail), 4 x 4 x 2 (no tail), 7 x 5 x 3, 17^3, 9 x 9 x 5 and 129 x 129 x 65 (two chunks of the layer shapes: 2^20 points,
      eight trips of the grid-stride loop, then 1 034 tiles and a tail of one): every point within delta (on the big lattice 8 192 random points of chunk
      one and all of chunk two); the points of 9 x 9 x 5 that are MFMA body points there and in 129 x 129 x 65 carry the same bits in both, wherever
      tile, lane, wave, trip or chunk puts them; the tail points, and on c2s all points, bit for bit from orc_mlp_forward on the device's own E
  (d) generate_mesh(32, 2.0) on 16 x 1 and 64 x 3: geometry bit for bit from orc.marching_cubes of the device's own lattice, every colour inside
      colour_of's interval of raw_bounds at the restated warp, regenerating gives the same bytes
The regime (raw3 max >= 6, >= 25 % of the hit rays break before sample 64) is asserted from the reference's wanted values.

Measured on an MI355X: DESIGN.md section 1, "Layer-chain inference at trained weights" (this file's output with -s)."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import field_grad_reference as fgr
import pose_reference as pr
import render_reference as rref
import stage_reference as sr
from test_gpu_mesh import _same_mesh

pytestmark = pytest.mark.gpu

R = 2048
PASS_RAYS = 16384            # kRenderChunkRays
LAYER_CHUNK = PASS_RAYS * 64  # ws_samples of a layer shape: samples per lattice chunk (c2s: R S)
READ = R * 32                # samples the read-back returns
SHAPES = {"16x1": dict(n_neurons=16, n_hidden_layers=1),                                   # Epad 32, W 16
          "16x4L5": dict(n_neurons=16, n_hidden_layers=4, n_levels=5),                     # Epad 16, W 16
          "32x3": dict(n_neurons=32, n_hidden_layers=3),                                   # Epad 32, W 32
          "32x4L8": dict(n_neurons=32, n_hidden_layers=4, n_levels=8),                     # Epad 16, W 32
          "64x3": dict(n_neurons=64, n_hidden_layers=3),                                   # Epad 32, W 64
          "64x4L6": dict(n_neurons=64, n_hidden_layers=4, n_levels=6),                     # Epad 16, W 64
          "128x2": dict(n_neurons=128, n_hidden_layers=2),                                 # Epad 32, W 128
          "128x2L6": dict(n_neurons=128, n_hidden_layers=2, n_levels=6),                   # Epad 16, W 128
          "c2s": dict(n_neurons=64, n_hidden_layers=1)}                                    # a fused shape under set_backend(0): k_mlp_forward throughout
MESH = ("16x1", "64x3")
SMALL = [(3, 3, 3), (4, 4, 2), (7, 5, 3), (17, 17, 17), (9, 9, 5)]
BIG = (129, 129, 65)
P_ = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _Shape:
    """one trained object, the oracle model that lends orc_encode / orc_mlp_forward / orc_render its shape, and the results every test shares"""

    def __init__(self, name, pkg, orc, sc, ds):
        kw = dict(SHAPES[name], rays_per_batch=R); self.name = name; self.fused = name == "c2s"
        self.ds, self.o = ge.make_problem(pkg, sc, kw, dataset=ds)
        if self.fused:
            self.o.set_backend(0)
        assert int(self.o.info().backend) == 0
        assert np.isfinite(self.o.train(300))
        self.net = fgr.net_of_object(self.o, orc)                             # the EMA weights: what a render reads once step > 0
        self.ref = ge.make_oracle(orc, sc, kw); self.ref.set_ema(self.net["params"])
        assert self.ref.Epad == self.net["Ep"] and self.ref.n_mlp == self.net["n_mlp"]
        self.chunk = READ if self.fused else LAYER_CHUNK
        self.cache = {}

    def close(self):
        self.o.close(); self.ref.close()

    def encode(self, u):
        u = np.ascontiguousarray(u, np.float32).reshape(-1, 3); n = u.shape[0]; E = np.zeros((n, self.ref.Epad), np.uint16)
        self.ref.L.orc_encode(self.ref.h, P_(self.net["params"]), P_(u), n, P_(E)); return E

    def mlp(self, E):
        E = np.ascontiguousarray(E, np.uint16); n = E.shape[0]; hid = np.zeros(n * self.ref.W * self.ref.NH, np.uint16); O = np.zeros((n, 4), np.uint16)
        self.ref.L.orc_mlp_forward(self.ref.h, P_(self.net["params"]), P_(E), n, P_(hid), P_(O)); return O

    def read(self, n_rays=0, n_samples=0):
        """the read-back of the last pass: ray rows [n_rays, 10] (o, d, t0, t1, flag, dn) and pts, tdist, E, O of the first n_samples samples"""
        o = self.o; out = {}
        if n_rays:
            b = {k: o.buffer("ray_" + k) for k in ("o", "d", "t0", "t1", "flag", "dn")}
            out["rows"] = np.column_stack([b["o"].reshape(-1, 3), b["d"].reshape(-1, 3), b["t0"], b["t1"], b["flag"].astype(np.float32), b["dn"]])[:n_rays]
        Ep = self.net["Ep"]
        out.update(pts=o.buffer("pts").reshape(-1, 3)[:n_samples], tdist=o.buffer("tdist")[:n_samples], E=o.buffer("E").reshape(-1, Ep)[:n_samples],
                   O=o.buffer("O").reshape(-1, 4)[:n_samples])
        return out


@pytest.fixture(scope="module")
def pool(pkg, orc, small_scene):
    """the shapes, each trained once, on first use"""
    assert pkg.device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Shape(name, pkg, orc, small_scene, next(iter(made.values())).ds if made else None)      # (one resident dataset)
        return made[name]
    yield get
    for s in made.values():
        s.close()
    if made:
        next(iter(made.values())).ds.close()


@pytest.fixture(scope="module", params=sorted(SHAPES))
def shape(request, pool):
    return pool(request.param)


def _scene_box(sc):
    ob = sc.objects[0]
    return ob, np.stack([-ob["half"], ob["half"]]).astype(np.float32)


def _check_pass(sh, sc, rect, which, rd, img):
    """One pass of a render, from its read-back rd (rows and sample buffers of the rays `which` of the rect) and its pixels img = (rgb, depth, mask):
    samples bit for bit from the device's rows, the pixels within the counted bound of the composite of the device's own buffers.  Returns what (a) goes on
    to check."""
    ob, aabb = _scene_box(sc); n = which.size; rows = rd["rows"]
    hit = rows[:, 8] > 0
    smp = rref.samples(sc, rect, ob["Tow"], aabb, ob["cls"], int(sh.o.cfg.sample_seed), which=which, rows=rows)
    tdist = rd["tdist"].reshape(n, 64); pts = rd["pts"].reshape(n, 64, 3)
    assert np.array_equal(_bits(tdist)[hit], _bits(smp["t"])[hit]), int((_bits(tdist) != _bits(smp["t"]))[hit].sum())
    assert np.array_equal(_bits(pts)[hit], _bits(smp["u"])[hit]), int((_bits(pts) != _bits(smp["u"]))[hit].sum())
    assert not _bits(tdist)[~hit].any() and not _bits(pts)[~hit].any()
    cr = rref.composite_render64(rd["O"].reshape(n, 64, 4), tdist, hit, rows[:, 9])
    rgb, depth, mask = (np.asarray(v, np.float64) for v in img)
    ok = ~cr["amb"]
    assert cr["amb"].sum() <= 0.01 * max(1, hit.sum()), (int(cr["amb"].sum()), int(hit.sum()))
    assert set(np.unique(mask)) <= {0.0, 1.0} and np.array_equal(mask[ok], cr["mask"][ok]), int((mask != cr["mask"])[ok].sum())
    off = mask == 0
    assert not (mask[~hit] != 0).any() and (rgb[off] == 1.0).all() and (depth[off] == 0.0).all()
    j = ok & (mask > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        use_rgb = (np.abs(rgb - cr["rgb"]) / cr["e_rgb"])[j]; use_d = (np.abs(depth - cr["depth"]) / cr["e_depth"])[j]
    print("%s: pass of %d rays, %d hit, %d masked in: share of the composite bound used, worst: rgb %.3f depth %.3f; ambiguous rays %d" % (
        sh.name, n, hit.sum(), j.sum(), use_rgb.max() if j.any() else 0.0, use_d.max() if j.any() else 0.0, cr["amb"].sum()))
    assert (np.abs(rgb - cr["rgb"]) <= cr["e_rgb"])[ok].all() and (np.abs(depth - cr["depth"]) <= cr["e_depth"])[ok].all()
    return smp, hit, cr, tdist, pts


# ------------------------------------------------------------------ (a)
def test_render_stages_single_pass(shape, ss, small_scene):
    sh = shape; sc = small_scene; ob, aabb = _scene_box(sc)
    rect, score = rref.choose_crop(sc, 0, 32)
    assert score >= 100, (rect, score)
    P = 32 * 32; assert P <= R // 2
    rgb, depth, mask = sh.o.render(rect, ss.colmajor(sc.Twc[int(rect[0])]))
    rd = sh.read(P, P * 64); which = np.arange(P)
    # ray_flag against the independent restatement of the ray row and the slab test
    own = pr.pose_rays(sc, [rect], ob["Tow"], aabb, ob["cls"], n_rays=0, sample_seed=int(sh.o.cfg.sample_seed))
    edge = rref.slab_edge(sc, int(rect[0]), ob["Tow"], aabb, own)
    flag = rd["rows"][:, 8] > 0
    print("%s: (a) rays near a slab edge %d of %d; the NumPy pixel_ray reproduces the device's t0 bit for bit on %.3f of the hit rays" % (
        sh.name, edge.sum(), P, (_bits(own["t0"]) == _bits(rd["rows"][:, 6]))[flag].mean()))
    assert edge.sum() <= 0.01 * P and np.array_equal(flag[~edge], own["hit"][~edge]), int((flag != own["hit"])[~edge].sum())
    smp, hit, cr, tdist, pts = _check_pass(sh, sc, rect, which, rd, (rgb.reshape(-1, 3), depth.reshape(-1), mask.reshape(-1)))
    # E: the oracle's encode at the device's own points, every sample of the pass
    assert np.array_equal(rd["E"], sh.encode(rd["pts"]))
    # O: every output of every hit sample within delta
    raw = np.zeros((P, 64, 4)); delta = np.zeros((P, 64, 4))
    r, d = rref.raw_bounds(sh.net, pts[hit].reshape(-1, 3)); raw[hit] = r.reshape(-1, 64, 4); delta[hit] = d.reshape(-1, 64, 4)
    got = sr.h2d(rd["O"]).reshape(P, 64, 4)
    ratio = (np.abs(got - raw)[hit] / delta[hit])
    rg = rref.chain_regime(raw, tdist, hit, rd["rows"][:, 9])
    print("%s: (a) regime %s" % (sh.name, rg))
    print("%s: (a) %d samples: |O - want| / delta worst %.3f median %.3g; equal fp16 on %.5f; delta3 median %.3g worst %.3g" % (
        sh.name, hit.sum() * 64, ratio.max(), np.median(ratio), (got == raw)[hit].mean(), np.median(delta[hit][..., 3]), delta[hit][..., 3].max()))
    assert rg["raw_max"] >= sr.REGIME_BARS["raw_max"] and rg["cut_share"] >= sr.REGIME_BARS["cut_share"], rg
    assert min(rg["n_in"], rg["n_out"], rg["n_miss"]) >= 100 and rg["n_amb"] <= 0.01 * rg["n_hit"], rg
    assert (ratio <= 1.0).all(), (float(ratio.max()), int((ratio > 1).sum()))
    if sh.fused:                                                              # k_mlp_forward: fp32 sums in the oracle's order
        assert np.array_equal(rd["O"], sh.mlp(rd["E"])), int((rd["O"] != sh.mlp(rd["E"])).sum())


# ------------------------------------------------------------------ (b)
def _two_pass_case(sc):
    """(rect, Twc, hits): a 160 x 108 rect (FrameId, x, y, h, w; 17 280 rays, 896 after ray 16 384) and its view's camera tilted about its own x axis so
    that the object's centre projects onto the row where ray 16 384 lies -- no dataset pose puts the object into a rect's last rows --, with the number
    of rays after ray 16 384 that hit object 0's box; decided from the scene's geometry alone.  The render takes any pose; the samples are restated from
    the device's own ray rows."""
    ob, aabb = _scene_box(sc); K4 = np.array([sc.fx, sc.fy, sc.cx, sc.cy]); best = None
    centre = np.linalg.inv(np.asarray(ob["Tow"], np.float64)) @ np.array([0.0, 0.0, 0.0, 1.0])
    for v in range(sc.n_views):
        for th in np.linspace(-0.7, 0.7, 141):
            c, s = np.cos(th), np.sin(th); T = np.asarray(sc.Twc[v], np.float64).copy(); T[:3, :3] = T[:3, :3] @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
            pc = np.linalg.inv(T) @ centre
            if pc[2] <= 0 or not 40 <= sc.fx * pc[0] / pc[2] + sc.cx <= 120:
                continue
            off = abs(sc.fy * pc[1] / pc[2] + sc.cy - PASS_RAYS / 160.0)
            if best is None or off < best[0]:
                best = (off, np.array([v, 0, 0, 108, 160], np.uint32), T)
    q = np.arange(PASS_RAYS, 160 * 108)
    o, d, _ = pr.camera_rays(K4, best[2], ob["Tow"], q % 160, q // 160)
    return best[1], best[2], int(pr.slab(aabb, o, d)[0].sum())


def test_two_passes(shape, ss, small_scene):
    sh = shape; sc = small_scene
    assert sc.W == 160 and sc.H == 120
    if "case" not in _two_pass_case.__dict__:
        _two_pass_case.case = _two_pass_case(sc)                              # (once for the module's scene)
    rect, Twc, n_hit = _two_pass_case.case
    assert n_hit >= 200, (rect, n_hit)
    P = int(rect[3]) * int(rect[4]); n2 = P - PASS_RAYS; which = np.arange(PASS_RAYS, P)      # (c2s: 16 passes of R / 2 = 1024 rays come first; the last begins here too)
    assert PASS_RAYS % (R // 2) == 0 and 0 < n2 <= R // 2
    pose = ss.colmajor(Twc)
    rgb, depth, mask = sh.o.render(rect, pose)
    rgb = rgb.reshape(-1, 3); depth = depth.reshape(-1); mask = mask.reshape(-1)
    rd = sh.read(n2, n2 * 64)
    _, hit, _, _, _ = _check_pass(sh, sc, rect, which, rd, (rgb[PASS_RAYS:], depth[PASS_RAYS:], mask[PASS_RAYS:]))
    assert hit.sum() >= 200 and (mask[PASS_RAYS:] > 0).sum() >= 30 and (mask[:PASS_RAYS] > 0).sum() >= 30, (int(hit.sum()), int((mask[PASS_RAYS:] > 0).sum()))
    orgb, odepth, omask = sh.ref.render(rect, pose)
    orgb = orgb.reshape(-1, 3); odepth = odepth.reshape(-1); omask = omask.reshape(-1)
    flips = float((mask != omask).mean()); same = mask == omask
    print("%s: (b) %d rays, %d masked in (%d in the last pass); against orc_render: flips %.4g, rgb %.3g, depth %.3g" % (
        sh.name, P, (mask > 0).sum(), (mask[PASS_RAYS:] > 0).sum(), flips, np.abs(rgb - orgb)[same].max(), np.abs(depth - odepth)[same].max()))
    assert flips < 5e-3
    assert np.abs(rgb - orgb)[same].max() < 4e-3 and np.abs(depth - odepth)[same].max() < 4e-3


# ------------------------------------------------------------------ (c)
def _lattice(sh, res3):
    """density_grid once per shape and lattice, with the read-back of its last chunk and the checks every lattice gets: the last chunk's points are
    lattice_u's, its E the oracle's encode of them, its O's fourth channel what density_grid returned, and its tail points (every point on c2s) the
    oracle's MLP on the device's own E, bit for bit"""
    if res3 in sh.cache:
        return sh.cache[res3]
    total = res3[0] * res3[1] * res3[2]
    dens = sh.o.density_grid(*res3)
    u = rref.lattice_u(*res3)
    p0 = (total - 1) // sh.chunk * sh.chunk; n_last = total - p0; nr = min(n_last, READ)
    rd = sh.read(0, nr)
    assert np.array_equal(_bits(rd["pts"]), _bits(u[p0:p0 + nr]))
    assert np.array_equal(rd["E"], sh.encode(rd["pts"]))
    assert np.array_equal(sr.h2d(rd["O"])[:, 3], dens[p0:p0 + nr].astype(np.float64))
    body = 0 if sh.fused else (n_last & ~31)                                  # mlp_forward_inference: n & ~31 on the MFMA kernel, the rest per sample
    assert body <= nr or body == n_last
    if body < nr:
        want = sh.mlp(rd["E"][body:])
        assert np.array_equal(rd["O"][body:], want), (res3, int((rd["O"][body:] != want).sum()))
    sh.cache[res3] = dict(dens=dens, u=u, p0=p0, n_last=n_last, body=body, total=total)
    return sh.cache[res3]


def _within_delta(sh, lat, idx, tag):
    raw, delta = rref.raw_bounds(sh.net, lat["u"][idx])
    ratio = np.abs(lat["dens"][idx].astype(np.float64) - raw[:, 3]) / delta[:, 3]
    print("%s: (c) %s: %d points, |raw3 - want| / delta worst %.3f median %.3g; equal fp16 on %.5f; delta3 median %.3g; raw3 max %.2f" % (
        sh.name, tag, idx.size, ratio.max(), np.median(ratio), (lat["dens"][idx] == raw[:, 3]).mean(), np.median(delta[:, 3]), raw[:, 3].max()))
    assert (ratio <= 1.0).all(), (tag, float(ratio.max()), int((ratio > 1).sum()))


@pytest.mark.parametrize("res3", SMALL, ids=["x".join(str(r) for r in q) for q in SMALL])
def test_small_lattices(shape, res3):
    lat = _lattice(shape, res3)
    assert lat["p0"] == 0 and (shape.fused or lat["body"] == {27: 0, 32: 32, 105: 96, 4913: 4896, 405: 384}[lat["total"]])
    _within_delta(shape, lat, np.arange(lat["total"]), "x".join(str(r) for r in res3))


def test_big_lattice(shape):
    sh = shape; lat = _lattice(sh, BIG)
    assert lat["total"] == 1081665 and lat["n_last"] == 33089 and lat["p0"] % LAYER_CHUNK == 0 and (sh.fused or (lat["p0"] == 1 << 20 and lat["body"] == 33088))
    first = np.sort(np.random.RandomState(5).choice(lat["p0"], 8192, replace=False))
    _within_delta(sh, lat, first, "129x129x65, before the last chunk")
    _within_delta(sh, lat, np.arange(lat["p0"], lat["total"]), "129x129x65, the last chunk")
    if sh.fused:                                                              # the whole lattice on k_mlp_forward: the oracle's bits
        want = sh.ref.density_grid(*BIG, use_ema=True)
        assert np.array_equal(_bits(lat["dens"]), _bits(want)), int((_bits(lat["dens"]) != _bits(want)).sum())


def test_position_invariance(shape):
    """9 x 9 x 5 is a sub-lattice of 129 x 129 x 65 with the same fp32 coordinates; a point evaluated by the MFMA kernel on both sides has the same bits,
    whichever tile, lane, wave, trip of the grid-stride loop or chunk holds it (body and tail points are not tied: the tail sums in another order)"""
    sh = shape; small = _lattice(sh, (9, 9, 5)); big = _lattice(sh, BIG)
    i = np.arange(405); x, y, z = i % 9, (i // 9) % 9, i // 81
    bi = 16 * x + 129 * (16 * y) + 129 * 129 * (16 * z)
    assert np.array_equal(_bits(small["u"]), _bits(big["u"][bi]))
    if sh.fused:                                                              # one thread per sample everywhere: every point
        shared = np.ones(405, bool)
    else:
        local = bi % LAYER_CHUNK; n_chunk = np.where(bi < LAYER_CHUNK, LAYER_CHUNK, big["n_last"])
        shared = (i < small["body"]) & (local < (n_chunk & ~31))
        assert shared.sum() == 384 and (shared & (bi >= LAYER_CHUNK)).sum() == 60 and not shared[404]
    diff = _bits(small["dens"])[shared] != _bits(big["dens"][bi])[shared]
    print("%s: (c) position invariance: %d shared points, %d in the last chunk, %d differ" % (sh.name, shared.sum(), (shared & (bi >= big["p0"])).sum(), diff.sum()))
    assert not diff.any(), int(diff.sum())


# ------------------------------------------------------------------ (d)
@pytest.mark.parametrize("name", MESH)
def test_mesh(pool, orc, small_scene, name):
    sh = pool(name); o = sh.o; _, aabb = _scene_box(small_scene)
    nv, ni = o.generate_mesh(32, 2.0)
    got = o.get_mesh(raw=True)
    assert got["verts"].shape[0] == nv and nv % 128 == 0 and got["indices"].size == ni and ni > 300 and nv <= READ
    warped = sh.read(0, nv)["pts"]                                            # (the colour pass's points: the last thing the chain wrote)
    dens = o.density_grid(32, 32, 32)
    _same_mesh(got, orc.marching_cubes(dens, (32, 32, 32), 2.0, aabb[0], aabb[1]))
    # colours: every vertex, padding included, inside colour_of's interval of raw_bounds at the restated warp with its counted position bound
    u, pos_err = rref.mesh_warp(got["verts"], aabb)
    assert np.array_equal(_bits(warped), _bits(u))
    raw, delta = rref.raw_bounds(sh.net, u, pos_err)
    lo, e_lo = rref.colour_of(raw[:, :3] - delta[:, :3]); hi, e_hi = rref.colour_of(raw[:, :3] + delta[:, :3]); want, _ = rref.colour_of(raw[:, :3])
    col = got["colors_f32"].astype(np.float64)
    use = np.where(col >= want, (col - want) / (hi + e_hi - want), (want - col) / (want - (lo - e_lo)))
    print("%s: (d) %d vertices (%d real), %d indices; colour |got - want| / half-width worst %.3f median %.3g" % (
        name, nv, got["n_verts_real"], ni, use.max(), np.median(use)))
    assert ((col >= lo - e_lo) & (col <= hi + e_hi)).all(), (float(use.max()), int((use > 1).sum()))
    o.generate_mesh(32, 2.0); again = o.get_mesh(raw=True)
    assert all(np.array_equal(again[k], got[k]) for k in ("verts", "normals", "colors", "indices", "normals_raw", "colors_f32"))
