"""Training-time occupancy skipping (mon_config::occupancy_skip) against the CPU oracle's restatement of the rule (-m gpu).

tests/test_occupancy.py compares the HIP chains with each other; here every comparison is with oracle/mon_oracle.c (occupancy section), itself pinned by
tests/test_occupancy_oracle_kat.py: the grid a refresh builds (k_occ_density + k_occ_dilate), a pinned all-ones grid against no grid, adversarial pinned
grids through one forward/backward and whole steps, a refresh taking effect in its own iteration, the refresh schedule, the debug dump under a grid, and
trained models.  Both forward chains run: lds_encode = 0 (gathers, masked loads) and 2 (level tiles, live-sample lists)."""
import time
import zlib

import numpy as np
import pytest

import __graft_entry__ as ge
from conftest import C1
from parity import CFGS, SCENE, close_f32, close_half, h2f, pattern_params, psnr
from test_occupancy_oracle_kat import N, WORDS, asked_iterations, numpy_dilate, occ_schedule, pack, unpack
from test_oracle_kat import numpy_occ_live

pytestmark = pytest.mark.gpu

SHAPES = {"c1": dict(C1, rays_per_batch=256), "c2s": dict(CFGS["c2s"]), "w64x2-l8": dict(rays_per_batch=256, n_levels=8, n_neurons=64, n_hidden_layers=2),
          "w128x1": dict(rays_per_batch=256, n_neurons=128, n_hidden_layers=1),
          "t19": dict(rays_per_batch=256, log2_hashmap_size=19, n_neurons=64, n_hidden_layers=1)}      # levels beyond LDS: ATOMIC_LEVELS, big scatter, lazy EMA
CHAINS = {"gather": 0, "tiles": 2}


class Chain:
    """lds_encode (read when an object is created) for the duration of a block; use_graph likewise; big_switch if given (1: the large levels' gradients
    always go through the binned exact scatter -- the default tcnn-style fp16 atomics add in arrival order and are not bit-reproducible)."""

    def __init__(self, pkg, lds, graph=0, big_switch=None):
        self.pkg, self.opts = pkg, dict(lds_encode=lds, use_graph=graph, **({} if big_switch is None else dict(big_switch=big_switch)))

    def __enter__(self):
        self.old = {k: self.pkg.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.pkg.set_option(k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            self.pkg.set_option(k, v)


def _problem(pkg, sc, kw, **extra):
    assert pkg.device_count() >= 1, "no HIP device visible"
    ds, obj = ge.make_problem(pkg, sc, dict(kw, **extra)); obj.set_backend(1)
    return ds, obj


def _grids(ref):
    """The adversarial grids of (c); `single`: the cell holding most of the oracle batch's samples (something must stay live)."""
    z, y, x = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    pts = ref.buffer("pts").reshape(-1, 3)
    c = np.clip(np.trunc(pts * np.float32(N)), 0, N - 1).astype(np.int64); cells = (c[:, 2] * N + c[:, 1]) * N + c[:, 0]
    single = np.zeros(N ** 3, bool); single[np.bincount(cells, minlength=N ** 3).argmax()] = True
    faces = (x == 0) | (x == N - 1) | (y == 0) | (y == N - 1) | (z == 0) | (z == N - 1)
    return {"dead": np.zeros(WORDS, np.uint32), "random": pack(np.random.RandomState(5).uniform(size=(N, N, N)) < 0.5), "half-x": pack(x < 32),
            "faces": pack(faces), "checker": pack((x + y + z) % 2 == 0), "single": pack(single.reshape(N, N, N))}


def _ulp16(v):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14))) - 10)


# ------------------------------------------------------------------ (a) the grid a refresh builds
@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_refreshed_grid_matches_the_oracle(pkg, orc, ss, shape, chain):
    sc = ss.make_scene(**SCENE); kw = SHAPES[shape]
    with Chain(pkg, CHAINS[chain]):
        ds, obj = _problem(pkg, sc, kw, occupancy_skip=1, sample_seed=31)
        obj.train(256); master, half = obj.get_params(0), obj.get_params(1)
        assert obj.occupancy_state() == (0, 0)
        obj.train(1)                                                                 # the refresh at 256 happens here
        assert obj.occupancy_state() == (256, 288)
        raw, dil, thr, _ = obj.occupancy_grid()
        obj.close(); ds.close()
    ref = ge.make_oracle(orc, sc, kw); ref.set_params(master)
    assert np.array_equal(ref.buffer("half"), half), "the oracle's fp16 copy of the device's master weights"
    assert thr == ref.occupancy_threshold
    oraw, odil, dens = ref.occupancy_update(); ref.close()
    g, o = unpack(raw), unpack(oraw)
    mism = (g != o).reshape(-1)
    band = 4 * _ulp16(thr)
    assert (np.abs(dens[mism] - thr) <= band).all(), "raw-bit mismatches outside the ambiguity band: %s" % np.abs(dens[mism] - thr).max()
    print("%s/%s: %d of %d raw cells differ (near-threshold), %.1f %% occupied" % (shape, chain, int(mism.sum()), mism.size, 100 * o.mean()))
    assert mism.sum() <= 1e-3 * mism.size
    assert np.array_equal(dil, numpy_dilate(raw)), "the device's dilation of its own raw grid"
    dmis = unpack(dil) != unpack(odil)
    assert not (dmis & ~unpack(numpy_dilate(pack(mism.reshape(N, N, N))))).any(), "dilated mismatches away from any raw mismatch"
    assert 0 < g.sum() < g.size and g[:, :, 31].any() and g[:, :, 32].any(), "a trivial grid tests nothing"


def test_occupancy_skip_is_inert_outside_the_fused_kernels(pkg, ss):
    """Shapes the fused kernels do not take (backend 0, layer kernels) get no grid: the switch changes nothing there."""
    sc = ss.make_scene(**SCENE); kw = dict(rays_per_batch=256, n_neurons=16, n_hidden_layers=1)
    ds, a = ge.make_problem(pkg, sc, dict(kw, occupancy_skip=1)); _, b = ge.make_problem(pkg, sc, kw, dataset=ds)
    with pytest.raises(pkg.MonError):
        a.occupancy_grid()
    with pytest.raises(pkg.MonError):
        a.set_train_occupancy(np.zeros(WORDS, np.uint32))
    a.train(300); b.train(300)
    assert a.occupancy_state() == (0, 0) and zlib.crc32(a.get_params(0).tobytes()) == zlib.crc32(b.get_params(0).tobytes())
    a.close(); b.close(); ds.close()


# ------------------------------------------------------------------ (b) a pinned all-ones grid is occupancy off
@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("shape", ["c1", "c2s", "t19"])
def test_pinned_all_ones_grid_trains_like_no_grid(pkg, ss, shape, chain, graph):
    sc = ss.make_scene(**SCENE); kw = SHAPES[shape]
    with Chain(pkg, CHAINS[chain], graph, big_switch=1 if shape == "t19" else None):
        ds, off = _problem(pkg, sc, kw, sample_seed=41); _, on = ge.make_problem(pkg, sc, dict(kw, sample_seed=41, occupancy_skip=1), dataset=ds)
        on.set_backend(1)
        on.set_train_occupancy(np.full(WORDS, 0xffffffff, np.uint32))
        assert on.occupancy_state()[0] != 0                                         # in use: the OCC / LIVE instantiations run, every sample live
        off.train(64); on.train(64)
        assert zlib.crc32(off.get_params(0).tobytes()) == zlib.crc32(on.get_params(0).tobytes())
        assert on.occupancy_state()[1] == 0                                         # pinned: no refresh was scheduled
        off.close(); on.close(); ds.close()


# ------------------------------------------------------------------ (c) adversarial pinned grids against the oracle with the same grid
def _compare_stages(obj, ref, chain, n_parts, grid_name):
    R, S = ref.R, ref.S; B = R * S; L = ref.cfg.n_levels
    assert int(obj.buffer("state")[2]) == ref.n_valid > 0
    live = ref.buffer("live").astype(bool)
    if chain == "tiles" and n_parts:
        x = obj.buffer("x_all").reshape(B, 4)[:, :3]; pts = ref.buffer("pts").reshape(B, 3)
        cx = np.clip(np.trunc(x * np.float32(N)), 0, N - 1); cp = np.clip(np.trunc(pts * np.float32(N)), 0, N - 1)
        bad = (cx != cp).any(1)
        assert not bad.any() or (np.abs(x - pts)[bad] > 0).all(), "a cell disagreement with identical positions"
        assert bad.sum() == 0, "%d samples in other cells" % int(bad.sum())
        close_f32(x, pts, "positions", 1e-6)
        e = obj.buffer("e_soa").reshape(L, B, 2).transpose(1, 0, 2).reshape(B, 2 * L)
        re = ref.buffer("E").reshape(B, ref.Epad)[:, :2 * L]
        assert np.array_equal(e[live], re[live]), "level-tile encode of the live samples must be bit-exact"
        cnt = obj.buffer("live_cnt").reshape(2, 64, 16)[0, :, 0]
        per_block = live.reshape(-1, 256).sum(1)
        want = np.bincount(np.arange(per_block.size) % n_parts, weights=per_block, minlength=64).astype(np.int64)
        assert int(cnt.sum()) == int(live.sum()) and np.array_equal(cnt.astype(np.int64), want), (cnt[:n_parts], want[:n_parts])
    for b, tol in (("rgb_ray", 2e-3), ("mask_ray", 2e-3), ("depth_ray", 3e-3), ("loss_ray", 5e-3)):
        close_f32(obj.buffer(b), ref.buffer(b), b, tol)
    gm, rm = obj.buffer("gmlp").astype(np.float64), ref.buffer("gmlp").astype(np.float64)
    gg = h2f(obj.buffer("ggrid_h")).astype(np.float64); rg = ref.buffer("ggrid").astype(np.float64); ra = ref.buffer("ggrid_abs").astype(np.float64)
    if not live.any():
        assert (rm == 0).all() and (gm == 0).all() and (gg == 0).all() and (rg == 0).all(), grid_name
        return
    assert np.abs(gm - rm).max() < 5e-3 * np.abs(rm).max(), (np.abs(gm - rm).max(), np.abs(rm).max())
    frac_bad = float((np.abs(gg - rg) > 2.0 ** -8 * ra + 2.0 ** -10 * np.abs(rg) + 1e-7).mean())
    assert frac_bad < 2e-3, "grid gradient: %.4f%% of entries outside the fp16 accumulation bound" % (100 * frac_bad)
    assert ((gg != 0) & (ra == 0)).mean() < 1e-4, "gradients on entries no live sample touches"


def _compare_steps(obj, ref, nm):
    a, b = obj.get_params(0), ref.buffer("master")
    close_f32(a[:nm], b[:nm], "MLP master weights", 2e-4)
    frac = float((np.abs(a[nm:] - b[nm:]) > 1e-4).mean())
    assert frac < 5e-3, "grid params: %.3f%% differ" % (100 * frac)
    st_a, st_b = obj.buffer("steps"), ref.buffer("steps")
    assert (st_a != st_b).mean() < 5e-3
    ea, eb = h2f(obj.get_params(2)), h2f(ref.buffer("ema"))
    assert (np.abs(ea - eb) > 2e-3 * np.maximum(np.abs(eb), 1e-2)).mean() < 5e-3


CASES_C = [("c2s", g) for g in ("dead", "random", "half-x", "faces", "checker", "single")] + [(s, g) for s in ("c1", "w64x2-l8", "w128x1", "t19")
                                                                                                for g in ("random", "faces")]


@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("shape,grid", CASES_C, ids=["%s-%s" % c for c in CASES_C])
def test_pinned_grids_match_the_oracle(pkg, orc, ss, shape, grid, chain):
    sc = ss.make_scene(**SCENE); kw = SHAPES[shape]
    ref = ge.make_oracle(orc, sc, kw); p = pattern_params(ref); ref.set_params(p); ref.generate_batch()
    bits = _grids(ref)[grid]
    ref.set_occupancy(bits); ref.forward_backward()
    with Chain(pkg, CHAINS[chain]):
        ds, obj = _problem(pkg, sc, kw, occupancy_skip=1); obj.set_params(p); obj.set_train_occupancy(bits)
        n_parts = obj.occupancy_grid()[3]
        assert n_parts > 0 or chain == "gather" or shape == "t19", "the level-tile chain without live-sample lists"
        obj.train_stages(1 | 2)
        _compare_stages(obj, ref, chain, n_parts, grid)
        obj.close(); ref.close()
        for steps in (1, 3):                                                         # whole steps from the same start
            obj = ge.make_problem(pkg, sc, dict(kw, occupancy_skip=1), dataset=ds)[1]
            obj.set_backend(1); obj.set_params(p); obj.set_train_occupancy(bits)
            ref = ge.make_oracle(orc, sc, kw); ref.set_params(p); ref.set_occupancy(bits)
            obj.train(steps); ref.train(steps)
            assert obj.info().train_step == ref.step
            _compare_steps(obj, ref, ref.n_mlp)
            obj.close(); ref.close()
        ds.close()


# ------------------------------------------------------------------ (d) a refresh takes effect in its own iteration
@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("shape", ["c1", "c2s"])
def test_refresh_takes_effect_in_its_own_iteration(pkg, orc, ss, shape, chain):
    sc = ss.make_scene(**SCENE); kw = SHAPES[shape]
    ref = ge.make_oracle(orc, sc, kw)
    with Chain(pkg, CHAINS[chain]):
        ds, obj = _problem(pkg, sc, kw, occupancy_skip=1)
        ref_it = 0                                                                   # iterations the oracle has been advanced by
        for before, at in ((256, 256), (31, 288)):                                    # 288: a refresh reached at a call boundary
            obj.train(before)
            master = obj.get_params(0)
            obj.train(1)                                                             # refresh + iteration `at`
            assert obj.occupancy_state()[0] == at
            _, dil, _, n_parts = obj.occupancy_grid()
            ref.set_params(master)
            while ref_it < at:
                ref.advance_iter(); ref_it += 1
            ref.set_occupancy(dil); ref.generate_batch(); ref.forward_backward(); ref.advance_iter(); ref_it += 1
            live = ref.buffer("live").astype(bool)
            assert 0 < live.sum() < live.size
            for b, tol in (("rgb_ray", 2e-3), ("mask_ray", 2e-3), ("depth_ray", 3e-3), ("loss_ray", 5e-3)):
                close_f32(obj.buffer(b), ref.buffer(b), "%s at %d" % (b, at), tol)
            if chain == "tiles" and n_parts:
                cnt = obj.buffer("live_cnt").reshape(2, 64, 16)[at & 1, :, 0]
                assert int(cnt.sum()) == int(live.sum()), "live samples of iteration %d: %d on the device, %d under the new grid" % (at, cnt.sum(), live.sum())
        obj.close(); ds.close()
    ref.close()


# ------------------------------------------------------------------ (e) schedule
@pytest.mark.parametrize("graph", [0, 1])
def test_refresh_schedule_over_2600_iterations(pkg, ss, graph):
    sc = ss.make_scene(**SCENE); calls = [1, 7, 64, 255, 3, 97, 128, 500, 1, 640, 333, 571]
    with Chain(pkg, 2, graph):
        ds, obj = _problem(pkg, sc, SHAPES["c1"], occupancy_skip=1)
        it, state = 0, (0, 0)
        for n in calls:
            # hipGraph replay only once the grid is in use (the first refresh changes a kernel argument): the eager path until then
            asked = [it + a for a in asked_iterations([n], bool(graph) and state[0] != 0)]
            state = occ_schedule(asked, state)[asked[-1]]
            obj.train(n); it += n
            assert obj.occupancy_state() == state, (it, obj.occupancy_state(), state)
        assert it >= 2600 and state[0] >= 2048
        obj.close(); ds.close()


# ------------------------------------------------------------------ (f) the debug dump honours the grid
def test_debug_dump_honours_the_grid(pkg, orc, ss):
    sc = ss.make_scene(**SCENE); kw = SHAPES["c2s"]
    ref = ge.make_oracle(orc, sc, kw); p = pattern_params(ref); ref.set_params(p); ref.generate_batch()
    bits = _grids(ref)["random"]; ref.set_occupancy(bits); ref.forward_backward()
    B, Ep, L, W, NH = ref.R * ref.S, ref.Epad, ref.cfg.n_levels, ref.W, ref.NH
    live = ref.buffer("live").astype(bool); assert 0 < live.sum() < B
    with Chain(pkg, 2):
        for dump in (1, 2):
            ds, obj = _problem(pkg, sc, kw, occupancy_skip=1); obj.set_params(p); obj.set_train_occupancy(bits); obj.set_debug_dump(dump)
            obj.train_stages(1 | 2)
            assert int(obj.buffer("state")[2]) == ref.n_valid
            E, rE = obj.buffer("E").reshape(B, Ep), ref.buffer("E").reshape(B, Ep)
            assert np.array_equal(E[live], rE[live]), "dump %d: features of the live samples" % dump
            assert (E[~live] == 0).all(), "dump %d: a dead sample's features" % dump
            dO = obj.buffer("dO").reshape(B, 4)
            assert (h2f(dO[~live]) == 0).all(), "dump %d: a dead sample carries dL/dO" % dump
            sel = lambda a, k: a.reshape(B, k)[live].reshape(-1)
            ex = close_half(sel(obj.buffer("Hid"), W * NH), sel(ref.buffer("Hid"), W * NH), "hidden activations", frac_ok=0.999)
            close_half(sel(obj.buffer("O"), 4), sel(ref.buffer("O"), 4), "network output", frac_ok=0.999)
            close_half(sel(dO, 4), sel(ref.buffer("dO"), 4), "dL/dO", ulps=4, frac_ok=0.999)
            close_half(sel(obj.buffer("dHid"), W * NH), sel(ref.buffer("dHid"), W * NH), "dL/dh", ulps=4, frac_ok=0.999)
            close_half(obj.buffer("dE").reshape(B, Ep)[live][:, :2 * L], ref.buffer("dE").reshape(B, Ep)[live][:, :2 * L], "dL/dE", ulps=4, frac_ok=0.999)
            assert ex > 0.9
            obj.close(); ds.close()
        # the dump must not change what is trained: dump 1 (gather chain) and 2 (level tiles) leave the parameters of dump 0
        crcs = []
        for dump in (0, 1, 2):
            ds, obj = _problem(pkg, sc, kw, occupancy_skip=1, sample_seed=43); obj.set_params(p); obj.set_train_occupancy(bits); obj.set_debug_dump(dump)
            obj.train(24); crcs.append(zlib.crc32(obj.get_params(0).tobytes())); obj.close(); ds.close()
        assert crcs[0] == crcs[1] == crcs[2], crcs
    ref.close()


# ------------------------------------------------------------------ (g) trained models
def test_trained_models_with_their_own_grids_match_the_oracle(pkg, orc, ss, small_scene):
    """C1 (R = 1024), 400 steps (refreshes at 256, 288, ..., 384): the HIP object with its own grid, the oracle with its own automatically refreshed grid;
    the bars of test_training_parity_psnr_c1 (tests/test_numerics_study.py trained_model_bars)."""
    from test_numerics_study import trained_model_bars
    mutual_floor, abs_tol = trained_model_bars()
    sc = small_scene; mutual, abs_hip, abs_ref = [], [], []
    t0 = time.time()
    for seed in (11, 12, 13):
        kw = dict(C1, sample_seed=seed)
        ds, obj = _problem(pkg, sc, kw, occupancy_skip=1); ref = ge.make_oracle(orc, sc, kw); ref.set_occupancy_auto(True)
        l_hip = obj.train(400); l_ref = ref.train(400)
        assert obj.occupancy_state() == ref.occupancy_state() == (384, 416)
        assert l_hip < 0.05 and abs(l_hip - l_ref) < max(l_ref, 0.02)
        for box in sc.objects[0]["boxes"][::4]:
            v, x, y, h, w = (int(q) for q in box); pose = ss.colmajor(sc.Twc[v])
            rgb, _, _ = obj.render(box, pose); rrgb, _, _ = ref.render(box, pose)
            gm = sc.instance[v, y:y + h, x:x + w] > 0; gtw = np.where(gm[..., None], sc.rgb[v, y:y + h, x:x + w] / 255.0, 1.0)
            mutual.append(psnr(rgb, rrgb)); abs_hip.append(psnr(rgb, gtw)); abs_ref.append(psnr(rrgb, gtw))
        obj.close(); ds.close(); ref.close()
    print("occupancy grid, 3 seeds x 400 steps (%.0f s): mutual PSNR min %.2f dB (bar %.2f), abs HIP %.2f dB, abs oracle %.2f dB (tol %.2f)" % (
        time.time() - t0, min(mutual), mutual_floor, np.mean(abs_hip), np.mean(abs_ref), abs_tol))
    assert min(mutual) > mutual_floor
    assert abs(np.mean(abs_hip) - np.mean(abs_ref)) < abs_tol and np.mean(abs_hip) > 24.0
