"""Known-answer tests of the oracle's occupancy-grid rule (oracle/mon_oracle.c, occupancy section; CPU only).

The grid is this repository's own opt-in feature (mon_config::occupancy_skip), without a counterpart in the reference, so the oracle's
restatement is pinned here by independent NumPy restatements: the one-cell dilation as a 3x3x3 maximum filter, the cell look-up, the assembly of the grid
from the oracle's own encode + MLP stage entry points at the cell centres, the trivial grids against closed forms, the whole backward chain under a random
grid against torch autograd, and the refresh schedule.  tests/test_occupancy_oracle.py then holds the HIP kernels to this restatement."""
import numpy as np
import pytest

import __graft_entry__ as ge
from conftest import C1
from parity import pattern_params
from test_oracle_kat import _in_child_process, end_to_end_autograd, numpy_occ_live

N = 64
WORDS = N ** 3 // 32


def unpack(bits):
    """8192 words -> bool [z, y, x] (cell = (z * 64 + y) * 64 + x, bit n of word w = cell 32 w + n)."""
    b = np.asarray(bits, np.uint32)
    return ((b[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(N, N, N)


def pack(cells):
    c = np.asarray(cells, bool).reshape(-1, 32).astype(np.uint64)
    return (c << np.arange(32, dtype=np.uint64)[None, :]).sum(1).astype(np.uint32)


def numpy_dilate(bits):
    """3x3x3 maximum filter with zeros outside the grid."""
    g = np.pad(unpack(bits), 1)
    out = np.zeros((N, N, N), bool)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out |= g[dz:dz + N, dy:dy + N, dx:dx + N]
    return pack(out)


def threshold_py(amin, amax, S):
    """model.cpp: dt = |box diagonal| / S in fp32, raw_threshold = log(1e-3 / max(dt, 1e-6))."""
    f = np.float32
    e = np.asarray(amax, f) - np.asarray(amin, f)
    diag2 = f(0)
    for a in range(3):
        diag2 = f(diag2 + f(e[a] * e[a]))
    dt = f(np.sqrt(diag2) / f(S))
    return f(np.log(f(1e-3) / max(dt, f(1e-6))))


def occ_schedule(asked, state=(0, 0)):
    """maybe_refresh_occupancy restated: `asked` = the iterations a refresh is asked for, in order, from `state` = (last refresh, next due); returns
    {iteration: (last refresh, next due)}."""
    (last, due), out = state, {}
    for it in asked:
        if it >= 256 and it >= due:
            every = 32 * (1 if it < 512 else 4 if it < 2048 else 16)
            last, due = it, (it // every + 1) * every
        out[it] = (last, due)
    return out


def asked_iterations(calls, use_graph):
    """The iterations train() asks for a refresh at, for a sequence of call sizes: every iteration (eager path), or -- hipGraph replay (calls of two
    iterations or more) -- the first iteration of every captured pair and the odd one left at the end."""
    it, asked = 0, []
    for n in calls:
        if use_graph and n >= 2:
            asked += [it + 2 * k for k in range(n // 2)] + ([it + n - 1] if n % 2 else [])
        else:
            asked += list(range(it, it + n))
        it += n
    return asked


# ------------------------------------------------------------------ dilation
def _single(x, y, z):
    c = np.zeros((N, N, N), bool); c[z, y, x] = True; return pack(c)


DILATION_CASES = ["random-2%", "random-50%", "x0", "x31", "x32", "x63", "corner", "x31-x32-pair", "zeros", "ones"]


@pytest.mark.parametrize("case", DILATION_CASES)
def test_dilation_matches_a_3x3x3_maximum_filter(orc, case):
    rs = np.random.RandomState(DILATION_CASES.index(case))
    bits = {"random-2%": lambda: pack(rs.uniform(size=(N, N, N)) < 0.02), "random-50%": lambda: pack(rs.uniform(size=(N, N, N)) < 0.5),
            "x0": lambda: _single(0, 17, 40), "x31": lambda: _single(31, 5, 63), "x32": lambda: _single(32, 0, 9), "x63": lambda: _single(63, 63, 33),
            "corner": lambda: _single(63, 63, 63), "x31-x32-pair": lambda: _single(31, 20, 20) | _single(32, 40, 40),
            "zeros": lambda: np.zeros(WORDS, np.uint32), "ones": lambda: np.full(WORDS, 0xffffffff, np.uint32)}[case]()
    got = orc.occupancy_dilate(bits); want = numpy_dilate(bits)
    assert np.array_equal(got, want), "%d words differ" % int((got != want).sum())
    if case.startswith("x3"):                    # the word boundary: a cell at x = 31 lights x = 32 of the next word, and the other way round
        g = unpack(got)
        if case == "x31":
            assert g[63, 5, 32] and g[62, 4, 30] and not g[63, 5, 33]
        if case == "x32":
            assert g[9, 0, 31] and g[10, 1, 33] and not g[9, 0, 30]
    if case == "ones":
        assert (got == 0xffffffff).all()
    if case == "zeros":
        assert (got == 0).all()


# ------------------------------------------------------------------ cell look-up
def test_cell_lookup_truncates_and_clamps(orc):
    f = np.float32
    xs = []
    for k in range(N + 1):
        v = f(k) / f(N)
        xs += [v, np.nextafter(v, f(0))]
    xs += [f(-0.3), f(-1e-7), f(-0.0), f(1.0), f(1.0 + 1e-6), f(1.5), f(7.0)]
    xs = np.array(xs, f)
    rs = np.random.RandomState(0)
    for _ in range(3):
        pts = np.stack([rs.permutation(xs), rs.permutation(xs), rs.permutation(xs)], 1)
        for p in pts:
            c = np.clip(np.trunc(p * f(N)), 0, N - 1).astype(np.int64)
            assert orc.occupancy_cell(p) == (c[2] * N + c[1]) * N + c[0], p
    # truncation at every cell boundary: k/64 is cell k, the float just below it cell k - 1
    for k in range(1, N):
        v = f(k) / f(N); below = np.nextafter(v, f(0))
        assert orc.occupancy_cell([v, 0, 0]) == k and orc.occupancy_cell([below, 0, 0]) == k - 1
        assert orc.occupancy_cell([0, v, 0]) == k * N and orc.occupancy_cell([0, 0, below]) == (k - 1) * N * N
    assert orc.occupancy_cell([1.0, 1.0, 1.0]) == N ** 3 - 1 and orc.occupancy_cell([-5.0, -5.0, -5.0]) == 0


def test_forward_backward_looks_the_cells_up_from_its_own_positions(orc, small_scene):
    """The live mask of forward_backward under a grid equals the NumPy look-up of the batch's positions (random 50 % grid and a single live cell)."""
    m = ge.make_oracle(orc, small_scene, dict(C1, rays_per_batch=256))
    m.set_params(pattern_params(m)); m.generate_batch(); assert m.n_valid > 0
    pts = m.buffer("pts").reshape(-1, 3)
    rs = np.random.RandomState(1)
    busiest = np.bincount(numpy_cells(pts), minlength=N ** 3).argmax()
    single = np.zeros(N ** 3, bool); single[busiest] = True
    for bits in (pack(rs.uniform(size=(N, N, N)) < 0.5), pack(single.reshape(N, N, N))):
        m.set_occupancy(bits); m.forward_backward()
        live = m.buffer("live"); want = numpy_occ_live(bits, pts)
        assert np.array_equal(live, want) and 0 < live.sum() < live.size
    m.close()


def numpy_cells(pts):
    c = np.clip(np.trunc(np.asarray(pts, np.float32) * np.float32(N)), 0, N - 1).astype(np.int64)
    return (c[:, 2] * N + c[:, 1]) * N + c[:, 0]


# ------------------------------------------------------------------ grid assembly
def _grid_model(orc, scale):
    """A C1-shaped oracle over a 0.6 x 0.8 x 1.0 box, pattern weights with the table scaled so the raw density straddles the threshold."""
    m = orc.OracleModel(orc.default_config(**C1))
    amin, amax = np.array([-0.3, -0.4, -0.5], np.float32), np.array([0.3, 0.4, 0.5], np.float32)
    m.set_object(np.eye(4, dtype=np.float32).reshape(-1), amin, amax, 1)
    p = pattern_params(m); p[m.n_mlp:] *= scale
    o_out = m.W * m.Epad + (m.NH - 1) * m.W * m.W; p[o_out + 3 * m.W:o_out + 4 * m.W] *= 6.0      # the density row: a wider spread
    m.set_params(p)
    return m, amin, amax


def test_grid_assembly_matches_numpy_over_the_oracles_stages(orc):
    """orc_occupancy_update against a NumPy assembly of orc_encode + orc_mlp_forward at the cell centres (c + 0.5) / 64, x fastest, bit n of word w =
    cell 32 w + n, raw density > the threshold restated in Python: bits exact.  Pins the centre offset, the ordering, the bit order and the threshold."""
    import ctypes as C
    m, amin, amax = _grid_model(orc, 8.0)
    thr = threshold_py(amin, amax, m.S)
    assert m.occupancy_threshold == thr, (m.occupancy_threshold, thr)
    f = np.float32
    z, y, x = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    pts = np.ascontiguousarray(np.stack([(x.astype(f) + f(0.5)) / f(N), (y.astype(f) + f(0.5)) / f(N), (z.astype(f) + f(0.5)) / f(N)], -1).reshape(-1, 3))
    n = pts.shape[0]; half = m.buffer("half")
    E = np.zeros(n * m.Epad, np.uint16); hid = np.zeros(n * m.W * m.NH, np.uint16); O = np.zeros(n * 4, np.uint16)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    m.L.orc_encode(m.h, P(half), P(pts), n, P(E)); m.L.orc_mlp_forward(m.h, P(half), P(E), n, P(hid), P(O))
    dens = orc.h2f(O.reshape(n, 4)[:, 3])
    occ = dens > thr
    assert 0.05 < occ.mean() < 0.95, occ.mean()              # a non-trivial grid
    raw, dil, d = m.occupancy_update()
    assert np.array_equal(d, dens)
    assert np.array_equal(raw, pack(occ)), "%d raw words differ" % int((raw != pack(occ)).sum())
    assert np.array_equal(dil, numpy_dilate(pack(occ)))
    g = unpack(raw)
    assert g[:, :, 31].any() and g[:, :, 32].any() and not g[:, :, 31].all()
    m.close()


# ------------------------------------------------------------------ trivial grids
def test_all_ones_grid_is_bit_identical_to_no_grid(orc, small_scene):
    outs = []
    for grid in (None, np.full(WORDS, 0xffffffff, np.uint32)):
        m = ge.make_oracle(orc, small_scene, dict(C1, rays_per_batch=256))
        m.set_params(pattern_params(m)); m.generate_batch(); m.set_occupancy(grid); m.forward_backward()
        outs.append({b: m.buffer(b) for b in ("E", "Hid", "O", "dO", "dHid", "dE", "rgb_ray", "depth_ray", "mask_ray", "loss_ray", "gmlp", "ggrid", "live")})
        outs[-1]["loss"] = m.loss; m.close()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    assert outs[0]["live"].all()


@pytest.mark.parametrize("use_depth", [False, True])
def test_all_dead_grid_gives_the_background_and_no_gradient(orc, small_scene, use_depth):
    m = ge.make_oracle(orc, small_scene, dict(C1, rays_per_batch=256), use_depth=use_depth)
    m.set_params(pattern_params(m)); m.generate_batch(); m.set_occupancy(np.zeros(WORDS, np.uint32)); m.forward_backward()
    R = m.R
    bg = m.buffer("bgcol").reshape(R, 3); tg = m.buffer("target").reshape(R, 3).astype(np.float64)
    assert np.array_equal(m.buffer("rgb_ray").reshape(R, 3), bg)
    assert (m.buffer("mask_ray") == 0).all() and (m.buffer("depth_ray") == 0).all() and (m.buffer("live") == 0).all()
    for b in ("dO", "gmlp", "ggrid", "E", "O", "Hid", "dE"):
        assert (m.buffer(b) == 0).all(), b
    # closed form: object rays mean((bg - target)^2) + 1 (+ |0 - depth| / 2 with depth), background rays 0
    flag = m.buffer("ray_flag").astype(bool); td = m.buffer("target_depth").astype(np.float64)
    want = np.where(flag, ((bg - tg) ** 2).mean(1) + 1.0 + np.where(td > 0, 0.5 * td, 0.0), 0.0)
    assert flag.any() and (~flag).any() and (td > 0).any() == use_depth
    assert np.allclose(m.buffer("loss_ray"), want, rtol=1e-6, atol=1e-7)
    assert abs(m.loss - want.mean()) < 1e-6 * max(1.0, want.mean())
    m.close()


# ------------------------------------------------------------------ second source: the whole backward chain under a grid
@pytest.mark.parametrize("kw", [dict(n_levels=4, n_neurons=32, n_hidden_layers=2), dict(n_levels=16, n_neurons=64, n_hidden_layers=1)], ids=["c1net", "c2net"])
@pytest.mark.parametrize("use_depth", [False, True])
def test_end_to_end_gradients_under_a_random_grid_match_torch_autograd(orc, small_scene, kw, use_depth, request):
    """test_oracle_kat's fp64 torch graph with a random 50 % grid: dead samples have zero features and alpha 0 (and no density penalty), live ones as
    before; the oracle's gmlp and grid gradient under the same bars."""
    if _in_child_process(request):
        return
    bits = pack(np.random.RandomState(7).uniform(size=(N, N, N)) < 0.5)
    end_to_end_autograd(orc, small_scene, kw, use_depth, occ_bits=bits)


# ------------------------------------------------------------------ schedule
def test_auto_refresh_follows_the_eager_schedule(orc, small_scene):
    """orc_set_occupancy_auto: refreshed before iteration 256, then at the next multiple of 32 / 128 / 512 (below 512 / below 2048 / after), checked after
    every call of an uneven sequence up to 2 600 iterations; the grid in use after a refresh is the dilated update of the weights it was computed from."""
    m = ge.make_oracle(orc, small_scene, dict(rays_per_batch=64, n_levels=2, n_neurons=32, n_hidden_layers=1))
    m.set_occupancy_auto(True)
    calls = [1, 7, 64, 255, 3, 97, 128, 500, 1, 640, 333, 571]
    want = occ_schedule(asked_iterations(calls, False))
    it = 0
    for n in calls:
        if it <= 256 < it + n:                  # stop right before the first refresh: check the grid it computes against occupancy_update
            m.train(256 - it); raw, dil, _ = m.occupancy_update(); m.train(1); m.generate_batch(); m.forward_backward()
            pts = m.buffer("pts").reshape(-1, 3)
            assert np.array_equal(m.buffer("live"), numpy_occ_live(dil, pts))
            m.train(it + n - 257)
        else:
            m.train(n)
        it += n
        assert m.occupancy_state() == want[it - 1], (it, m.occupancy_state(), want[it - 1])
    assert it >= 2600 and m.occupancy_state()[0] >= 2048
    m.close()


def test_schedule_restatement_known_answers():
    eager = occ_schedule(range(3000))
    assert eager[255] == (0, 0) and eager[256] == (256, 288) and eager[480] == (480, 512) and eager[512] == (512, 640)
    assert eager[1920] == (1920, 2048) and eager[2048] == (2048, 2560) and eager[2999] == (2560, 3072)
    graph = occ_schedule(asked_iterations([257, 64], True))
    assert graph[256] == (256, 288) and graph[289] == (289, 320)
