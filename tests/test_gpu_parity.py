"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against the CPU oracle on the same seeded
inputs, against the committed golden fixtures, and through size-independent properties at BASELINE sizes.
Nothing here reads /root/reference.  Tolerances: tests/parity.py."""
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from conftest import C1, C2
from parity import CFGS, SCENE, close_f32, close_half, grid_probe_indices, h2f, load_golden, pattern_params, psnr
from stage_reference import ulp16 as _ulp16          # fp16 spacing at |x|, the subnormal spacing 2^-24 below 2^-14

pytestmark = pytest.mark.gpu

BACKENDS = [0, 1]


def _need_gpu(pkg):
    assert pkg.device_count() >= 1, "no HIP device visible: the GPU tests must run on the MI355X box"


def _pair(pkg, orc, sc, kw, backend, use_depth=False):
    _need_gpu(pkg)
    ds, obj = ge.make_problem(pkg, sc, kw, use_depth=use_depth)
    try:
        obj.set_backend(backend)
    except pkg.MonError:
        obj.close(); ds.close(); pytest.skip("fused backend not available for this shape")
    if backend == 1:
        obj.set_debug_dump(True)          # also write E / h / O / dO / dE of the fused kernel for comparison
    ref = ge.make_oracle(orc, sc, kw, use_depth=use_depth)
    return ds, obj, ref


def test_mfma_fragment_layout(pkg):
    """The A/B/D lane mapping of v_mfma_f32_32x32x16_f16 the fused kernels rely on (asymmetric operands)."""
    _need_gpu(pkg)
    rs = np.random.RandomState(0)
    A = rs.uniform(-1, 1, (32, 16)).astype(np.float16); B = rs.uniform(-1, 1, (16, 32)).astype(np.float16)
    D = pkg.selftest_mfma(A.view(np.uint16), B.view(np.uint16))
    want = A.astype(np.float64) @ B.astype(np.float64)
    assert np.abs(D - want).max() < 1e-5
    assert np.abs(D - want.T).max() > 1e-2          # a transposed write would not pass


@pytest.mark.parametrize("kw", [C1, dict(rays_per_batch=256, n_levels=16, n_neurons=64, n_hidden_layers=1)], ids=["c1", "c2net"])
@pytest.mark.parametrize("use_depth", [False, True])
def test_batch_generation_matches_oracle(pkg, orc, small_scene, kw, use_depth):
    ds, obj, ref = _pair(pkg, orc, small_scene, kw, 0, use_depth)
    for it in range(2):
        obj.train_stages(1); ref.generate_batch()
        st = obj.buffer("state")
        assert int(st[2]) == ref.n_valid and ref.n_valid > 0                           # bit-exact compaction count
        assert np.array_equal(obj.buffer("ray_flag"), ref.buffer("ray_flag"))
        for b in ("ray_o", "ray_d", "ray_t0", "ray_t1", "ray_dn", "target", "target_depth", "bgcol", "pts", "tdist"):
            close_f32(obj.buffer(b), ref.buffer(b), b, 1e-6)
        # rollover property (fill_rollover_rays): ray j equals ray j mod n_valid
        nv = ref.n_valid; o = obj.buffer("ray_o").reshape(-1, 3)
        assert np.array_equal(o, o[np.arange(o.shape[0]) % nv])
        obj.train_stages(2 | 4); ref.train_step()                # finish the iteration on both sides (same batch again on the oracle)
    obj.close(); ds.close(); ref.close()


@pytest.mark.parametrize("hw", [(45, 67), (61, 83)], ids=["45x67", "61x83"])
def test_ragged_image_sizes_upload_exactly(pkg, orc, ss, hw):
    """Frames whose pixel count is not a multiple of 4 or 16 (the upload packs them with a kernel out of pinned staging, depth and pose behind the colour and
    instance bytes at 16-byte steps): every frame re-uses the same staging addresses, so a misaligned or out-of-date read shows up as a candidate mismatch in
    some later frame -- the batch of 4096 candidates over all frames is compared with the oracle's, with and without depth."""
    sc = ss.make_scene(n_views=12, H=hw[0], W=hw[1], f=55.0, seed=9)
    for use_depth in (False, True):
        kw = dict(rays_per_batch=4096, n_levels=4, n_neurons=32, n_hidden_layers=2)
        ds, obj, ref = _pair(pkg, orc, sc, kw, 0, use_depth)
        for it in range(2):
            obj.train_stages(1); ref.generate_batch()
            assert int(obj.buffer("state")[2]) == ref.n_valid and ref.n_valid > 0
            assert np.array_equal(obj.buffer("ray_flag"), ref.buffer("ray_flag"))
            for b in ("target", "target_depth", "ray_o", "ray_d"):
                close_f32(obj.buffer(b), ref.buffer(b), b, 1e-6)
            obj.train_stages(2 | 4); ref.train_step()
        obj.close(); ds.close(); ref.close()


def test_every_uploaded_frame_arrives_as_sent(pkg):
    """Frame upload read back from the device, frame by frame: 96 frames go through the SAME pinned staging addresses back to back (colour, instance,
    depth, pose), each with its own contents.  A read served from a cache line the previous frame's kernel left behind -- seen as frames arriving with
    the previous frame's pose -- shows up here directly (the staging reads are system-scope loads for that reason)."""
    H, W, n = 37, 53, 96
    rng = np.random.default_rng(5)
    ds = pkg.Dataset(0, H, W, 60.0, 60.0, W / 2, H / 2, n, use_depth=True)
    sent = []
    for k in range(n):
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8); inst = rng.integers(0, 4, (H, W), dtype=np.uint8)
        dep = rng.random((H, W), dtype=np.float32) * 3.0; pose = rng.standard_normal(16).astype(np.float32)
        ds.add_frame(k, rgb, inst, pose, depth=dep); sent.append((rgb, inst, dep, pose))
    for k, (rgb, inst, dep, pose) in enumerate(sent):
        rgba, d, p = ds.debug_read(k, with_depth=True)
        want = rgb[..., 0].astype(np.uint32) | (rgb[..., 1].astype(np.uint32) << 8) | (rgb[..., 2].astype(np.uint32) << 16) | (inst.astype(np.uint32) << 24)
        assert np.array_equal(rgba, want), "frame %d: colour / instance" % k
        assert np.array_equal(d, dep), "frame %d: depth" % k
        assert np.array_equal(p, pose), "frame %d: pose" % k
    ds.close()
    # a dataset whose zero-fill at creation takes ~1 ms (2 GB), and the LAST frame slot uploaded right away: the fill must not land after the upload
    free, _ = pkg.device_mem_info(0)
    if free > (8 << 30):
        cap = (2 << 30) // (H * W * 4)
        ds = pkg.Dataset(0, H, W, 60.0, 60.0, W / 2, H / 2, cap)
        rgb, inst, dep, pose = sent[0]
        for k in (cap - 1, cap // 2, 0):
            ds.add_frame(k, rgb, inst, pose)
        want = rgb[..., 0].astype(np.uint32) | (rgb[..., 1].astype(np.uint32) << 8) | (rgb[..., 2].astype(np.uint32) << 16) | (inst.astype(np.uint32) << 24)
        for k in (cap - 1, cap // 2, 0):
            rgba, _, p = ds.debug_read(k)
            assert np.array_equal(rgba, want) and np.array_equal(p, pose), "frame %d of a freshly created %d-frame dataset" % (k, cap)
        ds.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", sorted(CFGS))
def test_forward_backward_matches_oracle_and_golden(pkg, orc, ss, name, backend):
    sc = ss.make_scene(**SCENE); kw = CFGS[name]; g = load_golden(name)
    ds, obj, ref = _pair(pkg, orc, sc, kw, backend)
    p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
    obj.train_stages(1 | 2); ref.generate_batch(); ref.forward_backward()
    assert int(obj.buffer("state")[2]) == ref.n_valid == int(g["n_valid"])
    B, Ep = ref.R * ref.S, ref.Epad
    if True:                              # backend 1 dumps its on-chip intermediates in debug mode
        assert np.array_equal(obj.buffer("E"), ref.buffer("E")), "hash-grid encode must be bit-exact"
        assert np.array_equal(obj.buffer("E")[:g["E"].size], g["E"])
        # backend 1 sums the MLP dot products in MFMA order: a rounding-boundary flip of 1 fp16 ulp is allowed on 0.1 % of values
        fr = 1.0 if backend == 0 else 0.999
        ex = close_half(obj.buffer("Hid"), ref.buffer("Hid"), "hidden activations", frac_ok=fr)
        close_half(obj.buffer("O"), ref.buffer("O"), "network output", frac_ok=fr)
        close_half(obj.buffer("O")[:g["O"].size], g["O"], "network output vs golden", frac_ok=fr)
        close_half(obj.buffer("dO"), ref.buffer("dO"), "dL/dO", ulps=4, frac_ok=0.999)
        close_half(obj.buffer("dHid"), ref.buffer("dHid"), "dL/dh", ulps=4, frac_ok=0.999)
        nf = 2 * ref.cfg.n_levels                  # compare the real features; dL/dE of the zero-padded inputs is never used
        close_half(obj.buffer("dE").reshape(B, Ep)[:, :nf], ref.buffer("dE").reshape(B, Ep)[:, :nf], "dL/dE", ulps=4, frac_ok=0.999)
        assert ex > 0.9
    close_f32(obj.buffer("rgb_ray"), ref.buffer("rgb_ray"), "rgb_ray", 2e-3)
    close_f32(obj.buffer("rgb_ray")[:g["rgb_ray"].size], g["rgb_ray"], "rgb_ray vs golden", 2e-3)
    close_f32(obj.buffer("mask_ray"), ref.buffer("mask_ray"), "mask_ray", 2e-3)
    close_f32(obj.buffer("depth_ray"), ref.buffer("depth_ray"), "depth_ray", 3e-3)
    close_f32(obj.buffer("loss_ray"), ref.buffer("loss_ray"), "loss_ray", 5e-3)
    # MLP weight gradients (fp32): relative to the largest entry of each matrix
    gm, rm = obj.buffer("gmlp").astype(np.float64), ref.buffer("gmlp").astype(np.float64)
    assert np.abs(gm - rm).max() < 5e-3 * np.abs(rm).max(), (np.abs(gm - rm).max(), np.abs(rm).max())
    assert np.abs(gm - g["gmlp"]).max() < 5e-3 * np.abs(g["gmlp"]).max()
    # grid gradient: fp16 atomics in arbitrary order vs fp32 accumulation: |err| <= 2^-9 * sum|contrib| + ulp
    gg = h2f(obj.buffer("ggrid_h")).astype(np.float64); rg = ref.buffer("ggrid").astype(np.float64); ra = ref.buffer("ggrid_abs").astype(np.float64)
    bound = 2.0 ** -8 * ra + 2.0 ** -10 * np.abs(rg) + 1e-7
    frac_bad = float((np.abs(gg - rg) > bound).mean())
    assert frac_bad < 2e-3, "grid gradient: %.4f%% of entries outside the fp16 accumulation bound" % (100 * frac_bad)
    assert (gg != 0).sum() > 0 and abs(gg.sum() - rg.sum()) < 2e-2 * ra.sum() / max(1, np.sqrt((ra > 0).sum())) + 1e-3 * np.abs(rg).sum()
    gi = grid_probe_indices(ref.n_params - ref.n_mlp)
    assert (np.abs(gg[gi] - g["ggrid_probe"]) <= 2.0 ** -8 * g["ggrid_abs_probe"] + 2.0 ** -10 * np.abs(g["ggrid_probe"]) + 1e-7).mean() > 0.995
    obj.close(); ds.close(); ref.close()


@pytest.mark.parametrize("name,kw", [("c2s", dict(CFGS["c2s"])), ("c2", dict(C2))], ids=["c2s-R256", "c2-R4096"])
def test_benched_chain_forward_backward_matches_oracle(pkg, orc, ss, name, kw):
    """The instantiation bench.py times -- k_encode_tiles -> k_fused_train<PRE> -> k_grid_scatter -- against the oracle DIRECTLY (the other oracle comparisons
    of backend 1 run the gather chain's dump variant): mon_object_set_debug_dump(obj, 2) keeps the level-tile chain and compiles the dump into its kernel.
    base.json at the full batch (R = 4096) and the fixtures' small batch (level tiles forced)."""
    sc = ss.make_scene(**SCENE)
    old = pkg.get_option("lds_encode"); pkg.set_option("lds_encode", 2)
    try:
        _need_gpu(pkg)
        ds, obj = ge.make_problem(pkg, sc, kw); obj.set_backend(1); obj.set_debug_dump(2)
        ref = ge.make_oracle(orc, sc, kw)
        p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
        obj.train_stages(1 | 2); ref.generate_batch(); ref.forward_backward()
        assert int(obj.buffer("state")[2]) == ref.n_valid > 0
        B, Ep, L = ref.R * ref.S, ref.Epad, ref.cfg.n_levels
        e_soa = obj.buffer("e_soa").reshape(L, B, 2)                      # what k_encode_tiles wrote: the chain is the level-tile one
        assert np.array_equal(e_soa.transpose(1, 0, 2).reshape(B, 2 * L), ref.buffer("E").reshape(B, Ep)[:, :2 * L]), "level-tile encode must be bit-exact"
        assert np.array_equal(obj.buffer("E"), ref.buffer("E")), "the features k_fused_train<PRE> loaded"
        ex = close_half(obj.buffer("Hid"), ref.buffer("Hid"), "hidden activations", frac_ok=0.999)
        close_half(obj.buffer("O"), ref.buffer("O"), "network output", frac_ok=0.999)
        close_half(obj.buffer("dO"), ref.buffer("dO"), "dL/dO", ulps=4, frac_ok=0.999)
        close_half(obj.buffer("dHid"), ref.buffer("dHid"), "dL/dh", ulps=4, frac_ok=0.999)
        close_half(obj.buffer("dE").reshape(B, Ep)[:, :2 * L], ref.buffer("dE").reshape(B, Ep)[:, :2 * L], "dL/dE", ulps=4, frac_ok=0.999)
        assert ex > 0.9
        for b, tol in (("rgb_ray", 2e-3), ("mask_ray", 2e-3), ("depth_ray", 3e-3), ("loss_ray", 5e-3)):
            close_f32(obj.buffer(b), ref.buffer(b), b, tol)
        gm, rm = obj.buffer("gmlp").astype(np.float64), ref.buffer("gmlp").astype(np.float64)
        assert np.abs(gm - rm).max() < 5e-3 * np.abs(rm).max(), (np.abs(gm - rm).max(), np.abs(rm).max())
        # grid gradient = the sum of k_grid_scatter's partial tables (exact int32 accumulation per tile, one fp16 rounding per partial table)
        gg = h2f(obj.buffer("ggrid_h")).astype(np.float64); rg = ref.buffer("ggrid").astype(np.float64); ra = ref.buffer("ggrid_abs").astype(np.float64)
        frac_bad = float((np.abs(gg - rg) > 2.0 ** -8 * ra + 2.0 ** -10 * np.abs(rg) + 1e-7).mean())
        assert frac_bad < 2e-3 and (gg != 0).sum() > 0, frac_bad
        obj.close(); ds.close(); ref.close()
    finally:
        pkg.set_option("lds_encode", old)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", sorted(CFGS))
def test_one_training_step_matches_oracle_and_golden(pkg, orc, ss, name, backend):
    sc = ss.make_scene(**SCENE); kw = CFGS[name]; g = load_golden(name)
    ds, obj, ref = _pair(pkg, orc, sc, kw, backend)
    p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
    loss = obj.train(1); ref.train(1)
    assert abs(loss - ref.loss) < 2e-3 * max(1.0, abs(ref.loss)) and abs(loss - float(g["loss"])) < 2e-3
    a, b = obj.get_params(0), ref.buffer("master")
    nm = ref.n_mlp
    close_f32(a[:nm], b[:nm], "MLP master weights after one step", 2e-4)
    close_f32(a[:nm], g["master_mlp_after"], "MLP master weights vs golden", 2e-4)
    frac = float((np.abs(a[nm:] - b[nm:]) > 1e-4).mean())
    assert frac < 5e-3, "grid params: %.3f%% differ after one Adam step" % (100 * frac)
    st_a, st_b = obj.buffer("steps"), ref.buffer("steps")
    assert (st_a != st_b).mean() < 5e-3 and (st_a[:nm] == 1).all()
    ea, eb = h2f(obj.get_params(2)), h2f(ref.buffer("ema"))
    assert (np.abs(ea - eb) > 2e-3 * np.maximum(np.abs(eb), 1e-2)).mean() < 5e-3
    i = obj.info(); assert i.train_step == 1 and i.last_n_valid == ref.n_valid
    obj.close(); ds.close(); ref.close()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", sorted(CFGS))
def test_render_matches_oracle_and_golden(pkg, orc, ss, name, backend):
    sc = ss.make_scene(**SCENE); kw = CFGS[name]; g = load_golden(name)
    ds, obj, ref = _pair(pkg, orc, sc, kw, backend)
    p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
    box = g["render_box"]; pose = ss.colmajor(sc.Twc[int(box[0])])
    rgb, depth, mask = obj.render(box, pose)
    rrgb, rdepth, rmask = ref.render(box, pose, use_ema=False)
    # hard 0.5 opacity threshold (:1213): pixels within 1e-3 of it may flip; everything else must agree
    flips = float((mask != rmask).mean())
    assert flips < 5e-3, flips
    same = mask == rmask
    assert np.abs(rgb - rrgb)[same].max() < 4e-3 and np.abs(depth - rdepth)[same].max() < 4e-3
    gsame = mask.astype(np.uint8) == g["render_mask"]
    assert gsame.mean() > 0.995 and np.abs(rgb - g["render_rgb"].astype(np.float32))[gsame].max() < 5e-3
    # determinism: the render-time jitter is a fixed stream (reference re-seeds per call, SURVEY App.A-7)
    rgb2, depth2, mask2 = obj.render(box, pose)
    assert np.array_equal(rgb, rgb2) and np.array_equal(depth, depth2) and np.array_equal(mask, mask2)
    # object-frame pose path (RenderVideo): Toc = Tow * Twc gives the same image
    Toc = (sc.objects[0]["Tow"] @ sc.Twc[int(box[0])])
    rgb3, depth3, mask3 = obj.render(box, ss.colmajor(Toc), pose_is_Toc=True)
    assert (mask3 != mask).mean() < 5e-3 and np.abs(rgb3 - rgb)[mask3 == mask].max() < 5e-3
    if backend == 0:
        dg = obj.density_grid(9, 9, 9)
        assert np.abs(dg - g["density_probe"]).max() < 2e-2 * max(1.0, np.abs(g["density_probe"]).max())
    obj.close(); ds.close(); ref.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_render_crop_sizes_around_the_chunk_boundaries(pkg, orc, ss, backend):
    """Render works in passes of 16 384 rays: a single pixel, a crop one pixel short of / one pixel past a pass, and a whole 160x120 image
    (two passes, most rays miss the box) against the oracle; the whole-crop output buffers grow on demand."""
    sc = ss.make_scene(**SCENE); kw = CFGS["c2s"]
    ds, obj, ref = _pair(pkg, orc, sc, kw, backend)
    p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
    ob = sc.objects[0]["boxes"][2]; v, cx, cy = int(ob[0]), int(ob[1] + ob[4] // 2), int(ob[2] + ob[3] // 2)
    pose = ss.colmajor(sc.Twc[v])
    for (x, y, h, w) in [(cx, cy, 1, 1), (0, 0, 127, 129), (0, 0, 113, 145), (0, 0, sc.H, sc.W), (sc.W - 3, sc.H - 2, 2, 3)]:     # 16 383 and 16 385 pixels
        box = np.array([v, x, y, h, w], np.uint32)
        rgb, depth, mask = obj.render(box, pose); rrgb, rdepth, rmask = ref.render(box, pose, use_ema=False)
        assert rgb.shape == (h, w, 3) and mask.shape == (h, w)
        same = mask == rmask
        assert (~same).mean() <= 5e-3 + 1.0 / mask.size * (mask.size < 100), (h, w)
        if same.any():
            assert np.abs(rgb - rrgb)[same].max() < 4e-3 and np.abs(depth - rdepth)[same].max() < 4e-3, (h, w)
    assert mask.shape == (2, 3)
    obj.close(); ds.close(); ref.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_nondefault_hyperparameters_match_oracle(pkg, orc, small_scene, backend):
    """Everything base.json leaves at its default, moved: level geometry (base resolution 24, per-level scale 1.5: odd resolutions, dense
    and hashed levels of other sizes), 12 levels on a 32-wide network, a loss scale that is not a power of two (the optimizer's division
    path), Adam / L2 / EMA constants.  Forward/backward and three optimizer steps against the oracle."""
    kw = dict(rays_per_batch=256, base_resolution=24, per_level_scale=1.5, n_levels=12, log2_hashmap_size=15, n_neurons=32, n_hidden_layers=1,
              loss_scale=100.0, learning_rate=5e-3, beta1=0.8, beta2=0.95, epsilon=1e-8, l2_reg=1e-4, ema_decay=0.9)
    ds, obj, ref = _pair(pkg, orc, small_scene, kw, backend)
    p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
    obj.train_stages(1 | 2); ref.generate_batch(); ref.forward_backward()
    assert int(obj.buffer("state")[2]) == ref.n_valid > 0
    assert np.array_equal(obj.buffer("E"), ref.buffer("E")), "hash-grid encode must be bit-exact"
    close_half(obj.buffer("O"), ref.buffer("O"), "network output", frac_ok=1.0 if backend == 0 else 0.999)
    close_half(obj.buffer("dO"), ref.buffer("dO"), "dL/dO", ulps=4, frac_ok=0.999)
    gm, rm = obj.buffer("gmlp").astype(np.float64), ref.buffer("gmlp").astype(np.float64)
    assert np.abs(gm - rm).max() < 5e-3 * np.abs(rm).max()
    gg = h2f(obj.buffer("ggrid_h")).astype(np.float64); rg = ref.buffer("ggrid").astype(np.float64); ra = ref.buffer("ggrid_abs").astype(np.float64)
    assert float((np.abs(gg - rg) > 2.0 ** -8 * ra + 2.0 ** -10 * np.abs(rg) + 1e-7).mean()) < 2e-3 and (gg != 0).sum() > 0
    obj.close(); ds.close(); ref.close()
    ds, obj, ref = _pair(pkg, orc, small_scene, kw, backend)
    obj.set_debug_dump(False); obj.set_params(p); ref.set_params(p)
    for _ in range(3):
        la = obj.train(1); ref.train(1)
    assert abs(la - ref.loss) < 5e-3 * max(1.0, abs(ref.loss))
    nm = ref.n_mlp; a, b = obj.get_params(0), ref.buffer("master")
    close_f32(a[:nm], b[:nm], "MLP master weights after three steps", 1e-3)
    assert float((np.abs(a[nm:] - b[nm:]) > 3e-4).mean()) < 1e-2
    ea, eb = h2f(obj.get_params(2)), h2f(ref.buffer("ema"))
    assert (np.abs(ea - eb) > 4e-3 * np.maximum(np.abs(eb), 1e-2)).mean() < 1e-2
    obj.close(); ds.close(); ref.close()


@pytest.mark.parametrize("W,NH,L,backends", [(128, 1, 16, (0, 1)), (128, 1, 6, (1,)), (128, 2, 8, (0,)), (16, 1, 16, (0,)), (16, 2, 4, (0,)), (64, 3, 16, (0,)),
                                             (32, 4, 8, (0,)), (16, 4, 12, (0,)), (128, 2, 16, (0,)), (64, 4, 6, (0,)), (32, 3, 16, (0,))],
                         ids=["1x128", "1x128-L6", "2x128", "1x16", "2x16", "3x64", "4x32", "4x16", "2x128-L16", "4x64-L6", "3x32-L16"])
@pytest.mark.parametrize("lds", [1, 2], ids=["gather-encode", "tile-encode"])
def test_the_other_fully_fused_mlp_widths_match_oracle(pkg, orc, small_scene, W, NH, L, backends, lds):
    """tcnn's FullyFusedMLP takes 16 / 32 / 64 / 128 neurons and base.json:30-36 is the user's to edit: one hidden layer of 128 runs on the fused MFMA kernels
    (the default backend for it), 2 x 128, 16 neurons (half an MFMA tile) and three / four hidden layers on the layer-at-a-time kernels.  Forward / backward and three optimizer steps
    against the oracle, a render against the oracle's, both encoder paddings."""
    _need_gpu(pkg)
    kw = dict(rays_per_batch=256, n_levels=L, log2_hashmap_size=15, n_neurons=W, n_hidden_layers=NH)
    ds, o = ge.make_problem(pkg, small_scene, kw); assert int(o.info().backend) == (1 if (W == 128 and NH == 1) else 0); o.close(); ds.close()
    # lds = 2: the layer-kernel shapes' encode from LDS level tiles (what they use from 3072 rays per batch on), forced at this small batch -- same bars: the
    # features are bit-exact either way, three whole steps exercise k_optimizer keeping the tile image current, the stage-wise call its rebuild
    if lds == 2 and (W == 128 and NH == 1):
        pytest.skip("a fused shape: its tile chain has tests of its own")
    old_lds = pkg.get_option("lds_encode"); pkg.set_option("lds_encode", lds)
    try:
        _other_widths_body(pkg, orc, small_scene, W, NH, L, backends, kw, lds)
    finally:
        pkg.set_option("lds_encode", old_lds)


def _other_widths_body(pkg, orc, small_scene, W, NH, L, backends, kw, lds):
    for backend in backends:
        ds, obj, ref = _pair(pkg, orc, small_scene, kw, backend)
        p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
        obj.train_stages(1 | 2); ref.generate_batch(); ref.forward_backward()
        assert int(obj.buffer("state")[2]) == ref.n_valid > 0
        assert np.array_equal(obj.buffer("E"), ref.buffer("E")), "hash-grid encode must be bit-exact"
        if lds == 2 and backend == 0:                       # ... and it did come from the tiles: k_encode_tiles' output holds the same features
            B_, Ep_ = ref.R * ref.S, ref.Epad
            assert np.array_equal(obj.buffer("e_soa").reshape(L, B_, 2).transpose(1, 0, 2).reshape(B_, 2 * L), ref.buffer("E").reshape(B_, Ep_)[:, :2 * L])
        # (MFMA summation order -- the fused kernels, and since round 6 the layer-at-a-time kernels of the shapes outside them: a hidden activation on a
        # rounding boundary lands one fp16 ulp away now and then, and the layers behind it carry that on)
        close_half(obj.buffer("O"), ref.buffer("O"), "network output", frac_ok=0.999)
        close_half(obj.buffer("Hid"), ref.buffer("Hid"), "hidden activations", frac_ok=0.999)
        close_half(obj.buffer("dO"), ref.buffer("dO"), "dL/dO", ulps=4, frac_ok=0.999)
        close_half(obj.buffer("dHid"), ref.buffer("dHid"), "dL/dh", ulps=4, frac_ok=0.999)
        nf = 2 * L; B_, Ep_ = ref.R * ref.S, ref.Epad
        close_half(obj.buffer("dE").reshape(B_, Ep_)[:, :nf], ref.buffer("dE").reshape(B_, Ep_)[:, :nf], "dL/dE", ulps=4, frac_ok=0.999)
        gm, rm = obj.buffer("gmlp").astype(np.float64), ref.buffer("gmlp").astype(np.float64)
        assert gm.shape == rm.shape and np.abs(gm - rm).max() < 5e-3 * np.abs(rm).max()
        gg = h2f(obj.buffer("ggrid_h")).astype(np.float64); rg = ref.buffer("ggrid").astype(np.float64); ra = ref.buffer("ggrid_abs").astype(np.float64)
        assert float((np.abs(gg - rg) > 2.0 ** -8 * ra + 2.0 ** -10 * np.abs(rg) + 1e-7).mean()) < 2e-3 and (gg != 0).sum() > 0
        obj.close(); ds.close(); ref.close()
        ds, obj, ref = _pair(pkg, orc, small_scene, kw, backend)
        obj.set_debug_dump(False); obj.set_params(p); ref.set_params(p)
        for _ in range(3):
            la = obj.train(1); ref.train(1)
        assert abs(la - ref.loss) < 5e-3 * max(1.0, abs(ref.loss))
        nm = ref.n_mlp; a, b = obj.get_params(0), ref.buffer("master")
        # (three and four hidden layers: an activation that lands one fp16 ulp away is carried through more layers in both directions; measured 1.2e-3 on one
        # of 9 500 weights of 4 x 64, everything else below 1e-3)
        close_f32(a[:nm], b[:nm], "MLP master weights after three steps", 1e-3 * max(1.0, NH / 2.0))
        assert float((np.abs(a[:nm] - b[:nm]) > 1e-3).mean()) < 1e-3
        assert float((np.abs(a[nm:] - b[nm:]) > 3e-4).mean()) < 1e-2
        if not (W == 128 and NH == 1):
            # a shape outside the fused kernels: whole steps scatter through k_grid_scatter's exact LDS accumulation (k_rows_to_bins), not through global
            # atomics into the gradient table -- which therefore still holds the zeros the stage-wise call's optimizer-less run was started from
            assert not obj.buffer("ggrid_h").any() and (a[nm:] != p[nm:]).mean() > 0.01
        # NeRF_Model::Render with these weights (EMA after the steps): the oracle's image
        ob = small_scene.objects[0]["boxes"][1]; pose = ge.load_tools().colmajor(small_scene.Twc[int(ob[0])])
        ref.set_params(obj.get_params(0)); ref.set_ema(obj.get_params(2))
        rgb, dep, msk = obj.render(ob, pose); r2, d2, m2 = ref.render(ob, pose)
        same = msk == m2
        d = np.abs(rgb - r2)[same]; assert same.mean() > 0.99 and d.max() < 4e-3 and d.mean() < 1e-4          # (measured: max 5e-5 over the eight shapes)
        obj.close(); ds.close(); ref.close()


# sizes 4920 / 35944 / 131072 x 6: 64-bit whole, 64-bit per parity, parity halves cut into two ranges
@pytest.mark.parametrize("kw", [dict(log2_hashmap_size=17, n_levels=8, base_resolution=16),
                                # 262144-entry levels: four ranges per parity half, one sample partition
                                dict(log2_hashmap_size=18, n_levels=6, base_resolution=16),
                                # every hashed level a 64-bit whole-level tile (16384 entries)
                                dict(log2_hashmap_size=14, n_levels=16, base_resolution=16),
                                # base.json's first 13 levels: the last has res = 65536, whose index is x mod 65536 (tcnn's wrapped stride loop): the one-atomic
                                # path
                                dict(log2_hashmap_size=16, n_levels=13, base_resolution=16)],
                         ids=["T17", "T18", "T14", "T16_res65536"])
def test_grid_scatter_tile_modes_match_oracle(pkg, orc, small_scene, kw):
    """k_grid_scatter picks a tile shape per level from its size (whole level / one parity half / ranges of a parity half; 32- or 64-bit accumulators):
    one forward/backward against the oracle's grid gradient on tables that exercise every shape, at base.json's batch size of the LDS path."""
    kw = dict(kw, rays_per_batch=256, n_neurons=64, n_hidden_layers=1)
    ds, obj, ref = _pair(pkg, orc, small_scene, kw, 1)
    p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
    obj.train_stages(1 | 2); ref.generate_batch(); ref.forward_backward()
    assert int(obj.buffer("state")[2]) == ref.n_valid > 0
    assert np.array_equal(obj.buffer("E"), ref.buffer("E")), "hash-grid encode must be bit-exact"
    gg = h2f(obj.buffer("ggrid_h")).astype(np.float64); rg = ref.buffer("ggrid").astype(np.float64); ra = ref.buffer("ggrid_abs").astype(np.float64)
    bound = 2.0 ** -9 * ra + 2.0 ** -10 * np.abs(rg) + 1e-7              # exact integer accumulation, one fp16 rounding per sample partition
    bad = np.abs(gg - rg) > bound
    assert float(bad.mean()) < 1e-4 and (gg != 0).sum() > 1000, (float(bad.mean()), int((gg != 0).sum()))
    assert ((gg != 0) == (rg != 0)).mean() > 0.999                       # the same entries receive a gradient
    obj.close(); ds.close(); ref.close()
    ds, obj, ref = _pair(pkg, orc, small_scene, kw, 1)                    # and three optimizer steps: the optimizer reads the planes the scatter wrote
    obj.set_debug_dump(False); obj.set_params(p); ref.set_params(p)
    for _ in range(3):
        la = obj.train(1); ref.train(1)
    nm = ref.n_mlp; a, b = obj.get_params(0), ref.buffer("master")
    assert float((np.abs(a[nm:] - b[nm:]) > 3e-4).mean()) < 1e-2
    obj.close(); ds.close(); ref.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_learning_rate_decay_follows_the_oracle(pkg, orc, small_scene, backend):
    """ExponentialDecay (base.json:9-13: start 20000, interval 10000, base 0.33 -- never reached by the 5000 offline steps, reached
    online): with the schedule pulled forward to steps 3, 5, 7 the device-side learning rate (DevState, advanced by the optimizer's last
    block) and the MLP weights follow the oracle through 8 steps."""
    kw = dict(C1, decay_start=3, decay_interval=2, decay_base=0.5)
    ds, obj, ref = _pair(pkg, orc, small_scene, kw, backend)
    p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
    lrs = []
    for _ in range(8):
        obj.train(1); ref.train(1); lrs.append(float(obj.info().learning_rate))
    # the rate each step leaves behind for the next one: halved after steps 3, 5, 7
    assert np.allclose(lrs, np.array([1, 1, 0.5, 0.5, 0.25, 0.25, 0.125, 0.125]) * 1e-2, rtol=1e-6), lrs
    nm = ref.n_mlp; a, b = obj.get_params(0), ref.buffer("master")
    close_f32(a[:nm], b[:nm], "MLP master weights after 8 decayed steps", 2e-3)
    assert float((np.abs(a[nm:] - b[nm:]) > 5e-4).mean()) < 2e-2
    obj.close(); ds.close(); ref.close()


def _trained_pair_scores(pkg, orc, ss, sc, kw, backend, steps, every=4):
    """Trains the HIP object and the oracle on identical schedules; returns (mutual PSNRs per crop, abs PSNR HIP, abs PSNR oracle, losses)."""
    _need_gpu(pkg)
    ds, obj = ge.make_problem(pkg, sc, kw); obj.set_backend(backend); ref = ge.make_oracle(orc, sc, kw)
    l_hip = obj.train(steps); l_ref = ref.train(steps)
    mutual, a_hip, a_ref = [], [], []
    for box in sc.objects[0]["boxes"][::every]:
        v, x, y, h, w = (int(q) for q in box); pose = ss.colmajor(sc.Twc[v])
        rgb, depth, mask = obj.render(box, pose); rrgb, rdepth, rmask = ref.render(box, pose)
        gt = sc.rgb[v, y:y + h, x:x + w] / 255.0; gm = sc.instance[v, y:y + h, x:x + w] > 0
        gtw = np.where(gm[..., None], gt, 1.0)
        mutual.append(psnr(rgb, rrgb)); a_hip.append(psnr(rgb, gtw)); a_ref.append(psnr(rrgb, gtw))
    obj.close(); ds.close(); ref.close()
    return mutual, a_hip, a_ref, (l_hip, l_ref)


@pytest.mark.parametrize("backend", BACKENDS)
def test_training_parity_psnr_c1(pkg, orc, ss, small_scene, backend):
    """BASELINE configs[0]: identical schedules on both sides, 300 steps, three sampling seeds.  Training amplifies any last-place
    difference (the HIP path differs from the oracle by expf / summation-order ulps from step 0), so the bar for TRAINED models is
    derived from the committed chaos-floor fixture (tests/golden/numerics_study.json, tests/test_numerics_study.py): the oracle
    against itself started one fp16 ulp away reaches 33.1 dB (min) mutual PSNR and differs by up to 0.84 dB in mean-of-three
    absolute PSNR.  Required here: mutual PSNR (min over crops and seeds) above that floor minus 3 dB, mean-of-three absolute
    PSNR within the floor's own spread of the oracle's."""
    from test_numerics_study import trained_model_bars
    mutual_floor, abs_tol = trained_model_bars()
    sc = small_scene; steps = 300; abs_hip, abs_ref, mutual = [], [], []
    for seed in (11, 12, 13):
        mu, ah, ar, (l_hip, l_ref) = _trained_pair_scores(pkg, orc, ss, sc, dict(C1, sample_seed=seed), backend, steps)
        assert l_hip < 0.05 and abs(l_hip - l_ref) < max(l_ref, 0.02)          # last-iteration losses of two chaotic runs on the same batch
        mutual += mu; abs_hip += ah; abs_ref += ar
    print("backend %d: mutual PSNR min %.2f dB (bar %.2f), abs HIP %.2f dB, abs oracle %.2f dB (tol %.2f)" % (backend, min(mutual), mutual_floor,
            np.mean(abs_hip), np.mean(abs_ref), abs_tol))
    # backend 1 is deterministic (integer scatter); backend 0 sums the grid gradient with fp16 global atomics in arrival order, so
    # its trained weights differ from run to run on top of the floor: observed mean-of-3 absolute PSNR 30.4 .. 31.3 dB against the oracle's 31.33 dB
    assert min(mutual) > (mutual_floor if backend == 1 else mutual_floor - 2.0)
    assert abs(np.mean(abs_hip) - np.mean(abs_ref)) < (abs_tol if backend == 1 else 2.0 * abs_tol) and np.mean(abs_hip) > 24.0


@pytest.mark.parametrize("backend", BACKENDS)
def test_training_parity_psnr_c2_base_json_200_steps(pkg, orc, ss, backend):
    """BASELINE configs[1] (base.json defaults at the full batch: R=4096 x S=32, hash L=16, MLP 64x1): 200 training steps on identical
    schedules, HIP path against the oracle -- mutual and absolute PSNR of rendered training crops, same fixture-derived bar as C1
    (the larger network averages more samples per step; it stays well inside it)."""
    from test_numerics_study import trained_model_bars
    mutual_floor, abs_tol = trained_model_bars()
    sc = ss.make_scene(n_views=12, H=120, W=160, f=130.0, seed=0)
    # the oracle's serial grid scatter costs ~0.1 s per full-size step: use its parallel mode (same contributions, fp32 atomics in thread
    # order -- a summation-order difference far below the chaos floor) and a larger team for this one test
    orc.lib().orc_set_parallel_scatter(1); orc.lib().orc_set_threads(min(32, os.cpu_count() or 1))
    try:
        mu, ah, ar, (l_hip, l_ref) = _trained_pair_scores(pkg, orc, ss, sc, dict(C2, sample_seed=21), backend, 200, every=3)
    finally:
        orc.lib().orc_set_parallel_scatter(0); orc.lib().orc_set_threads(int(os.environ.get("MON_ORACLE_THREADS", min(16, os.cpu_count() or 1))))
    print("C2 backend %d: mutual PSNR min %.2f mean %.2f dB, abs HIP %.2f dB, abs oracle %.2f dB, loss %.5f / %.5f" % (backend, min(mu), np.mean(mu),
            np.mean(ah), np.mean(ar), l_hip, l_ref))
    assert np.isfinite(l_hip) and abs(l_hip - l_ref) < max(l_ref, 0.02)
    assert min(mu) > (mutual_floor if backend == 1 else mutual_floor - 2.0)
    assert abs(np.mean(ah) - np.mean(ar)) < 2.0 * abs_tol and np.mean(ah) > 24.0          # single seed: twice the mean-of-three tolerance


@pytest.mark.parametrize("backend", BACKENDS)
def test_full_size_properties_c2(pkg, ss, backend):
    """BASELINE configs[1] (base.json defaults, R=4096, B=131072): properties that need no oracle."""
    _need_gpu(pkg)
    sc = ss.make_scene(n_views=24, H=240, W=320, f=260.0, seed=1)
    ds, obj = ge.make_problem(pkg, sc, C2)
    try:
        obj.set_backend(backend)
    except pkg.MonError:
        obj.close(); ds.close(); pytest.skip("fused backend not available")
    i0 = obj.info(); assert i0.n_params == 3072 + 1908736 and i0.encoded_width == 32
    if backend == 1:
        obj.set_debug_dump(True)          # the fused kernel keeps the compacted rays on chip; dump them for the rollover check
    l0 = obj.train(1); nv = obj.info().last_n_valid
    obj.set_debug_dump(False)
    assert 0 < nv <= 4096 and np.isfinite(l0)
    flags = obj.buffer("ray_flag"); o = obj.buffer("ray_o").reshape(-1, 3)
    assert np.array_equal(o[nv:], o[np.arange(nv, 4096) % nv]) and np.array_equal(flags[nv:], flags[np.arange(nv, 4096) % nv])
    mr = obj.buffer("mask_ray"); assert (mr >= 0).all() and (mr <= 1).all()
    st = obj.buffer("steps"); touched = int((st[3072:] > 0).sum())
    assert (st[:3072] == 1).all() and 0 < touched < st.size - 3072          # sparse Adam: untouched grid entries skipped
    l1 = obj.train(300)
    assert l1 < 0.35 * l0 and obj.info().train_step == 301
    p = obj.get_params(0); assert np.isfinite(p).all()
    box = sc.objects[0]["boxes"][0]; v, x, y, h, w = (int(q) for q in box)
    rgb, depth, mask = obj.render(box, ss.colmajor(sc.Twc[v]))
    gm = sc.instance[v, y:y + h, x:x + w] > 0; gt = np.where(gm[..., None], sc.rgb[v, y:y + h, x:x + w] / 255.0, 1.0)
    iou = (mask.astype(bool) & gm).sum() / max(1, (mask.astype(bool) | gm).sum())
    assert iou > 0.9 and psnr(rgb, gt) > 20.0, (iou, psnr(rgb, gt))
    obj.close(); ds.close()


@pytest.mark.parametrize("kw", [dict(rays_per_batch=64), dict(rays_per_batch=16384), dict(rays_per_batch=256, n_samples=16),
        dict(rays_per_batch=128, n_samples=64)],
                         ids=["R64_min", "R16384_fused_max", "S16_unfused", "S64_unfused"])
def test_size_limits_match_oracle(pkg, orc, small_scene, kw):
    """Smallest / largest batch of the fused kernels (R = 64 .. 16 384 rays, S = 32) and sample counts only the layer-at-a-time kernels
    take (S != 32 selects backend 0 by itself): one forward/backward against the oracle on the base.json network."""
    _need_gpu(pkg)
    ds, obj = ge.make_problem(pkg, small_scene, kw); ref = ge.make_oracle(orc, small_scene, kw)
    assert int(obj.info().backend) == (1 if kw.get("n_samples", 32) == 32 else 0)
    if int(obj.info().backend) == 1:
        obj.set_debug_dump(True)
    p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
    obj.train_stages(1 | 2); ref.generate_batch(); ref.forward_backward()
    assert int(obj.buffer("state")[2]) == ref.n_valid > 0
    assert np.array_equal(obj.buffer("E"), ref.buffer("E")), "hash-grid encode must be bit-exact"
    close_f32(obj.buffer("rgb_ray"), ref.buffer("rgb_ray"), "rgb_ray", 2e-3)
    close_f32(obj.buffer("loss_ray"), ref.buffer("loss_ray"), "loss_ray", 5e-3)
    gm, rm = obj.buffer("gmlp").astype(np.float64), ref.buffer("gmlp").astype(np.float64)
    assert np.abs(gm - rm).max() < 5e-3 * np.abs(rm).max(), (np.abs(gm - rm).max(), np.abs(rm).max())
    gg = h2f(obj.buffer("ggrid_h")).astype(np.float64); rg = ref.buffer("ggrid").astype(np.float64); ra = ref.buffer("ggrid_abs").astype(np.float64)
    assert float((np.abs(gg - rg) > 2.0 ** -8 * ra + 2.0 ** -10 * np.abs(rg) + 1e-7).mean()) < 2e-3 and (gg != 0).sum() > 0
    obj.train_stages(4); l = obj.train(3)
    assert np.isfinite(l) and np.isfinite(obj.get_params(0)).all()
    obj.close(); ds.close(); ref.close()


def test_base_json_training_runs_on_the_fused_path_at_speed(pkg, ss):
    """Guard against a silent fall-back to the layer-at-a-time kernels (or a lost order of magnitude): base.json at the full batch must
    select the fused backend by itself and take well under 0.2 ms per step (measured 0.08-0.1 ms; the unfused kernels need 0.7 ms)."""
    _need_gpu(pkg)
    import time
    sc = ss.make_scene(n_views=16, H=240, W=320, f=260.0, seed=2)
    ds, obj = ge.make_problem(pkg, sc, {})
    assert int(obj.info().backend) == 1
    obj.train(50); pkg.lib().mon_device_synchronize(0)
    t0 = time.perf_counter(); obj.train(400); pkg.lib().mon_device_synchronize(0); dt = (time.perf_counter() - t0) / 400
    assert dt < 0.2e-3, "%.3f ms per step" % (1e3 * dt)
    obj.close(); ds.close()


def test_create_train_render_mesh_destroy_does_not_leak(pkg, ss, small_scene):
    """Device memory after 40 rounds of dataset + object create / train / render (growing crops) / mesh / destroy returns to where it was
    after the first rounds (allocator caches settle); online objects come and go with the map (LocalMapping.cc:1231)."""
    _need_gpu(pkg)
    sc = small_scene

    def round_trip(k):
        ds, obj = ge.make_problem(pkg, sc, dict(C1, sample_seed=k)); obj.train(5)
        for s in (8, 40, 100):                                  # whole-crop output buffers grow on demand
            obj.render(np.array([0, 0, 0, s, s], np.uint32), ss.colmajor(sc.Twc[0]))
        obj.generate_mesh(32, 2.0); obj.close(); ds.close()

    for k in range(4):
        round_trip(k)
    free0, _ = pkg.device_mem_info(0)
    for k in range(40):
        round_trip(100 + k)
    free1, _ = pkg.device_mem_info(0)
    assert free0 - free1 < 64 << 20, "device memory shrank by %.1f MB over 40 create/destroy rounds" % ((free0 - free1) / 2 ** 20)


def test_edge_cases(pkg, ss, small_scene):
    _need_gpu(pkg)
    sc = small_scene
    ds, obj = ge.make_problem(pkg, sc, C1)
    # boxes outside the image / unknown frame are rejected (the reference would read out of bounds)
    for bad in ([0, 150, 10, 20, 20], [99, 0, 0, 8, 8], [0, 0, 0, 0, 8]):
        with pytest.raises(pkg.MonError) as e:
            obj.add_boxes(np.array([bad], np.uint32))
        assert e.value.code == 1
    obj.close()
    # training before any box was supplied
    cfg = pkg.default_config(**C1); ob = sc.objects[0]
    o2 = pkg.ObjectNeRF(ds, cfg, ob["cls"], ss.colmajor(ob["Tow"]), -ob["half"], ob["half"])
    with pytest.raises(pkg.MonError) as e:
        o2.train(1)
    assert e.value.code == 5
    # a 3-D box nobody looks at: zero rays inside -> the step is skipped, parameters untouched (reference: UB)
    far = ob["Tow"].copy(); far[:3, 3] += 50.0
    o3 = pkg.ObjectNeRF(ds, cfg, ob["cls"], ss.colmajor(far), -ob["half"], ob["half"]); o3.add_boxes(ob["boxes"])
    before = o3.get_params(0); o3.train(3); after = o3.get_params(0)
    st = o3.buffer("state")
    assert int(st[0]) == 0 and int(st[1]) == 3 and int(st[2]) == 0 and int(st[7]) == 3 and np.array_equal(before, after)
    o3.close(); o2.close()
    # ragged ray count
    with pytest.raises(pkg.MonError):
        pkg.ObjectNeRF(ds, pkg.default_config(rays_per_batch=1000), 1, ss.colmajor(ob["Tow"]), -ob["half"], ob["half"])
    # rng_flags outside its definition (stream mode 3, stray bits, a million lanes)
    for bad_flags in (3, 1 << 8, (2048 << 16) | 1):
        c_bad = pkg.default_config(**C1); c_bad.rng_flags = bad_flags
        with pytest.raises(pkg.MonError) as e:
            pkg.ObjectNeRF(ds, c_bad, 1, ss.colmajor(ob["Tow"]), -ob["half"], ob["half"])
        assert e.value.code == 1
    # occluder: pixels of another instance id never become rays (nerf_model.cu:398-401)
    sc2 = ss.make_scene(n_views=8, H=120, W=160, f=130.0, n_objects=3, seed=4)
    ds2, o4 = ge.make_problem(pkg, sc2, C1, obj_index=1)
    o4.train_stages(1 | 2)
    assert int(o4.buffer("state")[2]) > 0
    o4.close(); ds2.close(); ds.close()


@pytest.mark.parametrize("kw", [C1, C2, dict(rays_per_batch=512, n_levels=13, n_neurons=64, n_hidden_layers=2)], ids=["c1", "c2", "l13w64x2"])
def test_optimizer_prepares_the_next_iteration(pkg, orc, small_scene, kw):
    """Fused backend: k_optimizer writes the MFMA fragment image while it updates the weights and generates the next iteration's
    candidate rays; both must equal what the stand-alone kernels produce (image from the new weights, GenerateRays of iter + 1)."""
    ds, obj, ref = _pair(pkg, orc, small_scene, kw, 1)
    obj.set_debug_dump(False)
    obj.train(3)
    assert np.array_equal(obj.buffer("frag_train"), obj.buffer("frag_ref"))          # image == rebuilt from the current fp16 weights
    pre = {b: obj.buffer(b).copy() for b in ("mask",)}
    it = int(obj.buffer("state")[1])
    ref.set_params(obj.get_params(0))
    for _ in range(it):
        ref.advance_iter()
    ref.generate_batch()
    nv = int(sum(bin(int(w)).count("1") for w in pre["mask"]))
    assert nv == ref.n_valid and nv > 0                                               # candidates of iteration `it` already sit in the buffers
    obj.train_stages(1)                                                               # a no-op now: nothing to regenerate
    assert np.array_equal(obj.buffer("mask"), pre["mask"])
    obj.add_boxes(small_scene.objects[0]["boxes"][:2]); ref.add_boxes(small_scene.objects[0]["boxes"][:2])   # invalidates the pre-generated batch
    obj.train_stages(1); ref.generate_batch()
    assert int(sum(bin(int(w)).count("1") for w in obj.buffer("mask"))) == ref.n_valid
    l0 = obj.train(5); assert np.isfinite(l0)
    assert np.array_equal(obj.buffer("frag_train"), obj.buffer("frag_ref"))
    obj.close(); ds.close(); ref.close()


def test_zero_gradient_skipping_is_exact_and_deterministic():
    """k_fused_train drops rays / samples whose fp16 dL/dO is all zeros before the backward MFMAs and the grid scatter.  The trained
    parameters must be bit-identical to a run that keeps every sample (option keep_zero_samples) and identical from run to run."""
    import subprocess, sys
    from conftest import ROOT
    def run(extra):
        env = dict(os.environ, **extra)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "param_crc.py"), "3", "150", "250"], capture_output=True, text=True, env=env,
                timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        rows = [ln.split() for ln in r.stdout.strip().split("\n") if ln.startswith("steps+")]
        return [w[2] for w in rows], [int(w[4]) for w in rows]
    crc_a, n_a = run({}); crc_b, n_b = run({}); crc_c, n_c = run({"MON_OPTIONS": "keep_zero_samples=1"})
    assert crc_a == crc_b == crc_c, (crc_a, crc_b, crc_c)
    crc_g, _ = run({"MON_OPTIONS": "use_graph=1"})                              # hipGraph replay of the same launches
    assert crc_g == crc_a, (crc_g, crc_a)
    assert n_c[-1] == 4096 * 32 and n_a[-1] < n_c[-1] // 2, (n_a, n_b, n_c)            # the skipping really happened in the default run


@pytest.mark.parametrize("kw", [dict(rays_per_batch=256, log2_hashmap_size=19, n_neurons=64, n_hidden_layers=1),
                                dict(rays_per_batch=256, log2_hashmap_size=20, n_levels=8, per_level_scale=2.0, n_neurons=32, n_hidden_layers=2)], ids=["T19",
                                        "T20L8"])
def test_large_tables_mix_lds_and_atomic_levels(pkg, orc, small_scene, kw):
    """Tables beyond 2^18 entries per level: the fine levels scatter with global packed-f16 atomics inside k_fused_train, the coarse ones
    through k_grid_scatter (compacted rows) -- one step against the oracle, then a short run that has to learn."""
    ds, obj, ref = _pair(pkg, orc, small_scene, kw, 1)
    p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
    obj.train_stages(1 | 2); ref.generate_batch(); ref.forward_backward()
    assert int(obj.buffer("state")[2]) == ref.n_valid
    assert np.array_equal(obj.buffer("E"), ref.buffer("E")), "hash-grid encode must be bit-exact"
    gg = h2f(obj.buffer("ggrid_h")).astype(np.float64); rg = ref.buffer("ggrid").astype(np.float64); ra = ref.buffer("ggrid_abs").astype(np.float64)
    bound = 2.0 ** -8 * ra + 2.0 ** -10 * np.abs(rg) + 1e-7           # fp16 atomics in arrival order vs fp32 accumulation
    assert float((np.abs(gg - rg) > bound).mean()) < 2e-3 and (gg != 0).sum() > 0
    obj.train_stages(4)
    obj.set_debug_dump(False)
    l0 = obj.train(1); l1 = obj.train(150)
    assert np.isfinite(l1) and l1 < 0.6 * l0, (l0, l1)
    obj.close(); ds.close(); ref.close()


def test_binned_large_level_scatter_is_exact_and_deterministic(pkg, orc, small_scene):
    """Levels beyond 2^18 entries while many samples carry a gradient (kernels_bigscatter.hip): contributions are counting-sorted by
    16 384-entry tile and summed exactly in LDS, so the fp16 gradient is the fp32 sum of tcnn's fp16 contributions rounded ONCE --
    tighter than arrival-order atomics -- and a run that never leaves the binned path (option big_switch = 1) is bit-reproducible."""
    import subprocess, sys
    from conftest import ROOT
    kw = dict(rays_per_batch=256, log2_hashmap_size=19, n_neurons=64, n_hidden_layers=1)
    ds, obj, ref = _pair(pkg, orc, small_scene, kw, 1)
    p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
    obj.train_stages(1 | 2); ref.generate_batch(); ref.forward_backward()
    gg = h2f(obj.buffer("ggrid_h")).astype(np.float64); rg = ref.buffer("ggrid").astype(np.float64); ra = ref.buffer("ggrid_abs").astype(np.float64)
    loose = 2.0 ** -8 * ra + 2.0 ** -10 * np.abs(rg) + 1e-7
    assert float((np.abs(gg - rg) > loose).mean()) < 1e-4 and (gg != 0).sum() > 0
    big = np.zeros(gg.size, bool); big[gg.size // 2:] = True                 # the fine (binned) levels sit in the upper half of the table
    # what is left: one fp16 rounding of the sum, and dL/dE rows that differ from the oracle's by an fp16 ulp
    err = np.abs(gg - rg)[big & (rg != 0)]; ref_mag = np.abs(rg)[big & (rg != 0)]
    assert np.median(err / ref_mag) < 2.0 ** -10, float(np.median(err / ref_mag))
    obj.close(); ds.close(); ref.close()

    def run(extra):
        env = dict(os.environ, MON_CRC_CFG='{"log2_hashmap_size": 19}', **extra)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "param_crc.py"), "2", "20"], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return [ln.split()[2] for ln in r.stdout.strip().split("\n") if ln.startswith("steps+")]
    a = run({"MON_OPTIONS": "big_switch=1"}); b = run({"MON_OPTIONS": "big_switch=1"})
    assert a == b and len(a) == 2, (a, b)


def test_atomic_path_marks_every_touched_chunk(pkg, small_scene, monkeypatch):
    """tcnn-style global atomics on the large levels (option big_switch = 0 forces them from the first step): every addition into the
    gradient table also sets its chunk's byte flag, so the lazy optimizer -- which only visits flagged chunks -- must leave the table
    all zero after each step, and must have stepped some of those entries."""
    _need_gpu(pkg)
    kw = dict(rays_per_batch=256, log2_hashmap_size=19, n_neurons=64, n_hidden_layers=1)
    old = pkg.get_option("big_switch"); pkg.set_option("big_switch", 0)
    try:
        ds, obj = ge.make_problem(pkg, small_scene, kw); obj.set_backend(1)
    finally:
        pkg.set_option("big_switch", old)                       # (read when the object is created)
    obj.train(6)
    gg = obj.buffer("ggrid_h"); st = obj.buffer("steps")
    assert not gg[gg.size // 2:].any(), "a gradient survived the optimizer: its chunk was not flagged"
    assert (st[st.size // 2:] > 0).sum() > 1000
    obj.close(); ds.close()


def test_stress_configuration_t22_full_size_properties(pkg, ss):
    """BASELINE configs[4] (T = 2^22: 105 M parameters, a 211 MB fp16 table) at the full batch: far beyond what the oracle finishes in
    seconds, so size-independent properties -- sparse Adam touches only entries that got a gradient, the loss falls, the lazily
    maintained EMA renders the object (mask IoU / PSNR against the synthetic ground truth), parameters stay finite."""
    _need_gpu(pkg)
    sc = ss.make_scene(n_views=16, H=240, W=320, f=260.0, seed=3)
    ds, obj = ge.make_problem(pkg, sc, dict(log2_hashmap_size=22)); obj.set_backend(1)
    n_mlp = obj.info().n_mlp_params
    l0 = obj.train(1); st = obj.buffer("steps")
    assert (st[:n_mlp] == 1).all() and 0 < int((st[n_mlp:] > 0).sum()) < 0.5 * (st.size - n_mlp)
    l1 = obj.train(400)
    assert np.isfinite(l1) and l1 < 0.35 * l0, (l0, l1)
    st = obj.buffer("state"); assert int(st[24]) > 0                         # gradient-carrying samples of the last iteration
    box = sc.objects[0]["boxes"][0]; v, x, y, h, w = (int(q) for q in box)
    rgb, depth, mask = obj.render(box, ss.colmajor(sc.Twc[v]))
    gm = sc.instance[v, y:y + h, x:x + w] > 0; gt = np.where(gm[..., None], sc.rgb[v, y:y + h, x:x + w] / 255.0, 1.0)
    iou = (mask.astype(bool) & gm).sum() / max(1, (mask.astype(bool) | gm).sum())
    assert iou > 0.85 and psnr(rgb, gt) > 18.0, (iou, psnr(rgb, gt))
    assert np.isfinite(h2f(obj.get_params(2))).all()                        # the EMA weights after k_ema_finalize
    obj.close(); ds.close()


@pytest.mark.parametrize("backend", BACKENDS)
def test_depth_supervised_gradient_matches_oracle(pkg, orc, small_scene, backend):
    """use_depth (dense depth offline, sparse depth online: CORE/src/nerf_model.cu:431-434, 869-872): the L1 depth term of the
    hand-derived gradient, forward/backward against the oracle."""
    kw = dict(rays_per_batch=256, n_levels=16, n_neurons=64, n_hidden_layers=1)
    ds, obj, ref = _pair(pkg, orc, small_scene, kw, backend, use_depth=True)
    p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
    obj.train_stages(1 | 2); ref.generate_batch(); ref.forward_backward()
    assert int(obj.buffer("state")[2]) == ref.n_valid and (ref.buffer("target_depth") > 0).sum() > 10
    if backend == 0:
        close_f32(obj.buffer("target_depth"), ref.buffer("target_depth"), "target depth", 1e-6)
    fr = 1.0 if backend == 0 else 0.999
    close_half(obj.buffer("O"), ref.buffer("O"), "network output", frac_ok=fr)
    close_half(obj.buffer("dO"), ref.buffer("dO"), "dL/dO with the depth term", ulps=4, frac_ok=0.999)
    close_f32(obj.buffer("depth_ray"), ref.buffer("depth_ray"), "depth_ray", 3e-3)
    close_f32(obj.buffer("loss_ray"), ref.buffer("loss_ray"), "loss_ray", 5e-3)
    gm, rm = obj.buffer("gmlp").astype(np.float64), ref.buffer("gmlp").astype(np.float64)
    assert np.abs(gm - rm).max() < 5e-3 * np.abs(rm).max()
    # the depth term is really in there: without depth supervision dL/dO differs
    ds2, obj2, ref2 = _pair(pkg, orc, small_scene, kw, backend, use_depth=False)
    obj2.set_params(p); obj2.train_stages(1 | 2)
    assert (h2f(obj2.buffer("dO")) != h2f(obj.buffer("dO"))).mean() > 0.01
    for o in (obj, ds, ref, obj2, ds2, ref2):
        o.close()


def test_lazy_ema_matches_eager_on_large_tables(pkg, small_scene):
    """Tables above 8 M parameters skip untouched chunks in the optimizer altogether and catch their EMA up in closed form when the chunk
    is touched again or the inference weights are read.  The device's EMA is compared with the eager step-by-step fp16 recurrence
    (tcnn ema_step_half_precision, restated here in NumPy) run on the weights the device itself produced after every step, so the
    comparison does not depend on the arrival order of the fine levels' global atomics."""
    _need_gpu(pkg)
    ds, obj = ge.make_problem(pkg, small_scene, dict(rays_per_batch=512, log2_hashmap_size=19))
    assert obj.info().n_grid_params > (8 << 20)
    d = np.float32(0.95); e = np.zeros(obj.info().n_params, np.float32); touched_any = np.zeros(e.size, bool); w_prev = h2f(obj.get_params(1))
    for t in range(1, 31):
        obj.train(1); w = h2f(obj.get_params(1)); touched_any = w != w_prev; w_prev = w
        deb_old = np.float32(1.0) - np.float32(float(d) ** (t - 1)); deb_new = np.float32(1.0) / (np.float32(1.0) - np.float32(float(d) ** t))
        e = (((e * d) * deb_old + w * (np.float32(1.0) - d)) * deb_new).astype(np.float16).astype(np.float32)
    got = h2f(obj.get_params(2))
    # a few fp16 ulps of the quantities being averaged: an EMA that has cancelled to far below |w| carries the rounding of its larger past
    # values in either schedule (grid values start at 1e-4: subnormal ulp 2^-24)
    err = np.abs(got - e); tol = 2.0 ** -9 * (np.abs(e) + np.abs(w)) + 3 * 2.0 ** -24
    assert (err > tol).mean() < 1e-3 and err.max() < 1e-3, (float((err > tol).mean()), float(err.max()))
    assert 0.001 < touched_any[obj.info().n_mlp_params:].mean() < 0.9                 # the last step really left most entries alone and changed some
    # reading the inference weights again changes nothing; training on and reading again stays consistent
    assert np.array_equal(h2f(obj.get_params(2)), got)
    obj.close(); ds.close()


LARGE = {"T19": dict(rays_per_batch=256, log2_hashmap_size=19, n_neurons=64, n_hidden_layers=1),
         "T20L8": dict(rays_per_batch=256, log2_hashmap_size=20, n_levels=8, per_level_scale=2.0, n_neurons=32, n_hidden_layers=2)}


@pytest.mark.parametrize("name", sorted(LARGE))
def test_large_table_optimizer_matches_oracle(pkg, orc, small_scene, name):
    """Tables above 8 M parameters (BASELINE configs[4]'s regime) run k_optimizer<false, true>: untouched chunks are skipped altogether (lazy EMA, closed-form
    catch-up), the state sits in 128-byte chunk records, touched chunks are found through byte flags, step counters are 16-bit.  Three WHOLE steps on both
    sides from the pattern parameters, binned scatter (deterministic) -- the shipping build here; the variant builds that keep the four state arrays, 32-bit
    counters or scan the gradient table instead of flags run the same test through tools/gpu_variants_large.sh (profiles/r06_variants.md) -- against the ORACLE's
    Trainer::optimizer_step (tcnn's rule, nerf_model.cu:1644: zero-gradient grid entries untouched, per-parameter bias correction, debiased EMA of every
    parameter every step), with the bars of the base-size step tests.  Entries that never saw a gradient must still hold the pattern bit for bit, with empty
    Adam state, and their lazily caught-up EMA must equal the oracle's eager step-by-step one."""
    _need_gpu(pkg)
    kw = LARGE[name]
    ref = ge.make_oracle(orc, small_scene, kw); p = pattern_params(ref); ref.set_params(p)
    for _ in range(3):
        ref.train(1)
    nm = ref.n_mlp; want = {b: ref.buffer(b) for b in ("master", "half", "ema", "m1", "m2", "steps")}; loss_ref = ref.loss; ref.close()
    old = {"big_switch": pkg.get_option("big_switch")}
    try:
        pkg.set_option("big_switch", 1)
        for combo in (("shipping",),):
            ds, obj = ge.make_problem(pkg, small_scene, kw); obj.set_backend(1)
            assert obj.info().n_grid_params > (8 << 20)
            obj.set_params(p)
            for _ in range(3):
                la = obj.train(1)
            assert abs(la - loss_ref) < 5e-3 * max(1.0, abs(loss_ref)), combo
            a = obj.buffer("master"); st = obj.buffer("steps"); m1 = obj.buffer("m1"); m2 = obj.buffer("m2")
            assert np.array_equal(a, obj.get_params(0))
            close_f32(a[:nm], want["master"][:nm], "MLP master weights after three steps %s" % (combo,), 1e-3)
            assert (st[:nm] == 3).all()
            touched = (st > 0) | (want["steps"] > 0); touched[:nm] = False
            assert 1000 < touched.sum() < 0.5 * touched.size, combo                  # most of such a table never sees a gradient in three small batches
            d = np.abs(a[touched] - want["master"][touched])
            assert float((d > 3e-4).mean()) < 1e-2, (combo, float((d > 3e-4).mean()))
            assert float((st[touched] != want["steps"][touched]).mean()) < 2e-2, (combo, float((st[touched] != want["steps"][touched]).mean()))
            same = touched & (st == want["steps"])
            for got, w, what, rel in ((m1, want["m1"], "m1", 2.0 ** -6), (m2, want["m2"], "m2", 2.0 ** -5)):
                bad = np.abs(got[same] - w[same]) > rel * np.abs(w[same]) + 1e-12
                assert float(bad.mean()) < 2e-2, (combo, what, float(bad.mean()))
            # never touched: the pattern itself, no Adam state (tcnn skips zero-gradient grid entries entirely)
            un = ~touched; un[:nm] = False
            assert np.array_equal(a[un], p[un]) and not m1[un].any() and not m2[un].any()
            hw = obj.get_params(1); assert np.array_equal(h2f(hw), a.astype(np.float16).astype(np.float32))          # fp16 copy == h(master) everywhere
            # EMA (inference weights, k_ema_finalize first): touched entries with the step bars, untouched ones -- closed-form catch-up over all three
            # steps against the eager recurrence -- within an fp16 ulp
            ea, eb = h2f(obj.get_params(2)), h2f(want["ema"])
            assert (np.abs(ea - eb)[touched] > 4e-3 * np.maximum(np.abs(eb[touched]), 1e-2)).mean() < 1e-2, combo
            err = np.abs(ea[un] - eb[un]); assert float((err > _ulp16(eb[un])).mean()) < 1e-4 and err.max() <= 2 * _ulp16(eb[un]).max(), (combo, err.max())
            assert (np.abs(ea[:nm] - eb[:nm]) > 4e-3 * np.maximum(np.abs(eb[:nm]), 1e-2)).mean() < 1e-2
            obj.close(); ds.close()
    finally:
        for n, v in old.items():
            pkg.set_option(n, v)


@pytest.mark.parametrize("variant", ["default", "binned"])
def test_large_table_optimizer_follows_the_oracle_over_30_steps_on_its_own_gradients(pkg, orc, small_scene, variant):
    """The large-table optimizer over a 30-step run, judged by the ORACLE's optimizer instead of a NumPy recurrence: every step the device's own gradients
    (fp32 MLP gradient; grid gradient = gradient table + partial tables as k_optimizer sums them) are handed to the oracle's Trainer::optimizer_step, so both
    sides integrate the SAME gradient sequence and the comparison is free of the training trajectory's chaos and of the arrival order of the fine levels'
    atomics: master weights, both Adam moments and the per-parameter step counters must agree to fp32 rounding after 1, 2, 5 and 30 steps, the fp16 copy up to
    rounding-boundary flips, and the LAZILY maintained EMA (chunks catch up in closed form when they are touched again or the inference weights are read)
    must equal the oracle's eager every-parameter-every-step EMA.  `default`: the shipping library (records, flags, 16-bit counters, binned -> atomic switch);
    `binned`: the binned scatter throughout, with the inference weights also read in the middle of the run (finalize, then train on).  The variant builds
    (arrays / 32-bit counters / no flags) run both through tools/gpu_variants_large.sh."""
    _need_gpu(pkg)
    kw = dict(rays_per_batch=512, log2_hashmap_size=19)
    opts = {} if variant == "default" else dict(big_switch=1)
    old = {n: pkg.get_option(n) for n in opts}
    try:
        for n, v in opts.items():
            pkg.set_option(n, v)
        ds, obj = ge.make_problem(pkg, small_scene, kw); obj.set_backend(1)
    finally:
        for n, v in old.items():
            pkg.set_option(n, v)                                       # (read when the object is created)
    assert obj.info().n_grid_params > (8 << 20)
    ref = ge.make_oracle(orc, small_scene, kw); nm = ref.n_mlp
    p = obj.get_params(0); ref.set_params(p)                         # the same initial weights (pcg32 init on both sides; taken from the device to be sure)
    ever = np.zeros(p.size, bool); per_step = []
    for t in range(1, 31):
        obj.train_stages(1 | 2)
        gm = obj.buffer("gmlp"); gg = obj.buffer("ggrid_f32")
        obj.train_stages(4); ref.optimizer_step_with(gm, gg)
        ever[nm:] |= gg != 0; per_step.append(float((gg != 0).mean()))
        if variant != "default" and t == 12:
            ea, eb = h2f(obj.get_params(2)), h2f(ref.buffer("ema"))
            err = np.abs(ea - eb); tol = 2.0 ** -9 * (np.abs(eb) + np.abs(h2f(ref.buffer("half")))) + 3 * 2.0 ** -24
            assert (err > tol).mean() < 1e-3 and err.max() < 1e-3, (t, float((err > tol).mean()), float(err.max()))
        if t in (1, 2, 5, 30):
            a, b = obj.buffer("master"), ref.buffer("master")
            assert np.array_equal(obj.buffer("steps"), ref.buffer("steps")), "per-parameter step counters after %d steps" % t
            d = np.abs(a - b); assert d.max() <= 5e-6 and float((d > 1e-6).mean()) < 1e-4, (t, float(d.max()))
            for name, rel in (("m1", 1e-5), ("m2", 1e-5)):
                x, y = obj.buffer(name), ref.buffer(name)
                # (a moment that has cancelled to far below its terms carries their rounding: bounded against the largest moment instead)
                e = np.abs(x - y); assert float((e > rel * np.abs(y)).mean()) < 1e-5 and e.max() <= 1e-6 * np.abs(y).max(), (t, name, float(e.max()))
            # fp16 copy = h(master): masters that agree to 1e-6 sit on either side of a rounding boundary now and then (grid values start at 1e-4,
            # where the fp16 spacing is 6e-8) -- never further apart than one fp16 step
            ha, hb = h2f(obj.get_params(1)), h2f(ref.buffer("half"))
            assert float((ha != hb).mean()) < 1e-3 and (np.abs(ha - hb) <= _ulp16(hb)).all()
    st = ref.buffer("steps")
    # every step leaves most of the table alone (the lazy path is what ran), over the run nearly every entry is stepped, some again and again
    assert (st[:nm] == 30).all() and 0.001 < min(per_step) and max(per_step) < 0.5 and (st[nm:] > 0).mean() > 0.5 and st[nm:].max() > 3, (min(per_step), max(per_step))
    assert np.array_equal(st > 0, ever | (np.arange(st.size) < nm))                                     # exactly the entries that ever had a gradient
    ea, eb = h2f(obj.get_params(2)), h2f(ref.buffer("ema")); w = h2f(ref.buffer("half"))
    # a few fp16 ulps of the quantities being averaged: the closed form rounds once where the recurrence rounds every step
    err = np.abs(ea - eb); tol = 2.0 ** -9 * (np.abs(eb) + np.abs(w)) + 3 * 2.0 ** -24
    assert (err > tol).mean() < 1e-3 and err.max() < 1e-3, (float((err > tol).mean()), float(err.max()))
    assert np.array_equal(h2f(obj.get_params(2)), ea)                 # reading the inference weights again changes nothing
    obj.close(); ds.close(); ref.close()


@pytest.mark.parametrize("chain", ["b0", "gather", "tiles"])
def test_base_size_optimizer_follows_the_oracle_over_30_steps_on_its_own_gradients(pkg, orc, small_scene, chain):
    """The base-size k_optimizer -- the kernel the benchmark times; otherwise compared with the oracle after one and three whole steps only, where Adam's
    first steps are +-lr whatever the gradient -- judged like the large-table one above: every step the device's own gradients (gmlp, ggrid_f32) are handed
    to the oracle's Trainer::optimizer_step, and master weights, both moments, the step counters and the fp16 copy are compared after 1, 2, 5 and 30 steps
    with the same bars.  c2s on backend 0, the gather chain and the level-tile chain of backend 1.  After each checkpoint the optimizer's other outputs too:
    half == h(master), the tile image == the fp16 grid in tile order (level-tile chain), the MFMA fragment image == one rebuilt from the weights (backend 1).
    Then 30 further steps from parameters trained 150 steps on the device, on a fresh pair (set_params keeps the Adam state on both sides, so it is a fresh
    object and a fresh oracle that start from empty moments -- checked): the same bars at gradients of the trained regime, mostly exact zeros."""
    _need_gpu(pkg)
    kw = dict(CFGS["c2s"])
    def pair():
        old = pkg.get_option("lds_encode")
        try:
            if chain == "tiles":
                pkg.set_option("lds_encode", 2)
            ds, obj = ge.make_problem(pkg, small_scene, kw)
        finally:
            pkg.set_option("lds_encode", old)                              # (read when the object is created)
        obj.set_backend(0 if chain == "b0" else 1)
        return ds, obj, ge.make_oracle(orc, small_scene, kw)
    def follow(obj, ref, what):
        nm = ref.n_mlp; ever = np.zeros(ref.n_params, bool); per_step = []
        for name in ("m1", "m2", "steps"):
            assert not obj.buffer(name).any() and not ref.buffer(name).any(), (what, name, "a fresh pair starts from empty Adam state")
        for t in range(1, 31):
            obj.train_stages(1 | 2)
            gm = obj.buffer("gmlp"); gg = obj.buffer("ggrid_f32")
            obj.train_stages(4); ref.optimizer_step_with(gm, gg)
            ever[nm:] |= gg != 0; per_step.append(float((gg != 0).mean()))
            if t in (1, 2, 5, 30):
                a, b = obj.buffer("master"), ref.buffer("master")
                assert np.array_equal(obj.buffer("steps"), ref.buffer("steps")), "%s: per-parameter step counters after %d steps" % (what, t)
                d = np.abs(a - b); assert d.max() <= 5e-6 and float((d > 1e-6).mean()) < 1e-4, (what, t, float(d.max()))
                for name, rel in (("m1", 1e-5), ("m2", 1e-5)):
                    x, y = obj.buffer(name), ref.buffer(name)
                    e = np.abs(x - y); assert float((e > rel * np.abs(y)).mean()) < 1e-5 and e.max() <= 1e-6 * np.abs(y).max(), (what, t, name, float(e.max()))
                ha, hb = h2f(obj.get_params(1)), h2f(ref.buffer("half"))
                assert float((ha != hb).mean()) < 1e-3 and (np.abs(ha - hb) <= _ulp16(hb)).all(), (what, t)
                with np.errstate(over="ignore"):
                    assert np.array_equal(ha, a.astype(np.float16).astype(np.float32)), "%s: fp16 copy == h(master) after %d steps" % (what, t)
                if chain == "tiles":
                    half = obj.buffer("half")[nm:].reshape(-1, 2); tiles = obj.buffer("half_tiles").reshape(-1, 2); off = 0
                    for size in _level_sizes(obj.cfg):
                        lv = half[off:off + size]
                        want = lv if size <= 163840 // 4 else np.concatenate([lv[0::2], lv[1::2]])
                        assert np.array_equal(tiles[off:off + size], want), "%s: tile image of the level at entry offset %d after %d steps" % (what, off, t)
                        off += size
                if chain != "b0":
                    assert np.array_equal(obj.buffer("frag_train"), obj.buffer("frag_ref")), "%s: fragment image after %d steps" % (what, t)
        st = ref.buffer("steps")
        assert (st[:nm] == 30).all() and np.array_equal(st > 0, ever | (np.arange(st.size) < nm))       # exactly the entries that ever had a gradient
        ea, eb = h2f(obj.get_params(2)), h2f(ref.buffer("ema")); w = h2f(ref.buffer("half"))
        err = np.abs(ea - eb); tol = 2.0 ** -9 * (np.abs(eb) + np.abs(w)) + 3 * 2.0 ** -24
        assert (err > tol).mean() < 1e-3 and err.max() < 1e-3, (what, float((err > tol).mean()), float(err.max()))
        return per_step
    ds, obj, ref = pair()
    ref.set_params(obj.get_params(0))                                  # the same initial weights, taken from the device
    dense = follow(obj, ref, "from the initial weights")
    obj.close(); ds.close(); ref.close()
    ds, obj = ge.make_problem(pkg, small_scene, kw); obj.train(150); p = obj.get_params(0); obj.close(); ds.close()
    ds, obj, ref = pair()
    obj.set_params(p); ref.set_params(p)
    sparse = follow(obj, ref, "from trained weights")
    assert np.mean(sparse) < np.mean(dense), (dense[:3], sparse[:3])   # the trained regime: fewer grid entries see a gradient than from the start
    obj.close(); ds.close(); ref.close()


def test_stress_configuration_t22_matches_oracle(pkg, orc, small_scene):
    """BASELINE configs[4]'s table itself -- T = 2^22: 105 M parameters, levels whose res^3 overflows 32 bits -- against the oracle at a batch the oracle
    finishes in seconds (R = 256, base.json otherwise): encode bit-exact on every level, network output and dL/dO within the fp16 bars, the grid gradient
    inside the fp16 accumulation bound, and one whole optimizer step (chunk records, touched flags, lazy EMA) with the one-step bars on the entries that
    received a gradient; everything else untouched.  (~3.5 GB of host memory for the oracle's state.)"""
    kw = dict(rays_per_batch=256, log2_hashmap_size=22)
    ds, obj, ref = _pair(pkg, orc, small_scene, kw, 1)
    assert obj.info().n_grid_params > (100 << 20)
    p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
    obj.train_stages(1 | 2); ref.generate_batch(); ref.forward_backward()
    assert int(obj.buffer("state")[2]) == ref.n_valid > 0
    assert np.array_equal(obj.buffer("E"), ref.buffer("E")), "hash-grid encode must be bit-exact at T = 2^22"
    close_half(obj.buffer("O"), ref.buffer("O"), "network output", frac_ok=0.999)
    close_half(obj.buffer("dO"), ref.buffer("dO"), "dL/dO", ulps=4, frac_ok=0.999)
    gm, rm = obj.buffer("gmlp").astype(np.float64), ref.buffer("gmlp").astype(np.float64)
    assert np.abs(gm - rm).max() < 5e-3 * np.abs(rm).max()
    gg = h2f(obj.buffer("ggrid_h")); rg = ref.buffer("ggrid"); ra = ref.buffer("ggrid_abs")
    nz = (gg != 0) | (rg != 0)
    assert 10000 < nz.sum() < 0.1 * nz.size
    bound = 2.0 ** -8 * ra[nz].astype(np.float64) + 2.0 ** -10 * np.abs(rg[nz]).astype(np.float64) + 1e-7
    assert float((np.abs(gg[nz].astype(np.float64) - rg[nz]) > bound).mean()) < 2e-3
    del gg, rg, ra
    obj.train_stages(4); ref.train_step()                                # the oracle redoes the same batch, then steps
    nm = ref.n_mlp; a, b = obj.buffer("master"), ref.buffer("master")
    close_f32(a[:nm], b[:nm], "MLP master weights after one step", 2e-4)
    st_a, st_b = obj.buffer("steps"), ref.buffer("steps")
    touched = (st_a > 0) | (st_b > 0); touched[:nm] = False
    assert (st_a[:nm] == 1).all() and int(st_a.max()) == 1 and float((st_a[touched] != st_b[touched]).mean()) < 5e-3
    assert float((np.abs(a[touched] - b[touched]) > 1e-4).mean()) < 5e-3
    un = ~touched; un[:nm] = False
    assert np.array_equal(a[un], p[un])
    ea, eb = h2f(obj.get_params(2)), h2f(ref.buffer("ema"))
    assert (np.abs(ea[touched] - eb[touched]) > 2e-3 * np.maximum(np.abs(eb[touched]), 1e-2)).mean() < 5e-3
    assert float((np.abs(ea[un] - eb[un]) > _ulp16(eb[un])).mean()) < 1e-4
    i = obj.info(); assert i.train_step == 1 and i.last_n_valid == ref.n_valid
    obj.close(); ds.close(); ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["base", "large"])
def test_every_combination_of_the_equivalence_switches_trains_the_same_parameters(pkg, small_scene, group):
    """The A/B switches of mon_set_option that claim "same parameters either way" are flipped in EVERY combination, not one at a time: level-tile encode or
    gathers, hipGraph replay, zero-gradient samples kept, training lanes (base.json-sized tables); level-tile encode, zero-gradient samples kept, hipGraph
    replay (tables above 8 M parameters, binned scatter; the record / flag / counter switches of rounds 4-5 are variant builds since round 6, checked against
    the oracle instead: tools/gpu_variants_large.sh).  Master weights, fp16 weights and EMA must have one CRC over all combinations of a group."""
    _need_gpu(pkg)
    import itertools, zlib
    if group == "base":
        kw, steps = dict(rays_per_batch=1024), 40
        switches = {"lds_encode": (1, 0), "use_graph": (0, 1), "keep_zero_samples": (0, 1), "train_lanes": (2, 0)}
        fixed = {}
    else:
        kw, steps = dict(rays_per_batch=1024, log2_hashmap_size=20, n_levels=8, per_level_scale=2.0, n_neurons=32, n_hidden_layers=2), 10
        switches = {"lds_encode": (1, 0), "keep_zero_samples": (0, 1), "use_graph": (0, 1)}
        fixed = {"big_switch": 1}                                                   # always binned: no global-atomic arrival order in the comparison
    names = list(switches) + list(fixed)
    old = {n: pkg.get_option(n) for n in names}
    seen = {}
    try:
        for n, v in fixed.items():
            pkg.set_option(n, v)
        for combo in itertools.product(*switches.values()):
            for n, v in zip(switches, combo):
                pkg.set_option(n, v)
            ds, obj = ge.make_problem(pkg, small_scene, kw); obj.set_backend(1)
            if group == "large":
                assert obj.info().n_grid_params > (8 << 20)
            obj.train(steps)
            seen[combo] = tuple(zlib.crc32(obj.get_params(w).tobytes()) for w in (0, 1, 2))
            obj.close(); ds.close()
    finally:
        for n, v in old.items():
            pkg.set_option(n, v)
    assert len(seen) == 2 ** len(switches) and len(set(seen.values())) == 1, {k: v for k, v in seen.items() if v != seen[next(iter(seen))]}


def _level_sizes(cfg):
    """tcnn's level table (grid.h): entries per level = min(round_up(res^3, 8), 2^T), res = ceil(base * scale^l - 1) + 1."""
    sizes = []
    for l in range(cfg.n_levels):
        scale = np.float32(2.0 ** (l * np.log2(cfg.per_level_scale)) * cfg.base_resolution - 1.0)
        res = int(np.ceil(scale)) + 1
        sizes.append(min(((res ** 3 + 7) // 8) * 8, 1 << cfg.log2_hashmap_size))
    return sizes


@pytest.mark.parametrize("kw", [C1, dict(rays_per_batch=256), dict(rays_per_batch=320, n_levels=6, base_resolution=20, per_level_scale=1.235,
        log2_hashmap_size=16),
                                dict(rays_per_batch=8192, n_levels=3, log2_hashmap_size=14)], ids=["c1", "c2net", "dense_parity_levels", "two_chunks"])
def test_level_tile_encode_matches_oracle_and_the_gather_path(pkg, orc, small_scene, kw):
    """The default forward pass of the fused backend: positions by k_sample_points / k_optimizer's position blocks, hash-grid encode by k_encode_tiles from
    LDS-resident level tiles (whole levels and even / odd parity tiles), features loaded by k_fused_train<PRE>.  Positions and encoded features must equal
    the oracle's bit for bit, the tile image must be the tile_slot permutation of the fp16 grid, and training must give the same parameters as the gather
    path."""
    # (the default takes the tile chain from 3072 rays up: below that its fixed costs lose against the gathers)
    pkg.set_option("lds_encode", 2)
    try:
        ds, obj, ref = _pair(pkg, orc, small_scene, kw, 1)
    finally:
        pkg.set_option("lds_encode", 1)
    obj.set_debug_dump(False)
    p = pattern_params(ref); obj.set_params(p); ref.set_params(p)
    L, B = obj.cfg.n_levels, obj.R * obj.S
    Ep = obj.info().encoded_width
    def check_batch():
        x = obj.buffer("x_all").reshape(B, 4); close_f32(x[:, :3], ref.buffer("pts").reshape(B, 3), "positions", 1e-6)
        close_f32(x[:, 3], ref.buffer("tdist"), "distances", 1e-6)
        e = obj.buffer("e_soa").reshape(L, B, 2); want = ref.buffer("E").reshape(B, Ep)[:, :2 * L].reshape(B, L, 2).transpose(1, 0, 2)
        assert np.array_equal(e, want), "level-tile encode must be bit-exact (levels differing: %s)" % sorted(set(np.argwhere(e != want)[:, 0].tolist()))
    obj.train_stages(1 | 2); ref.generate_batch(); ref.forward_backward()          # iteration 0: stand-alone position kernel
    assert int(obj.buffer("state")[2]) == ref.n_valid
    check_batch()
    obj.train_stages(4); ref.train_step()
    # the tile image after an optimizer step: a permutation of the fp16 grid, level by level
    half = obj.buffer("half")[obj.info().n_mlp_params:].reshape(-1, 2); tiles = obj.buffer("half_tiles").reshape(-1, 2)
    off = 0
    for size in _level_sizes(obj.cfg):
        lv = half[off:off + size]
        want = lv if size <= 163840 // 4 else np.concatenate([lv[0::2], lv[1::2]])
        assert np.array_equal(tiles[off:off + size], want), "tile image of the level at entry offset %d" % off
        off += size
    # iteration 1: candidates by k_encode_tiles' level-0 workgroups, positions by k_optimizer's blocks, the oracle restarted from the device's weights
    ref.set_params(obj.get_params(0))                                              # (train_step advanced the oracle's iteration counter)
    obj.train_stages(1 | 2); ref.generate_batch(); ref.forward_backward()
    assert int(obj.buffer("state")[2]) == ref.n_valid
    check_batch()
    obj.train_stages(4)
    crc_pre = obj.get_params(0).tobytes()
    obj.close(); ds.close(); ref.close()
    # the same two steps with the gathers inside k_fused_train
    pkg.set_option("lds_encode", 0)
    try:
        ds, obj = ge.make_problem(pkg, small_scene, kw); obj.set_backend(1); obj.set_params(p)
        obj.train(2)
        assert obj.get_params(0).tobytes() == crc_pre
        obj.close(); ds.close()
    finally:
        pkg.set_option("lds_encode", 1)


def test_level_tile_encode_trains_bit_identically_to_the_gather_path():
    """base.json on the bench scene, 400 steps: the level-tile encode (default), the same under hipGraph replay, and the gathers inside k_fused_train
    (option lds_encode = 0) must leave bit-identical parameters, through the dense and the sparse-gradient regime."""
    import subprocess, sys
    from conftest import ROOT
    def run(extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "param_crc.py"), "3", "150", "250"], capture_output=True, text=True,
                env=dict(os.environ, **extra), timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return [ln.split()[2] for ln in r.stdout.strip().split("\n") if ln.startswith("steps+")]
    a = run({}); b = run({"MON_OPTIONS": "lds_encode=0"}); c = run({"MON_OPTIONS": "use_graph=1"})
    assert a == b == c, (a, b, c)


def test_training_parity_c2_three_seeds_against_the_serial_oracle_fixture(pkg, ss):
    """BASELINE configs[1] (base.json defaults, full batch), 200 steps, THREE sampling seeds, against the oracle run with its SERIAL grid scatter in the build
    container (tests/golden/c2_trained.npz, generator next to it: 13 minutes of CPU): mutual PSNR of every rendered training crop above the chaos floor's bar,
    mean-of-three absolute PSNR within the floor's own spread of the oracle's (tests/test_numerics_study.py::trained_model_bars)."""
    from test_numerics_study import trained_model_bars
    _need_gpu(pkg)
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c2_trained.npz")))
    mutual_floor, abs_tol = trained_model_bars()
    sc = ss.make_scene(n_views=12, H=120, W=160, f=130.0, seed=0)
    steps, every = int(g["steps"]), int(g["every"]); mutual, a_hip, a_ref = [], [], []
    for seed in (int(s) for s in g["seeds"]):
        ds, obj = ge.make_problem(pkg, sc, dict(C2, sample_seed=seed)); obj.set_backend(1)
        loss = obj.train(steps)
        assert np.isfinite(loss) and abs(loss - float(g["loss_s%d" % seed])) < max(float(g["loss_s%d" % seed]), 0.02)
        for i, box in enumerate(sc.objects[0]["boxes"][::every]):
            v, x, y, h, w = (int(q) for q in box)
            rgb, depth, mask = obj.render(box, ss.colmajor(sc.Twc[v]))
            gm = sc.instance[v, y:y + h, x:x + w] > 0; gt = np.where(gm[..., None], sc.rgb[v, y:y + h, x:x + w] / 255.0, 1.0)
            mutual.append(psnr(rgb, g["rgb_s%d_c%d" % (seed, i)])); a_hip.append(psnr(rgb, gt)); a_ref.append(float(g["psnr_s%d" % seed][i]))
            # the hard 0.5 opacity mask agrees on all but silhouette pixels
            assert (mask.astype(bool) != g["mask_s%d_c%d" % (seed, i)].astype(bool)).mean() < 0.02
        obj.close(); ds.close()
    print("C2 x 3 seeds vs serial oracle: mutual PSNR min %.2f mean %.2f dB (bar %.2f), abs HIP %.2f dB, abs oracle %.2f dB (tol %.2f)" % (min(mutual),
            np.mean(mutual), mutual_floor, np.mean(a_hip), np.mean(a_ref), abs_tol))
    assert min(mutual) > mutual_floor
    assert abs(np.mean(a_hip) - np.mean(a_ref)) < abs_tol and np.mean(a_hip) > 24.0


def test_parameter_trajectory_against_both_numeric_models_of_the_oracle(pkg, orc, small_scene):
    """Between the 1 / 3 / 8-step parameter checks and the trained-model PSNR: the parameters after 1, 2, 4, 8, 16, 32 steps (BASELINE configs[0], the default
    fused path) against the oracle under the numeric contract AND under its model of tiny-cuda-nn's fp16 accumulation (tcnn_half_accum).  Measure: the fraction
    of parameters further than 1e-4 (1 % of a learning rate) from the oracle's.  Adam's early steps have magnitude lr whatever the gradient, so a gradient that
    rounds to the other side of zero moves a weight by 2 lr and the trajectories decorrelate from there: the bound is a GROWTH bound (it doubles per doubling
    of the step count from what one step leaves), and the distance to the contract must not exceed the distance to the tcnn-half model -- the implementation
    sits on the contract's side of the reference's own numerics."""
    _need_gpu(pkg)
    kw = dict(C1, sample_seed=31)
    ds, obj = ge.make_problem(pkg, small_scene, kw); obj.set_backend(1)
    ref = ge.make_oracle(orc, small_scene, kw); th = ge.make_oracle(orc, small_scene, dict(kw, tcnn_half_accum=1))
    nm = ref.n_mlp; done = 0; rows = []
    for k in (1, 2, 4, 8, 16, 32):
        obj.train(k - done); ref.train(k - done); th.train(k - done); done = k
        a, b, c = obj.get_params(0), ref.buffer("master"), th.buffer("master")
        far = lambda u, v, s: float((np.abs(u[s] - v[s]) > 1e-4).mean())
        rows.append((k, far(a, b, slice(0, nm)), far(a, b, slice(nm, None)), far(a, c, slice(0, nm)), far(a, c, slice(nm, None)), far(b, c, slice(0, nm)),
                far(b, c, slice(nm, None))))
    for r in rows:
        print("step %2d: HIP vs contract MLP %.4f grid %.4f | HIP vs tcnn-half MLP %.4f grid %.4f | contract vs tcnn-half MLP %.4f grid %.4f" % r)
    for k, m_c, g_c, m_t, g_t, m_ct, g_ct in rows:
        # growth bound: one step leaves < 0.5 % (parity.py), doubling per doubling
        assert m_c <= min(1.0, 5e-3 * 2 * k) and g_c <= min(1.0, 5e-3 * 2 * k), (k, m_c, g_c)
        # never further from the contract than from the tcnn-half model
        assert m_c <= m_t + 0.02 and g_c <= g_t + 0.02, (k, m_c, m_t, g_c, g_t)
    assert np.isfinite(obj.get_params(0)).all()
    obj.close(); ds.close(); ref.close(); th.close()
