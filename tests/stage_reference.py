"""Shared reference of the trained-regime stage tests (a helper module like parity.py and pose_reference.py, not a test file): fp64 NumPy restatements of the
training stages -- MLP layers forward and backward, weight gradient, composite and dL/dO (composite_ray / gradient_ray of oracle/mon_oracle.c, the contract,
not an autograd graph), grid scatter -- each fed the dumped INPUTS of the stage under test, so that errors cannot compound from stage to stage, and each
returning next to the wanted value the sum of absolute terms its error bar is made of.  NumPy only; not imported by the product; reads nothing outside the
repository.  Arrays come in the layout ObjectNeRF.buffer() / OracleModel.buffer() return (fp16 as uint16 bit patterns).

Bars (u = 2^-24, the unit roundoff of fp32; K the inner dimension; A the sum of absolute terms):
  fp16 outputs of a dot product   |got - want| <= 1/2 ulp16(want) + K u A     any fp32 summation order of exact fp16 x fp16 products, then one h()
  dL/dO                           |got - want| <= 1/2 ulp16(want) + k u A     A: the running error bound of composite_and_gradient; k = DLDO_K_ORACLE for
                                                                              the fp32 oracle, 4 x that for the device
  gmlp                            |got - want| <= n u A                       n = samples with a non-zero d
  grid gradient                   |got - want| <= 2^-9 A + count u            one h() per partial table, fp32 final sum, one-ulp flips of h(w dE)
                                  (a running fp16 sum in any order -- tcnn's atomics, backend 0 --: (count + 1) 2^-11 A + count u)"""
import ctypes as C

import numpy as np

U = 2.0 ** -24                                              # fp32 unit roundoff; also the fp16 subnormal spacing
EPS = float(np.float32(1e-4))                               # kTransmittanceEps as the fp32 the kernels compare with
OUT = 4                                                     # real rows of the [16][W] output matrix
# dL/dO: A is a running first-order error bound in units of u, so an evaluation whose every operation (expf included) is good to one fp32 ulp stays within
# k = 1; the fp32 ORACLE measures 0.25 (c2s) and 0.03 (c1) at trained weights (tests/test_stage_reference.py asserts k <= 1).  Composite outputs: the
# oracle's worst error against this module, rounded up.  The device's bars are 4 x these: its wave scans reorder the 32-term products and sums, and
# __expf is not libm's expf.
DLDO_K_ORACLE = 1.0
COMPOSITE_ERR_ORACLE = 3.1e-7


def h2d(a):
    """fp16 bit patterns -> fp64"""
    return np.asarray(a, np.uint16).view(np.float16).astype(np.float64)


def h(x):
    """round to fp16 (subnormals kept), back in fp64"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def ulp16(x):
    """fp16 spacing at |x|: 2^(floor(log2 |x|) - 10) in the normal range, the subnormal spacing 2^-24 below 2^-14; no floor relative to any tensor"""
    return np.maximum(2.0 ** (np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14))) - 10), 2.0 ** -24)


def half_bar(want, slack):
    """1/2 ulp16 + slack, the ulp taken at the larger binade where `want` sits within the slack of a binade edge"""
    return 0.5 * ulp16(np.abs(want) + slack) + slack


def layer_matrices(half, n_mlp, Ep, W, NH):
    """the NH + 1 matrices of the `half` buffer in fp64: [W, Ep], (NH - 1) x [W, W], [16, W] (rows = outputs)"""
    p = h2d(half[:n_mlp]); mats = []; o = 0
    for layer in range(NH + 1):
        rows = 16 if layer == NH else W; cols = Ep if layer == 0 else W
        mats.append(p[o:o + rows * cols].reshape(rows, cols)); o += rows * cols
    assert o == n_mlp
    return mats


# ------------------------------------------------------------------ MLP stages
def mlp_forward_layer(a_in, Wl, relu=True):
    """(max(a_in @ Wl.T, 0) -- without the max for the output layer --, |a_in| @ |Wl|.T)"""
    y = a_in @ Wl.T
    return (np.maximum(y, 0.0) if relu else y), np.abs(a_in) @ np.abs(Wl).T


def mlp_backward_layer(d_out, Wl, relu_mask=None):
    """((d_out @ Wl) * mask, (|d_out| @ |Wl|) * mask); mask = Hid > 0 of the layer below, None for dL/dE"""
    y = d_out @ Wl; A = np.abs(d_out) @ np.abs(Wl)
    if relu_mask is not None:
        y = y * relu_mask; A = A * relu_mask
    return y, A


def weight_gradient(d, a):
    """(d.T @ a, |d|.T @ |a|)"""
    return d.T @ a, np.abs(d).T @ np.abs(a)


# ------------------------------------------------------------------ composite and dL/dO
def composite_and_gradient(O, tdist, bgcol, target, target_depth, ray_flag, R, loss_scale):
    """composite_ray and gradient_ray of oracle/mon_oracle.c for all R rays at once in fp64: the first interval from t = 0, the cut BEFORE a sample once
    T < 1e-4, clamp(raw, +-15) in dsig, the sign rules of dlm and dl_dd, the background rays' 0.01 dsig term and unconditional colour gradient, zeros after
    the cut.  Returns a dict: rgb [R, 3], depth, mask, loss [R]; dO [R, S, 4] (before its h()); A [R, S, 4], the running first-order error bound of the contract's
    fp32 evaluation of each dO in units of u (the absolute terms of every sum and difference, carried through the products); n_act [R] (samples before the cut);
    amb_cut [R] (some T within 1e-3 relative of the cut) and amb_depth [R] (target_depth > 0 and |depth - target_depth| < 1e-5)."""
    v = h2d(O).reshape(R, -1, 4); S = v.shape[1]
    t = np.asarray(tdist, np.float64).reshape(R, S); bg = np.asarray(bgcol, np.float64).reshape(R, 3); tg = np.asarray(target, np.float64).reshape(R, 3)
    td = np.asarray(target_depth, np.float64).reshape(R); obj = np.asarray(ray_flag).reshape(R) != 0
    c = 1.0 / (1.0 + np.exp(-v[..., :3])); cc = c * (1.0 - c)
    dt = t - np.concatenate([np.zeros((R, 1)), t[:, :-1]], 1)
    x = np.exp(v[..., 3]) * dt; om = np.exp(-x); alpha = -np.expm1(-x)       # om = 1 - alpha
    # E_*: running first-order error bounds of the contract's fp32 evaluation, in units of u (every operation adds |its result|, a product x y propagates
    # E_x |y| + |x| E_y, exp() multiplies by its value).  The contract forms alpha = 1 - exp(-sigma dt) and T (1 - alpha): alpha and 1 - alpha carry the
    # ABSOLUTE rounding of exp() -- a small alpha has a large relative error, and behind an alpha close to 1 the new T has that of the old one
    E_c = 3.0 * c; E_cc = E_c + 2.0 * cc
    E_om = om * (3.0 * x + 1.0); E_al = E_om + alpha; E_omc = E_al + om
    T = np.ones(R); E_T = np.zeros(R); act = np.zeros((R, S), bool); alive = np.ones(R, bool); amb_cut = np.zeros(R, bool)
    Tb = np.zeros((R, S)); Ta = np.zeros((R, S)); E_Tb = np.zeros((R, S)); E_Ta = np.zeros((R, S))      # T before / after each composited sample
    for n in range(S):
        amb_cut |= alive & (np.abs(T - EPS) <= 1e-3 * EPS)
        alive = alive & (T >= EPS); act[:, n] = alive
        Tb[:, n] = T; E_Tb[:, n] = E_T
        E_T = np.where(alive, E_T * om[:, n] + T * E_omc[:, n] + T * om[:, n], E_T); T = np.where(alive, T * om[:, n], T)
        Ta[:, n] = T; E_Ta[:, n] = E_T
    w = np.where(act, alpha * Tb, 0.0); E_w = np.where(act, E_al * Tb + alpha * E_Tb + w, 0.0)
    pc = np.cumsum(w[..., None] * c, 1); pd = np.cumsum(w * t, 1)             # prefixes including the sample (r2, d2)
    E_pc = np.cumsum(E_w[..., None] * c + w[..., None] * (E_c + c) + pc, 1); E_pd = np.cumsum(E_w * t + w * t + pd, 1)
    rgb = pc[:, -1] + T[:, None] * bg; depth = pd[:, -1]; mask = 1.0 - T
    E_rgb = E_pc[:, -1] + (E_T + T)[:, None] * bg + rgb; E_depth = E_pd[:, -1]; E_mask = E_T + mask
    e = rgb - tg; g = 2.0 * e; E_g = 2.0 * (E_rgb + np.abs(e))
    dl_dd = np.where(td > 0, 0.5 * np.where(depth - td >= 0, 1.0, -1.0), 0.0)
    loss = (e * e).sum(1) / 3.0 + np.where(obj, dl_dd * (depth - td) + (1.0 - mask), mask)
    ls = loss_scale / R
    dO = np.zeros((R, S, 4)); A = np.zeros((R, S, 4))
    ag = np.abs(g)[:, None, :]; w3 = w[..., None]
    dO[..., :3] = ls * w3 * g[:, None, :] * cc
    A[..., :3] = ls * (E_w[..., None] * ag * cc + w3 * E_g[:, None, :] * cc + w3 * ag * E_cc + 3.0 * w3 * ag * cc)
    dsig = np.exp(np.clip(v[..., 3], -15.0, 15.0))
    suf = rgb[:, None, :] - pc; E_suf = E_rgb[:, None, :] + E_pc + np.abs(suf)
    term = Ta[..., None] * c - suf; E_term = E_Ta[..., None] * c + Ta[..., None] * (E_c + c) + E_suf + np.abs(term)
    dot = (g[:, None, :] * term).sum(2); E_dot = (E_g[:, None, :] * np.abs(term) + ag * E_term + 3.0 * ag * np.abs(term)).sum(2)
    rest = depth[:, None] - pd; inner_d = Ta * t - rest
    dsup = dl_dd[:, None] * inner_d
    E_dsup = np.abs(dl_dd)[:, None] * (E_Ta * t + Ta * t + E_depth[:, None] + E_pd + np.abs(rest) + np.abs(inner_d)) + np.abs(dsup)
    dmask = (1.0 - mask)[:, None]; E_dmask = (E_mask + 1.0 - mask)[:, None]
    dlm = 0.5 * np.where(mask >= 1.0, 1.0, -1.0)[:, None]
    inner = dot + dsup + dlm * dmask; E_inner = E_dot + E_dsup + 0.5 * (E_dmask + dmask) + 2.0 * np.abs(inner)
    dl_obj = dsig * dt * inner; A_obj = dsig * dt * E_inner + 5.0 * np.abs(dl_obj)
    first = dsig * dt * 0.5 * dmask; dl_bg = first + dsig * 0.01; A_bg = dsig * dt * 0.5 * E_dmask + 5.0 * first + 2.0 * dsig * 0.01 + 2.0 * dl_bg
    dO[..., 3] = ls * np.where(obj[:, None], dl_obj, dl_bg); A[..., 3] = ls * np.where(obj[:, None], A_obj, A_bg)
    dO *= act[..., None]; A *= act[..., None]
    amb_depth = (td > 0) & (np.abs(depth - td) < 1e-5)
    return dict(rgb=rgb, depth=depth, mask=mask, loss=loss, dO=dO, A=A, n_act=act.sum(1), act=act, amb_cut=amb_cut, amb_depth=amb_depth, raw=v[..., 3], obj=obj)


# ------------------------------------------------------------------ the hash grid
def level_table(cfg):
    from oracle_binding import lib
    off = np.zeros(17, np.uint32); sc = np.zeros(16, np.float32); res = np.zeros(16, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                # noqa: E731
    lib().orc_level_table(C.byref(cfg), p(off), p(sc), p(res))
    return off, sc, res


def numpy_corners(cfg, x):
    """tcnn's grid walk re-derived in NumPy, independent of the oracle's level_corners: yields (level, corner k, global entry index [n], weight [n] fp64)
    for positions x [n, 3] -- fractional position from the kernel's fp32 `scale * x + 0.5`, everything after that in fp64 / exact integers."""
    L = cfg.n_levels
    off, sc, res = level_table(cfg)
    for l in range(L):
        size = int(off[l + 1] - off[l]); r = int(res[l])
        pos = np.float32(sc[l]) * x.astype(np.float32) + np.float32(0.5)        # fp32 like the kernel; fmaf vs mul+add differ < 1 ulp
        pos = pos.astype(np.float64)
        g = np.floor(pos); fr = pos - g; g = g.astype(np.int64)
        for k in range(8):
            w = np.ones(x.shape[0]); q = []
            for d in range(3):
                if k & (1 << d):
                    w = w * fr[:, d]; q.append(g[:, d] + 1)
                else:
                    w = w * (1 - fr[:, d]); q.append(g[:, d])
            qx, qy, qz = (np.asarray(v, np.uint64) & 0xffffffff for v in q)
            # tcnn grid_index: linear index while the running stride (uint32) fits the table, otherwise the prime hash
            stride, dense = 1, np.zeros(x.shape[0], np.uint64)
            for coord in (qx, qy, qz):
                if stride <= size:
                    dense = (dense + coord * stride) & 0xffffffff; stride = (stride * r) & 0xffffffff
            if size < stride:
                idx = ((qx ^ (qy * 2654435761 & 0xffffffff) ^ (qz * 805459861 & 0xffffffff)) & 0xffffffff) % size
            else:
                idx = dense % size
            yield l, k, idx.astype(np.int64) + int(off[l]), w


def grid_scatter(dE, pts, cfg):
    """tcnn's kernel_grid_backward per entry and feature, [n_entries, 2] each: sum of h(w dE) over the eight corners of every level (fp64 np.add.at of the
    fp16-rounded contributions), sum of |h(w dE)|, and the number of contributions (a sample whose two dE of a level are both zero contributes none).
    dE: fp64 [B, >= 2 L] (the stage's fp16 input), pts: fp32 [B, 3]."""
    off, _, _ = level_table(cfg); n_ent = int(off[cfg.n_levels])
    want = np.zeros((n_ent, 2)); A = np.zeros((n_ent, 2)); cnt = np.zeros((n_ent, 2))
    rows = np.flatnonzero((dE[:, :2 * cfg.n_levels] != 0).any(1)); x = np.asarray(pts, np.float32).reshape(-1, 3)[rows]; d = dE[rows]
    for l, _, idx, w in numpy_corners(cfg, x):
        nz = (d[:, 2 * l] != 0) | (d[:, 2 * l + 1] != 0)
        for f in range(2):
            c = h(w[nz] * d[nz, 2 * l + f])
            np.add.at(want[:, f], idx[nz], c); np.add.at(A[:, f], idx[nz], np.abs(c)); np.add.at(cnt[:, f], idx[nz], 1)
    return want, A, cnt


# ------------------------------------------------------------------ the stage comparisons (the CPU test runs them on the oracle, the GPU tests on the device)
def err_report(got, want, slack):
    """figures of an fp16 stage: exact-match share against h(want), share within one ulp, worst error in ulps, elements outside half_bar(want, slack)"""
    hw = h(want); err = np.abs(got - want); ul = ulp16(want)
    return dict(exact=float((got == hw).mean()), within1=float((np.abs(got - hw) <= ul).mean()), worst_ulp=float((np.abs(got - hw) / ul).max()),
                n_bad=int((err > half_bar(want, slack)).sum()), worst_err=float(err.max()))


def mlp_stages(bufs, n_mlp, Ep, W, NH, L):
    """Every forward and backward layer and the weight gradient of one dumped forward/backward against the restatement, each stage fed the dump's own
    inputs.  bufs: dict of half, E, Hid, O, dO, dHid, dE, gmlp.  Returns {stage: figures}; figures carry n_bad (elements outside the bar), the extras
    of the zero and subnormal rows, and for gmlp the pad rows."""
    mats = layer_matrices(bufs["half"], n_mlp, Ep, W, NH)
    B = bufs["O"].size // 4
    E = h2d(bufs["E"]).reshape(B, Ep); Hid = h2d(bufs["Hid"]).reshape(B, NH, W); O = h2d(bufs["O"]).reshape(B, 4)
    dO = h2d(bufs["dO"]).reshape(B, 4); dH = h2d(bufs["dHid"]).reshape(B, NH, W); dE = h2d(bufs["dE"]).reshape(B, Ep)[:, :2 * L]
    out = {}
    for l in range(NH):
        a_in = E if l == 0 else Hid[:, l - 1]
        want, A = mlp_forward_layer(a_in, mats[l]); K = a_in.shape[1]
        out["Hid%d" % l] = dict(err_report(Hid[:, l], want, K * U * A), k=_k_of(Hid[:, l], want, A))
    want, A = mlp_forward_layer(Hid[:, NH - 1], mats[NH][:OUT], relu=False)
    out["O"] = dict(err_report(O, want, W * U * A), k=_k_of(O, want, A))
    zero = ~(dO != 0).any(1)                                                     # samples whose dL/dO is all zero
    sub = ~zero & (np.abs(dO) < 2.0 ** -14).all(1)                              # non-zero and all subnormal
    for l in range(NH - 1, -1, -1):
        d_out = dO if l == NH - 1 else dH[:, l + 1]; Wl = mats[NH][:OUT] if l == NH - 1 else mats[l + 1]
        want, A = mlp_backward_layer(d_out, Wl, (Hid[:, l] > 0).astype(np.float64)); K = d_out.shape[1]
        out["dHid%d" % l] = dict(err_report(dH[:, l], want, K * U * A), k=_k_of(dH[:, l], want, A), zero_rows_exact=bool(not dH[zero, l].any()),
                                 wanted_nonzero_subnormal=float(_sub_share(want)))
    want, A = mlp_backward_layer(dH[:, 0], mats[0][:, :2 * L])
    nzs = h(want[sub]) != 0
    out["dE"] = dict(err_report(dE, want, W * U * A), k=_k_of(dE, want, A), zero_rows_exact=bool(not dE[zero].any()),
                     wanted_nonzero_subnormal=float(_sub_share(want)), sub_rows=int(sub.sum()), sub_wanted_nonzero=int(nzs.sum()),
                     sub_got_nonzero=int((dE[sub][nzs] != 0).sum()), zero_rows=int(zero.sum()))
    # weight gradients: layer 0 from E, hidden layers from the activation below, the output matrix from dL/dO (rows 4..15: no gradient)
    gm = np.asarray(bufs["gmlp"], np.float64); o = 0; n_bad = 0; worst = 0.0; pad_zero = True
    for l in range(NH + 1):
        rows = 16 if l == NH else W; cols = Ep if l == 0 else W
        got = gm[o:o + rows * cols].reshape(rows, cols); o += rows * cols
        d = dO if l == NH else dH[:, l]; a = E if l == 0 else Hid[:, l - 1]
        want, A = weight_gradient(d, a); n = int((d != 0).any(1).sum())
        if l == NH:
            pad_zero = bool(not got[OUT:].any()); got = got[:OUT]
        err = np.abs(got - want); bar = n * U * A
        n_bad += int((err > bar).sum()); worst = max(worst, float((err / np.maximum(U * A, 1e-300))[A > 0].max()) if (A > 0).any() else 0.0)
        n_bad += int((got[A == 0] != 0).sum())
    out["gmlp"] = dict(n_bad=n_bad, worst_over_uA=worst, pad_rows_zero=pad_zero, n=n)
    return out


def _k_of(got, want, A):
    """worst (|got - want| - 1/2 ulp16(want)) / (u A) over the elements with A > 0 (an element with A = 0 must be an exact zero: reported as inf)"""
    ex = np.abs(got - want) - 0.5 * ulp16(want)
    if ((A == 0) & (got != 0)).any():
        return float("inf")
    m = A > 0
    return float(max(0.0, (ex[m] / (U * A[m])).max())) if m.any() else 0.0


def _sub_share(want):
    hw = h(want)
    return ((hw != 0) & (np.abs(hw) < 2.0 ** -14)).mean()


def regime(cg, dE_sub_share):
    """the regime figures of one batch from the reference's wanted values: share of samples with all-zero wanted dL/dO, share of object rays ended by the
    cut, samples whose non-zero wanted dL/dO is all subnormal, share of non-zero subnormals among the wanted dL/dE, largest raw density"""
    hw = h(cg["dO"]); zero = ~(hw != 0).any(2); sub = ~zero & (np.abs(hw) < 2.0 ** -14).all(2)
    S = hw.shape[1]
    return dict(zero_share=float(zero.mean()), cut_share=float((cg["n_act"][cg["obj"]] < S).mean()) if cg["obj"].any() else 0.0, sub_rows=int(sub.sum()),
                dE_sub_share=float(dE_sub_share), raw_max=float(cg["raw"].max()), raw_min=float(cg["raw"].min()))


def composite_stages(bufs, R, loss_scale, k_bar):
    """rgb / mask / depth / loss per ray and dL/dO of one dumped forward/backward against composite_and_gradient of the dump's own O and ray inputs.
    Returns (figures, cg): worst absolute error of the four ray outputs over the unambiguous rays, and for dL/dO the elements outside
    1/2 ulp16 + k_bar u A, the measured k, the exact-match shares, the samples whose zero pattern differs and the ambiguous-ray share."""
    cg = composite_and_gradient(bufs["O"], bufs["tdist"], bufs["bgcol"], bufs["target"], bufs["target_depth"], bufs["ray_flag"], R, loss_scale)
    ok = ~(cg["amb_cut"] | cg["amb_depth"])
    f = dict(ambiguous=float((~ok).mean()), amb_cut=int(cg["amb_cut"].sum()), amb_depth=int(cg["amb_depth"].sum()))
    for name, got in (("rgb", np.asarray(bufs["rgb_ray"], np.float64).reshape(R, 3)), ("mask", bufs["mask_ray"]), ("depth", bufs["depth_ray"]),
                      ("loss", bufs["loss_ray"])):
        f[name] = float(np.abs(np.asarray(got, np.float64) - cg[name])[ok].max())
    got = h2d(bufs["dO"]).reshape(cg["dO"].shape)[ok]; want = cg["dO"][ok]; A = cg["A"][ok]
    f["dO"] = dict(err_report(got, want, k_bar * U * A), k=_k_of(got, want, A),
                   zero_pattern_diff=int(((got != 0).any(2) != (h(want) != 0).any(2)).sum()), after_cut_nonzero=int((got[~cg["act"][ok]] != 0).sum()))
    return f, cg


REGIME_BARS = dict(zero_share=0.50, cut_share=0.25, sub_rows=200, dE_sub_share=0.01, raw_max=6.0)
