"""Shared reference of the camera-refinement tests (a helper module like pose_reference.py, not a test file): a numpy restatement of k_scene_pose_rays and
the objects' sample placement for K objects under a candidate camera pose, an fp64 numpy restatement of the merged composite's loss and its backward
(k_scene_composite_grad), and one fp64 torch autograd graph of the whole objective of include/mon_core.h (mon_scene_pose_loss), run in a child process
(`python tests/scene_pose_reference.py IN.npz OUT.npz`) as pose_reference.reference does: torch and the HIP library do not share a process."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import pose_reference as pref                               # noqa: E402
from pose_reference import EPS, ROOT, huber                 # noqa: E402,F401


# ------------------------------------------------------------------ rays and sample placement
def scene_rays(sc, boxes, Twc, objects, n_rays=0, seed=1, iteration=0, use_depth=True):
    """k_scene_pose_rays and the objects' sample placement in numpy.  boxes: [(FrameId, x, y, h, w)] of one frame; Twc: the candidate pose (4 x 4);
    objects: dicts of Tow (4 x 4), aabb (2 x 3), cls, sample_seed.  Pixels and jitter as pose_reference.pose_rays (n_rays = 0: every pixel, object j's own
    render jitter; else the draws of (seed, iteration), one jitter for every object).  Returns per-ray x, y, dn, uc [P, 3] (unit camera ray), cstar [P, 3],
    inst [P], dstar [P], and per object a dict of hit, t0, t1, t [P, 64], x_o [P, 64, 3], mstar [P]."""
    boxes = np.asarray(boxes, np.int64).reshape(-1, 5)
    assert (boxes[:, 0] == boxes[0, 0]).all()
    area = boxes[:, 3] * boxes[:, 4]
    prefix = np.concatenate([[0], np.cumsum(area)]).astype(np.int64); total = int(prefix[-1])
    n = n_rays if n_rays else total
    i = np.arange(n, dtype=np.int64)
    p = pref.draw(seed, iteration, n, total).astype(np.int64) if n_rays else i
    b = np.searchsorted(prefix, p, side="right") - 1
    q = p - prefix[b]
    x = boxes[b, 1] + q % boxes[b, 4]; y = boxes[b, 2] + q // boxes[b, 4]
    v = int(boxes[0, 0]); f32 = np.float32
    K4 = np.array([sc.fx, sc.fy, sc.cx, sc.cy])
    fx, fy, cx, cy = (f32(u) for u in K4)
    dc = np.stack([(x.astype(f32) - cx) / fx, (y.astype(f32) - cy) / fy, np.ones(n, f32)], -1)
    nn = np.sqrt((dc * dc).sum(-1, dtype=f32)).astype(f32)
    out = dict(i=i, x=x, y=y, dn=nn, uc=(dc / nn[:, None]).astype(f32), cstar=sc.rgb[v, y, x].astype(f32) / f32(255.0), inst=sc.instance[v, y, x].astype(np.int64),
               dstar=(sc.depth[v, y, x].astype(np.float64) if use_depth else np.zeros(n)), objs=[])
    k = np.arange(64, dtype=np.uint64)[None, :]
    for ob in objects:
        o, d, _ = pref.camera_rays(K4, np.asarray(Twc, np.float64), np.asarray(ob["Tow"], np.float64), x, y)
        hit, t0, t1 = pref.slab(np.asarray(ob["aabb"], f32), o, d)
        if n_rays:
            u = pref.rand01(seed, pref.STREAM_POSE, iteration, i.astype(np.uint64)[:, None] * np.uint64(64) + k)
        else:
            u = pref.rand01(ob["sample_seed"], pref.STREAM_RENDER, 0, q.astype(np.uint64)[:, None] * np.uint64(64) + k)
        dtr = (t1 - t0) / f32(64.0)
        t = (dtr[:, None] * (np.arange(64, dtype=f32)[None, :] + u) + t0[:, None]).astype(f32)
        pos = (t[..., None] * d[:, None, :] + o[:, None, :]).astype(f32)
        out["objs"].append(dict(hit=hit, t0=t0, t1=t1, t=t, x_o=pos, mstar=(out["inst"] == ob["cls"]).astype(np.float64)))
    return out


# ------------------------------------------------------------------ the merged composite, its loss and its backward (fp64 numpy)
def np_composite_grad(t, alpha, rgb, count, cstar, mstar, dstar, dn, w, amb_u=0.0):
    """Lists [K, P, 64] (rgb [K, P, 64, 3]) with count [K, P], merged by (t, list, slot) and composited front to back with the cut at the first T < EPS;
    targets cstar [P, 3], mstar [K, P], dstar [P], dn [P]; w = (w_rgb, w_mask, w_depth, huber).  Returns dict of l [P], W [K, P], D [P], dalpha [K, P, 64]
    (dL/dalpha of each list slot, the cut held), dc [K, P, 64, 3], amb [P] (the stopping point within 0.1 % of EPS, as np_composite flags it), ncut [P]
    (merged samples in front of the cut) and ntot [P].  amb_u > 0 (the unit roundoff of the arithmetic under test) widens amb's window for long
    sequences as np_composite's does: max(1e-3, 4 (i + 1) amb_u) at merged sample i."""
    w_rgb, w_mask, w_depth, hub = (float(v) for v in w)
    K, P = count.shape; N = K * 64
    slot = np.arange(64)
    valid = slot[None, None, :] < count[..., None]
    tt = np.where(valid, t, np.inf).transpose(1, 0, 2).reshape(P, N).astype(np.float64)
    aa = np.where(valid, alpha, 0.0).transpose(1, 0, 2).reshape(P, N).astype(np.float64)
    cc = np.where(valid[..., None], rgb, 0.0).transpose(1, 0, 2, 3).reshape(P, N, 3).astype(np.float64)
    kk = np.broadcast_to(np.arange(K)[:, None, None], (K, P, 64)).transpose(1, 0, 2).reshape(P, N)
    ii = np.broadcast_to(slot, (P, K, 64)).reshape(P, N)
    order = np.lexsort((ii, kk, tt), axis=-1)
    tt, aa, kk, ii = (np.take_along_axis(v, order, 1) for v in (tt, aa, kk, ii))
    cc = np.take_along_axis(cc, order[..., None], 1)
    tz = np.where(np.isfinite(tt), tt, 0.0)
    incl = np.cumprod(1.0 - aa, axis=1)
    T = np.concatenate([np.ones((P, 1)), incl[:, :-1]], 1)
    active = np.logical_and.accumulate(T >= EPS, axis=1)
    wgt = np.where(active, aa * T, 0.0)
    cs = np.asarray(cstar, np.float64); ms = np.asarray(mstar, np.float64); ds = np.asarray(dstar, np.float64); dnn = np.asarray(dn, np.float64)
    r = (wgt[..., None] * (cc - cs[:, None, :])).sum(1)
    W = np.stack([(wgt * (kk == k)).sum(1) for k in range(K)], 0)
    D = (wgt * tz).sum(1) / dnn
    M = ms.max(0)
    dep_on = (w_depth != 0) & (M != 0) & (ds > 0)
    l = w_rgb * M * (r * r).sum(1) / 3 + w_mask * ((W - ms) ** 2).sum(0) + np.where(dep_on, w_depth * huber(D - ds, hub), 0.0)
    G = w_rgb * M[:, None] * 2.0 * r / 3.0
    GD = np.where(dep_on, w_depth * np.clip(D - ds, -hub, hub) / dnn, 0.0)
    qm = 2.0 * w_mask * (W - ms)                                            # [K, P]
    q = (G[:, None, :] * (cc - cs[:, None, :])).sum(-1) + GD[:, None] * tz + np.take_along_axis(qm.T, kk, 1)
    wq = wgt * q
    sfx = np.concatenate([np.cumsum(wq[:, ::-1], 1)[:, ::-1][:, 1:], np.zeros((P, 1))], 1)      # sum over n > i
    om = 1.0 - aa
    with np.errstate(divide="ignore", invalid="ignore"):
        dal = np.where(active, T * q - np.where(om > 0, sfx / np.where(om > 0, om, 1.0), 0.0), 0.0)
    dcm = wgt[..., None] * G[:, None, :]
    dalpha = np.zeros((P, K, 64)); dc = np.zeros((P, K, 64, 3))
    fin = np.isfinite(tt)
    pi = np.broadcast_to(np.arange(P)[:, None], (P, N))
    dalpha[pi[fin], kk[fin], ii[fin]] = dal[fin]; dc[pi[fin], kk[fin], ii[fin]] = dcm[fin]
    win = np.maximum(1e-3, 4.0 * amb_u * (np.arange(N) + 1.0))
    amb = (np.abs(T / EPS - 1.0) < win).any(1) | (np.abs(incl / EPS - 1.0) < win).any(1)
    return dict(l=l, W=W, D=D, dalpha=dalpha.transpose(1, 0, 2), dc=dc.transpose(1, 0, 2, 3), amb=amb, ncut=(active & fin).sum(1), ntot=fin.sum(1),
                order_k=kk, order_fin=fin, active=active)


def np_composite_grad_seq32(t, alpha, rgb, count, cstar, mstar, dstar, dn, w):
    """The fp32 sequential twin of np_composite_grad: the same merged order and the same formulas with every product and sum taken front to back in
    float32 (np.cumprod / np.cumsum with dtype=float32; the suffix sums back to front).  Its distance from np_composite_grad is the rounding error of one
    plain fp32 evaluation of these lists: the yardstick for a kernel that reorders the sums.  Returns l, W, D, dalpha, dc as np_composite_grad does."""
    f32 = np.float32
    w_rgb, w_mask, w_depth, hub = (f32(v) for v in w)
    K, P = count.shape; N = K * 64
    slot = np.arange(64)
    valid = slot[None, None, :] < count[..., None]
    tt = np.where(valid, t, np.inf).transpose(1, 0, 2).reshape(P, N).astype(f32)
    aa = np.where(valid, alpha, 0.0).transpose(1, 0, 2).reshape(P, N).astype(f32)
    cc = np.where(valid[..., None], rgb, 0.0).transpose(1, 0, 2, 3).reshape(P, N, 3).astype(f32)
    kk = np.broadcast_to(np.arange(K)[:, None, None], (K, P, 64)).transpose(1, 0, 2).reshape(P, N)
    ii = np.broadcast_to(slot, (P, K, 64)).reshape(P, N)
    order = np.lexsort((ii, kk, tt), axis=-1)
    tt, aa, kk, ii = (np.take_along_axis(v, order, 1) for v in (tt, aa, kk, ii))
    cc = np.take_along_axis(cc, order[..., None], 1)
    fin = np.isfinite(tt); tz = np.where(fin, tt, f32(0))
    om = f32(1) - aa
    incl = np.cumprod(om, axis=1, dtype=f32)
    T = np.concatenate([np.ones((P, 1), f32), incl[:, :-1]], 1)
    active = np.logical_and.accumulate(T >= f32(EPS), axis=1)
    wgt = np.where(active, aa * T, f32(0))
    cs = np.asarray(cstar, f32); ms = np.asarray(mstar, f32); ds = np.asarray(dstar, f32); dnn = np.asarray(dn, f32)
    last = lambda v: np.cumsum(v, axis=1, dtype=f32)[:, -1]                               # noqa: E731
    r = np.stack([last(wgt * (cc[..., c] - cs[:, None, c])) for c in range(3)], 1)
    pi = np.broadcast_to(np.arange(P)[:, None], (P, N))
    wl = np.zeros((P, K, 64), f32); wl[pi[fin], kk[fin], ii[fin]] = wgt[fin]               # (a list's samples keep their slot order in the merged one)
    W = np.cumsum(wl, axis=2, dtype=f32)[..., -1].T
    D = last(wgt * tz) / dnn
    M = ms.max(0)
    dep_on = (w_depth != 0) & (M != 0) & (ds > 0)
    lmask = np.cumsum((W - ms) ** 2, axis=0, dtype=f32)[-1]
    l = w_rgb * M * last(r * r) / f32(3) + w_mask * lmask + np.where(dep_on, w_depth * huber(D - ds, hub).astype(f32), f32(0))
    G = w_rgb * M[:, None] * f32(2) * r / f32(3)
    GD = np.where(dep_on, w_depth * np.clip(D - ds, -hub, hub) / dnn, f32(0)).astype(f32)
    qm = f32(2) * w_mask * (W - ms)
    q = np.cumsum(G[:, None, :] * (cc - cs[:, None, :]), axis=2, dtype=f32)[..., -1] + GD[:, None] * tz + np.take_along_axis(qm.T, kk, 1)
    wq = wgt * q
    sfx = np.concatenate([np.cumsum(wq[:, ::-1], 1, dtype=f32)[:, ::-1][:, 1:], np.zeros((P, 1), f32)], 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        dal = np.where(active, T * q - np.where(om > 0, sfx / np.where(om > 0, om, f32(1)), f32(0)), f32(0))
    dcm = wgt[..., None] * G[:, None, :]
    dalpha = np.zeros((P, K, 64), f32); dc = np.zeros((P, K, 64, 3), f32)
    dalpha[pi[fin], kk[fin], ii[fin]] = dal[fin]; dc[pi[fin], kk[fin], ii[fin]] = dcm[fin]
    assert all(v.dtype == f32 for v in (l, W, D, dal, dcm)), [v.dtype for v in (l, W, D, dal, dcm)]
    return dict(l=l, W=W, D=D, dalpha=dalpha.transpose(1, 0, 2), dc=dc.transpose(1, 0, 2, 3))


def lists_from_raw(raw, t, hit):
    """one object's lists from its dumped raw outputs [P, 64, 4] and distances (fp64): alpha, colour and count (own cut: tile 1 only if T after tile 0 >= EPS)"""
    raw = raw.astype(np.float64); t = t.astype(np.float64); P = t.shape[0]
    sigma = np.exp(raw[..., 3]); col = 1.0 / (1.0 + np.exp(-raw[..., :3]))
    dt = t - np.concatenate([np.zeros((P, 1)), t[:, :-1]], 1)
    alpha = np.where(hit[:, None], 1.0 - np.exp(-sigma * dt), 0.0)
    T32 = np.cumprod(1.0 - alpha[:, :32], 1)[:, -1]
    count = np.where(hit, np.where(T32 >= EPS, 64, 32), 0).astype(np.uint32)
    return alpha, col, count


# ------------------------------------------------------------------ the fp64 autograd graph of the whole chain
def reference(tmp_path, nets, cases, w, tag="sref"):
    """Runs the fp64 graph in a child process.  nets: per object pose_reference.net_inputs(...) plus aabb (2 x 3) and Toc (4 x 4, = Tow Twc of the case's
    pose; per case in cases[c]["Toc"][j]).  cases: dicts of x_o [K, P, 64, 3] (the device's own fp32 object-frame positions), x_c [K, P, 64, 3], t [K, P, 64],
    count [K, P] (the device's evaluated tiles), dn [P], cstar [P, 3], mstar [K, P], dstar [P], Toc [K, 4, 4], optionally lw [Lmax].
    Returns per case: loss, g6 (camera frame, of the mean), l [P], gs [K, P, 64, 3] (dL/dx_o of the SUM over rays), W [K, P], D [P], amb [P]."""
    data = dict(n_objs=len(nets), n_cases=len(cases), w=np.asarray(w, np.float64))
    for j, net in enumerate(nets):
        for key, val in net.items():
            data["net%d_%s" % (j, key)] = val
    for c, cs in enumerate(cases):
        for key, val in cs.items():
            if val is not None:
                data["c%d_%s" % (c, key)] = val
    inp, outp = os.path.join(str(tmp_path), tag + "_in.npz"), os.path.join(str(tmp_path), tag + "_out.npz")
    np.savez(inp, **data)
    r = subprocess.run([sys.executable, os.path.join(HERE, "scene_pose_reference.py"), inp, outp], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    z = np.load(outp)
    return [dict(loss=float(z["loss%d" % c]), g6=z["g6_%d" % c], l=z["l%d" % c], gs=z["gs%d" % c], W=z["W%d" % c], D=z["D%d" % c], amb=z["amb%d" % c] > 0)
            for c in range(len(cases))]


def _torch_child(inp, outp):
    import torch
    z = np.load(inp)
    K = int(z["n_objs"]); w_rgb, w_mask, w_depth, hub = (float(v) for v in z["w"])
    h16 = lambda v: v + (v.detach().to(torch.float16).to(torch.float64) - v.detach())     # noqa: E731
    f64 = torch.float64
    nets = []
    for j in range(K):
        g = lambda key: z["net%d_%s" % (j, key)]                                          # noqa: E731
        L, W, NH, Ep, nm = int(g("L")), int(g("W")), int(g("NH")), int(g("Ep")), int(g("n_mlp"))
        prm = g("params").view(np.float16).astype(np.float64)
        mats = []; o = 0
        for layer in range(NH + 1):
            rows = 16 if layer == NH else W; cols = Ep if layer == 0 else W
            mats.append(torch.tensor(prm[o:o + rows * cols].reshape(rows, cols))); o += rows * cols
        nets.append(dict(L=L, W=W, NH=NH, Ep=Ep, table=torch.tensor(prm[nm:].reshape(-1, 2)), mats=mats, off=g("off"), scl=g("scl"), res=g("res"),
                         aabb=g("aabb")))
    out = {}
    for c in range(int(z["n_cases"])):
        g = lambda key: z["c%d_%s" % (c, key)]                                            # noqa: E731
        x_o, x_c, t, count = g("x_o"), g("x_c"), g("t").astype(np.float64), g("count").astype(np.int64)
        P = t.shape[1]; N = K * 64
        lwc = g("lw").astype(np.float64) if ("c%d_lw" % c) in z.files else None
        leaves, alphas, cols = [], [], []
        for j, net in enumerate(nets):
            L, Ep, NH = net["L"], net["Ep"], net["NH"]; aabb = net["aabb"]; ext = (aabb[1] - aabb[0]).astype(np.float32)
            lw = np.ones(L) if lwc is None else lwc[:L]
            xg = x_o[j].reshape(-1, 3).astype(np.float32)
            xl = torch.tensor(xg.astype(np.float64), requires_grad=True); leaves.append(xl)
            xn = (xl - torch.tensor(aabb[0].astype(np.float64))) / torch.tensor(ext.astype(np.float64)); dxn = xn - xn.detach()
            xn32 = ((xg - aabb[0]) / ext).astype(np.float32)
            feats = [torch.zeros(P * 64, 2, dtype=f64) for _ in range(L)]
            for l, k, idx, frac in pref.corners(net["off"], net["scl"], net["res"], L, xn32):
                fr = torch.tensor(frac) + float(net["scl"][l]) * (lw[l] * dxn)
                wk = torch.ones(P * 64, dtype=f64)
                for d in range(3):
                    wk = wk * (fr[:, d] if (k >> d) & 1 else 1 - fr[:, d])
                feats[l] = feats[l] + wk[:, None] * net["table"][torch.tensor(idx)]
            a = h16(torch.cat(feats + [torch.zeros(P * 64, Ep - 2 * L, dtype=f64)], 1))
            for layer in range(NH):
                a = h16(torch.relu(a @ net["mats"][layer].T))
            raw = h16((a @ net["mats"][NH].T)[:, :4]).reshape(P, 64, 4)
            tj = torch.tensor(t[j]); dt = tj - torch.cat([torch.zeros(P, 1, dtype=f64), tj[:, :-1]], 1)
            ev = torch.tensor(np.arange(64)[None, :] < count[j][:, None])                  # the device's evaluated tiles (its own cut, held)
            zero = torch.zeros_like(dt)
            sigma = torch.exp(torch.where(ev, raw[..., 3], zero))
            alphas.append(torch.where(ev, 1 - torch.exp(-sigma * torch.where(ev, dt, zero)), zero)); cols.append(torch.sigmoid(raw[..., :3]))
        valid = (np.arange(64)[None, None, :] < count[..., None])
        tt = np.where(valid, t, np.inf).transpose(1, 0, 2).reshape(P, N)
        kk = np.broadcast_to(np.arange(K)[:, None, None], (K, P, 64)).transpose(1, 0, 2).reshape(P, N)
        ii = np.broadcast_to(np.arange(64), (P, K, 64)).reshape(P, N)
        order = np.lexsort((ii, kk, tt), axis=-1); ot = torch.tensor(order)
        tt = np.take_along_axis(tt, order, 1); kk = np.take_along_axis(kk, order, 1); fin = np.isfinite(tt)
        aa = torch.gather(torch.stack(alphas, 1).reshape(P, N), 1, ot)
        cc = torch.gather(torch.stack(cols, 1).reshape(P, N, 3), 1, ot[..., None].expand(P, N, 3))
        tz = torch.tensor(np.where(fin, tt, 0.0))
        with torch.no_grad():
            incl = torch.cumprod(1 - aa, 1); T0 = torch.cat([torch.ones(P, 1, dtype=f64), incl[:, :-1]], 1)
            act = torch.tensor(np.logical_and.accumulate((T0 >= EPS).numpy(), axis=1)) & torch.tensor(fin)
            amb = ((T0 / EPS - 1).abs() < 1e-3).any(1) | ((incl / EPS - 1).abs() < 1e-3).any(1)
        a2 = torch.where(act, aa, torch.zeros_like(aa))
        T2 = torch.cumprod(torch.cat([torch.ones(P, 1, dtype=f64), 1 - a2[:, :-1]], 1), 1)
        wgt = a2 * T2
        cs = torch.tensor(g("cstar").astype(np.float64)); ms = torch.tensor(g("mstar").astype(np.float64)); dd = torch.tensor(g("dstar").astype(np.float64))
        dn = torch.tensor(g("dn").astype(np.float64))
        r = (wgt[..., None] * (cc - cs[:, None, :])).sum(1)
        Wj = torch.stack([(wgt * torch.tensor(kk == k)).sum(1) for k in range(K)], 0)
        D = (wgt * tz).sum(1) / dn
        M = ms.max(0).values
        err = D - dd; ae = err.abs()
        hub_v = torch.where(ae <= hub, 0.5 * err * err, hub * (ae - 0.5 * hub))
        l = w_rgb * M * (r * r).sum(1) / 3 + w_mask * ((Wj - ms) ** 2).sum(0) + w_depth * M * (dd > 0).double() * hub_v
        l.sum().backward()
        Toc = g("Toc").astype(np.float64)
        g6 = np.zeros(6); gs = []
        for j in range(K):
            go = leaves[j].grad.numpy().reshape(-1, 3); gs.append(go.reshape(P, 64, 3))
            gc = go @ Toc[j][:3, :3]                                                      # R^T g_o, row-wise
            xc = x_c[j].reshape(-1, 3).astype(np.float64)
            g6 += np.concatenate([gc.sum(0), np.cross(xc, gc).sum(0)]) / P
        out["g6_%d" % c] = g6; out["gs%d" % c] = np.stack(gs); out["l%d" % c] = l.detach().numpy(); out["loss%d" % c] = float(l.detach().mean())
        out["W%d" % c] = Wj.detach().numpy(); out["D%d" % c] = D.detach().numpy(); out["amb%d" % c] = amb.numpy().astype(np.uint8)
    np.savez(outp, **out)


if __name__ == "__main__":
    _torch_child(sys.argv[1], sys.argv[2])
