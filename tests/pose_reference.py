"""Shared reference of the pose-refinement tests (a helper module like parity.py, not a test file): a numpy restatement of k_pose_rays in both modes (the
pixel, box, ray, slab, targets and jittered sample distances of every drawn ray) and one fp64 torch autograd graph of the objective of include/mon_core.h
for any subset of rays, any fused shape (encoder width 16 / 32, 32 / 64 / 128 neurons, 1 / 2 hidden layers, 1-16 levels), optional level weights and a
dataset with or without depth.  The graph runs in a child process (`python tests/pose_reference.py IN.npz OUT.npz`): torch and the HIP library do not share
a process."""
import os
import subprocess
import sys

import numpy as np

EPS = 1e-4                                                  # kTransmittanceEps
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STREAM_RENDER, STREAM_POSE, STREAM_POSE_XY = 3, 4, 5       # device_common.h / model.h
MAX_UNION = 1 << 28                                         # pixels the boxes may hold together (kPoseMaxRays * 64)


# ------------------------------------------------------------------ the counter RNG
def rand_mix(seed, stream, step, idx):
    """device_common.h rand_mix (the 64-bit mix of the key) in numpy uint64 arithmetic"""
    idx = np.asarray(idx, np.uint64)
    ctr = (np.uint64(stream) << np.uint64(60)) | (np.uint64(step) << np.uint64(28)) | (idx & np.uint64(0x0fffffff))
    with np.errstate(over="ignore"):
        z = ctr + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        z = z ^ (z >> np.uint64(30)); z = z * np.uint64(0xBF58476D1CE4E5B9)
        z = z ^ (z >> np.uint64(27)); z = z * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z


def rand01(seed, stream, step, idx):
    """device_common.h rand01: the mix's top 24 bits / 2^24"""
    return (rand_mix(seed, stream, step, idx) >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def draw(seed, iteration, n, total):
    """k_pose_rays' pixel of drawn rays 0..n-1 over a union of `total` pixels: ((z >> 40) total) >> 24 up to 2^24 pixels, ((z >> 32) total) >> 32 above"""
    z = rand_mix(seed, STREAM_POSE_XY, iteration, np.arange(n, dtype=np.uint64))
    if total <= 1 << 24:
        return ((z >> np.uint64(40)) * np.uint64(total)) >> np.uint64(24)
    return ((z >> np.uint64(32)) * np.uint64(total)) >> np.uint64(32)


def draw24(seed, iteration, n, total):
    """the draw before the fix: 24 bits at every total"""
    z = rand_mix(seed, STREAM_POSE_XY, iteration, np.arange(n, dtype=np.uint64))
    return ((z >> np.uint64(40)) * np.uint64(total)) >> np.uint64(24)


def reachable24(p, total):
    """whether pixel p is the 24-bit draw of some u in [0, 2^24): the smallest u with (u total) >> 24 >= p is ceil(p 2^24 / total)"""
    p = np.asarray(p, np.uint64); T = np.uint64(total)
    u = ((p << np.uint64(24)) + T - np.uint64(1)) // T
    return (u < np.uint64(1 << 24)) & (((u * T) >> np.uint64(24)) == p)


# ------------------------------------------------------------------ the hash grid
def level_table(orc, cfg):
    import ctypes as C
    off = np.zeros(17, np.uint32); sc = np.zeros(16, np.float32); res = np.zeros(16, np.uint32)
    orc.lib().orc_level_table(C.byref(cfg), off.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p))
    return off, sc, res


def corners(off, scl, res, L, x):
    for l in range(L):
        size = int(off[l + 1] - off[l]); r = int(res[l])
        pos = (np.float64(scl[l]) * x.astype(np.float64) + 0.5).astype(np.float32).astype(np.float64)       # fmaf: the product is exact in fp64
        g = np.floor(pos); gi = g.astype(np.int64)
        for k in range(8):
            q = [gi[:, d] + ((k >> d) & 1) for d in range(3)]
            qx, qy, qz = (np.asarray(v, np.uint64) & np.uint64(0xffffffff) for v in q)
            stride, dense = 1, np.zeros(x.shape[0], np.uint64)
            for coord in (qx, qy, qz):
                if stride <= size:
                    dense = (dense + coord * np.uint64(stride)) & np.uint64(0xffffffff); stride = (stride * r) & 0xffffffff
            if size < stride:
                idx = ((qx ^ (qy * np.uint64(2654435761) & np.uint64(0xffffffff)) ^ (qz * np.uint64(805459861) & np.uint64(0xffffffff)))
                       & np.uint64(0xffffffff)) % np.uint64(size)
            else:
                idx = dense % np.uint64(size)
            yield l, k, idx.astype(np.int64) + int(off[l]), pos - g


# ------------------------------------------------------------------ rays
def camera_rays(K, Twc, Tow, px, py):
    """pixel_ray (device_common.h) in float32 numpy for pixels (px, py) of one frame: origin, direction (object frame) and |camera ray|"""
    f32 = np.float32
    fx, fy, cx, cy = (f32(v) for v in K[:4])
    px = np.asarray(px, np.float32); py = np.asarray(py, np.float32)
    dc = np.stack([(px - cx) / fx, (py - cy) / fy, np.ones_like(px)], -1).reshape(-1, 3)
    n = np.sqrt((dc * dc).sum(-1, dtype=np.float32)).astype(np.float32)
    dn = dc / n[:, None]
    Rwc = Twc[:3, :3].astype(np.float32); Row = Tow[:3, :3].astype(np.float32)
    dw = dn @ Rwc.T; d = (dw @ Row.T).astype(np.float32)
    o = (Row @ Twc[:3, 3].astype(np.float32) + Tow[:3, 3].astype(np.float32)).astype(np.float32)
    return np.broadcast_to(o, d.shape).copy(), d, n


def rays(K, Twc, Tow, box):
    """camera_rays of every pixel of one box, row-major"""
    v, x0, y0, h, w = (int(q) for q in box)
    py, px = np.mgrid[y0:y0 + h, x0:x0 + w].astype(np.float32)
    return camera_rays(K, Twc, Tow, px.reshape(-1), py.reshape(-1))


def slab(aabb, o, d):
    """ray_intersect: (hit, max(t0, 0), t1)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        a = (aabb[0][None] - o) / d; b = (aabb[1][None] - o) / d
    lo = np.minimum(a, b); hi = np.maximum(a, b)
    t0 = lo.max(1); t1 = hi.min(1)
    return t0 <= t1, np.maximum(t0, np.float32(0.0)), t1


def targets(sc, box, cls):
    v, x0, y0, h, w = (int(q) for q in box)
    rgb = sc.rgb[v, y0:y0 + h, x0:x0 + w].reshape(-1, 3).astype(np.float32) / np.float32(255.0)
    m = (sc.instance[v, y0:y0 + h, x0:x0 + w].reshape(-1) == cls).astype(np.float64)
    d = sc.depth[v, y0:y0 + h, x0:x0 + w].reshape(-1).astype(np.float64)
    return rgb.astype(np.float64), m, d


def pose_rays(sc, boxes, Tow, aabb, cls, n_rays=0, seed=1, iteration=0, sample_seed=0, use_depth=True, which=None):
    """k_pose_rays and k_pose_grad's sample placement in numpy for the rays `which` (all by default) of one evaluation.
    n_rays = 0: ray i is pixel i of the union (box order, then row-major), jitter of sample k rand01(sample_seed, 3, 0, q * 64 + k), q the pixel inside its
    box; n_rays > 0: pixel draw(seed, iteration), jitter rand01(seed, 4, iteration, i * 64 + k).  Returns a dict of per-ray arrays: i, p (pixel of the
    union), b (box), x, y, o, d, dn, hit, t0, t1, t [P, 64] (float32), pos [P, 64, 3] (float32) and tgt [P, 5] (r, g, b, m*, d*; d* = 0 without depth)."""
    boxes = np.asarray(boxes, np.int64).reshape(-1, 5)
    area = boxes[:, 3] * boxes[:, 4]
    prefix = np.concatenate([[0], np.cumsum(area)]).astype(np.int64); total = int(prefix[-1])
    assert total <= MAX_UNION
    n = n_rays if n_rays else total
    i = np.arange(n, dtype=np.int64) if which is None else np.asarray(which, np.int64)
    p = draw(seed, iteration, n, total)[i].astype(np.int64) if n_rays else i
    b = np.searchsorted(prefix, p, side="right") - 1                         # the last box with prefix[b] <= p
    q = p - prefix[b]
    x = boxes[b, 1] + q % boxes[b, 4]; y = boxes[b, 2] + q // boxes[b, 4]
    P = i.size; f32 = np.float32
    o = np.zeros((P, 3), f32); d = np.zeros((P, 3), f32); dn = np.zeros(P, f32)
    for bb in np.unique(b):
        s = b == bb; v = int(boxes[bb, 0])
        o[s], d[s], dn[s] = camera_rays(np.array([sc.fx, sc.fy, sc.cx, sc.cy]), sc.Twc[v], Tow, x[s], y[s])
    hit, t0, t1 = slab(np.asarray(aabb, f32), o, d)
    k = np.arange(64, dtype=np.uint64)[None, :]
    if n_rays:
        u = rand01(seed, STREAM_POSE, iteration, i.astype(np.uint64)[:, None] * np.uint64(64) + k)
    else:
        u = rand01(sample_seed, STREAM_RENDER, 0, q.astype(np.uint64)[:, None] * np.uint64(64) + k)
    dtr = (t1 - t0) / f32(64.0)
    t = (dtr[:, None] * (np.arange(64, dtype=f32)[None, :] + u) + t0[:, None]).astype(f32)
    pos = (t[..., None] * d[:, None, :] + o[:, None, :]).astype(f32)
    v = boxes[b, 0]
    tgt = np.zeros((P, 5))
    tgt[:, :3] = sc.rgb[v, y, x].astype(f32) / f32(255.0)
    tgt[:, 3] = sc.instance[v, y, x] == cls
    if use_depth:
        tgt[:, 4] = sc.depth[v, y, x]
    return dict(i=i, p=p, b=b, x=x, y=y, o=o, d=d, dn=dn, hit=hit, t0=t0, t1=t1, t=t, pos=pos, tgt=tgt)


def huber(x, delta):
    ax = np.abs(x)
    return np.where(ax <= delta, 0.5 * x * x, delta * (ax - 0.5 * delta))


def composite_loss(raw, t, hit, dn, tgt, w):
    """per-ray loss in fp64 numpy from given raw network outputs [P, 64, 4] (the early cut and the second tile's evaluation as the kernel takes them)"""
    w_rgb, w_mask, w_depth, hub = (float(v) for v in w)
    raw = raw.astype(np.float64); t = t.astype(np.float64); P = t.shape[0]
    sigma = np.exp(raw[..., 3]); col = 1.0 / (1.0 + np.exp(-raw[..., :3]))
    dt = np.where(hit[:, None], t - np.concatenate([np.zeros((P, 1)), t[:, :-1]], 1), 0.0)     # (a miss has t0 > t1: no samples)
    alpha = 1.0 - np.exp(-sigma * dt)
    incl = np.cumprod(1.0 - alpha, 1); T = np.concatenate([np.ones((P, 1)), incl[:, :-1]], 1)
    ev = np.ones((P, 64), bool); ev[:, 32:] = (T[:, 32] >= EPS)[:, None]
    act = np.logical_and.accumulate(T >= EPS, 1) & ev & hit[:, None]
    a2 = np.where(act, alpha, 0.0)
    T2 = np.cumprod(np.concatenate([np.ones((P, 1)), 1.0 - a2[:, :-1]], 1), 1)
    wgt = a2 * T2; Tend = T2[:, -1] * (1.0 - a2[:, -1])
    r = (wgt[..., None] * (col - tgt[:, None, :3])).sum(1)
    O = 1.0 - Tend; D = (wgt * t).sum(1) / dn.astype(np.float64); m = tgt[:, 3]; dd = tgt[:, 4]
    return w_rgb * m * (r * r).sum(1) / 3 + w_mask * (O - m) ** 2 + w_depth * m * (dd > 0) * huber(D - dd, hub)


# ------------------------------------------------------------------ the fp64 autograd graph
def net_inputs(o, orc, prm):
    """the object's network and grid for the child: its EMA weights (side 0's, and the snapshot published at the end of train()), shape and level table"""
    cfg = o.cfg; info = o.info()
    off, scl, res = level_table(orc, orc.default_config(n_levels=cfg.n_levels, log2_hashmap_size=cfg.log2_hashmap_size, base_resolution=cfg.base_resolution,
                                                        per_level_scale=cfg.per_level_scale, n_neurons=cfg.n_neurons, n_hidden_layers=cfg.n_hidden_layers))
    return dict(params=o.get_params(2), n_mlp=info.n_mlp_params, L=cfg.n_levels, W=cfg.n_neurons, NH=cfg.n_hidden_layers, Ep=info.encoded_width,
                off=off, scl=scl, res=res, w=np.array([prm.w_rgb, prm.w_mask, prm.w_depth, prm.depth_huber]))


def reference(tmp_path, net, aabb, cases, tag="ref"):
    """Runs the fp64 graph in a child process.  cases: dicts of x [P, 64, 3] (the device's own fp32 positions), t [P, 64], hit [P], dn [P], tgt [P, 5] and
    optionally lw [L] (level weights).  Returns per case: l [P] (per-ray loss), gs [P, 64, 3] (dL/dx of the SUM over the rays, before the 1/N scale),
    loss (the mean), g6 (grad6 of the mean), ev [P, 64] (samples evaluated), ev1 [P] (tile 1 evaluated), D [P] (depth of the ray)."""
    data = dict(net, aabb=np.asarray(aabb, np.float32), n_cases=len(cases))
    for c, cs in enumerate(cases):
        for key in ("x", "t", "hit", "dn", "tgt", "lw"):
            if key in cs and cs[key] is not None:
                data["%s%d" % (key, c)] = cs[key]
    inp, outp = os.path.join(str(tmp_path), tag + "_in.npz"), os.path.join(str(tmp_path), tag + "_out.npz")
    np.savez(inp, **data)
    r = subprocess.run([sys.executable, os.path.join(HERE, "pose_reference.py"), inp, outp], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    z = np.load(outp)
    return [dict(l=z["l%d" % c], gs=z["gs%d" % c], loss=float(z["loss%d" % c]), g6=z["g6_%d" % c], ev=z["ev%d" % c] > 0, ev1=z["ev1%d" % c] > 0,
                 D=z["D%d" % c]) for c in range(len(cases))]


def _torch_child(inp, outp):
    """The objective as one fp64 autograd graph in the sample positions, per case; level l's dependence on the position scaled by lw[l] where given
    (x_l = x.detach() + lw[l] (x - x.detach()); the loss is unchanged)."""
    import torch
    z = np.load(inp)
    L, W, NH, Ep, nm = int(z["L"]), int(z["W"]), int(z["NH"]), int(z["Ep"]), int(z["n_mlp"])
    w_rgb, w_mask, w_depth, hub = (float(v) for v in z["w"])
    prm = z["params"].view(np.float16).astype(np.float64)
    table = torch.tensor(prm[nm:].reshape(-1, 2)); mats = []; o = 0
    for layer in range(NH + 1):
        rows = 16 if layer == NH else W; cols = Ep if layer == 0 else W
        mats.append(torch.tensor(prm[o:o + rows * cols].reshape(rows, cols))); o += rows * cols
    h16 = lambda v: v + (v.detach().to(torch.float16).to(torch.float64) - v.detach())     # noqa: E731
    aabb = z["aabb"]; ext = (aabb[1] - aabb[0]).astype(np.float32)
    out = {}
    for c in range(int(z["n_cases"])):
        xg = z["x%d" % c].reshape(-1, 3).astype(np.float32); P = xg.shape[0] // 64
        t = z["t%d" % c].astype(np.float64).reshape(P, 64); hit = z["hit%d" % c].astype(bool); dn = z["dn%d" % c].astype(np.float64); tg = z["tgt%d" % c]
        lw = z["lw%d" % c].astype(np.float64) if ("lw%d" % c) in z.files else np.ones(L)
        # the graph runs on the device's own fp32 positions (the parent checks them against the restatement): at the finest levels (scale 2^19) one ulp of
        # x is a few hundredths of a cell, so the trilinear weights are taken from the same fp32 arithmetic the kernel does (normalised position by fp32
        # subtract / divide, fmaf(scale, x, 0.5) exactly), and only their derivative comes from the graph
        xl = torch.tensor(xg.astype(np.float64), requires_grad=True)
        xn = (xl - torch.tensor(aabb[0].astype(np.float64))) / torch.tensor(ext.astype(np.float64))
        dxn = xn - xn.detach()
        xn32 = ((xg - aabb[0]) / ext).astype(np.float32)
        feats = [torch.zeros(P * 64, 2, dtype=torch.float64) for _ in range(L)]
        for l, k, idx, frac in corners(z["off"], z["scl"], z["res"], L, xn32):
            fr = torch.tensor(frac) + float(z["scl"][l]) * (lw[l] * dxn)
            wk = torch.ones(P * 64, dtype=torch.float64)
            for d in range(3):
                wk = wk * (fr[:, d] if (k >> d) & 1 else 1 - fr[:, d])
            feats[l] = feats[l] + wk[:, None] * table[torch.tensor(idx)]
        a = h16(torch.cat(feats + [torch.zeros(P * 64, Ep - 2 * L, dtype=torch.float64)], 1))
        for layer in range(NH):
            a = h16(torch.relu(a @ mats[layer].T))
        raw = h16((a @ mats[NH].T)[:, :4]).reshape(P, 64, 4)
        tt = torch.tensor(t); dt = tt - torch.cat([torch.zeros(P, 1, dtype=torch.float64), tt[:, :-1]], 1)
        # the early cut and the second tile's evaluation held at the forward's values
        with torch.no_grad():
            alpha = 1 - torch.exp(-torch.exp(raw[..., 3]) * dt)
            incl = torch.cumprod(1 - alpha, 1); T = torch.cat([torch.ones(P, 1, dtype=torch.float64), incl[:, :-1]], 1)
            ev1 = T[:, 32] >= EPS
            ev = torch.ones(P, 64, dtype=torch.bool); ev[:, 32:] = ev1[:, None]
            act = (T >= EPS) & ev & torch.tensor(hit)[:, None]
        # samples the kernel does not composite (misses, past the cut) enter the graph as 0 before any exp: their dt and raw outputs may be anything
        # (a miss has t0 > t1), and a masked inf would turn the zero gradient into a NaN
        zero = torch.zeros_like(dt)
        sigma = torch.exp(torch.where(act, raw[..., 3], zero)); col = torch.sigmoid(raw[..., :3])
        a2 = torch.where(act, 1 - torch.exp(-sigma * torch.where(act, dt, zero)), zero)
        T2 = torch.cumprod(torch.cat([torch.ones(P, 1, dtype=torch.float64), 1 - a2[:, :-1]], 1), 1)
        wgt = a2 * T2
        Tend = T2[:, -1] * (1 - a2[:, -1])
        c_t = torch.tensor(tg[:, :3]); m = torch.tensor(tg[:, 3]); dd = torch.tensor(tg[:, 4])
        r = (wgt[..., None] * (col - c_t[:, None, :])).sum(1)
        O = 1 - Tend; D = (wgt * tt).sum(1) / torch.tensor(dn)
        err = D - dd; ae = err.abs()
        hub_v = torch.where(ae <= hub, 0.5 * err * err, hub * (ae - 0.5 * hub))
        l = w_rgb * m * (r * r).sum(1) / 3 + w_mask * (O - m) ** 2 + w_depth * m * (dd > 0).double() * hub_v
        l.sum().backward()
        gx = xl.grad.numpy().reshape(-1, 3)
        xo = xg.astype(np.float64)
        out["g6_%d" % c] = np.concatenate([gx.sum(0), np.cross(xo, gx).sum(0)]) / P
        out["gs%d" % c] = gx.reshape(P, 64, 3); out["l%d" % c] = l.detach().numpy(); out["loss%d" % c] = float(l.detach().mean())
        out["ev%d" % c] = (ev.numpy() & hit[:, None]).astype(np.uint8); out["ev1%d" % c] = (ev1.numpy() & hit).astype(np.uint8)
        out["D%d" % c] = D.detach().numpy()
    np.savez(outp, **out)


if __name__ == "__main__":
    _torch_child(sys.argv[1], sys.argv[2])
