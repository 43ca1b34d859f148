"""Shared reference of the point-gradient tests (a helper module like pose_reference.py, not a test file): an fp64 numpy restatement of d raw3 / d u, the
derivative of an object's raw log density with respect to the unit-cube point, per hash-grid level, for any fused shape (encoder width 16 / 32, 32 / 64 /
128 neurons, 1 / 2 hidden layers, 1-16 levels), on the object's fp16 parameters.

What is differentiated is what include/mon_core.h states: each level's corners are the ones the fp32 forward gathers (fmaf(scale, u, 0.5) rounded to fp32,
as pose_reference.corners forms it), the activations are rounded to fp16 after every layer with the rounding held constant (a straight-through step), the
ReLU masks are those of this module's own fp64 forward, and level l's dependence on the point is scaled by lw[l].  With delta a displacement of u,
    frac_l(delta) = frac_l + scale_l lw_l delta,     raw(delta) = net(trilinear(frac(delta)) + the forward's rounding residuals),
and the reference is d raw3 / d delta at 0.  `forward` evaluates raw(delta) itself, so that tests can difference it; `python tests/field_grad_reference.py
IN.npz OUT.npz` takes the same derivative by torch fp64 autograd in a child process (torch and the HIP library do not share a process)."""
import os
import subprocess
import sys

import numpy as np

import pose_reference as pr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def n_mlp_params(W, NH, Ep):
    return W * Ep + (NH - 1) * W * W + 16 * W


def net_of(params_u16, off, scl, res, L, W, NH):
    """The dict the functions below take, from an fp16 parameter vector (uint16 view: MLP matrices, then the grid) and pose_reference.level_table's rows"""
    Ep = ((2 * L + 15) // 16) * 16
    return dict(params=np.ascontiguousarray(params_u16, np.uint16), n_mlp=n_mlp_params(W, NH, Ep), L=L, W=W, NH=NH, Ep=Ep, off=off, scl=scl, res=res)


def net_of_object(o, orc):
    """... of a device object: its EMA weights (what side 0 reads and what the last train call published to side 1)"""
    class _NoWeights:
        w_rgb = w_mask = w_depth = depth_huber = 0.0
    d = pr.net_inputs(o, orc, _NoWeights)
    return {k: d[k] for k in ("params", "n_mlp", "L", "W", "NH", "Ep", "off", "scl", "res")}


def matrices(net):
    prm = net["params"].view(np.float16).astype(np.float64); W, NH, Ep = int(net["W"]), int(net["NH"]), int(net["Ep"])
    mats, o = [], 0
    for layer in range(NH + 1):
        rows = 16 if layer == NH else W; cols = Ep if layer == 0 else W
        mats.append(prm[o:o + rows * cols].reshape(rows, cols)); o += rows * cols
    return mats, prm[int(net["n_mlp"]):].reshape(-1, 2)


def gather(net, u):
    """The corners of every level at the fp32 unit-cube points u (n, 3): frac [L, n, 3] (fp64 of the fp32 position's fraction) and feat [L, n, 8, 2]"""
    u = np.ascontiguousarray(u, np.float32); n = u.shape[0]; L = int(net["L"])
    _, table = matrices(net)
    frac = np.zeros((L, n, 3)); feat = np.zeros((L, n, 8, 2))
    for l, k, idx, fr in pr.corners(net["off"], net["scl"], net["res"], L, u):
        frac[l] = fr; feat[l, :, k] = table[idx]
    return frac, feat


def _h16(v):
    return v.astype(np.float16).astype(np.float64)


def _encode(net, frac, feat, delta, lw):
    L = int(net["L"]); n = frac.shape[1]
    E = np.zeros((n, int(net["Ep"])))
    for l in range(L):
        fr = frac[l] + float(net["scl"][l]) * lw[l] * delta
        for k in range(8):
            wk = np.ones(n)
            for d in range(3):
                wk = wk * (fr[:, d] if (k >> d) & 1 else 1 - fr[:, d])
            E[:, 2 * l:2 * l + 2] += wk[:, None] * feat[l, :, k]
    return E


def forward(net, g, delta=None, lw=None, resid=None):
    """raw(delta) (n, 4) in fp64.  resid None: every layer's output is rounded to fp16 (the forward the device runs, up to its fp32 accumulation); returns
    (raw, resid, masks) with resid the rounding residuals and masks the ReLU masks (rounded activation > 0, the kernel's rule).  resid given: the
    residuals are added instead of rounding again (the rounding held constant), the ReLUs act on the values themselves and masks holds the signs of
    the pre-activations (z > 0)."""
    frac, feat = g; n = frac.shape[1]; NH = int(net["NH"]); mats, _ = matrices(net)
    delta = np.zeros((n, 3)) if delta is None else np.asarray(delta, np.float64)
    lw = np.ones(int(net["L"])) if lw is None else np.asarray(lw, np.float64)
    out_res, masks = [], []

    def rnd(v, i):
        if resid is not None:
            return v + resid[i]
        r = _h16(v); out_res.append(r - v); return r
    a = rnd(_encode(net, frac, feat, delta, lw), 0)
    for layer in range(NH):
        z = a @ mats[layer].T
        a = rnd(np.maximum(z, 0.0), 1 + layer)
        masks.append(a > 0 if resid is None else z > 0)
    raw = rnd((a @ mats[NH].T)[:, :4], 1 + NH)
    return raw, out_res, masks


def gradient(net, u, lw=None):
    """(raw (n, 4): the rounded forward, grad (n, 3) = d raw3 / d u, per_level (L, n, 3): level l's term, lw[l] included)"""
    g = gather(net, u); frac, feat = g; L = int(net["L"]); NH = int(net["NH"]); n = frac.shape[1]; mats, _ = matrices(net)
    lw = np.ones(L) if lw is None else np.asarray(lw, np.float64)
    raw, _, masks = forward(net, g)
    dv = np.broadcast_to(mats[NH][3], (n, mats[NH].shape[1])).copy()               # d raw3 / d (last hidden activation)
    for layer in range(NH - 1, -1, -1):
        dv = (dv * masks[layer]) @ mats[layer]                                      # through the ReLU and the layer: d raw3 / d (its input)
    per = np.zeros((L, n, 3))
    for l in range(L):
        fr = frac[l]
        for k in range(8):
            f = dv[:, 2 * l] * feat[l, :, k, 0] + dv[:, 2 * l + 1] * feat[l, :, k, 1]
            for d in range(3):
                wk = np.full(n, 1.0 if (k >> d) & 1 else -1.0)
                for e in range(3):
                    if e != d:
                        wk = wk * (fr[:, e] if (k >> e) & 1 else 1 - fr[:, e])
                per[l, :, d] += wk * f
        per[l] *= float(net["scl"][l]) * lw[l]
    return raw, per.sum(0), per


def torch_gradient(tmp_path, net, u, lw=None, tag="fieldgrad"):
    """d raw3 / d u by torch fp64 autograd in a child process: (raw3 (n,), grad (n, 3)).  The graph adds this module's rounding residuals instead of
    rounding again: two fp64 sums in different orders may round to different fp16 neighbours, and the derivative, not the rounding, is what is compared."""
    g = gather(net, u); frac, feat = g
    _, resid, _ = forward(net, g)
    inp, outp = os.path.join(str(tmp_path), tag + "_in.npz"), os.path.join(str(tmp_path), tag + "_out.npz")
    np.savez(inp, frac=frac, feat=feat, lw=np.ones(int(net["L"])) if lw is None else np.asarray(lw, np.float64),
             **{"resid%d" % i: r for i, r in enumerate(resid)}, **{k: net[k] for k in ("params", "n_mlp", "L", "W", "NH", "Ep", "scl")})
    r = subprocess.run([sys.executable, os.path.join(HERE, "field_grad_reference.py"), inp, outp], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    z = np.load(outp)
    return z["raw3"], z["grad"]


def _torch_child(inp, outp):
    import torch
    z = np.load(inp)
    L, W, NH, Ep, nm = int(z["L"]), int(z["W"]), int(z["NH"]), int(z["Ep"]), int(z["n_mlp"])
    prm = z["params"].view(np.float16).astype(np.float64); mats = []; o = 0
    for layer in range(NH + 1):
        rows = 16 if layer == NH else W; cols = Ep if layer == 0 else W
        mats.append(torch.tensor(prm[o:o + rows * cols].reshape(rows, cols))); o += rows * cols
    rnd = lambda v, i: v + torch.tensor(z["resid%d" % i])     # noqa: E731
    frac = torch.tensor(z["frac"]); feat = torch.tensor(z["feat"]); n = frac.shape[1]
    delta = torch.zeros(n, 3, dtype=torch.float64, requires_grad=True)
    feats = []
    for l in range(L):
        fr = frac[l] + float(z["scl"][l]) * float(z["lw"][l]) * delta
        acc = torch.zeros(n, 2, dtype=torch.float64)
        for k in range(8):
            wk = torch.ones(n, dtype=torch.float64)
            for d in range(3):
                wk = wk * (fr[:, d] if (k >> d) & 1 else 1 - fr[:, d])
            acc = acc + wk[:, None] * feat[l, :, k]
        feats.append(acc)
    a = rnd(torch.cat(feats + [torch.zeros(n, Ep - 2 * L, dtype=torch.float64)], 1), 0)
    for layer in range(NH):
        a = rnd(torch.relu(a @ mats[layer].T), 1 + layer)
    raw3 = rnd((a @ mats[NH].T)[:, :4], 1 + NH)[:, 3]
    raw3.sum().backward()
    np.savez(outp, raw3=raw3.detach().numpy(), grad=delta.grad.numpy())


if __name__ == "__main__":
    _torch_child(sys.argv[1], sys.argv[2])
