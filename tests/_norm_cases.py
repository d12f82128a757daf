"""The BatchNorm / Scale / Sigmoid cases (csrc/norm.hip) of
tests/test_norm_kernel_coverage.py and tests/test_gpu_norm_kernels.py, their
inputs, and the reference arithmetic (batch_norm_layer.cpp:87-242,
scale_layer.cpp, relu_layer.cu, sigmoid_layer.cu) written once for two number
formats: float64 is the checker, float32 with the reference's order of
operations and left-to-right sums is the restatement whose error sets the
bounds (tests/golden/make_norm_bounds.py -> tests/golden/norm_bounds.json).
Each shape is the smallest that still takes its path.
"""
import numpy as np

EPS, MAF = 1e-5, 0.999

# name -> shape (N, C, H, W), the ids of forward / backward (training statistics, no Scale), what it is for
BN_CASES = {
    "a": dict(shape=(3, 5, 7, 7), fwd=["bn_stats_plane<1>", "bn_stats_finalize", "norm_apply<4>"],
              bwd=["norm_bwd_reduce_plane<1>", "norm_bwd_finalize", "norm_bwd<4>"]),     # odd inner, C < a wave
    "b": dict(shape=(4, 3, 64, 65), fwd=["bn_stats_plane<4>", "bn_stats_finalize", "norm_apply<4>"],
              bwd=["norm_bwd_reduce_plane<4>", "norm_bwd_finalize", "norm_bwd<4>"]),     # m = 16640: 5 slices, loops
    "c1": dict(shape=(2, 513, 1, 1), fwd=["bn_stats_cols", "bn_stats_finalize", "norm_apply<4>"],
               bwd=["norm_bwd_reduce_cols", "norm_bwd_finalize", "norm_bwd<4>"]),
    "c2": dict(shape=(64, 1024, 1, 1), fwd=["bn_stats_cols", "bn_stats_finalize", "norm_apply<4>"],
               bwd=["norm_bwd_reduce_cols", "norm_bwd_finalize", "norm_bwd<4>"]),        # 16 channel blocks x 4 slices
    "d": dict(shape=(1, 4, 1, 1), fwd=["bn_stats_cols", "bn_stats_finalize", "norm_apply<4>"],
              bwd=["norm_bwd_reduce_cols", "norm_bwd_finalize", "norm_bwd<4>"]),         # m = 1: variance 0
    "g": dict(shape=(4, 6, 5, 6), fwd=["bn_stats_plane<1>", "bn_stats_finalize", "norm_apply<4>"],
              bwd=["norm_bwd_reduce_plane<1>", "norm_bwd_finalize", "norm_bwd<4>"]),     # the fold; inner = 30
    "g4": dict(shape=(2, 8, 4, 4), fwd=["bn_stats_plane<4>", "bn_stats_finalize", "norm_apply<4>"],
               bwd=["norm_bwd_reduce_plane<4>", "norm_bwd_finalize", "norm_bwd<4>"]),    # the fold, one channel per vector
}
SIGMOID_N = 1031


def nci(shape):
    n, c = shape[0], shape[1]
    return n, c, int(np.prod(shape[2:]))


def inputs(name):
    """x, dy (N, C, inner) float32, gamma, beta (C) float32; fixed per case."""
    n, c, i = nci(BN_CASES[name]["shape"])
    r = np.random.RandomState(sum(map(ord, name)) + 1701)
    z = r.standard_normal((n, c, i))
    x = (100.0 + 0.1 * z) if name == "b" else (0.5 + 2.0 * z)
    dy = r.standard_normal((n, c, i))
    gamma = 0.5 + r.uniform(0.0, 1.5, c)
    gamma[0] = -0.75           # a channel with gamma < 0
    if c > 1:
        gamma[1] = 0.0         # and one with gamma = 0
    beta = r.standard_normal(c) * 0.3
    return tuple(a.astype(np.float32) for a in (x, dy, gamma, beta))


def sigmoid_inputs():
    r = np.random.RandomState(99)
    x = r.standard_normal(SIGMOID_N) * 4.0
    x[:4] = [100.0, -100.0, 0.0, -0.0]
    return x.astype(np.float32), r.standard_normal(SIGMOID_N).astype(np.float32)


# ------------------------------------------------------------- the arithmetic
def _sum(a, axis, dt):
    """float64: numpy's sum; float32: left to right, as a plain gemv accumulates."""
    if dt == np.float64:
        return a.sum(axis=axis)
    return np.take(np.cumsum(a, axis=axis, dtype=np.float32), -1, axis=axis)


def _chan_mean(a, dt):
    """batch_norm_layer.cpp:107-113: the spatial sums (gemv, alpha = 1 / m), then the batch sum (gemv)."""
    m = a.shape[0] * a.shape[2]
    return _sum(_sum(a, 2, dt) * dt(1.0 / m), 0, dt)


def bn_train(x, dt, one_pass=False):
    """mean, biased var, rstd, xhat (batch_norm_layer.cpp:107-166); one_pass: var = E[x^2] - E[x]^2 instead."""
    x = x.astype(dt)
    mean = _chan_mean(x, dt)
    cen = x - mean[None, :, None]
    var = (_chan_mean(x * x, dt) - mean * mean) if one_pass else _chan_mean(cen * cen, dt)
    std = np.sqrt(var + dt(EPS))
    return mean, var, (dt(1) / std), cen / std[None, :, None]


def running(mean, var, m, state, dt):
    """batch_norm_layer.cpp:138-146 on state = (run_mean, run_var, factor)."""
    rm, rv, f = (np.asarray(s, dt) for s in state)
    corr = dt(m / (m - 1.0)) if m > 1 else dt(1)
    return mean + dt(MAF) * rm, corr * var + dt(MAF) * rv, f * dt(MAF) + dt(1)


def bn_global(state, dt):
    """batch_norm_layer.cpp:98-105: mean, rstd from the running blobs."""
    rm, rv, f = (np.asarray(s, dt) for s in state)
    s = dt(0) if f == 0 else dt(1) / f
    return s * rm, dt(1) / np.sqrt(s * rv + dt(EPS))


def fold_fwd(xhat, gamma, beta, relu, dt):
    y = xhat.astype(dt)
    if gamma is not None:
        y = y * gamma.astype(dt)[None, :, None]
    if beta is not None:
        y = y + beta.astype(dt)[None, :, None]
    return np.maximum(y, 0) if relu else y


def bn_bwd(dy, y, xhat, rstd, gamma, relu, dt, centred=True):
    """Scale's and ReLU's backward, then batch_norm_layer.cpp:180-241: dx, dgamma, dbeta."""
    g = dy.astype(dt) * (y > 0) if relu else dy.astype(dt)
    xhat = xhat.astype(dt)
    dgamma = _sum(_sum(g * xhat, 2, dt), 0, dt)
    dbeta = _sum(_sum(g, 2, dt), 0, dt)
    t = g * gamma.astype(dt)[None, :, None] if gamma is not None else g
    if centred:
        t = t - _chan_mean(t, dt)[None, :, None] - _chan_mean(t * xhat, dt)[None, :, None] * xhat
    return t * rstd.astype(dt)[None, :, None], dgamma, dbeta


def sigmoid(x, dy, dt):
    with np.errstate(over="ignore"):
        y = dt(1) / (dt(1) + np.exp(-x.astype(dt)))
    return y, dy.astype(dt) * y * (dt(1) - y)


def quantities(name, dt, one_pass=False):
    """Every checked quantity of a case in one number format."""
    x, dy, gamma, beta = inputs(name)
    n, c, i = x.shape
    mean, var, rstd, xhat = bn_train(x, dt, one_pass)
    rm, rv, f = running(mean, var, n * i, (np.zeros(c), np.zeros(c), 0.0), dt)
    q = dict(mean=mean, rstd=rstd, xhat=xhat, run_mean=rm, run_var=rv)
    q["dx"], _, _ = bn_bwd(dy, None, xhat, rstd, None, False, dt)
    y = fold_fwd(xhat, gamma, beta, True, dt)
    q["y_fold"] = y
    q["dx_fold"], q["dgamma"], q["dbeta"] = bn_bwd(dy, y, xhat, rstd, gamma, True, dt)
    q["dx_global"], _, _ = bn_bwd(dy, y, xhat, rstd, gamma, True, dt, centred=False)
    # the stand-alone Scale on x itself
    q["scale_y"] = fold_fwd(x, gamma, beta, False, dt)
    q["scale_dx"], q["scale_dgamma"], q["scale_dbeta"] = bn_bwd(dy, None, x, np.ones(c), gamma, False, dt, centred=False)
    return q


def running_sequence(dt):
    """(e): three training forwards of case 'a''s shape on different inputs, then the TEST statistics."""
    n, c, i = nci(BN_CASES["a"]["shape"])
    r = np.random.RandomState(4242)
    xs = [(k + 0.5 * r.standard_normal((n, c, i)) * (k + 1)).astype(np.float32) for k in range(3)]
    xt = r.standard_normal((n, c, i)).astype(np.float32)
    state = (np.zeros(c), np.zeros(c), 0.0)
    for x in xs:
        mean, var, _, _ = bn_train(x, dt)
        state = running(mean, var, n * i, state, dt)
    gm, gr = bn_global(state, dt)
    y = (xt.astype(dt) - gm[None, :, None]) * gr[None, :, None]
    return xs, xt, dict(run_mean=state[0], run_var=state[1], factor=np.asarray(state[2]), y_test=y)


def ulp32(v):
    return float(np.spacing(np.float32(max(float(v), np.finfo(np.float32).tiny))))


def bound(q32, q64):
    """8 x the float32 restatement's largest error, floored at 4 ulp of the quantity's largest magnitude."""
    err = float(np.max(np.abs(q32.astype(np.float64) - q64)))
    return max(8.0 * err, 4.0 * ulp32(np.max(np.abs(q64))))


# ------------------------------------------------------------------ the tiny net
# data (4, 3, 8, 8) -> conv 3x3 pad 1 (8) -> BN -> Scale -> ReLU -> pool 2x2 -> fc16 -> BN -> Scale -> ReLU -> fc10
# -> softmax loss (tests/test_gpu_norm_layers.py), forward, backward and momentum SGD in one number format.
TINY_LR, TINY_WD, TINY_MOM, TINY_ITERS = 0.01, 0.004, 0.9, 3
# net.params() order; the BatchNorm blobs (run_mean, run_var, factor) take no gradient
TINY_PARAMS = ["conv_w", "conv_b", "bn1_mean", "bn1_var", "bn1_factor", "g1", "b1", "fc1_w", "fc1_b",
               "bn2_mean", "bn2_var", "bn2_factor", "g2", "b2", "fc2_w", "fc2_b"]
TINY_BN = ("bn1_mean", "bn1_var", "bn1_factor", "bn2_mean", "bn2_var", "bn2_factor")


def tiny_inputs():
    """data, label and the initial parameters (float32), fixed."""
    r = np.random.RandomState(2024)
    p = dict(conv_w=0.2 * r.standard_normal((8, 3, 3, 3)), conv_b=0.1 * r.standard_normal(8),
             g1=0.5 + r.uniform(0, 1, 8), b1=0.3 * r.standard_normal(8),
             fc1_w=0.1 * r.standard_normal((16, 128)), fc1_b=0.1 * r.standard_normal(16),
             g2=0.5 + r.uniform(0, 1, 16), b2=0.3 * r.standard_normal(16),
             fc2_w=0.3 * r.standard_normal((10, 16)), fc2_b=0.1 * r.standard_normal(10))
    for k, n in (("bn1", 8), ("bn2", 16)):
        p[k + "_mean"], p[k + "_var"], p[k + "_factor"] = np.zeros(n), np.zeros(n), np.zeros(1)
    data = r.uniform(-1, 1, (4, 3, 8, 8))
    label = r.randint(0, 10, 4)
    return data.astype(np.float32), label.astype(np.float32), {k: p[k].astype(np.float32) for k in TINY_PARAMS}


def _dot(a, b, dt):
    """a (..., K) . b (..., K) over the last axis, broadcast, summed as _sum does."""
    return _sum(a * b, -1, dt)


def tiny_step(data, label, p, dt):
    """One forward / backward: loss, the gradients, and the BatchNorm blobs the forward leaves."""
    x = data.astype(dt)
    n = x.shape[0]
    # conv 3x3 pad 1 as im2col x weights (base_conv_layer.cpp)
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    col = np.stack([xp[:, :, i:i + 8, j:j + 8] for i in range(3) for j in range(3)], axis=2)   # (N, 3, 9, 8, 8)
    col = col.reshape(n, 27, 64).transpose(0, 2, 1)                                            # (N, 64, 27)
    w = p["conv_w"].astype(dt).reshape(8, 27)
    c1 = _dot(col[:, None, :, :], w[None, :, None, :], dt) + p["conv_b"].astype(dt)[None, :, None]   # (N, 8, 64)
    m1, v1, r1, xh1 = bn_train(c1, dt)
    y1 = fold_fwd(xh1, p["g1"], p["b1"], True, dt)
    t = y1.reshape(n, 8, 4, 2, 4, 2).transpose(0, 1, 2, 4, 3, 5).reshape(n, 8, 16, 4)           # 2x2 windows
    arg = t.argmax(-1)
    pool = np.take_along_axis(t, arg[..., None], -1)[..., 0].reshape(n, 128)
    f1 = _dot(pool[:, None, :], p["fc1_w"].astype(dt)[None], dt) + p["fc1_b"].astype(dt)       # (N, 16)
    m2, v2, r2, xh2 = bn_train(f1[:, :, None], dt)
    y2 = fold_fwd(xh2, p["g2"], p["b2"], True, dt)[:, :, 0]
    z = _dot(y2[:, None, :], p["fc2_w"].astype(dt)[None], dt) + p["fc2_b"].astype(dt)          # (N, 10)
    e = np.exp(z - z.max(1, keepdims=True))
    prob = e / _sum(e, 1, dt)[:, None]
    lab = label.astype(int)
    loss = _sum(-np.log(prob[np.arange(n), lab]), 0, dt) / dt(n)
    # backward
    dz = prob.copy()
    dz[np.arange(n), lab] -= 1
    dz = dz / dt(n)
    g = {}
    g["fc2_w"] = _sum(dz.T[:, None, :] * y2.T[None, :, :], -1, dt)
    g["fc2_b"] = _sum(dz, 0, dt)
    dy2 = _dot(dz[:, None, :], p["fc2_w"].astype(dt).T[None], dt)
    df1, g["g2"], g["b2"] = bn_bwd(dy2[:, :, None], y2[:, :, None], xh2, r2, p["g2"], True, dt)
    df1 = df1[:, :, 0]
    g["fc1_w"] = _sum(df1.T[:, None, :] * pool.T[None, :, :], -1, dt)
    g["fc1_b"] = _sum(df1, 0, dt)
    dpool = _dot(df1[:, None, :], p["fc1_w"].astype(dt).T[None], dt).reshape(n, 8, 16)
    dt4 = np.zeros((n, 8, 16, 4), dt)
    np.put_along_axis(dt4, arg[..., None], dpool[..., None], -1)
    dy1 = dt4.reshape(n, 8, 4, 4, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(n, 8, 64)
    dc1, g["g1"], g["b1"] = bn_bwd(dy1, y1, xh1, r1, p["g1"], True, dt)
    g["conv_w"] = _sum(_sum(dc1[:, :, None, :] * col.transpose(0, 2, 1)[:, None, :, :], -1, dt), 0, dt).reshape(8, 3, 3, 3)
    g["conv_b"] = _sum(_sum(dc1, 2, dt), 0, dt)
    bn = {}
    for k, (mm, vv, cnt) in (("bn1", (m1, v1, n * 64)), ("bn2", (m2, v2, n))):
        bn[k + "_mean"], bn[k + "_var"], f = running(mm, vv, cnt, (p[k + "_mean"], p[k + "_var"], p[k + "_factor"][0]), dt)
        bn[k + "_factor"] = np.asarray(f, dt).reshape(1)
    return loss, g, bn


def tiny_train(dt, iters=TINY_ITERS):
    """Momentum SGD with L2 decay (sgd_solver.cpp: h = mom h + lr (g + wd w); w -= h), lr_mult = decay_mult = 1 and
    0 for the BatchNorm blobs: per iteration the loss, the gradients, and the parameters after the update."""
    data, label, p = tiny_inputs()
    p = {k: v.astype(dt) for k, v in p.items()}
    h = {k: np.zeros_like(v) for k, v in p.items()}
    out = []
    for _ in range(iters):
        loss, g, bn = tiny_step(data, label, p, dt)
        p.update(bn)
        for k in g:
            h[k] = dt(TINY_MOM) * h[k] + dt(TINY_LR) * (g[k] + dt(TINY_WD) * p[k])
            p[k] = p[k] - h[k]
        out.append(dict(loss=np.asarray(loss), grads={k: v.copy() for k, v in g.items()}, params={k: v.copy() for k, v in p.items()}))
    return out


def bn_on_data(dt):
    """data (4, 3, 8, 8) -> BatchNorm -> in-place Scale (bias) -> fc10 -> softmax loss: the BatchNorm's bottom takes no
    diff, so only the Scale's gradients make its backward run.  loss, dgamma, dbeta."""
    data, label, p = tiny_inputs()
    r = np.random.RandomState(77)
    gamma, beta = (0.5 + r.uniform(0, 1, 3)).astype(np.float32), (0.3 * r.standard_normal(3)).astype(np.float32)
    w, b = (0.1 * r.standard_normal((10, 192))).astype(np.float32), np.zeros(10, np.float32)
    n = data.shape[0]
    _, _, rstd, xh = bn_train(data.reshape(n, 3, 64), dt)
    y = fold_fwd(xh, gamma, beta, False, dt)
    z = _dot(y.reshape(n, 1, 192), w.astype(dt)[None], dt) + b.astype(dt)
    e = np.exp(z - z.max(1, keepdims=True))
    prob = e / _sum(e, 1, dt)[:, None]
    lab = label.astype(int)
    loss = _sum(-np.log(prob[np.arange(n), lab]), 0, dt) / dt(n)
    dz = prob.copy()
    dz[np.arange(n), lab] -= 1
    dz = dz / dt(n)
    dy = _dot(dz[:, None, :], w.astype(dt).T[None], dt).reshape(n, 3, 64)
    _, dgamma, dbeta = bn_bwd(dy, None, xh, rstd, gamma, False, dt)
    return dict(gamma=gamma, beta=beta, w=w, b=b), dict(loss=np.asarray(loss), dgamma=dgamma, dbeta=dbeta)
