"""fp64 layer references with an error scale, for the per-layer parity checks.

Each helper evaluates one Convolution / InnerProduct layer of the reference's
definition (caffe_conv, test_convolution_layer.cpp:21-139; InnerProduct
top = X·Wᵀ + b, inner_product_layer.cpp:83-96) in float64 on the CPU, and
returns it with the layer's error scale Σ|a·b| + |bias| (the same expression
evaluated on absolute values).  A fp32 GEMM of any summation order differs from
the exact value by at most ~K·2^-24 of that scale, so the bound

    |got - ref| <= 1e-4 · scale          (north_star: 1e-4 relative, fp32)

is the scale-aware form of "within 1e-4 relative" that holds for every output
element, including the ones where cancellation makes the plain relative error
meaningless.  Inputs are the GPU's own bottom blobs, so each layer is checked
on its own (no error propagation between layers).
"""
from __future__ import annotations

import numpy as np

TOL = 1e-4


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def conv64(x, w, b, stride=1, pad=0, group=1, dilation=1):
    import torch
    F = torch.nn.functional
    x64, w64 = _t(x), _t(w)
    b64 = _t(b) if b is not None else None
    ref = F.conv2d(x64, w64, b64, stride, pad, dilation, group)
    scale = F.conv2d(x64.abs(), w64.abs(), b64.abs() if b is not None else None, stride, pad, dilation, group)
    return ref.numpy(), scale.numpy()


def ip64(x, w, b):
    x64 = np.asarray(x, np.float64).reshape(len(x), -1)
    w64 = np.asarray(w, np.float64).reshape(-1, x64.shape[1])
    ref = x64 @ w64.T
    scale = np.abs(x64) @ np.abs(w64).T
    if b is not None:
        ref = ref + np.asarray(b, np.float64)
        scale = scale + np.abs(np.asarray(b, np.float64))
    return ref, scale


def assert_scaled(got, ref, scale, what, tol=TOL, relu=False):
    got = np.asarray(got, np.float64).reshape(ref.shape)
    if relu:
        ref = np.maximum(ref, 0.0)
    err = np.abs(got - ref)
    bound = tol * scale
    bad = err > bound
    if bad.any():
        r = err / np.maximum(scale, 1e-300)
        i = int(np.argmax(r))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements exceed {tol}·Σ|a·b| "
                             f"(worst err/scale {r.flat[i]:.3e}: got {got.flat[i]!r}, ref {ref.flat[i]!r})")
    return float((err / np.maximum(scale, 1e-300)).max())


def check_conv(got, x, w, b, stride=1, pad=0, group=1, relu=False, what="conv"):
    ref, scale = conv64(x, w, b, stride, pad, group)
    return assert_scaled(got, ref, scale, what, relu=relu)


def check_ip(got, x, w, b, relu=False, what="ip"):
    ref, scale = ip64(x, w, b)
    return assert_scaled(got, ref, scale, what, relu=relu)


def lrn64(x, size, alpha, beta, k=1.0):
    """lrn_layer.cpp CrossChannelForward: x · (k + alpha/size · Σ x²)^-beta, fp64."""
    x = np.asarray(x, np.float64)
    n, c = x.shape[:2]
    pre = (size - 1) // 2
    sq = np.zeros((n, c + size - 1) + x.shape[2:])
    sq[:, pre:pre + c] = x * x
    s = np.full(x.shape, k)
    for ch in range(c):
        s[:, ch] += (alpha / size) * sq[:, ch:ch + size].sum(axis=1)
    return x * np.power(s, -beta)


def maxpool64(x, k, s):
    import math
    x = np.asarray(x, np.float64)
    H, W = x.shape[2:]
    PH = int(math.ceil((H - k) / s)) + 1
    PW = int(math.ceil((W - k) / s)) + 1
    out = np.empty(x.shape[:2] + (PH, PW))
    for a in range(PH):
        for b_ in range(PW):
            out[:, :, a, b_] = x[:, :, a * s:min(a * s + k, H), b_ * s:min(b_ * s + k, W)].max(axis=(2, 3))
    return out


# ---------------------------------------------------------------------------
# Support layers (csrc/layers.hip), vectorised over N and C: the only Python
# loops run over window taps.  tests/test_gpu_layer_kernel_matrix.py.
# ---------------------------------------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)


def pool_shape(H, W, kh, kw, sh, sw, ph, pw):
    """pooling_layer.cpp:90-104: ceil rule; with padding the last window must start inside the image."""
    PH = -(-(H + 2 * ph - kh) // sh) + 1
    PW = -(-(W + 2 * pw - kw) // sw) + 1
    if ph or pw:
        if (PH - 1) * sh >= H + ph:
            PH -= 1
        if (PW - 1) * sw >= W + pw:
            PW -= 1
    return PH, PW


def _taps(L, P, k, s, p):
    """Per tap a < k: (input index clipped into [0, L), inside the image?) for the P window starts."""
    st = np.arange(P) * s - p
    return [(np.clip(st + a, 0, L - 1), (st + a >= 0) & (st + a < L)) for a in range(k)]


def _ave_size(L, P, k, s, p):
    """AvePoolForward's divisor along one axis: the window clipped to [-pad, L + pad)."""
    st = np.arange(P) * s - p
    return np.minimum(st + k, L + p) - st


def maxpool_scan(x, kh, kw, sh, sw, ph, pw):
    """MaxPoolForward (pooling_layer.cu:11-47) on float32 x [N, C, H, W]: the
    window clipped to the image, -FLT_MAX start, strict '>' in row-major order,
    so the first maximum wins and a NaN never does.  (values float32, argmax
    int32 or -1); comparisons only, so this is exact."""
    x = np.asarray(x, np.float32)
    H, W = x.shape[2:]
    PH, PW = pool_shape(H, W, kh, kw, sh, sw, ph, pw)
    m = np.full(x.shape[:2] + (PH, PW), -FLT_MAX, np.float32)
    mi = np.full(m.shape, -1, np.int32)
    for h, okh in _taps(H, PH, kh, sh, ph):
        for w, okw in _taps(W, PW, kw, sw, pw):
            v = x[:, :, h[:, None], w[None, :]]
            with np.errstate(invalid="ignore"):
                up = (okh[:, None] & okw[None, :]) & (v > m)
            m = np.where(up, v, m)
            mi = np.where(up, (h[:, None] * W + w[None, :]).astype(np.int32), mi)
    return m, mi


def avepool64(x, kh, kw, sh, sw, ph, pw):
    """AvePoolForward (pooling_layer.cu:52-84): (float64 mean over Caffe's padded window size, Σ|term|)."""
    x = np.asarray(x, np.float64)
    H, W = x.shape[2:]
    PH, PW = pool_shape(H, W, kh, kw, sh, sw, ph, pw)
    s = np.zeros(x.shape[:2] + (PH, PW))
    sa = np.zeros_like(s)
    for h, okh in _taps(H, PH, kh, sh, ph):
        for w, okw in _taps(W, PW, kw, sw, pw):
            v = x[:, :, h[:, None], w[None, :]] * (okh[:, None] & okw[None, :])
            s += v
            sa += np.abs(v)
    size = (_ave_size(H, PH, kh, sh, ph)[:, None] * _ave_size(W, PW, kw, sw, pw)[None, :]).astype(np.float64)
    return s / size, sa / size


def maxpool_bwd64(dy, mask, H, W):
    """MaxPoolBackward: dx[mask] += dy per plane (mask -1: nowhere).  (dx, Σ|term|) float64."""
    dy = np.asarray(dy, np.float64)
    N, C = dy.shape[:2]
    plane = np.arange(N * C, dtype=np.int64).reshape(N, C, 1, 1) * (H * W)
    ok = mask >= 0
    idx = (plane + np.where(ok, mask, 0))[ok]
    dx = np.bincount(idx, weights=dy[ok], minlength=N * C * H * W)
    sc = np.bincount(idx, weights=np.abs(dy[ok]), minlength=N * C * H * W)
    return dx.reshape(N, C, H, W), sc.reshape(N, C, H, W)


def avepool_bwd64(dy, H, W, kh, kw, sh, sw, ph, pw):
    """AvePoolBackward (pooling_layer.cu:245-279): every covering window's dy / its padded size."""
    dy = np.asarray(dy, np.float64)
    PH, PW = dy.shape[2:]
    size = (_ave_size(H, PH, kh, sh, ph)[:, None] * _ave_size(W, PW, kw, sw, pw)[None, :]).astype(np.float64)
    t = dy / size
    dx = np.zeros(dy.shape[:2] + (H, W))
    sc = np.zeros_like(dx)
    for h, okh in _taps(H, PH, kh, sh, ph):
        for w, okw in _taps(W, PW, kw, sw, pw):     # within one tap every window hits its own element
            a, b = np.nonzero(okh)[0], np.nonzero(okw)[0]
            dx[:, :, h[a][:, None], w[b][None, :]] += t[:, :, a[:, None], b[None, :]]
            sc[:, :, h[a][:, None], w[b][None, :]] += np.abs(t[:, :, a[:, None], b[None, :]])
    return dx, sc


def relu64(v, slope):
    """relu_layer.cu:9-15 on any float array (slope as the float32 the kernel gets)."""
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, v, v * np.asarray(np.float32(slope), v.dtype))


def relu_bwd_factor(y, slope):
    """relu_layer.cu:35-44: (y > 0) + (y <= 0) * slope (a NaN y gives 0)."""
    with np.errstate(invalid="ignore"):
        return (y > 0) + (y <= 0) * np.float64(np.float32(slope))


def lrn_scale64(x, size, alpha, k=1.0):
    x = np.asarray(x, np.float64)
    c = x.shape[1]
    pre = (size - 1) // 2
    sq = np.zeros((x.shape[0], c + size - 1) + x.shape[2:])
    sq[:, pre:pre + c] = x * x
    s = np.full(x.shape, float(k))
    for j in range(size):
        s += (alpha / size) * sq[:, j:j + c]
    return s


def lrn_bwd64(x, y, scale, dy, size, alpha, beta):
    """LRNComputeDiff (lrn_layer.cu:120-165) of the given x, y, scale, dy:
    dx = dy scale^-beta - 2 alpha beta / size · x · Σ_{j: c in window j} dy_j y_j / scale_j.  (dx, Σ|term|)."""
    x, y, scale, dy = (np.asarray(a, np.float64) for a in (x, y, scale, dy))
    c = x.shape[1]
    pre = (size - 1) // 2
    post = size - pre - 1
    r = np.zeros((x.shape[0], c + size - 1) + x.shape[2:])
    r[:, post:post + c] = dy * y / scale
    ra = np.abs(r)
    acc, acca = np.zeros_like(x), np.zeros_like(x)
    for j in range(size):                    # channels c - post .. c + pre
        acc += r[:, j:j + c]
        acca += ra[:, j:j + c]
    cr = 2.0 * alpha * beta / size
    a = dy * np.power(scale, -beta)
    return a - cr * x * acc, np.abs(a) + cr * np.abs(x) * acca


def _within_sizes(H, W, size):
    pre = (size - 1) // 2
    return (_ave_size(H, H, size, 1, pre)[:, None] * _ave_size(W, W, size, 1, pre)[None, :]).astype(np.float64)


def _window_sum(v, size):
    """Σ of v over the size x size window centred on each element, clipped to the image."""
    pre = (size - 1) // 2
    H, W = v.shape[2:]
    p = np.zeros(v.shape[:2] + (H + size - 1, W + size - 1))
    p[:, :, pre:pre + H, pre:pre + W] = v
    out = np.zeros_like(v)
    for a in range(size):
        for b in range(size):
            out += p[:, :, a:a + H, b:b + W]
    return out


def lrn_within64(x, size, alpha, beta):
    """lrn_layer.cpp WithinChannelForward: (y, scale) with scale = 1 + alpha · AVE-pool(x²) (Caffe's padded divisor)."""
    x = np.asarray(x, np.float64)
    sc = 1.0 + alpha * _window_sum(x * x, size) / _within_sizes(*x.shape[2:], size)
    return x * np.power(sc, -beta), sc


def lrn_within_bwd64(x, scale, dy, size, alpha, beta):
    """WithinChannelBackward of the given x, scale, dy:
    dx = dy scale^-beta - 2 alpha beta · x · Σ_{windows p holding the element} dy_p x_p scale_p^(-beta-1) / n_p."""
    x, scale, dy = (np.asarray(a, np.float64) for a in (x, scale, dy))
    t = dy * x * np.power(scale, -beta - 1.0) / _within_sizes(*x.shape[2:], size)
    a = dy * np.power(scale, -beta)
    return (a - 2.0 * alpha * beta * x * _window_sum(t, size),
            np.abs(a) + 2.0 * alpha * beta * np.abs(x) * _window_sum(np.abs(t), size))


def softmax64(x):
    """softmax_layer.cu over axis 1 of [outer, C, inner] (-Inf entries allowed beside a finite one)."""
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def softmax_loss64(prob, label, ignore=-1):
    """softmax_loss_layer.cpp:95-112: (loss, Σ|term| / N, #valid) with the FLT_MIN clamp."""
    prob = np.asarray(prob, np.float64)
    lab = np.asarray(label).astype(np.int64)                    # [outer, inner]
    valid = np.ones(lab.shape, bool) if ignore < 0 else lab != ignore
    p = np.take_along_axis(prob, np.where(valid, lab, 0)[:, None, :], 1)[:, 0, :]
    t = -np.log(np.maximum(p, FLT_MIN)) * valid
    n = max(int(valid.sum()), 1)
    return t.sum() / n, np.abs(t).sum() / n, int(valid.sum())


def softmax_loss_bwd64(prob, label, ignore=-1, loss_weight=1.0):
    """softmax_loss_layer.cu backward: (prob - onehot) · loss_weight / #valid, 0 at ignored columns.
    The scale is the float32 quotient the host (or the fused kernel) forms.  (dx, |prob| + onehot) · scale."""
    prob = np.asarray(prob, np.float64)
    lab = np.asarray(label).astype(np.int64)
    valid = np.ones(lab.shape, bool) if ignore < 0 else lab != ignore
    onehot = (np.arange(prob.shape[1])[None, :, None] == lab[:, None, :]).astype(np.float64)
    sc = float(np.float32(loss_weight) / np.float32(max(int(valid.sum()), 1)))
    v = valid[:, None, :]
    return (prob - onehot) * sc * v, (np.abs(prob) + onehot) * sc * v


def accuracy64(x, label, top_k=1, ignore=-1):
    """accuracy_layer.cpp:48-90: (#correct, #counted); the label's (value, index) pair within the top_k."""
    x = np.asarray(x)
    lab = np.asarray(label).astype(np.int64)
    valid = np.ones(lab.shape, bool) if ignore < 0 else lab != ignore
    l0 = np.where(valid, lab, 0)[:, None, :]
    v = np.take_along_axis(x, l0, 1)
    c = np.arange(x.shape[1])[None, :, None]
    rank = ((x > v) | ((x == v) & (c > l0))).sum(axis=1)
    return int(((rank < top_k) & valid).sum()), int(valid.sum())


# fp32-level guard of the bf16x6 engine (tests/test_gpu_fp32_guard.py): per
# layer, errors in units of Σ|a·b| (max, mean) of the bf16x6 kernel and of the
# fp32-MFMA kernel on the same data.  The 1e-4 gate above would pass a kernel
# that had lost fp32 accuracy; these bounds do not (tests/test_x6_guard_emulation.py).
X6_GUARD_MAX = 1e-6
X6_GUARD_RATIO = 2.0


def x6_guard_failures(x6, f32):
    """x6, f32 = (max, mean) error / Σ|a·b|; the list of violated bounds."""
    bad = []
    if not x6[0] <= X6_GUARD_MAX:
        bad.append(f"max {x6[0]:.3e} > {X6_GUARD_MAX}")
    if not x6[0] <= X6_GUARD_RATIO * f32[0]:
        bad.append(f"max {x6[0]:.3e} > {X6_GUARD_RATIO} x fp32 MFMA max {f32[0]:.3e}")
    if not x6[1] <= X6_GUARD_RATIO * f32[1]:
        bad.append(f"mean {x6[1]:.3e} > {X6_GUARD_RATIO} x fp32 MFMA mean {f32[1]:.3e}")
    return bad
