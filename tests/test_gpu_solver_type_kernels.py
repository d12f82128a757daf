"""The Nesterov, AdaGrad, RMSProp, AdaDelta and Adam update kernels and the
fused training tail for any solver type, bit for bit.

The oracle is a numpy float32 restatement of the reference kernels
(src/caffe/solvers/{nesterov,adagrad,rmsprop,adadelta,adam}_solver.cu),
written here operation by operation: every product, sum, quotient and square
root is one float32 numpy operation, so one IEEE rounding each, in the
expressions' left-to-right order; 1 - momentum, 1 + momentum and 1 - rms_decay
are float32 too.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
ONE = F(1)
KINDS = ["Nesterov", "AdaGrad", "RMSProp", "AdaDelta", "Adam"]
TWO_HISTORIES = ("AdaDelta", "Adam")
# solver-wide scalars per type: momentum / beta1, momentum2 (beta2; rms_decay for RMSProp), delta
HYPER = {"SGD": (F(0.9), F(0.999), F(1e-8)), "Nesterov": (F(0.9), F(0.999), F(1e-8)),
         "AdaGrad": (F(0), F(0.999), F(1e-8)), "RMSProp": (F(0), F(0.95), F(1e-8)),
         "AdaDelta": (F(0.95), F(0.999), F(1e-6)), "Adam": (F(0.9), F(0.999), F(1e-8))}


def T(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def N(t):
    return t.detach().cpu().numpy()


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def np_update(kind, g, h, h2, hyper, lr):
    """The type's kernel on float32 arrays: (g', h', h2'); one rounding per operation."""
    a, b, delta = hyper
    lr = F(lr)
    assert g.dtype == h.dtype == np.float32
    with np.errstate(all="ignore"):
        if kind == "SGD":                                   # sgd_solver.cu:6-12
            v = a * h + lr * g
            return v, v.copy(), h2
        if kind == "Nesterov":                              # nesterov_solver.cu:10-12
            hn = a * h + lr * g
            return (ONE + a) * hn - a * h, hn, h2
        if kind == "AdaGrad":                               # adagrad_solver.cu:10-12
            hn = h + g * g
            return lr * g / (np.sqrt(hn) + delta), hn, h2
        if kind == "RMSProp":                               # rmsprop_solver.cu:10-12 (b: rms_decay)
            hn = b * h + (ONE - b) * g * g
            return lr * g / (np.sqrt(hn) + delta), hn, h2
        if kind == "AdaDelta":                              # adadelta_solver.cu:10-14
            hn = a * h + (ONE - a) * g * g
            u = g * np.sqrt((h2 + delta) / (hn + delta))
            h2n = a * h2 + (ONE - a) * u * u
            return lr * u, hn, h2n
        if kind == "Adam":                                  # adam_solver.cu:10-13
            m = h * a + g * (ONE - a)
            v = h2 * b + g * g * (ONE - b)
            return lr * m / (np.sqrt(v) + delta), m, v
    raise AssertionError(kind)


def gpu_update(kind, g, h, h2, hyper, lr):
    from rramsim import ops
    a, b, delta = (float(x) for x in hyper)
    lr = float(lr)
    if kind == "SGD":
        ops.sgd_update(g, h, a, lr)
    elif kind == "Nesterov":
        ops.nesterov_update(g, h, a, lr)
    elif kind == "AdaGrad":
        ops.adagrad_update(g, h, delta, lr)
    elif kind == "RMSProp":
        ops.rmsprop_update(g, h, b, delta, lr)
    elif kind == "AdaDelta":
        ops.adadelta_update(g, h, h2, a, delta, lr)
    else:
        ops.adam_update(g, h, h2, a, b, delta, lr)


def _hist(rng, kind, n):
    """Histories as the solvers leave them: signed for the momentum-like ones
    (Nesterov's h, Adam's m), non-negative averages of squares otherwise."""
    h = rng.standard_normal(n).astype(F)
    if kind in ("AdaGrad", "RMSProp", "AdaDelta"):
        h = np.abs(h)
    h2 = np.abs(rng.standard_normal(n)).astype(F) * F(0.01) if kind in TWO_HISTORIES else None
    return h, h2


def _grad(rng, n, scale=1.0):
    """Gradients bounded away from 0 (AdaGrad's 0/0 on a zero history is the
    reference's behaviour too and is not under test)."""
    g = rng.standard_normal(n).astype(F)
    g = np.where(np.abs(g) < 0.05, np.copysign(F(0.05), g), g).astype(F)
    return (g * F(scale)).astype(F)


@pytest.mark.parametrize("kind", KINDS)
def test_update_kernel_bit_exact(device, kind):
    """Each stand-alone kernel == its numpy float32 restatement bit for bit:
    n = 10 007 (no multiple of the block), pointers one float past an aligned
    base, the first 64 histories zero (the first iteration; h2 = 0 too)."""
    import torch
    rng = np.random.default_rng(100 + KINDS.index(kind))
    n = 10_007
    g = _grad(rng, n)
    h, h2 = _hist(rng, kind, n)
    h[:64] = 0
    if h2 is not None:
        h2[:64] = 0
    hyper, lr = HYPER[kind], F(0.01)

    def off(a):                                     # a view starting one float past the allocation's base
        if a is None:
            return None
        t = torch.empty(n + 1, dtype=torch.float32, device=device)
        assert t.data_ptr() % 16 == 0
        v = t[1:]
        v.copy_(torch.from_numpy(a))
        return v
    tg, th, th2 = off(g), off(h), off(h2)
    gpu_update(kind, tg, th, th2, hyper, lr)
    eg, eh, eh2 = np_update(kind, g, h, h2, hyper, lr)
    assert np.isfinite(eg).all()
    assert bits_equal(N(tg), eg), np.flatnonzero(N(tg).view(np.uint32) != eg.view(np.uint32))[:8]
    assert bits_equal(N(th), eh)
    if h2 is not None:
        assert bits_equal(N(th2), eh2)


def _calibrated_threshold(kind, w, g, h, h2, hyper, lr, decay):
    """The median |update| of this input (from the numpy restatement, a
    property of the test's data): half the elements fall under it."""
    gg = (F(decay) * w + g) if decay else g
    u, _, _ = np_update(kind, gg, h, h2, hyper, lr)
    return F(np.median(np.abs(u)))


@pytest.mark.parametrize("kind", KINDS)
def test_fused_tail_equals_unfused_sequence(device, kind):
    """rram_fused_opt_update_fail == axpy(decay), the type's update kernel,
    threshold_strategy, axpy(-1), fail_apply, bit for bit in w, g, h, h2,
    endurance and the broken count (and == the numpy restatement of the update
    up to the threshold); decay 0 and 0.004, a faultable and a non-faultable
    blob, endurance values exactly at the decrement, and a threshold that
    clears some hundreds of updates and keeps some hundreds."""
    from rramsim import _kernels as K
    from rramsim import ops
    rng = np.random.default_rng(200 + KINDS.index(kind))
    n = 4099
    w = rng.standard_normal(n).astype(F)
    g = _grad(rng, n)
    h, h2 = _hist(rng, kind, n)
    h[:64] = 0
    if h2 is not None:
        h2[:64] = 0
    e = rng.normal(150, 100, n).astype(F)
    e[:64] = 100.0                                  # exactly-zero crossings at decrement 100
    v = rng.integers(-1, 2, n).astype(F)
    hyper, lr = HYPER[kind], F(0.01)
    hy = ops.solver_hyper(*(float(x) for x in hyper))
    for decay in (0.0, 0.004):
        thr = _calibrated_threshold(kind, w, g, h, h2, hyper, lr, decay)
        for faulty in (True, False):
            tw, tg, th = T(w, device), T(g, device), T(h, device)
            th2 = T(h2, device) if h2 is not None else None
            te, tv = (T(e, device), T(v, device)) if faulty else (None, None)
            cnt = ops.counters(1, device)
            ops.fused_opt_update_fail(K.SOLVER_KINDS[kind], hy, tw, tg, th, th2, te, tv, decay, float(lr), True,
                                      float(thr), counter=cnt if faulty else None)
            uw, ug, uh = T(w, device), T(g, device), T(h, device)
            uh2 = T(h2, device) if h2 is not None else None
            if decay:
                ops.axpy(decay, uw, ug)
            gpu_update(kind, ug, uh, uh2, hyper, lr)
            cleared = ops.counters(1, device)
            ops.threshold_strategy(ug, float(thr), cleared)
            ops.axpy(-1.0, ug, uw)
            c2 = ops.counters(1, device)
            if faulty:
                ue = T(e, device)
                ops.fail_apply(ug, uw, ue, T(v, device), counter=c2)
                assert bits_equal(N(te), N(ue))
                assert int(N(cnt)[0]) == int(N(c2)[0]) > 0
            assert bits_equal(N(tw), N(uw)) and bits_equal(N(tg), N(ug)) and bits_equal(N(th), N(uh))
            if h2 is not None:
                assert bits_equal(N(th2), N(uh2))
            # the threshold fired on some hundreds and spared some hundreds
            n_cleared = int(N(cleared)[0])
            got_g = N(tg)
            assert n_cleared >= 300 and int((got_g != 0).sum()) >= 300, (n_cleared, int((got_g != 0).sum()))
            assert int((got_g == 0).sum()) == n_cleared
            # and the histories / surviving updates are the numpy restatement's
            gg = (F(decay) * w + g) if decay else g
            eg, eh, eh2 = np_update(kind, gg, h, h2, hyper, lr)
            eg = np.where(np.abs(eg) <= thr, F(0), eg)
            assert bits_equal(got_g, eg) and bits_equal(N(th), eh)
            if h2 is not None:
                assert bits_equal(N(th2), eh2)


def _np_flip(w, G, cin, cout, taps):
    """w [G*cout][cin][taps] -> [G*cin][cout][taps], transposed per group and rotated 180 degrees."""
    return np.ascontiguousarray(w.reshape(G, cout, cin, taps).transpose(0, 2, 1, 3)[..., ::-1]).reshape(-1)


@pytest.mark.parametrize("kind", ["SGD"] + KINDS)
def test_batched_equals_per_blob(device, kind):
    """rram_fused_opt_update_fail_batched == one rram_fused_opt_update_fail per
    blob: sizes straddling the 2048-element chunk, a 216-element convolution
    blob with its flipped copy, one segment without fault state, two segments
    sharing one counter, per-segment decay / rate / threshold.  For SGD the
    entry also == rram_fused_update_fail_batched (the same kernel behind the
    narrower segment, the convolution blob's flipped copy included)."""
    import torch
    from rramsim import _kernels as K
    from rramsim import ops
    rng = np.random.default_rng(300 + (["SGD"] + KINDS).index(kind))
    G, cin, cout, taps = 2, 3, 4, 9
    sizes = [1, 2047, 2048, 2049, 6145, 17, G * cin * cout * taps]
    conv = len(sizes) - 1
    hyper = HYPER[kind]
    hy = ops.solver_hyper(*(float(x) for x in hyper))
    two = kind in TWO_HISTORIES
    blobs = []
    for k, n in enumerate(sizes):
        w = rng.standard_normal(n).astype(F)
        g = _grad(rng, n)
        h, h2 = _hist(rng, kind if kind != "SGD" else "Nesterov", n)
        e = rng.normal(150, 100, n).astype(F)
        v = rng.integers(-1, 2, n).astype(F)
        faulty = k != 2
        lr, decay = F(0.01 * (k + 1)), 0.004 * (k % 2)
        thr = _calibrated_threshold(kind, w, g, h, h2, hyper, lr, decay)
        blobs.append((w, g, h, h2, e if faulty else None, v if faulty else None, decay, lr, faulty, thr))
    cnt_b, cnt_u, cnt_s = (ops.counters(len(sizes), device) for _ in range(3))
    flip_b, flip_s = (torch.zeros(sizes[conv], dtype=torch.float32, device=device) for _ in range(2))
    segs, sgd_segs, outs_b, outs_u, outs_s = [], [], [], [], []
    for k, (w, g, h, h2, e, v, decay, lr, faulty, thr) in enumerate(blobs):
        mk = lambda: [T(x, device) if x is not None else None for x in (w, g, h, h2, e, v)]  # noqa: E731
        tb, tu, ts = mk(), mk(), mk()
        slot = 0 if k in (0, 5) else k                  # blobs 0 and 5 share counter 0
        cb, cu, cs = (c[slot:slot + 1] if faulty else None for c in (cnt_b, cnt_u, cnt_s))
        segs.append((*tb, decay, float(lr), faulty, float(thr), cb,
                     (flip_b, G, cin, cout, taps) if k == conv else None))
        ops.fused_opt_update_fail(K.SOLVER_KINDS[kind], hy, *tu, decay, float(lr), faulty, float(thr), counter=cu)
        sgd_segs.append((ts[0], ts[1], ts[2], ts[4], ts[5], decay, float(lr), faulty, float(thr), cs,
                         (flip_s, G, cin, cout, taps) if k == conv else None))
        outs_b.append(tb)
        outs_u.append(tu)
        outs_s.append(ts)
    ops.fused_opt_update_fail_batched(K.SOLVER_KINDS[kind], hy, segs)
    for k, (tb, tu) in enumerate(zip(outs_b, outs_u)):
        for j, (a, b) in enumerate(zip(tb, tu)):
            if a is not None and (j != 3 or two):
                assert bits_equal(N(a), N(b)), (k, j)
        # against the numpy restatement: g after the threshold, both histories
        w, g, h, h2, e, v, decay, lr, faulty, thr = blobs[k]
        gg = (F(decay) * w + g) if decay else g
        eg, eh, eh2 = np_update(kind, gg, h, h2, hyper, lr)
        if faulty:
            eg = np.where(np.abs(eg) <= thr, F(0), eg)
        assert bits_equal(N(tb[1]), eg) and bits_equal(N(tb[2]), eh), k
        if two:
            assert bits_equal(N(tb[3]), eh2), k
    assert (N(cnt_b) == N(cnt_u)).all() and int(N(cnt_b).sum()) > 0
    assert bits_equal(N(flip_b), _np_flip(N(outs_b[conv][0]), G, cin, cout, taps))
    if kind == "SGD":
        ops.fused_update_fail_batched(sgd_segs, float(hyper[0]))
        for k, (tb, ts) in enumerate(zip(outs_b, outs_s)):
            for j in (0, 1, 2, 4):
                if tb[j] is not None:
                    assert bits_equal(N(tb[j]), N(ts[j])), (k, j)
        assert (N(cnt_b) == N(cnt_s)).all()
        assert bits_equal(N(flip_s), _np_flip(N(outs_s[conv][0]), G, cin, cout, taps))
