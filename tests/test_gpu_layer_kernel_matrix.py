"""Every support-layer kernel and dispatch branch (csrc/layers.hip) against float64.

tests/_layer_cases.py holds one case per kernel and branch, with the kernel
ids its entry points record (tests/test_layer_kernel_coverage.py checks the
table on the CPU).  Each case runs here with its ids asserted again, against
the float64 references of tests/_ref64.py on inputs drawn on the CPU with a
fixed seed (the GPU is never its own reference: a backward gets the
reference's mask / scale / y as inputs), in two passes:

  exact     small integers with many ties; MAX pools also see +-0, +-Inf, NaN
            and -FLT_MAX.  Bit-equal to the reference: MAX values and masks
            (the first index wins, a NaN never does), MAX backward, ReLU,
            concat, accuracy counts, i32 -> f32, Euclidean diff / dx, and the
            softmax-loss gradient at loss_weight 1 on probabilities that are
            multiples of 1/8.  AVE forward: the window sum of integers is exact
            in fp32, so the kernel's one rounding is that of s / size.  The
            Makefile compiles with -O3 and neither -ffast-math nor
            -fno-hip-fp32-correctly-rounded-divide-sqrt, so hipcc's default holds
            and fp32 '/' is correctly rounded (the v_div_scale / v_div_fmas /
            v_div_fixup sequence); rounding the float64 quotient to fp32 is that
            same value (53 >= 2 * 24 + 2 bits: no double rounding for a
            quotient), so the assertion is equality, not 1 ulp.
  gaussian  normal inputs; bounds derived or the project's, none tuned here:
            AVE forward / backward  (terms + 1) 2^-24 Σ|term|, terms = window
                                    size / covering windows
            LRN forward             rtol 2e-5, atol 1e-6 (test_gpu_layers.py's;
                                    the kernels use the hardware log / exp pair)
            LRN backward            1e-4 Σ|term| + 1e-5
            softmax                 rtol 1e-5, atol 1e-7; columns sum to 1
                                    within (C / 64 + 8) 2^-24
            losses                  1e-5 Σ|term| / N
            MAX values, masks and the elementwise kernels stay bit-equal.

The _relu_ forms are checked against the reference's own ReLU (slope 0.25: the
product is exact), never against the unfused kernels.  Every output starts as
a sentinel and is followed by a guard band that must stay untouched, so a
kernel that skips elements or writes past its count fails.  Each test prints
the worst error over its bound per float kernel (pytest -s)."""
import numpy as np
import pytest

import _ref64 as R
from _layer_cases import AVE, LAYER_CASES, MAX, geom, ids_of, label, name, want_ids

pytestmark = pytest.mark.gpu

IDS = [label(i) for i in range(len(LAYER_CASES))]
PASSES = ["exact", "gaussian"]
GUARD, SENT, ISENT = 64, -7777.25, -77
SLOPE = 0.25
U = 2.0 ** -24
WORST = {}


def _note(kernel, err, bound):
    """Record and print max(err / bound) for one float kernel."""
    r = float(np.max(err / bound)) if np.size(err) else 0.0
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)
    print(f"layer-matrix {kernel}: worst err / bound {r:.3g}, worst |err| {float(np.max(err)) if np.size(err) else 0:.3g}")
    return r


def _in(a, device, off=0):
    """a on the device, its base address `off` floats past a 16-byte boundary."""
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a)
    buf = torch.empty(a.size + 8, dtype=t.dtype, device=device)
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def _out(shape, device, dtype=np.float32):
    """(view, whole buffer): sentinel-filled, a guard band behind the view."""
    import torch
    n = int(np.prod(shape))
    td, s = (torch.float32, SENT) if dtype == np.float32 else (torch.int32, ISENT)
    buf = torch.full((n + GUARD,), s, dtype=td, device=device)
    return buf[:n].view(tuple(shape)), buf


def _get(pair, what):
    """The output as numpy, after checking the guard band and that no sentinel is left."""
    view, buf = pair
    a = buf.cpu().numpy()
    n = a.size - GUARD
    s = SENT if a.dtype == np.float32 else ISENT
    assert (a[n:] == s).all(), f"{what}: wrote past its {n} outputs"
    left = int((a[:n] == s).sum())
    assert left == 0, f"{what}: {left} of {n} outputs left unwritten"
    return a[:n].reshape(tuple(view.shape))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, ref, what):
    ref = np.asarray(ref, np.float32)
    bad = (_bits(got) != _bits(ref).reshape(got.shape)) & ~(np.isnan(got) & np.isnan(ref).reshape(got.shape))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ in bits " \
                          f"(first: got {got[bad][0]!r}, ref {ref.reshape(got.shape)[bad][0]!r})"


def _equal(got, ref64, what):
    """got (fp32) equals the float64 reference as a value (-0 == +0)."""
    bad = got.astype(np.float64) != np.asarray(ref64).reshape(got.shape)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ " \
                          f"(first: got {got[bad][0]!r}, ref {np.asarray(ref64).reshape(got.shape)[bad][0]!r})"


def _within(got, ref, bound, what, kernel):
    err = np.abs(got.astype(np.float64) - np.asarray(ref).reshape(got.shape))
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    r = _note(kernel, err, np.maximum(bound, 1e-300))
    bad = err > bound
    assert not bad.any(), f"{what} ({kernel}): {int(bad.sum())} of {bad.size} elements outside the bound, " \
                          f"worst err / bound {r:.3g}"


def _draw(rng, shape, exact, scale=1.0):
    if exact:
        return rng.integers(-2, 3, size=shape).astype(np.float32)
    return (scale * rng.standard_normal(shape)).astype(np.float32)


def _specials(rng, x):
    """+-0, +-Inf, NaN and -FLT_MAX scattered over x, a plane of signed zeros and an all-NaN window."""
    f = x.reshape(-1)
    n = f.size
    for v, d in ((0.0, 20), (-0.0, 20), (np.nan, 60), (np.inf, 90), (-np.inf, 90), (-R.FLT_MAX, 90)):
        f[rng.integers(0, n, size=max(n // d, 1))] = v
    x[0, 0] = -0.0
    x[0, 0, ::2, 1::2] = 0.0
    x[-1, -1, :6, :6] = np.nan
    return x


# ------------------------------------------------------------------ pooling
def _run_pool(i, cs, exact, device):
    from rramsim import ops
    rng = np.random.default_rng(9000 + i)
    g = geom(cs)
    N, C, H, W, PH, PW = g[:6]
    kh, kw, sh, sw, ph, pw = g[6:]
    win = (kh, kw, sh, sw, ph, pw)
    method, relu = cs["method"], cs["relu"]
    fwd = name(cs["ids"][0])
    x = _draw(rng, cs["x"], exact)
    if exact and method == MAX:
        x = _specials(rng, x)
    xd = _in(x, device, cs["off"])
    y = _out((N, C, PH, PW), device)
    m = _out((N, C, PH, PW), device, np.int32) if cs["mask"] else None
    if relu:
        ops.pool_relu_fwd(xd, y[0], m and m[0], g, method, SLOPE)
    else:
        ops.pool_fwd(xd, y[0], m and m[0], g, method)
    got = _get(y, "y")
    if method == MAX:
        ref, mi = R.maxpool_scan(x, *win)
        _same_bits(got, R.relu64(ref, SLOPE) if relu else ref, "MAX y")      # comparisons only: both passes
        if m is not None:
            assert np.array_equal(_get(m, "mask"), mi), "MAX mask"
    else:
        ref, scale = R.avepool64(x, *win)
        mi = None
        if exact:
            r32 = ref.astype(np.float32)
            _equal(got, R.relu64(r32, SLOPE) if relu else r32, "AVE y")
        else:
            _within(got, R.relu64(ref, SLOPE) if relu else ref, (kh * kw + 1) * U * scale, "AVE y", fwd)
    if not cs["bwd"]:
        return
    dy = _draw(rng, (N, C, PH, PW), exact)
    dx = _out(cs["x"], device)
    md = _in(mi, device) if method == MAX else None
    ry = np.where(np.isnan(x), np.float32(-1.0), x)          # the ReLU output the factor is read from
    if relu:
        ops.pool_relu_bwd(_in(dy, device), md, dx[0], g, method, _in(ry, device), SLOPE)
    else:
        ops.pool_bwd(_in(dy, device), md, dx[0], g, method)
    gdx = _get(dx, "dx")
    if method == MAX:
        rdx, sc = R.maxpool_bwd64(dy, mi, H, W)
    else:
        rdx, sc = R.avepool_bwd64(dy, H, W, *win)
    if relu:
        f = R.relu_bwd_factor(ry.astype(np.float64), SLOPE)
        rdx, sc = rdx * f, sc * f
    if exact and method == MAX:
        _equal(gdx, rdx, "MAX dx")                           # integer sums: exact in any order
    else:
        terms = -(-kh // sh) * -(-kw // sw)                  # windows covering one element
        _within(gdx, rdx, (terms + 1) * U * sc, "dx", cs["bwd"][0] + (":ave" if method == AVE else ":max"))


# ---------------------------------------------------------------------- LRN
def _rel(ref, rtol, atol):
    return atol + rtol * np.abs(ref)


def _run_lrn(i, cs, exact, device):
    from rramsim import ops
    rng = np.random.default_rng(9000 + i)
    N, C, H, W = cs["x"]
    size, alpha, beta, k = cs["size"], 0.3, 0.75, 1.5
    x = _draw(rng, cs["x"], exact, 2.0)
    y = _out(cs["x"], device)
    sc = _out(cs["x"], device) if cs["scale"] else None
    ops.lrn_fwd(_in(x, device), y[0], sc and sc[0], N, C, H, W, size, alpha, beta, k)
    s64, y64 = R.lrn_scale64(x, size, alpha, k), R.lrn64(x, size, alpha, beta, k)
    _within(_get(y, "y"), y64, _rel(y64, 2e-5, 1e-6), "y", cs["ids"][0])
    if sc is not None:
        _within(_get(sc, "scale"), s64, _rel(s64, 2e-5, 1e-6), "scale", cs["ids"][0] + ":scale")
    if not cs["bwd"]:
        return
    dy = _draw(rng, cs["x"], exact)
    y32, s32 = y64.astype(np.float32), s64.astype(np.float32)
    dx = _out(cs["x"], device)
    ops.lrn_bwd(_in(x, device), _in(y32, device), _in(s32, device), _in(dy, device), dx[0], N, C, H, W, size, alpha, beta)
    rdx, scale = R.lrn_bwd64(x, y32, s32, dy, size, alpha, beta)
    _within(_get(dx, "dx"), rdx, 1e-4 * scale + 1e-5, "dx", "lrn_bwd")


def _run_within(i, cs, exact, device):
    from rramsim import ops
    rng = np.random.default_rng(9000 + i)
    N, C, H, W = cs["x"]
    size, alpha, beta = cs["size"], 0.3, 0.75
    x = _draw(rng, cs["x"], exact, 2.0)
    y, sc = _out(cs["x"], device), _out(cs["x"], device)
    ops.lrn_within_fwd(_in(x, device), y[0], sc[0], N, C, H, W, size, alpha, beta)
    y64, s64 = R.lrn_within64(x, size, alpha, beta)
    _within(_get(y, "y"), y64, _rel(y64, 2e-5, 1e-6), "y", "lrn_within_fwd")
    _within(_get(sc, "scale"), s64, _rel(s64, 2e-5, 1e-6), "scale", "lrn_within_fwd:scale")
    y0 = _out(cs["x"], device)                               # scale = NULL: the same y
    ops.lrn_within_fwd(_in(x, device), y0[0], None, N, C, H, W, size, alpha, beta)
    _same_bits(_get(y0, "y without scale"), _get(y, "y"), "y without scale")
    dy = _draw(rng, cs["x"], exact)
    s32 = s64.astype(np.float32)
    dx = _out(cs["x"], device)
    args = (_in(x, device), _in(s32, device), _in(dy, device), dx[0], N, C, H, W, size, alpha, beta)
    if cs["relu"]:
        ops.lrn_within_relu_bwd(*args, SLOPE)
    else:
        ops.lrn_within_bwd(*args)
    rdx, scale = R.lrn_within_bwd64(x, s32, dy, size, alpha, beta)
    if cs["relu"]:
        f = R.relu_bwd_factor(x.astype(np.float64), SLOPE)
        rdx, scale = rdx * f, scale * f
    _within(_get(dx, "dx"), rdx, 1e-4 * scale + 1e-5, "dx", cs["ids"][1])


# ------------------------------------------------------------------ softmax
def _run_softmax(i, cs, exact, device):
    from rramsim import ops
    rng = np.random.default_rng(9000 + i)
    outer, C, inner = cs["outer"], cs["C"], cs["inner"]
    x = _draw(rng, (outer, C, inner), exact, 3.0)
    if not exact:                     # the max subtraction: large logits, an all-equal column, -Inf entries
        x[0, :, 0] *= 80.0 / 3.0
        x[1, :, 0] *= 1e4 / 3.0
        x[2, :, 0] = 1.25
        x[3, 1::2, 0] = -np.inf
        x[4, :-1, -1] = -np.inf
    y = _out((outer, C, inner), device)
    ops.softmax_fwd(_in(x, device), y[0], outer, C, inner)
    got = _get(y, "y")
    ref = R.softmax64(x)
    _within(got, ref, _rel(ref, 1e-5, 1e-7), "y", cs["ids"][0])
    s = got.astype(np.float64).sum(axis=1)
    assert np.abs(s - 1.0).max() <= (C / 64 + 8) * U, f"a column sums to 1 {np.abs(s - 1.0).max():+.3g}"


def _probs(rng, cs, exact):
    """(prob fp32 [G * outer, C, inner], label fp32 [G * outer, inner])."""
    outer, C, inner = cs["G"] * cs["outer"], cs["C"], cs["inner"]
    if exact:                         # multiples of 1/8 summing to 1: p - 1 and its product with the scale are exact
        p = rng.multinomial(8, np.full(C, 1.0 / C), size=(outer, inner)).transpose(0, 2, 1) / 8.0
    else:
        p = R.softmax64(3.0 * rng.standard_normal((outer, C, inner)))
    p = np.ascontiguousarray(p, np.float32)
    lab = rng.integers(0, C, size=(outer, inner))
    if cs["ignore"] >= 0:
        lab[rng.random(lab.shape) < 0.3] = cs["ignore"]
        lab[0, 0] = (cs["ignore"] + 1) % C
    if cs["data"] == "all_ignored":
        lab[:] = cs["ignore"]
    if cs["data"] == "clamp":
        np.put_along_axis(p, lab[:, None, :], 0.0, 1)
    return p, lab.astype(np.float32)


def _fold(out, live, sum0):
    """k_fold_groups: acc_sum += v_g in group order, in fp32."""
    s = np.float32(sum0)
    for g in range(live):
        s = np.float32(s + out[g])
    return s


def _run_loss(i, cs, exact, device):
    import torch
    from rramsim import ops
    rng = np.random.default_rng(9000 + i)
    outer, C, inner, ig, form, G = cs["outer"], cs["C"], cs["inner"], cs["ignore"], cs["form"], cs["G"]
    p, lab = _probs(rng, cs, exact)
    pd, ld = _in(p, device), _in(lab, device)
    lw = 1.0 if exact else 0.7
    loss = _out((G,), device)
    dx = _out(p.shape, device)
    if form == "fwd":
        ops.softmax_loss_fwd(pd, ld, loss[0], outer, C, inner, ig)
    elif form == "fwd_bwd":
        ops.softmax_loss_fwd_bwd(pd, ld, loss[0], dx[0], outer, C, inner, ig, lw)
    elif form == "bwd":
        ops.softmax_loss_bwd(pd, ld, dx[0], outer, C, inner, ig, lw)
    else:
        acc = torch.full((1,), 0.5, device=device) if cs["fold"] else None
        rows = _out((2 * G,), device) if cs["fold"] else None
        ops.softmax_loss_fwd_groups(pd, ld, loss[0], G, outer, C, inner, ig, acc, rows and rows[0], 2, cs["live"])
    if form != "bwd":
        got = _get(loss, "loss")
        for g in range(G):
            sl = slice(g * outer, (g + 1) * outer)
            ref, scale, valid = R.softmax_loss64(p[sl], lab[sl], ig)
            if valid == 0:
                assert got[g] == 0.0, "every label ignored: the loss is exactly 0"
            _within(got[g:g + 1], ref, 1e-5 * scale, "loss", cs["ids"][0])
            if cs["data"] == "clamp":
                _within(got[g:g + 1], -np.log(R.FLT_MIN), 1e-5 * -np.log(R.FLT_MIN), "clamped loss", cs["ids"][0])
        if form == "fwd_groups" and cs["fold"]:
            assert acc.cpu().numpy()[0] == _fold(got, cs["live"], 0.5)
            r = rows[1].cpu().numpy()
            assert (r[2 * G:] == SENT).all()
            want = np.full(2 * G, SENT, np.float32)
            want[0:2 * cs["live"]:2] = got[:cs["live"]]
            _same_bits(r[:2 * G], want, "acc_rows")
    if form in ("bwd", "fwd_bwd"):
        gdx = _get(dx, "dx")
        rdx, scale = R.softmax_loss_bwd64(p, lab, ig, lw)
        if cs["data"] == "all_ignored":
            assert not gdx.any(), "every label ignored: the gradient is exactly 0"
        if exact:
            _same_bits(gdx, rdx.astype(np.float32) + np.float32(0.0), "dx")
        else:
            _within(gdx, rdx, 1e-5 * scale, "dx", cs["ids"][-1] + ":dx")


def test_softmax_loss_fwd_bwd_refuses_65537(device):
    import torch
    from rramsim import _kernels as K
    from rramsim import ops
    p, lab = torch.full((65537,), 1.0, device=device), torch.zeros(65537, device=device)
    loss, dx = _out((1,), device), _out((65537,), device)
    with pytest.raises(K.RramError, match="more than 65536"):
        ops.softmax_loss_fwd_bwd(p, lab, loss[0], dx[0], 65537, 1, 1)
    assert (loss[1].cpu().numpy() == SENT).all() and (dx[1].cpu().numpy() == SENT).all()


# ----------------------------------------------------------------- accuracy
def _run_acc(i, cs, exact, device):
    import torch
    from rramsim import ops
    rng = np.random.default_rng(9000 + i)
    outer, C, inner, G = cs["outer"], cs["C"], cs["inner"], max(cs["G"], 1)
    x = _draw(rng, (G * outer, C, inner), exact)
    lab = rng.integers(0, C, size=(G * outer, inner))
    lab[::3] = C - 1 - x[::3, ::-1].argmax(axis=1)        # a share of hits: the last maximum (ties rank by index)
    if cs["ignore"] >= 0:
        lab[rng.random(lab.shape) < 0.3] = cs["ignore"]
    cor, cnt = _out((G,), device), _out((G,), device)
    rat = _out((G,), device) if cs["ratio"] else None
    xd, ld = _in(x, device), _in(lab.astype(np.float32), device)
    if cs["G"]:
        acc = torch.full((1,), 0.5, device=device) if cs["fold"] else None
        rows = _out((2 * G,), device) if cs["fold"] else None
        ops.accuracy_groups(xd, ld, cor[0], cnt[0], rat[0], G, outer, C, inner, cs["top_k"], cs["ignore"], acc,
                            rows and rows[0], 2, cs["live"])
    else:
        ops.accuracy(xd, ld, cor[0], cnt[0], outer, C, inner, cs["top_k"], cs["ignore"], rat and rat[0])
    gc, gn = _get(cor, "correct"), _get(cnt, "count")
    want = [R.accuracy64(x[g * outer:(g + 1) * outer], lab[g * outer:(g + 1) * outer], cs["top_k"], cs["ignore"])
            for g in range(G)]
    assert [(float(a), float(b)) for a, b in zip(gc, gn)] == [(float(a), float(b)) for a, b in want]
    assert 0 < sum(a for a, _ in want) < sum(b for _, b in want)      # hits and misses both occur
    if rat is not None:
        gr = _get(rat, "ratio")
        _same_bits(gr, np.array([np.float32(a) / np.float32(max(b, 1)) for a, b in want], np.float32), "ratio")
        if cs["G"] and cs["fold"]:
            assert acc.cpu().numpy()[0] == _fold(gr, cs["live"], 0.5)
            r = rows[1].cpu().numpy()
            w = np.full(2 * G + GUARD, SENT, np.float32)
            w[0:2 * cs["live"]:2] = gr[:cs["live"]]
            _same_bits(r, w, "acc_rows")


# -------------------------------------------------------------- elementwise
def _run_relu(i, cs, exact, device):
    from rramsim import ops
    rng = np.random.default_rng(9000 + i)
    n = cs["n"]
    x, dy = _draw(rng, (n,), exact), _draw(rng, (n,), exact)
    x[:8] = [0.0, -0.0, np.inf, -np.inf, R.FLT_MAX, -R.FLT_MAX, 1e-45, -1e-45]
    for slope in (0.0, SLOPE):
        y, dx = _out((n,), device), _out((n,), device)
        ops.relu_fwd(_in(x, device), y[0], slope)
        ops.relu_bwd(_in(x, device), _in(dy, device), dx[0], slope)
        _same_bits(_get(y, "y"), R.relu64(x, slope), "relu y")
        _same_bits(_get(dx, "dx"), (dy * R.relu_bwd_factor(x.astype(np.float64), slope)).astype(np.float32), "relu dx")


def _run_concat(i, cs, exact, device):
    from rramsim import ops
    rng = np.random.default_rng(9000 + i)
    num, sci, dci, off = cs["num"], cs["sci"], cs["dci"], cs["off"]
    src = _draw(rng, (num, sci), exact)
    dst = _out((num, dci), device)
    ops.concat_copy(_in(src, device), dst[0], num, sci, dci, off)
    got = dst[1].cpu().numpy()
    want = np.full((num, dci), SENT, np.float32)
    want[:, off:off + sci] = src
    _same_bits(got[:num * dci], want, "concat top")
    assert (got[num * dci:] == SENT).all()
    top = _draw(rng, (num, dci), exact)
    back = _out((num, sci), device)
    ops.concat_copy(back[0], _in(top, device), num, sci, dci, off, backward=True)
    _same_bits(_get(back, "bottom diff"), top[:, off:off + sci], "concat bottom diff")


def _run_i32(i, cs, exact, device):
    from rramsim import ops
    rng = np.random.default_rng(9000 + i)
    x = rng.integers(-2 ** 31, 2 ** 31, size=cs["n"], dtype=np.int64).astype(np.int32)
    x[:6] = [0, -1, 2 ** 31 - 1, -2 ** 31, 2 ** 24 + 1, -(2 ** 24) - 3]
    if exact:
        x[6:] = x[6:] >> 12                                 # argmax-sized values: exactly representable
    y = _out((cs["n"],), device)
    ops.i32_to_f32(_in(x, device), y[0])
    _same_bits(_get(y, "y"), x.astype(np.float32), "i32 -> f32")


def _run_euclidean(i, cs, exact, device):
    from rramsim import ops
    rng = np.random.default_rng(9000 + i)
    n, num = cs["n"], cs["num"]
    a, b = _draw(rng, (n,), exact), _draw(rng, (n,), exact)
    diff, loss, dx = _out((n,), device), _out((1,), device), _out((n,), device)
    ops.euclidean_loss_fwd(_in(a, device), _in(b, device), diff[0], loss[0], num)
    d64 = a.astype(np.float64) - b.astype(np.float64)
    gd = _get(diff, "diff")
    _same_bits(gd, d64.astype(np.float32) + np.float32(0.0), "diff")
    d = gd.astype(np.float64)
    ref = (d * d).sum() / num / 2.0
    if exact:
        _equal(_get(loss, "loss"), np.float64(np.float32(np.float32((d * d).sum()) / np.float32(num)) / np.float32(2)),
               "loss")                                       # an integer sum below 2^24: only the division rounds
    _within(_get(loss, "loss"), ref, 1e-5 * ref, "loss", "euclidean_fwd")
    alpha = np.float32(-0.7 / num)
    ops.euclidean_loss_bwd(diff[0], dx[0], float(alpha))
    _same_bits(_get(dx, "dx"), (np.float64(alpha) * d).astype(np.float32), "dx")


RUN = {"pool": _run_pool, "lrn": _run_lrn, "within": _run_within, "softmax": _run_softmax, "loss": _run_loss,
       "acc": _run_acc, "relu": _run_relu, "concat": _run_concat, "i32_to_f32": _run_i32, "euclidean": _run_euclidean}


@pytest.mark.parametrize("mode", PASSES)
@pytest.mark.parametrize("i", range(len(LAYER_CASES)), ids=IDS)
def test_layer_kernel(device, i, mode):
    cs = LAYER_CASES[i]
    assert ids_of(cs) == want_ids(cs)       # the kernels these calls launch
    RUN[cs["entry"]](i, cs, mode == "exact", device)


def test_worst_errors_report(device):
    """Runs last in this file: the worst err / bound per float kernel over all cases (pytest -s)."""
    for k in sorted(WORST):
        print(f"layer-matrix-summary {k}: {WORST[k]:.3g} of its bound")
    assert all(v <= 1.0 for v in WORST.values())
