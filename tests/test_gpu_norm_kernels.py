"""The kernels of csrc/norm.hip against float64 (tests/_norm_cases.py holds
the cases, their inputs and the reference arithmetic).  The bounds come from
tests/golden/norm_bounds.json (tests/golden/make_norm_bounds.py: 8 x the error
of a float32 restatement of the reference's order of operations, floored at
4 ulp), never from the kernels under test."""
import json
from pathlib import Path

import numpy as np
import pytest

import _norm_cases as nc

pytestmark = pytest.mark.gpu
BOUNDS = json.loads((Path(__file__).parent / "golden" / "norm_bounds.json").read_text())["cases"]
_REF = {}


def ref64(name):
    if name not in _REF:
        _REF[name] = nc.quantities(name, np.float64)
    return _REF[name]


def N(t):
    import torch
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def dev(a, off=0):
    """a on the device, starting `off` floats past a 16-byte boundary."""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    return t


def empty(shape, off=0):
    return dev(np.full(shape, np.nan, np.float32), off)


def close(got, want, bound, what):
    err = float(np.max(np.abs(got - want)))
    print(f"{what}: error {err:.3e}, bound {bound:.3e}")
    assert np.isfinite(got).all() and err <= bound, (what, err, bound)


def bn_train(name, off=0, y_off=None, inplace=False, fold=False, relu=False):
    """Training forward + backward of a case through the entry points; fold: gamma / beta (/ relu) in the passes."""
    import torch
    from rramsim import ops
    x, dy, gamma, beta = nc.inputs(name)
    n, c, i = x.shape
    y_off = off if y_off is None else y_off
    xd, dyd = dev(x, off), dev(dy, y_off)
    g, b = (dev(gamma), dev(beta)) if fold else (None, None)
    mean, rstd = empty((c,)), empty((c,))
    rm, rv, f = dev(np.zeros(c)), dev(np.zeros(c)), dev(np.zeros(1))
    nws = ops.norm_workspace_floats(n, c, i)
    ws = empty((nws,))
    ops.bn_stats_train(xd, mean, rstd, ws[:nws - 3 * c], nc.EPS, nc.MAF, rm, rv, f)
    xhat = empty(x.shape, y_off)
    y = xd if inplace else empty(x.shape, y_off)
    ops.norm_apply(xd, y, mean, rstd, g, b, relu, xhat_out=xhat)
    coef = ws[nws - 3 * c:]
    dg, db = (dev(np.zeros(c)), dev(np.zeros(c))) if fold else (None, None)
    ops.norm_bwd_reduce(dyd, xhat, ws[:nws - 3 * c], relu_y=y if relu else None, gamma=g, rstd=rstd, dgamma=dg,
                        dbeta=db, coef=coef)
    dx = dyd if inplace else empty(x.shape, off)
    ops.norm_bwd_apply(dyd, dx, relu_y=y if relu else None, xhat=xhat, coef=coef)
    out = dict(mean=mean, rstd=rstd, run_mean=rm, run_var=rv, factor=f, xhat=xhat, y=y, dx=dx, dgamma=dg, dbeta=db)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items() if v is not None}


def check_plain(name, got):
    r, b = ref64(name), BOUNDS[name]
    for k in ("mean", "rstd", "run_mean", "run_var", "xhat", "dx"):
        close(N(got[k]), r[k], b[k], f"{name}.{k}")
    close(N(got["y"]), r["xhat"], b["xhat"], f"{name}.y")
    assert N(got["factor"])[0] == 1.0


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_a_odd_inner_and_base_offsets(device, off):
    check_plain("a", bn_train("a", off=off))


def test_a_operands_with_different_offsets(device):
    """x and y one float apart: the scalar streaming kernels (norm_apply<1>, norm_bwd<1>)."""
    check_plain("a", bn_train("a", off=1, y_off=2))


def test_b_large_mean_small_spread(device):
    """100 + 0.1 z over 5 slices: a one-pass E[x^2] - E[x]^2 misses rstd's bound by orders of magnitude
    (norm_bounds.json one_pass_check_b)."""
    check_plain("b", bn_train("b"))


@pytest.mark.parametrize("name", ["c1", "c2", "d"])
def test_cd_fc_form(device, name):
    got = bn_train(name)
    check_plain(name, got)
    if name == "d":     # m = 1: variance 0, correction factor 1
        assert np.array_equal(N(got["run_var"]), np.zeros(4)) and np.array_equal(N(got["xhat"]).ravel(), np.zeros(4))
        assert np.allclose(N(got["rstd"]), 1.0 / np.sqrt(np.float32(nc.EPS)), rtol=1e-6)


def test_e_running_statistics_then_test_phase(device):
    from rramsim import ops
    xs, xt, _ = nc.running_sequence(np.float64)
    _, _, want = nc.running_sequence(np.float64)
    n, c, i = xs[0].shape
    rm, rv, f = dev(np.zeros(c)), dev(np.zeros(c)), dev(np.zeros(1))
    mean, rstd = empty((c,)), empty((c,))
    ws = empty((ops.norm_workspace_floats(n, c, i),))
    for x in xs:
        ops.bn_stats_train(dev(x), mean, rstd, ws, nc.EPS, nc.MAF, rm, rv, f)
    ops.bn_stats_global(rm, rv, f, mean, rstd, nc.EPS)
    y = empty(xt.shape)
    ops.norm_apply(dev(xt), y, mean, rstd)
    b = BOUNDS["e"]
    close(N(rm), want["run_mean"], b["run_mean"], "e.run_mean")
    close(N(rv), want["run_var"], b["run_var"], "e.run_var")
    close(N(f)[0], want["factor"], b["factor"], "e.factor")
    close(N(y), want["y_test"], b["y_test"], "e.y_test")


def test_e_fresh_test_phase_has_factor_zero(device):
    """factor == 0: mean = var = 0, so y = x / sqrt(eps)."""
    from rramsim import ops
    x = nc.inputs("a")[0]
    c = x.shape[1]
    mean, rstd, y = empty((c,)), empty((c,)), empty(x.shape)
    ops.bn_stats_global(dev(np.ones(c)), dev(np.ones(c)), dev(np.zeros(1)), mean, rstd, nc.EPS)
    ops.norm_apply(dev(x), y, mean, rstd)
    want = x.astype(np.float64) / np.sqrt(nc.EPS)
    close(N(y), want, 4 * nc.ulp32(np.abs(want).max()), "fresh.y")
    assert not N(mean).any()


@pytest.mark.parametrize("name", ["a", "b", "c2", "g4"])
def test_f_in_place_equals_out_of_place(device, name):
    """y == x and dx == dy: the same bits as with separate tensors, folded and unfolded."""
    for fold in (False, True):
        a, b = bn_train(name, fold=fold, relu=fold), bn_train(name, fold=fold, relu=fold, inplace=True)
        for k in ("y", "dx", "xhat", "mean", "rstd"):
            assert np.array_equal(N(a[k]).view(np.uint64), N(b[k]).view(np.uint64)), (name, fold, k)


def test_f_scale_and_sigmoid_in_place(device):
    from rramsim import ops
    x, dy, gamma, beta = nc.inputs("a")
    y, xi = empty(x.shape), dev(x)
    ops.scale_fwd(dev(x), y, dev(gamma), dev(beta))
    ops.scale_fwd(xi, xi, dev(gamma), dev(beta))
    assert np.array_equal(N(y), N(xi))
    dx, di = empty(x.shape), dev(dy)
    ops.norm_bwd_apply(dev(dy), dx, gamma=dev(gamma))
    ops.norm_bwd_apply(di, di, gamma=dev(gamma))
    assert np.array_equal(N(dx), N(di))
    sx, sdy = nc.sigmoid_inputs()
    sy, si = empty(sx.shape), dev(sx)
    ops.sigmoid_fwd(dev(sx), sy)
    ops.sigmoid_fwd(si, si)
    assert np.array_equal(N(sy), N(si))
    sdx, sdi = empty(sx.shape), dev(sdy)
    ops.sigmoid_bwd(sy, dev(sdy), sdx)
    ops.sigmoid_bwd(sy, sdi, sdi)
    assert np.array_equal(N(sdx), N(sdi))


@pytest.mark.parametrize("name", ["g", "g4", "a", "c2"])
def test_g_fold_against_three_launches(device, name):
    """gamma / beta / ReLU in the BatchNorm passes: the forward bit for bit the BatchNorm, Scale and ReLU
    launches one after the other; dx, dgamma, dbeta against float64 (gamma < 0 and gamma = 0 included)."""
    from rramsim import ops
    x, dy, gamma, beta = nc.inputs(name)
    assert gamma[0] < 0 and gamma[1] == 0
    got = bn_train(name, fold=True, relu=True)
    plain = bn_train(name)
    y3 = empty(x.shape)
    ops.scale_fwd(plain["y"], y3, dev(gamma), dev(beta))
    ops.relu_fwd(y3, y3)
    assert np.array_equal(N(got["y"]).astype(np.float32).view(np.uint32), N(y3).astype(np.float32).view(np.uint32))
    r, b = ref64(name), BOUNDS[name]
    close(N(got["y"]), r["y_fold"], b["y_fold"], f"{name}.y_fold")
    # the ReLU mask is the kernel's own y > 0; a y within its bound of 0 may fall on the other side of float64's
    flips = (N(got["y"]) > 0) != (r["y_fold"] > 0)
    assert not flips.any(), f"{name}: {flips.sum()} ReLU masks differ from float64's (an input too close to 0)"
    close(N(got["dx"]), r["dx_fold"], b["dx_fold"], f"{name}.dx_fold")
    close(N(got["dgamma"]), r["dgamma"], b["dgamma"], f"{name}.dgamma")
    close(N(got["dbeta"]), r["dbeta"], b["dbeta"], f"{name}.dbeta")
    # global statistics with the fold: dx = g gamma rstd
    dxg = empty(x.shape)
    ops.norm_bwd_apply(dev(dy), dxg, relu_y=got["y"], gamma=dev(gamma), rstd=got["rstd"])
    close(N(dxg), r["dx_global"], b["dx_global"], f"{name}.dx_global")


@pytest.mark.parametrize("name", ["a", "c2", "g4"])
def test_scale_stand_alone(device, name):
    from rramsim import ops
    x, dy, gamma, beta = nc.inputs(name)
    n, c, i = x.shape
    r, b = ref64(name), BOUNDS[name]
    y = empty(x.shape)
    ops.scale_fwd(dev(x), y, dev(gamma), dev(beta))
    close(N(y), r["scale_y"], b["scale_y"], f"{name}.scale_y")
    y2 = empty(x.shape)
    ops.scale_fwd(dev(x), y2, dev(gamma))                       # bias_term: false
    close(N(y2), r["scale_y"] - beta.astype(np.float64)[None, :, None], b["scale_y"], f"{name}.scale_y_nobias")
    dg, db, dx = dev(np.ones(c)), dev(np.ones(c)), empty(x.shape)
    ws = empty((ops.norm_workspace_floats(n, c, i),))
    ops.scale_bwd(dev(x), dev(dy), dev(gamma), ws, dgamma=dg, dbeta=db, dx=dx)
    close(N(dx), r["scale_dx"], b["scale_dx"], f"{name}.scale_dx")
    # parameter gradients accumulate, as InnerProduct's dW does
    close(N(dg) - 1.0, r["scale_dgamma"], b["scale_dgamma"] + 4 * nc.ulp32(1 + np.abs(r["scale_dgamma"]).max()), f"{name}.scale_dgamma")
    close(N(db) - 1.0, r["scale_dbeta"], b["scale_dbeta"] + 4 * nc.ulp32(1 + np.abs(r["scale_dbeta"]).max()), f"{name}.scale_dbeta")


@pytest.mark.parametrize("name", sorted(nc.BN_CASES))
def test_h_reductions_are_bit_identical_run_to_run(device, name):
    a, b = bn_train(name, fold=True, relu=True), bn_train(name, fold=True, relu=True)
    for k in ("mean", "rstd", "run_mean", "run_var", "dgamma", "dbeta", "dx"):
        assert np.array_equal(N(a[k]).view(np.uint64), N(b[k]).view(np.uint64)), (name, k)


def test_i_sigmoid(device):
    from rramsim import ops
    x, dy = nc.sigmoid_inputs()
    assert abs(x[0]) == abs(x[1]) == 100.0
    y, dx = empty(x.shape), empty(x.shape)
    ops.sigmoid_fwd(dev(x), y)
    ops.sigmoid_bwd(y, dev(dy), dx)
    wy, wdx = nc.sigmoid(x, dy, np.float64)
    close(N(y), wy, BOUNDS["sigmoid"]["y"], "sigmoid.y")
    close(N(dx), wdx, BOUNDS["sigmoid"]["dx"], "sigmoid.dx")
    assert N(y)[0] == 1.0 and N(y)[1] == 0.0 and N(y)[2] == 0.5
