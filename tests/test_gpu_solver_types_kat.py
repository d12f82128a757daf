"""The reference's least-squares known-answer tests for the Nesterov, AdaGrad,
RMSProp, AdaDelta and Adam solvers, on the reference's own data.

src/caffe/test/test_gradient_based_solver.cpp runs, for each solver class,
the cases test_gpu_solver_kat.py restates for SGD: K iterations, the analytic
(K+1)th update from the net's own state (ComputeLeastSquaresUpdate, :224-347;
the per-type expressions at :296-334), K+1 iterations of the solver, and the
comparison at max(1e-7, 1e-2 * min(|expected|, |got|)) (:349-371).  The
parameter sets are each class's: AdaGrad :710-748, Nesterov :810-882, AdaDelta
:943-1011, Adam :1077-1113 (momentum2 0.999), RMSProp :1177-1216 (rms_decay
0.95).  Also per class: the history count (:290-295), accumulation
(CheckAccumulation, iter_size 2 against batch 4), snapshot -> restore ->
continue bit for bit (TestSnapshot, k = 1..4), and the constructor refusals.
The analytic update is evaluated in float64.
"""
from pathlib import Path

import numpy as np
import pytest

from test_gpu_solver_kat import D, NUM, _ip_params, _list_file, _near, net_proto

pytestmark = pytest.mark.gpu

DELTA = 1e-8            # SolverParameter's default (caffe.proto:217), the reference tests' delta_
MOMENTUM2 = 0.999       # AdamSolverTest::InitSolver (:1069)
RMS_DECAY = 0.95        # RMSPropSolverTest::InitSolver (:1168)
KINDS = ["Nesterov", "AdaGrad", "RMSProp", "AdaDelta", "Adam"]


def solver_proto(kind, lr, wd, mom, max_iter, iter_size=1, snapshot=0, prefix=None, fmt=None, legacy=False):
    s = f'max_iter: {max_iter} base_lr: {lr} lr_policy: "fixed" iter_size: {iter_size} random_seed: 1701\n'
    s += f"solver_type: {kind.upper()}\n" if legacy else f'type: "{kind}"\n'
    if wd != 0:
        s += f"weight_decay: {wd}\n"
    if kind == "Adam":                              # AdamSolverTest::InitSolver: momentum 0.9, momentum2 0.999
        s += f"momentum: 0.9 momentum2: {MOMENTUM2}\n"
    elif mom != 0:
        s += f"momentum: {mom}\n"
    if kind == "RMSProp":
        s += f"rms_decay: {RMS_DECAY}\n"
    if prefix:
        s += f'snapshot_prefix: "{prefix}/"\n'
    if snapshot:
        s += f"snapshot: {snapshot}\n"
    if fmt:
        s += f"snapshot_format: {fmt}\n"
    return s


def _solver(tmp_path, kind, lr, wd, mom, iters, iter_size=1, share=False, **kw):
    from rramsim import caffe
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    return caffe.Solver(solver_proto(kind, lr, wd, mom, iters, iter_size, **kw),
                        net_proto(_list_file(tmp_path), NUM // iter_size, share))


def _flat(blobs):
    return np.concatenate([b.cpu().numpy().reshape(-1) for b in blobs]).astype(np.float64)


def compute_update(s, kind, lr, wd, mom, num_iters):
    """ComputeLeastSquaresUpdate (:224-347) for solver class `kind`, float64."""
    net = s.net
    net.forward()
    X = net.blob("data").cpu().numpy().astype(np.float64).reshape(NUM, D)
    y = net.blob("targets").cpu().numpy().astype(np.float64).reshape(NUM)
    w, b = _ip_params(s)
    hist = s.history()
    assert len(hist) == (4 if kind in ("AdaDelta", "Adam") else 2)      # :290-295
    h = _flat(hist[:2])
    Xa = np.concatenate([X, np.ones((NUM, 1))], axis=1)
    wa = np.concatenate([w, b])
    grad = (Xa.T @ (Xa @ wa) - Xa.T @ y) / NUM + wd * wa
    update = lr * grad
    temp = mom * h
    if kind == "Nesterov":                                              # :303-306
        update = (1 + mom) * (update + temp) - temp
    elif kind == "AdaGrad":                                             # :307
        update = update / (np.sqrt(h + grad * grad) + DELTA)
    elif kind == "RMSProp":                                             # :309-311
        update = update / (np.sqrt(RMS_DECAY * h + grad * grad * (1 - RMS_DECAY)) + DELTA)
    elif kind == "AdaDelta":                                            # :313-319
        uh = _flat(hist[2:4])
        avg = mom * h + (1 - mom) * (grad * grad)
        update = grad * np.sqrt((uh + DELTA) / (avg + DELTA)) * lr
    elif kind == "Adam":                                                # :324-334
        v = _flat(hist[2:4])
        val_m = (1 - mom) * grad + mom * h
        val_v = (1 - MOMENTUM2) * grad * grad + MOMENTUM2 * v
        alpha_t = lr * np.sqrt(1 - MOMENTUM2 ** num_iters) / (1 - mom ** num_iters)
        update = alpha_t * val_m / (np.sqrt(val_v) + DELTA)
    else:
        raise AssertionError(kind)
    return wa - update


def least_squares_case(tmp_path, kind, lr=1.0, wd=0.0, mom=0.0, iter_to_check=0, share=False):
    """TestLeastSquaresUpdate (:453-488), devices = 1."""
    s = _solver(tmp_path, kind, lr, wd, mom, iter_to_check, share=share)
    assert s.type == kind
    s.step(iter_to_check)
    expected = compute_update(s, kind, lr, wd, mom, iter_to_check + 1)
    s.close()
    s = _solver(tmp_path, kind, lr, wd, mom, iter_to_check + 1, share=share)
    s.step(iter_to_check + 1)
    _near(expected, np.concatenate(_ip_params(s)))                      # CheckLeastSquaresUpdate :349-371
    s.close()


# (lr, wd, mom, iterations checked, share) per reference test
CASES = {
    "AdaGrad": [(1.0, 0.0, 0.0, [0], False),                            # :710-712
                (0.01, 0.0, 0.0, [0], False),                           # :714-718
                (0.01, 0.5, 0.0, [0], False),                           # :720-725
                (0.01, 0.5, 0.0, range(5), False),                      # :727-736
                (0.01, 0.5, 0.0, range(5), True)],                      # :738-748
    "Nesterov": [(1.0, 0.0, 0.0, [0], False),                           # :810-812
                 (0.01, 0.0, 0.0, [0], False),                          # :814-818
                 (0.01, 0.5, 0.0, [0], False),                          # :820-825
                 (0.01, 0.5, 0.0, range(5), False),                     # :827-837
                 (0.01, 0.0, 0.5, range(2), False),                     # :839-848
                 (0.01, 0.0, 0.5, range(5), False),                     # :850-859
                 (0.01, 0.5, 0.9, range(5), False),                     # :861-870
                 (0.01, 0.5, 0.9, range(5), True)],                     # :872-882
    "AdaDelta": [(0.1, 0.0, 0.0, [0], False),                           # :943-947
                 (0.1, 0.5, 0.95, [0], False),                          # :949-955
                 (0.1, 0.0, 0.5, [0], False),                           # :957-966
                 (0.1, 0.0, 0.95, [0], False),                          # :968-977
                 (0.1, 0.0, 0.95, range(5), False),                     # :979-988
                 (0.1, 0.1, 0.95, range(5), False),                     # :990-999
                 (0.1, 0.1, 0.95, range(5), True)],                     # :1001-1011
    "Adam": [(0.01, 0.0, 0.9, [0], False),                              # :1077-1083
             (0.01, 0.5, 0.9, [0], False),                              # :1085-1091
             (0.01, 0.5, 0.9, range(5), False),                         # :1093-1102
             (0.01, 0.5, 0.9, range(5), True)],                         # :1104-1113
    "RMSProp": [(1.0, 0.5, 0.0, [0], False),                            # :1177-1182
                (0.01, 0.0, 0.0, range(5), False),                      # :1184-1193
                (0.01, 0.5, 0.0, range(5), False),                      # :1195-1204
                (0.01, 0.5, 0.0, range(5), True)],                      # :1206-1216
}
# each class's "everything" set: accumulation and snapshot run with it
EVERYTHING = {"AdaGrad": (0.01, 0.5, 0.0), "Nesterov": (0.01, 0.5, 0.9), "AdaDelta": (0.1, 0.1, 0.95),
              "Adam": (0.01, 0.5, 0.9), "RMSProp": (0.01, 0.5, 0.0)}


@pytest.mark.parametrize("kind", KINDS)
def test_least_squares_update(device, tmp_path, kind):
    for lr, wd, mom, iters, share in CASES[kind]:
        for i in iters:
            least_squares_case(tmp_path, kind, lr, wd, mom, i, share)


@pytest.mark.parametrize("kind", ["SGD"] + KINDS)
def test_history_count(device, tmp_path, kind):
    """:290-295: 2 history blobs, 4 for AdaDelta and Adam (zero before the first step)."""
    s = _solver(tmp_path, kind, 0.01, 0.0, 0.0, 1)
    hist = s.history()
    assert len(hist) == (4 if kind in ("AdaDelta", "Adam") else 2)
    assert [h.numel() for h in hist] == [D, 1] * (len(hist) // 2)
    assert all(not h.cpu().numpy().any() for h in hist)
    s.close()


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_accumulation(device, tmp_path, kind, share):
    """CheckAccumulation (:399-436): 4 iterations at batch 4 == 4 iterations of
    iter_size 2 at batch 2 (the unfused path: iter_size > 1)."""
    lr, wd, mom = EVERYTHING[kind]
    s = _solver(tmp_path, kind, lr, wd, mom, 4, share=share)
    s.step(4)
    ref = np.concatenate(_ip_params(s))
    s.close()
    s = _solver(tmp_path, kind, lr, wd, mom, 4, iter_size=2, share=share)
    s.step(4)
    _near(ref, np.concatenate(_ip_params(s)))
    s.close()


@pytest.mark.parametrize("kind,fmt", [("Nesterov", None), ("AdaGrad", None), ("RMSProp", None),
                                      ("AdaDelta", "HDF5"), ("Adam", None)])
def test_snapshot(device, tmp_path, kind, fmt):
    """TestSnapshot (:490-558), k = 1..4: params, diffs and every history blob
    bit for bit after snapshot -> restore -> continue; AdaDelta through HDF5."""
    lr, wd, mom = EVERYTHING[kind]
    for k in range(1, 5):
        s = _solver(tmp_path, kind, lr, wd, mom, 2 * k)
        s.step(2 * k)
        ref_p = [(p["data"].cpu().numpy().copy(), p["diff"].cpu().numpy().copy()) for p in s.net.params()]
        ref_h = [h.cpu().numpy().copy() for h in s.history()]
        s.close()
        prefix = Path(tmp_path) / f"snap{kind}{k}"
        prefix.mkdir()
        s = _solver(tmp_path, kind, lr, wd, mom, k, snapshot=k, prefix=str(prefix), fmt=fmt)
        s.step(k)
        s.close()
        state = prefix / (f"_iter_{k}.solverstate" + (".h5" if fmt == "HDF5" else ""))
        assert state.exists(), list(prefix.iterdir())
        s = _solver(tmp_path, kind, lr, wd, mom, 2 * k)
        s.restore(str(state))
        for _ in range(s.iter):                                     # advance the data layer (:188-190)
            s.net.forward()
        s.solve()
        hist = s.history()
        assert len(hist) == len(ref_h) == (4 if kind in ("AdaDelta", "Adam") else 2)
        for (d0, g0), p in zip(ref_p, s.net.params()):
            assert np.array_equal(d0.view(np.uint32), p["data"].cpu().numpy().view(np.uint32))
            assert np.array_equal(g0.view(np.uint32), p["diff"].cpu().numpy().view(np.uint32))
        for h0, h in zip(ref_h, hist):
            assert np.array_equal(h0.view(np.uint32), h.cpu().numpy().view(np.uint32))
        s.close()


def _refused(tmp_path, text):
    from rramsim import caffe
    from rramsim._kernels import RramError
    caffe.set_stream_from_torch()
    with pytest.raises((RramError, RuntimeError)) as ei:
        caffe.Solver('max_iter: 1 base_lr: 0.01 lr_policy: "fixed"\n' + text, net_proto(_list_file(tmp_path), NUM))
    return str(ei.value)


def test_refusals_name_their_cause(device, tmp_path):
    """sgd_solvers.hpp:77,97-101 and the type / solver_type pair."""
    assert "Momentum cannot be used with AdaGrad" in _refused(tmp_path, 'type: "AdaGrad" momentum: 0.9')
    assert "rms_decay" in _refused(tmp_path, 'type: "RMSProp" rms_decay: 1.0')
    msg = _refused(tmp_path, 'type: "Adam" solver_type: SGD')
    assert "Adam" in msg and "SGD" in msg and "solver_type" in msg
    assert "Bogus" in _refused(tmp_path, 'type: "Bogus"')


def test_legacy_solver_type_enum(device, tmp_path):
    """caffe.proto:233-242: the deprecated enum alone selects the class."""
    from rramsim import caffe
    caffe.set_stream_from_torch()
    s = caffe.Solver(solver_proto("Adam", 0.01, 0.0, 0.9, 1, legacy=True), net_proto(_list_file(tmp_path), NUM))
    assert s.type == "Adam" and len(s.history()) == 4
    s.close()
    s = caffe.Solver('max_iter: 1 base_lr: 0.01 lr_policy: "fixed"', net_proto(_list_file(tmp_path), NUM))
    assert s.type == "SGD"
    s.close()
