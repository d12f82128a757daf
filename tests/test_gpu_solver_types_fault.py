"""Fault-aware training with every solver type: LeNet (two convolutions, two
InnerProducts), batch 8, a gaussian failure pattern and the threshold strategy.

The one-launch fused tail (rram_fused_opt_update_fail_batched, SGD one kind of
its kernel like the others) must leave the bits of the reference order
ComputeUpdate -> ApplyStrategy -> ApplyUpdate -> Fail (solver.cpp:299-305) run
as separate kernels; the types must differ from one another; a remapping
strategy takes the unfused path; hipGraph replay equals eager, Adam staying
eager because its corrected rate moves every iteration.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ["SGD", "Nesterov", "AdaGrad", "RMSProp", "AdaDelta", "Adam"]
# endurance ~ N(250, 100) at decrement 100: a cell written three times is
# broken after three iterations unless it started above 300 (SGD included)
FAIL_MEAN, FAIL_STD = 250.0, 100.0


def N(t):
    return t.detach().cpu().numpy().copy()


def _solver_text(kind, extra="", threshold=0.001, **kw):
    from rramsim import models
    mom = 0.0 if kind in ("AdaGrad", "RMSProp") else (0.95 if kind == "AdaDelta" else 0.9)
    sp = models.solver(base_lr=0.01, momentum=mom, weight_decay=0.0005, max_iter=100, failure_mean=FAIL_MEAN,
                       failure_std=FAIL_STD, failure_prob=(5, 90, 5), threshold=threshold, **kw)
    return sp + f'type: "{kind}"\n' + extra


def _train(kind, iters, fused=True, graph=False, extra="", threshold=0.001):
    from rramsim import caffe, models
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    s = caffe.Solver(_solver_text(kind, extra, threshold), models.lenet(train_batch=8, test_batch=8),
                     dict(models.net_options("lenet"), fused_update=fused))
    assert s.type == kind
    if graph:
        s.set_graph(True)
    for n in iters:
        s.step(n)
    fs = s.fail_state()
    st = dict(params=[N(p["data"]) for p in s.net.params()], hist=[N(h) for h in s.history()],
              endurance=[N(e) for e, v in fs], stuck=[N(v) for e, v in fs], broken=s.broken_counts(),
              graph_active=s.graph_active())
    s.close()
    return st


def _same_bits(a, b):
    for key in ("params", "hist", "endurance", "stuck"):
        assert len(a[key]) == len(b[key]), key
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (key, i)
    assert a["broken"] == b["broken"]


@pytest.fixture(scope="module")
def fused_runs(device):
    """3 fused iterations per solver type, computed once."""
    return {k: _train(k, [3], fused=True) for k in KINDS}


@pytest.mark.parametrize("kind", KINDS)
def test_fused_equals_unfused(device, fused_runs, kind):
    got = fused_runs[kind]
    ref = _train(kind, [3], fused=False)
    n = len(ref["params"])
    assert len(ref["hist"]) == (2 * n if kind in ("AdaDelta", "Adam") else n)
    _same_bits(got, ref)
    assert any(c > 0 for c in got["broken"]), got["broken"]
    assert all(np.isfinite(p).all() for p in got["params"])


def test_kinds_differ(device):
    """After one iteration any two types' weights differ somewhere (a type
    silently falling back to SGD, or to another type, cannot pass)."""
    one = {k: _train(k, [1], fused=True)["params"] for k in KINDS}
    for i, a in enumerate(KINDS):
        for b in KINDS[i + 1:]:
            assert any(not np.array_equal(x, y) for x, y in zip(one[a], one[b])), (a, b)


def test_remapping_strategy_takes_unfused_path(device, tmp_path):
    """A remapping strategy turns fusion off (Step's can_fuse): Adam trains 2
    iterations through ComputeUpdateValue's switch without error."""
    pf = tmp_path / "prune_order.txt"
    pf.write_text(" ".join(str(x) for x in np.random.default_rng(5).permutation(500)) + "\n")
    extra = f'failure_strategy {{ type: "remapping" start: 0 period: 1 prune_order_file: "{pf}" }}\n'
    st = _train("Adam", [2], fused=True, extra=extra, threshold=None)
    assert len(st["hist"]) == 2 * len(st["params"])
    assert all(np.isfinite(p).all() for p in st["params"])
    assert all(h.any() for h in st["hist"])


def test_graph_replay_rmsprop(device):
    """RMSProp replays as SGD does: same bits as eager over 4 iterations, graph active."""
    ref = _train("RMSProp", [4], graph=False)
    got = _train("RMSProp", [4], graph=True)
    assert got["graph_active"] and not ref["graph_active"]
    _same_bits(got, ref)


def test_graph_replay_adam_stays_eager(device):
    """Adam's corrected rate moves every iteration (adam_solver.cpp:39-41), so
    set_graph(True) keeps the eager path, as lr_policy "inv" does: same bits,
    no graph instantiated."""
    ref = _train("Adam", [4], graph=False)
    got = _train("Adam", [4], graph=True)
    assert not got["graph_active"] and not ref["graph_active"]
    _same_bits(got, ref)
