"""BatchNorm / Scale / Sigmoid through the host: a tiny net
data (4, 3, 8, 8) -> conv 3x3 pad 1 (8) -> BN -> Scale -> ReLU -> pool -> fc16 -> BN -> Scale -> ReLU -> fc10 -> loss
trained by the fault-aware solver with the BatchNorm + Scale + ReLU fold on and off, its BatchNorm blobs under
weight decay, snapshots, the captured-graph mode, MonteCarlo map batching, and one iteration of the VGG11."""
import json
from pathlib import Path

import numpy as np
import pytest

import _norm_cases as nc

pytestmark = pytest.mark.gpu
BOUNDS = json.loads((Path(__file__).parent / "golden" / "norm_bounds.json").read_text())
TINY_BOUNDS = BOUNDS["tiny_net"]
REF64 = nc.tiny_train(np.float64)
OPTS = dict(data_shape="3,8,8", num_classes=10)


def N(t):
    import torch
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def tiny(batch=4):
    from rramsim import models
    p = models._P("tiny_bn")
    models._data(p, train_batch=batch, test_batch=batch)
    g = dict(type="gaussian", std=0.1)
    models._conv(p, "conv1", "data", 8, 3, pad=1, wf=g)
    models._bn(p, "bn1", "conv1")
    models._scale(p, "scale1", "bn1")
    models._relu(p, "relu1", "bn1")
    models._pool(p, "pool1", "bn1", "MAX", 2, 2)
    models._ip(p, "fc1", "pool1", 16, wf=g)
    models._bn(p, "bn2", "fc1")
    models._scale(p, "scale2", "bn2")
    models._relu(p, "relu2", "bn2")
    models._ip(p, "fc2", "bn2", 10, wf=g)
    models._heads(p, "fc2")
    return p.text()


def solver(tmp=None, snapshot=0, max_iter=100, wd=0.004, **kw):
    from rramsim import models
    s = models.solver(base_lr=0.01, momentum=0.9, weight_decay=wd, max_iter=max_iter, failure_mean=5e4,
                      failure_std=1.5e4, failure_prob=(5, 90, 5), threshold=0.0001, **kw)
    if snapshot:
        s += f'snapshot: {snapshot}\nsnapshot_prefix: "{tmp}/"\n'
    return s


def train(iters, fuse=True, graph=False, **kw):
    from rramsim import caffe
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    s = caffe.Solver(solver(**kw), tiny(), dict(OPTS, fused_update=True, fuse_bn_scale=fuse))
    s.set_graph(graph)
    losses = []
    for n in iters:
        s.step(n)
        losses.append(_loss(s))
    out = dict(params=[N(p["data"]) for p in s.net.params()], lr=[p["lr_mult"] for p in s.net.params()],
               hist=[N(h) for h in s.history()], losses=losses, graph=s.graph_active(),
               layers=[l[:2] for l in s.net.layers()])
    s.close()
    return out


def _load(net, data, label, params):
    """The fixed inputs of tests/_norm_cases.py into a net (its synthetic Data layer never rewrites its tops)."""
    import torch
    net.blob("data").copy_(torch.from_numpy(data).to("cuda").view_as(net.blob("data")))
    net.blob("label").copy_(torch.from_numpy(label).to("cuda").view_as(net.blob("label")))
    ps = net.params()
    assert len(ps) == len(params)
    for p, v in zip(ps, params):
        p["data"].copy_(torch.from_numpy(np.ascontiguousarray(v, np.float32).ravel()).to("cuda"))


def _tiny_solver(fuse, fault):
    from rramsim import caffe, models
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    sp = solver() if fault else models.solver(base_lr=nc.TINY_LR, momentum=nc.TINY_MOM, weight_decay=nc.TINY_WD,
                                              max_iter=100)
    s = caffe.Solver(sp, tiny(), dict(OPTS, fused_update=True, fuse_bn_scale=fuse))
    data, label, p = nc.tiny_inputs()
    _load(s.net, data, label, [p[k] for k in nc.TINY_PARAMS])
    return s


def _loss(s):
    """The loss of the iteration just run: the train net's loss top (smoothed_loss is kept only for display)."""
    return float(N(s.net.outputs()["loss"]).ravel()[0])


def _close(got, want, bound, what):
    err = float(np.max(np.abs(np.asarray(got, np.float64).ravel() - np.asarray(want, np.float64).ravel())))
    print(f"{what}: error {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("fuse", [True, False], ids=["fold", "three_layers"])
def test_first_iteration_against_float64(device, fuse):
    """Forward and backward of the first iteration, fold on and off, against the float64 numpy net of
    tests/_norm_cases.py: the loss, every parameter gradient, and the BatchNorm blobs the forward leaves."""
    want = REF64[0]
    s = _tiny_solver(fuse, fault=False)
    s.net.clear_param_diffs()
    loss = s.net.forward()
    s.net.backward()
    _close(loss, want["loss"], TINY_BOUNDS[0]["loss"], "loss")
    for k, p in zip(nc.TINY_PARAMS, s.net.params()):
        if k in nc.TINY_BN:
            _close(N(p["data"]), want["params"][k], TINY_BOUNDS[0]["params"][k], k)
            assert not N(p["diff"]).any(), k
        else:
            _close(N(p["diff"]), want["grads"][k], TINY_BOUNDS[0]["grads"][k], "d" + k)
    s.close()


@pytest.mark.parametrize("fuse", [True, False], ids=["fold", "three_layers"])
def test_three_sgd_iterations_against_float64(device, fuse):
    """Momentum SGD with weight decay: the parameters after each of three updates and each iteration's loss."""
    s = _tiny_solver(fuse, fault=False)
    for it in range(nc.TINY_ITERS):
        s.step(1)
        _close(_loss(s), REF64[it]["loss"], TINY_BOUNDS[it]["loss"], f"loss[{it}]")
        for k, p in zip(nc.TINY_PARAMS, s.net.params()):
            _close(N(p["data"]), REF64[it]["params"][k], TINY_BOUNDS[it]["params"][k], f"{k}[{it}]")
    s.close()


def test_fold_on_equals_fold_off_fault_aware(device):
    """Three fault-aware SGD iterations (gaussian failure pattern, threshold strategy, Fail), fold on against off.
    The fault tail is the same function of the gradients in both runs and adds no arithmetic of its own (it zeroes
    an update or pins a weight), so two runs that each stay within a bound of float64 stay within twice that bound
    of each other: twice the three-iteration bound of norm_bounds.json, per parameter.  The same parameter list."""
    runs = []
    for fuse in (True, False):
        s = _tiny_solver(fuse, fault=True)
        losses = []
        for _ in range(nc.TINY_ITERS):
            s.step(1)
            losses.append(_loss(s))
        runs.append(([N(p["data"]) for p in s.net.params()], losses, s.broken_counts()))
        s.close()
    (on, lon, bon), (off, loff, boff) = runs
    assert len(on) == len(off) == len(nc.TINY_PARAMS) and bon == boff
    last = TINY_BOUNDS[nc.TINY_ITERS - 1]
    for k, a, b in zip(nc.TINY_PARAMS, on, off):
        _close(a, b, 2 * last["params"][k], k)
    for it, (a, b) in enumerate(zip(lon, loff)):
        _close(a, b, 2 * TINY_BOUNDS[it]["loss"], f"loss[{it}]")
    assert lon[0] == loff[0]                                     # nothing differs before the first backward


def _bn_on_data_net():
    from rramsim import models
    p = models._P("bn_on_data")
    models._data(p, train_batch=4, test_batch=4)
    models._bn(p, "bn", "data")
    models._scale(p, "scale", "bn")
    models._ip(p, "fc", "bn", 10)
    models._heads(p, "fc")
    return p.text()


@pytest.mark.parametrize("fuse", [True, False], ids=["fold", "three_layers"])
def test_scale_trains_when_the_batch_norm_bottom_takes_no_diff(device, fuse):
    """BatchNorm directly on the data blob: nothing below it needs a gradient and its own blobs have rate 0, yet
    with the fold its backward is what writes the Scale's dgamma / dbeta."""
    from rramsim import caffe
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    net = caffe.Net(_bn_on_data_net(), "train", dict(OPTS, fuse_bn_scale=fuse))
    data, label, _ = nc.tiny_inputs()
    p, want = nc.bn_on_data(np.float64)
    _load(net, data, label, [np.zeros(3), np.zeros(3), np.zeros(1), p["gamma"], p["beta"], p["w"], p["b"]])
    net.clear_param_diffs()
    loss = net.forward()
    net.backward()
    b = BOUNDS["bn_on_data"]
    ps = net.params()
    _close(loss, want["loss"], b["loss"], "loss")
    _close(N(ps[3]["diff"]), want["dgamma"], b["dgamma"], "dgamma")
    _close(N(ps[4]["diff"]), want["dbeta"], b["dbeta"], "dbeta")
    assert N(ps[3]["diff"]).any() and N(ps[4]["diff"]).any()
    net.close()


def test_batch_norm_lr_mult_and_weight_decay(device):
    """No `param` spec: lr_mult 0 for the three blobs, and a rate of 0 really updates nothing.  The data layer's
    batch is fixed, so after two iterations a bare TRAIN forward sees what iteration 3's forward sees: the
    BatchNorm blobs it leaves are, bit for bit, those of a run of three iterations with weight_decay 0.5."""
    from rramsim import caffe
    got = train([3], wd=0.5)
    bn = [i for i, lr in enumerate(got["lr"]) if lr == 0.0]
    assert bn == [2, 3, 4, 9, 10, 11]
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    s = caffe.Solver(solver(wd=0.5), tiny(), dict(OPTS, fused_update=True))
    s.step(2)
    s.net.forward()
    ps = s.net.params()
    for i in bn:
        assert np.array_equal(N(ps[i]["data"]).view(np.uint32), got["params"][i].view(np.uint32)), i
        assert N(ps[i]["data"]).any()
    want = np.float32(0)
    for _ in range(3):
        want = np.float32(want * np.float32(0.999) + np.float32(1))
    assert N(ps[4]["data"])[0] == want
    s.close()


def test_snapshot_restore_continue(device, tmp_path):
    from rramsim import caffe
    ref = train([4])
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    s = caffe.Solver(solver(tmp_path, snapshot=2), tiny(), dict(OPTS, fused_update=True))
    s.step(2)
    s.close()
    state = Path(tmp_path) / "_iter_2.solverstate"
    model = Path(tmp_path) / "_iter_2.caffemodel"
    assert state.exists() and model.exists(), list(Path(tmp_path).iterdir())
    rows = caffe.caffemodel_describe(str(model))
    assert len([r for r in rows if r[0] == "bn1"]) == 3 and len([r for r in rows if r[0] == "bn2"]) == 3
    caffe.set_random_seed(1701)
    s = caffe.Solver(solver(), tiny(), dict(OPTS, fused_update=True))
    s.restore(str(state))
    s.step(2)
    for a, p in zip(ref["params"], s.net.params()):
        assert np.array_equal(a.view(np.uint32), N(p["data"]).view(np.uint32))
    s.close()


def test_graph_training_equals_eager(device):
    ref, got = train([1, 1, 1]), train([1, 1, 1], graph=True)
    assert got["graph"] and not ref["graph"]
    for a, b in zip(got["params"] + got["hist"], ref["params"] + ref["hist"]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_monte_carlo_map_batch_equals_sequential(device):
    """TEST-phase BatchNorm treats images independently: 8 maps at map_batch 4 equal 8 sequential maps."""
    import torch
    from rramsim import caffe, make_inject_cfg
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    b, K = 4, 4
    a = caffe.Net(tiny(b), "test", OPTS)
    # statistics a training run would have left
    for p in a.params():
        if p["lr_mult"] == 0.0:
            p["data"].copy_(torch.rand_like(p["data"]) + 0.5)
    params = [N(p["data"]) for p in a.params()]
    src = {k: N(a.blob(k)) for k in ("data", "label")}
    mc = caffe.MonteCarlo(a, make_inject_cfg(0.05), seed=5, max_maps=16)
    mc.run(0, 8)
    ref = mc.stats()
    mc.close()
    a.close()
    n = caffe.Net(tiny(K * b), "test", OPTS)
    for p, v in zip(n.params(), params):
        p["data"].copy_(torch.from_numpy(v).to(p["data"].device))
    for k, v in src.items():
        t = n.blob(k)
        t[:b].copy_(torch.from_numpy(v).to(t.device))
    mc = caffe.MonteCarlo(n, make_inject_cfg(0.05), seed=5, max_maps=16, map_batch=K)
    mc.tile_inputs()
    mc.run(0, 8)
    st = mc.stats()
    mc.close()
    n.close()
    assert st["per_map"] == ref["per_map"] and st["broken"] == ref["broken"] and sum(st["broken"]) > 0
    assert len({tuple(r) for r in st["per_map"]}) > 1


def test_vgg11_runs(device):
    from rramsim import caffe, models
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    from rramsim import tools
    # the reference's own solver template for this net drives the run (max_iter, snapshot and display lie far out)
    tpl = (Path(__file__).parent / "golden" / "cifar10_vgg11_solver_template.prototxt").read_text()
    sp = tools.experiment_solver(tpl, 5e6, 1e6, threshold=0.0001).replace("test_iter: 100", "test_iter: 1")
    s = caffe.Solver(sp, models.cifar10_vgg11(train_batch=4, test_batch=4),
                     dict(models.net_options("cifar10_vgg11"), fused_update=True))
    assert list(s.net.blob("pool5").shape) == [4, 512, 1, 1] and list(s.net.blob("fc3").shape) == [4, 10]
    s.step(1)
    assert np.isfinite(_loss(s))
    for p in s.net.params():
        assert np.isfinite(N(p["data"])).all()
    out = s.test(0)
    assert len(out) == 2 and all(np.isfinite(v) for v in out)
    s.close()


def test_sigmoid_bn_net_runs(device):
    from rramsim import caffe, models
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    s = caffe.Solver(solver(), models.cifar10_full_sigmoid_bn(train_batch=4, test_batch=4),
                     dict(models.net_options("cifar10_full_sigmoid_bn"), fused_update=True))
    s.step(2)
    assert np.isfinite(_loss(s))
    assert all(np.isfinite(N(p["data"])).all() for p in s.net.params())
    s.close()
