"""Monte-Carlo map batching end to end (include/rram_caffe.h
rram_mc_set_map_batch; no reference counterpart).  A net built at batch
K x B carries K fault maps of B images along its batch axis; with the K
slices holding the same B images the statistics must be the sequential
driver's on the batch-B net, bit for bit: per-map accuracy / loss, their
float running sums, the broken-cell counts and the faulted weights.  A wrong
split, fold order, map id or a batch-dependent plan of a prefix layer would
each break the equality.  B = 20, K = 4, ten maps: two full groups and a short
one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, K, MAPS, SEED = 20, 4, 10, 77
CFGS = {"stuck": dict(), "quant_lognormal": dict(quant_levels=16, g_max=0.5, var_sigma=0.1)}


def N(t):
    import torch
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def _build(model):
    from rramsim import models
    return (models.cifar10_quick, "cifar10_quick") if model == "cifar" else (models.lenet, "lenet")


def _sequential(model, cfg_kw, calls, b=B):
    """Net A at batch B, the untouched sequential driver: (stats, map 9's weights, params, sources)."""
    from rramsim import caffe, make_inject_cfg, models
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    build, name = _build(model)
    net = caffe.Net(build(test_batch=b), "test", models.net_options(name))
    params = [N(p["data"]) for p in net.params()]
    src = {k: N(net.blob(k)) for k in ("data", "label")}
    mc = caffe.MonteCarlo(net, make_inject_cfg(0.05, **cfg_kw), seed=SEED, max_maps=64)
    for begin, count in calls:
        mc.run(begin, count)
    st = mc.stats()
    last = [N(f["data"]) for f in net.failure_params()]
    mc.close()
    net.close()
    return st, last, params, src


def _batched_net(model, params, src, b=B):
    """Net B at batch K x B with A's parameters and A's B images in its first slice."""
    import torch
    from rramsim import caffe, models
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    build, name = _build(model)
    net = caffe.Net(build(test_batch=K * b), "test", models.net_options(name))
    for p, a in zip(net.params(), params):
        p["data"].copy_(torch.from_numpy(a).to(p["data"].device))
    for k, a in src.items():
        t = net.blob(k)
        t[:b].copy_(torch.from_numpy(a).to(t.device))
        t[b:].zero_()                                   # tile_inputs() must fill these
    return net


def _batched(model, cfg_kw, calls, after=None, b=B):
    from rramsim import caffe, make_inject_cfg
    ref = _sequential(model, cfg_kw, calls, b)
    net = _batched_net(model, ref[2], ref[3], b)
    mc = caffe.MonteCarlo(net, make_inject_cfg(0.05, **cfg_kw), seed=SEED, max_maps=64, map_batch=K)
    mc.tile_inputs()
    for begin, count in calls:
        mc.run(begin, count)
    st = mc.stats()
    stacks = [N(mc.map_stack(i)) for i in range(len(net.failure_params()))]
    extra = after(mc, net) if after else None
    mc.close()
    net.close()
    return ref, st, stacks, extra


def _assert_equal(ref, st, stacks):
    rst, last = ref[0], ref[1]
    assert st["maps"] == rst["maps"] == MAPS
    assert st["per_map"] == rst["per_map"]
    assert st["sums"] == rst["sums"]
    assert st["broken"] == rst["broken"] and sum(st["broken"]) > 0
    # map 9 is slot 1 of the short last group (maps 8, 9)
    for s, a in zip(stacks, last):
        assert s.shape == (K, a.size)
        assert np.array_equal(s[(MAPS - 1) % K].view(np.uint32), a.view(np.uint32))
    assert len({tuple(r) for r in st["per_map"]}) > 1      # the maps do differ


@pytest.mark.parametrize("engine", ["f32", "bf16x6"])
@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_cifar_map_batch_equals_sequential(device, cfg, engine):
    """cifar10_quick under either engine setting: the engine and plan every
    contraction gets must not depend on the batch (the batch-invariance check)."""
    from rramsim import ops
    prev = ops.set_f32_engine(ops.ENGINE_F32 if engine == "f32" else ops.ENGINE_BF16X6)
    try:
        ref, st, stacks, _ = _batched("cifar", CFGS[cfg], [(0, MAPS)])
    finally:
        ops.set_f32_engine(prev)
    _assert_equal(ref, st, stacks)


@pytest.mark.parametrize("model", ["cifar", "lenet"])
def test_map_batch_pins_conv_split_plan(device, model):
    """B = 100, K = 4: at batch 400 the fp32 engine's convolutions (cifar conv2 /
    conv3, LeNet conv2) would drop the split-K they take at batch 100 and sum
    an image's products in another order; the grouped layers pin the batch-100
    plan (rram_set_conv_plan_num), so the bits stay the sequential maps'."""
    ref, st, stacks, _ = _batched(model, CFGS["stuck"], [(0, MAPS)], b=100)
    _assert_equal(ref, st, stacks)


def test_lenet_map_batch_equals_sequential(device):
    ref, st, stacks, _ = _batched("lenet", CFGS["stuck"], [(0, MAPS)])
    _assert_equal(ref, st, stacks)


def test_two_runs_equal_one_and_map_batch_one_continues(device):
    """run(0, 4) + run(4, 6) equals run(0, 10) (of both drivers); then
    set_map_batch(1) puts the sequential driver back on net B: it runs, and
    the statistics continue (one more map, a finite row of its own)."""
    def after(mc, net):
        mc.set_map_batch(1)
        assert mc.map_stack(0) is None
        mc.run(MAPS, 1)
        return mc.stats()
    ref, st, stacks, st1 = _batched("cifar", CFGS["stuck"], [(0, 4), (4, 6)], after=after)
    one = _sequential("cifar", CFGS["stuck"], [(0, MAPS)])
    assert ref[0]["per_map"] == one[0]["per_map"] and ref[0]["sums"] == one[0]["sums"]
    _assert_equal(ref, st, stacks)
    assert st1["maps"] == MAPS + 1 and st1["per_map"][:MAPS] == st["per_map"]
    acc, loss = st1["per_map"][MAPS]
    assert 0.0 <= acc <= 1.0 and np.isfinite(loss)
    # the eleventh map of net B: all K x B = 4 copies of the B images under one map
    assert st1["sums"][0] == pytest.approx(st["sums"][0] + acc, rel=1e-6)
    assert sum(st1["broken"]) > sum(st["broken"])


def test_map_batch_refusals(device):
    from rramsim import caffe, make_inject_cfg, models
    from rramsim._kernels import RramError
    caffe.set_stream_from_torch()
    caffe.set_random_seed(1701)
    cfg = make_inject_cfg(0.05)
    net = caffe.Net(models.cifar10_quick(test_batch=K * B), "test", models.net_options("cifar10_quick"))
    mc = caffe.MonteCarlo(net, cfg, seed=SEED, max_maps=8)
    with pytest.raises(RramError, match="not divisible by map_batch 3"):
        mc.set_map_batch(3)
    with pytest.raises(RramError, match="map_batch must be >= 1"):
        mc.set_map_batch(0)
    # prefix reuse / graph replay first, then K > 1
    mc.set_reuse_prefix(True)
    with pytest.raises(RramError, match="prefix reuse is on"):
        mc.set_map_batch(K)
    mc.set_reuse_prefix(False)
    mc.set_graph(True)
    with pytest.raises(RramError, match="graph replay is on"):
        mc.set_map_batch(K)
    mc.set_graph(False)
    # K > 1 first, then the setters
    mc.set_map_batch(K)
    with pytest.raises(RramError, match="prefix reuse: not available while map batching"):
        mc.set_reuse_prefix(True)
    with pytest.raises(RramError, match="graph replay: not available while map batching"):
        mc.set_graph(True)
    mc.run(0, 2)                                         # still usable after the refusals
    assert mc.stats()["maps"] == 2
    mc.close()
    net.close()

    # the conv-fault extension is not batched
    net = caffe.Net(models.cifar10_quick(test_batch=K * B), "test",
                    models.net_options("cifar10_quick", fault_layers="InnerProduct,Convolution"))
    with pytest.raises(RramError, match="Convolution layer conv1.*conv-fault extension is not batched"):
        caffe.MonteCarlo(net, cfg, seed=SEED, max_maps=8, map_batch=K)
    net.close()

    # a loss that mixes the images of a batch
    txt = ('layer { name: "x" type: "DummyData" top: "x" top: "t" dummy_data_param { shape { dim: 8 dim: 6 } '
           'shape { dim: 8 dim: 3 } data_filler { type: "gaussian" std: 1 } } }\n'
           'layer { name: "fc" type: "InnerProduct" bottom: "x" top: "fc" inner_product_param { num_output: 3 '
           'weight_filler { type: "gaussian" std: 0.1 } } }\n'
           'layer { name: "l2" type: "EuclideanLoss" bottom: "fc" bottom: "t" top: "l2" }\n')
    net = caffe.Net(txt, "test")
    mc = caffe.MonteCarlo(net, cfg, seed=SEED, max_maps=8)
    with pytest.raises(RramError, match=r"l2 \(EuclideanLoss\) mixes the images"):
        mc.set_map_batch(2)
    mc.run(0, 1)                                         # the sequential driver is intact
    assert mc.stats()["maps"] == 1
    mc.close()
    net.close()
