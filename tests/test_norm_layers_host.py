"""BatchNorm / Scale / Sigmoid on the host side (no GPU): the two model
generators parse into the expected layer tables, the exclusions are clean
errors, and both libraries export the new symbols."""
import ctypes as C

import pytest


def _shapes_through(table, hw=32):
    """Spatial size after the convolutions (3x3 pad 1: unchanged) and 2x2 / 2 pools of a layer table."""
    for _, typ, _, _ in table:
        if typ == "Pooling":
            hw //= 2
    return hw


def test_vgg11_layer_table():
    from rramsim import caffe, models
    for phase in ("train", "test"):
        t = caffe.describe(models.cifar10_vgg11(), phase)
        types = [r[1] for r in t]
        assert types.count("Convolution") == 8 and types.count("InnerProduct") == 3 and types.count("Pooling") == 5
        assert types.count("BatchNorm") == types.count("Scale") == types.count("ReLU") == 10
        by = {r[0]: r for r in t}
        # every BatchNorm's top is read by an in-place Scale, then an in-place ReLU
        for i, r in enumerate(t):
            if r[1] == "BatchNorm":
                assert t[i + 1][1] == "Scale" and t[i + 1][2] == t[i + 1][3] == r[3]
                assert t[i + 2][1] == "ReLU" and t[i + 2][2] == t[i + 2][3] == r[3]
        assert by["fc1"][2] == ["pool5"] and _shapes_through(t) == 1          # 512 x 1 x 1 into fc1
        assert by["fc3"][1] == "InnerProduct"
    txt = models.cifar10_vgg11()
    assert txt.count('type: "msra"') == 11 and "num_output: 10" in txt and txt.count("num_output: 1024") == 2
    assert "num_output: 2048" in models.cifar10_vgg11(fc=2048)
    assert models.net_options("cifar10_vgg11")["num_classes"] == 10
    assert "reconstruction" in models.cifar10_vgg11.__doc__


def test_full_sigmoid_bn_layer_table():
    from rramsim import caffe, models
    t = caffe.describe(models.cifar10_full_sigmoid_bn(), "train")
    assert [r[:2] for r in t if r[1] in ("BatchNorm", "Sigmoid")] == [
        ("bn1", "BatchNorm"), ("Sigmoid1", "Sigmoid"), ("bn2", "BatchNorm"), ("Sigmoid2", "Sigmoid"),
        ("bn3", "BatchNorm"), ("Sigmoid3", "Sigmoid")]
    by = {r[0]: r for r in t}
    assert by["bn1"][2] == ["pool1"] and by["conv2"][2] == ["Sigmoid1"] and by["ip1"][2] == ["pool3"]
    assert models.net_options("cifar10_full_sigmoid_bn")["data_shape"] == "3,32,32"


def test_vgg11_solver_template_is_accepted():
    """The reference's solver template for this net, as shipped (tests/golden, settings only): a failure_pattern
    block over several lines.  tests/test_gpu_norm_layers.py trains the reconstructed net with the result."""
    from rramsim import caffe, tools
    from pathlib import Path
    tpl = (Path(__file__).parent / "golden" / "cifar10_vgg11_solver_template.prototxt").read_text()
    assert "failure_pattern: {\n" in tpl                       # the block spans lines
    rows = caffe.solver_describe(tools.experiment_solver(tpl, 4e6, 2e6, snapshot_prefix="out"))
    assert [r for r in rows if r[0] == "failure_pattern"] == [["failure_pattern", "gaussian", "4000000", "2000000",
                                                               "10", "20", "10"]]
    assert [r for r in rows if r[0] == "solver"][0][1:] == ["step", "0.005", "50000", "5000", "out/"]


@pytest.mark.parametrize("lib,names", [
    ("kernels", ["rram_norm_workspace_floats", "rram_bn_stats_train", "rram_bn_stats_global", "rram_norm_apply",
                 "rram_norm_bwd_reduce", "rram_norm_bwd_apply", "rram_sigmoid_fwd", "rram_sigmoid_bwd",
                 "rram_bn_fwd_kernel_ids", "rram_bn_bwd_kernel_ids", "rram_scale_kernel_ids",
                 "rram_sigmoid_kernel_ids", "rram_norm_kernel_list"]),
    ("caffe", ["rram_layer_type_registered", "rram_norm_layer_check"])])
def test_symbols_exported(lib, names):
    import re
    from pathlib import Path
    from rramsim import _kernels as K
    from rramsim import caffe
    K.load()
    so = K.load() if lib == "kernels" else C.CDLL(str(K.CAFFE_SO))
    hdr = Path(__file__).resolve().parents[1] / "include" / ("rram_kernels.h" if lib == "kernels" else "rram_caffe.h")
    declared = set(re.findall(r"\b(rram_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr.read_text(), flags=re.S)))
    for n in names:
        assert n in declared and hasattr(so, n), n
        assert n in (K.SIGNATURES if lib == "kernels" else caffe.SIGNATURES), n


def test_layer_types_registered():
    from rramsim import caffe
    for t in ("BatchNorm", "Scale", "Sigmoid", "Convolution"):
        assert caffe.layer_type_registered(t), t
    assert not caffe.layer_type_registered("NoSuchLayer")


BN = 'name: "bn" type: "BatchNorm" bottom: "x" top: "y" '


def test_batch_norm_lr_mult_is_zero_without_specs():
    from rramsim import caffe
    assert caffe.norm_layer_check(BN) == [0.0, 0.0, 0.0]
    assert caffe.norm_layer_check(BN + "param { lr_mult: 0 } param { lr_mult: 0 } param { lr_mult: 0 }") == [0.0] * 3
    assert caffe.norm_layer_check(BN + "batch_norm_param { use_global_stats: true eps: 0.001 }", bottom_axes=2) == [0.0] * 3


@pytest.mark.parametrize("spec", ["param { lr_mult: 1 }", "param { lr_mult: 0 } param { lr_mult: 0.5 }",
                                  "param { decay_mult: 0 }"])
def test_batch_norm_rejects_a_trained_statistic(spec):
    from rramsim import caffe
    from rramsim._kernels import RramError
    with pytest.raises(RramError, match="Cannot configure batch normalization statistics"):
        caffe.norm_layer_check(BN + spec)


def test_exclusions_are_clean_errors():
    from rramsim import caffe
    from rramsim._kernels import RramError
    sc = 'name: "sc" type: "Scale" bottom: "x" top: "x" '
    caffe.norm_layer_check(sc + "scale_param { bias_term: true }")
    caffe.norm_layer_check(sc + "scale_param { axis: -3 }")                       # axis 1 of 4
    with pytest.raises(RramError, match="two-bottom Scale"):
        caffe.norm_layer_check(sc + 'bottom: "s"', num_bottoms=2)
    with pytest.raises(RramError, match="axis 1, num_axes 1"):
        caffe.norm_layer_check(sc + "scale_param { axis: 0 }")
    with pytest.raises(RramError, match="axis 1, num_axes 1"):
        caffe.norm_layer_check(sc + "scale_param { num_axes: 2 }")
    with pytest.raises(RramError, match="at least 2 axes"):
        caffe.norm_layer_check(BN, bottom_axes=1)
