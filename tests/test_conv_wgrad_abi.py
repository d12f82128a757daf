"""Host side of the bf16x6 weight-gradient selector (rram_set_bwd_weight_engine):
no GPU work, only the planning entry points."""
import pytest

from test_gpu_conv_wgrad_x6 import CASES, _desc

BIG = 1 << 30


@pytest.fixture
def x6_on():
    from rramsim import ops
    prev = ops.set_bwd_weight_engine(ops.ENGINE_BF16X6)
    yield ops
    ops.set_bwd_weight_engine(prev)


def test_selector_round_trip():
    from rramsim import _kernels as K, ops
    assert ops.get_bwd_weight_engine() == ops.ENGINE_F32          # the default
    assert ops.set_bwd_weight_engine(ops.ENGINE_BF16X6) == ops.ENGINE_F32
    assert ops.get_bwd_weight_engine() == ops.ENGINE_BF16X6
    assert K.load().rram_set_bwd_weight_engine(7) == K.load().rram_set_bwd_weight_engine(-1) < 0   # RRAM_EINVAL
    assert ops.get_bwd_weight_engine() == ops.ENGINE_BF16X6
    assert ops.set_bwd_weight_engine(ops.ENGINE_F32) == ops.ENGINE_BF16X6


def test_unserved_shapes_keep_f32(x6_on):
    ops = x6_on
    served = ops.conv_desc((4, 8, 12, 12), 8, 3, 1, 1)
    need = ops.conv2d_bwd_workspace(served, 4)
    assert ops.bwd_weight_engine_for_conv(served, need) == ops.ENGINE_BF16X6
    assert ops.bwd_weight_engine_for_conv(served, 64) == ops.ENGINE_F32          # too small a workspace
    for k, s, p, dil in ((3, 2, 1, 1), (3, 1, 2, 2), (1, 1, 0, 1), (7, 1, 3, 1)):
        d = ops.conv_desc((4, 8, 12, 12), 8, k, s, p, dil)
        assert ops.bwd_weight_engine_for_conv(d, BIG) == ops.ENGINE_F32, (k, s, p, dil)


def test_selector_off_serves_nothing():
    from rramsim import ops
    for cs in CASES:
        d = _desc(cs)
        assert ops.bwd_weight_engine_for_conv(d, BIG) == ops.ENGINE_F32
        assert not [k for k in ops.conv_bwd_kernel_ids(d, ws_bytes=BIG) if k.startswith("wgrad_x6")]


def test_every_wgrad_kernel_is_selected_by_a_gpu_case(x6_on):
    ops = x6_on
    built = ops.conv_wgrad_kernel_list()
    picked = set()
    for cs in CASES:
        d = _desc(cs)
        ids = ops.conv_bwd_kernel_ids(d, ws_bytes=ops.conv2d_bwd_workspace(d, cs["x"][0]))
        picked |= {k.split("/")[0] for k in ids if k.startswith("wgrad_x6")}
    assert built and picked == set(built)
    assert not set(built) & (set(ops.f32_kernel_list()) | set(ops.conv_fwd_kernel_list()))
