"""Which kernels of csrc/norm.hip each case of tests/_norm_cases.py launches,
and that the cases reach every kernel of the file (host logic, no GPU).  The
queries call the entry points themselves with the launches recorded instead of
issued, so no threshold of the dispatch is restated here.
tests/test_gpu_norm_kernels.py runs the same cases against float64."""
import pytest

from _norm_cases import BN_CASES, SIGMOID_N, nci

NAMES = sorted(BN_CASES)


def _reached():
    from rramsim import ops
    got = []
    for name in NAMES:
        n, c, i = nci(BN_CASES[name]["shape"])
        for off in range(4):
            got += ops.bn_fwd_kernel_ids(n, c, i, x_off=off, y_off=off)
            got += ops.bn_bwd_kernel_ids(n, c, i, scale=True, dy_off=off, dx_off=off)
        got += ops.bn_fwd_kernel_ids(n, c, i, x_off=1, y_off=2)          # operands that do not share an offset
        got += ops.bn_bwd_kernel_ids(n, c, i, dy_off=0, dx_off=3)
        got += ops.bn_fwd_kernel_ids(n, c, i, global_stats=True)
        got += ops.bn_bwd_kernel_ids(n, c, i, global_stats=True)
        got += ops.scale_kernel_ids(n, c, i) + ops.scale_kernel_ids(n, c, i, backward=True)
    got += ops.sigmoid_kernel_ids(SIGMOID_N) + ops.sigmoid_kernel_ids(SIGMOID_N, backward=True)
    return got


@pytest.mark.parametrize("name", NAMES)
def test_case_selects_its_kernels(name):
    from rramsim import ops
    n, c, i = nci(BN_CASES[name]["shape"])
    assert ops.bn_fwd_kernel_ids(n, c, i) == BN_CASES[name]["fwd"]
    assert ops.bn_bwd_kernel_ids(n, c, i) == BN_CASES[name]["bwd"]


def test_every_kernel_has_a_case():
    from rramsim import ops
    ids = ops.norm_kernel_list()
    assert len(ids) == len(set(ids)) == 15
    assert set(_reached()) == set(ids), (sorted(set(ids) - set(_reached())), sorted(set(_reached()) - set(ids)))


def test_list_is_disjoint_from_the_support_layers():
    from rramsim import ops
    layer = ops.layer_kernel_list()
    assert len(layer) == len(set(layer)) == 35
    assert not set(layer) & set(ops.norm_kernel_list())


def test_dispatch_forms():
    from rramsim import ops
    # a base offset keeps the 16-byte streaming pass but not the aligned reduction
    assert ops.bn_fwd_kernel_ids(4, 3, 4160, x_off=1, y_off=1) == ["bn_stats_plane<1>", "bn_stats_finalize", "norm_apply<4>"]
    assert ops.bn_fwd_kernel_ids(4, 3, 4160, x_off=1, y_off=2)[-1] == "norm_apply<1>"
    assert ops.bn_fwd_kernel_ids(2, 513, 1, global_stats=True) == ["bn_global_stats", "norm_apply<4>"]
    assert ops.bn_bwd_kernel_ids(2, 8, 16, global_stats=True) == ["norm_bwd<4>"]             # dx = g rstd: no reduction
    assert ops.bn_bwd_kernel_ids(2, 8, 16, global_stats=True, scale=True)[:2] == ["norm_bwd_reduce_plane<4>", "norm_bwd_finalize"]
    assert ops.scale_kernel_ids(2, 8, 1, backward=True) == ["norm_bwd_reduce_cols", "norm_bwd_finalize", "norm_bwd<4>"]
    # the fold costs no launch: forward 3 (2 with global statistics), backward 3
    assert len(ops.bn_bwd_kernel_ids(100, 64, 1024, scale=True)) == 3


def test_queries_report_errors():
    import ctypes as C
    from rramsim import _kernels as K
    lib = K.load()
    buf = C.create_string_buffer(64)
    assert lib.rram_bn_fwd_kernel_ids(0, 4, 1, 0, 0, 0, buf, 64) == K.RRAM_EINVAL
    assert lib.rram_bn_fwd_kernel_ids(1 << 16, 1 << 16, 1, 0, 0, 0, buf, 64) == K.RRAM_EINVAL      # 2^32 elements
    assert lib.rram_norm_workspace_floats(0, 4, 1) == 0
    assert lib.rram_norm_workspace_floats(100, 64, 1024) >= 3 * 64
    assert lib.rram_sigmoid_fwd(None, None, 0, None) == K.RRAM_OK                                  # launches again
