"""CPU tests of the map-batching C-ABI (no compute calls): the new symbols are
exported by the two libraries and declared in the two headers, and the host
plan query rram_ip_fwd_groups_fused answers without a GPU."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

KERNEL_SYMBOLS = ["rram_inject_rng_maps", "rram_ip_fwd_groups", "rram_ip_fwd_groups_fused",
                  "rram_softmax_loss_fwd_groups", "rram_accuracy_groups", "rram_set_conv_plan_num"]
CAFFE_SYMBOLS = ["rram_mc_set_map_batch", "rram_mc_tile_inputs", "rram_mc_map_stack"]


def declared(header: Path):
    text = header.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(rram_[a-z0-9_]+)\s*\(", text))


def test_map_batch_kernel_symbols_declared_and_exported():
    from rramsim import _kernels as K
    lib = K.load()
    names = declared(ROOT / "include" / "rram_kernels.h")
    for n in KERNEL_SYMBOLS:
        assert n in names, n
        assert hasattr(lib, n), n
        assert n in K.SIGNATURES, n


def test_map_batch_caffe_symbols_declared_and_exported():
    from rramsim import _kernels as K
    from rramsim import caffe
    K.load()
    lib = ctypes.CDLL(str(K.CAFFE_SO))
    names = declared(ROOT / "include" / "rram_caffe.h")
    for n in CAFFE_SYMBOLS:
        assert n in names, n
        assert hasattr(lib, n), n
        assert n in caffe.SIGNATURES, n


def test_ip_fwd_groups_fused_plan_host_side():
    """C2 ip1 (M = 100, N = 64, K = 1024) splits K on the fp32 engine: fused
    when the workspace holds G groups of partials, a loop when there is no
    workspace for them (the split itself is never changed)."""
    from rramsim import ops
    from rramsim import _kernels as K
    lib = K.load()
    prev = ops.set_f32_engine(ops.ENGINE_F32)
    try:
        G, M, N, Kd = 3, 100, 64, 1024
        ws = G * 16 * M * N * 4                       # >= G x (split <= 16) partial slabs
        assert lib.rram_ip_fwd_groups_fused(G, M, N, Kd, 0, ws) == 1
        # one group's partials fit, three groups' do not: the M = 100 plan still splits, so it loops
        one = 16 * M * N * 4
        assert lib.rram_ip_fwd_groups_fused(G, M, N, Kd, 0, one) == 0
        # C2 ip2 (K = 64: no split) and the M = 1 GEMV plan are one launch whatever the workspace
        assert lib.rram_ip_fwd_groups_fused(3, 100, 10, 64, 0, 0) == 1
        assert lib.rram_ip_fwd_groups_fused(2, 1, 10, 64, 0, 0) == 1
    finally:
        ops.set_f32_engine(prev)


def test_ip_fwd_groups_fused_zero_workspace():
    """No workspace while the M = 100 plan wants split-K (8 chunks of 128 for
    K = 1024): not fused.  Exactly G x 8 slabs of 100 x 64 floats: fused."""
    from rramsim import ops
    from rramsim import _kernels as K
    lib = K.load()
    prev = ops.set_f32_engine(ops.ENGINE_F32)
    try:
        assert lib.rram_ip_fwd_groups_fused(3, 100, 64, 1024, 0, 0) == 0
        assert lib.rram_ip_fwd_groups_fused(3, 100, 64, 1024, 0, 3 * 8 * 100 * 64 * 4 - 1) == 0
        assert lib.rram_ip_fwd_groups_fused(3, 100, 64, 1024, 0, 3 * 8 * 100 * 64 * 4) == 1
    finally:
        ops.set_f32_engine(prev)
