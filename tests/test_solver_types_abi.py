"""CPU tests of the solver-type entries at the C-ABI boundary: the five update
kernels' entries and the fused tail for any solver type are exported and have
ctypes signatures, the new segment struct matches the header, and argument
validation answers on the host before any launch (there is no GPU here)."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]

NEW_KERNEL_SYMBOLS = ["rram_nesterov_update", "rram_adagrad_update", "rram_rmsprop_update", "rram_adadelta_update",
                      "rram_adam_update", "rram_fused_opt_update_fail", "rram_fused_opt_update_fail_batched"]


def _header(name):
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / name).read_text(), flags=re.S)


def test_new_symbols_declared_exported_and_signed():
    from rramsim import _kernels as K
    from rramsim import caffe
    lib = K.load()
    text = _header("rram_kernels.h")
    for n in NEW_KERNEL_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n), n
        assert n in K.SIGNATURES, n
    assert re.search(r"\brram_solver_type\s*\(", _header("rram_caffe.h"))
    host = ctypes.CDLL(str(K.CAFFE_SO))
    assert hasattr(host, "rram_solver_type")
    assert "rram_solver_type" in caffe.SIGNATURES


def test_solver_kind_enum_matches_header():
    from rramsim import _kernels as K
    text = _header("rram_kernels.h")
    for name in ("SGD", "NESTEROV", "ADAGRAD", "RMSPROP", "ADADELTA", "ADAM"):
        m = re.search(r"\bRRAM_SOLVER_%s\s*=\s*(\d+)" % name, text)
        assert m, name
        assert int(m.group(1)) == getattr(K, "RRAM_SOLVER_" + name)
    assert sorted(K.SOLVER_KINDS.values()) == list(range(6))


def test_opt_seg_matches_header():
    """rram_opt_seg is rram_update_seg (96 bytes, pinned by test_abi.py) plus
    one pointer: same offsets for the shared fields, h2 at 96, 104 bytes."""
    from rramsim import _kernels as K
    assert ctypes.sizeof(K.OptSeg) == ctypes.sizeof(K.UpdateSeg) + 8 == 104
    for name, _ in K.UpdateSeg._fields_:
        assert getattr(K.OptSeg, name).offset == getattr(K.UpdateSeg, name).offset, name
    assert K.OptSeg.h2.offset == 96
    # the header's field order, as declared
    body = re.search(r"typedef struct rram_opt_seg \{(.*?)\} rram_opt_seg;", _header("rram_kernels.h"), flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", decl.strip())]
    assert names == [n for n, _ in K.OptSeg._fields_], names
    assert ctypes.sizeof(K.SolverHyper) == 12
    assert [n for n, _ in K.SolverHyper._fields_] == ["momentum", "momentum2", "delta"]


def test_bad_arguments_return_einval_without_a_launch():
    from rramsim import _kernels as K
    lib = K.load()
    hy = K.SolverHyper(0.9, 0.999, 1e-8)
    hp = ctypes.byref(hy)
    p16 = ctypes.c_void_p(16)

    def seg(n=100, h2=None):
        return K.OptSeg(p16, p16, p16, None, None, n, 0.0, 0.01, 0.0, 0, None, None, 0, 0, 0, 0, h2)

    batched = lib.rram_fused_opt_update_fail_batched
    # nsegs 33
    assert batched(None, 33, K.RRAM_SOLVER_ADAM, hp, 100.0, 1e-20, None) == K.RRAM_EINVAL
    assert b"nsegs" in lib.rram_last_error()
    # a negative n
    s = seg(n=-1)
    assert batched(ctypes.byref(s), 1, K.RRAM_SOLVER_NESTEROV, hp, 100.0, 1e-20, None) == K.RRAM_EINVAL
    assert b"n < 0" in lib.rram_last_error()
    # kind out of range
    s = seg()
    for kind in (-1, 6):
        assert batched(ctypes.byref(s), 1, kind, hp, 100.0, 1e-20, None) == K.RRAM_EINVAL
        assert b"kind" in lib.rram_last_error()
    # h2 == NULL for the two-history types
    for kind in (K.RRAM_SOLVER_ADADELTA, K.RRAM_SOLVER_ADAM):
        assert batched(ctypes.byref(s), 1, kind, hp, 100.0, 1e-20, None) == K.RRAM_EINVAL
        assert b"h2" in lib.rram_last_error()
        assert lib.rram_fused_opt_update_fail(p16, p16, p16, None, None, None, 100, kind, hp, 0.0, 0.01, 0, 0.0, 100.0,
                                              1e-20, None, None) == K.RRAM_EINVAL
    # NULL segs with nsegs > 0
    assert batched(None, 1, K.RRAM_SOLVER_RMSPROP, hp, 100.0, 1e-20, None) == K.RRAM_EINVAL
    assert b"segs is NULL" in lib.rram_last_error()
    # a flipped-kernel destination whose geometry does not cover the segment
    s = K.OptSeg(p16, p16, p16, None, None, 100, 0.0, 0.0, 0.0, 0, None, p16, 2, 3, 4, 9, None)
    assert batched(ctypes.byref(s), 1, K.RRAM_SOLVER_ADAGRAD, hp, 100.0, 1e-20, None) == K.RRAM_EINVAL
    assert b"flip geometry" in lib.rram_last_error()
    # the stand-alone kernels: negative n, NULL pointers
    assert lib.rram_nesterov_update(p16, p16, -1, 0.9, 0.01, None) == K.RRAM_EINVAL
    assert lib.rram_adagrad_update(None, p16, 8, 1e-8, 0.01, None) == K.RRAM_EINVAL
    assert lib.rram_rmsprop_update(p16, None, 8, 0.99, 1e-8, 0.01, None) == K.RRAM_EINVAL
    assert lib.rram_adadelta_update(p16, p16, None, 8, 0.95, 1e-8, 0.01, None) == K.RRAM_EINVAL
    assert lib.rram_adam_update(p16, p16, None, 8, 0.9, 0.999, 1e-8, 0.01, None) == K.RRAM_EINVAL
    # n == 0 is a successful no-op that never touches the device
    s = seg(n=0)
    for kind in range(6):
        assert batched(ctypes.byref(s), 1, kind, hp, 100.0, 1e-20, None) == K.RRAM_OK
        assert lib.rram_fused_opt_update_fail(None, None, None, None, None, None, 0, kind, hp, 0.0, 0.01, 0, 0.0,
                                              100.0, 1e-20, None, None) == K.RRAM_OK
    assert batched(None, 0, K.RRAM_SOLVER_ADAM, hp, 100.0, 1e-20, None) == K.RRAM_OK
    assert lib.rram_adam_update(None, None, None, 0, 0.9, 0.999, 1e-8, 0.01, None) == K.RRAM_OK
