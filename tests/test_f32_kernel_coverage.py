"""Which fp32-MFMA kernels each case of tests/_f32_cases.py launches, and that
the table reaches every instantiation (host logic, no GPU).

ops.gemm_kernel_ids and its siblings run the entry points' own planning code
with the launches recorded instead of issued, so a planner change that moves a
shape to another tile, split or reduce kernel, or a new instantiation that no
case runs, fails here; tests/test_gpu_f32_kernel_matrix.py then runs every
case of the same table against fp64."""
import re

import pytest

from _f32_cases import (F32_CASES, FLOP_CAP, NEVER_RAGGED_ROWS, REACHED, SEARCH_BOX, UNREACHED, epilogue, exact_ok,
                        flops, ids_of, key, label, name, ragged, tile)

IDS = [label(i) for i in range(len(F32_CASES))]


def _lines():
    return [ln for c in F32_CASES for ln in c["ids"] if not ln.startswith("aux:")]


@pytest.mark.parametrize("i", range(len(F32_CASES)), ids=IDS)
def test_case_selects_its_kernels(i):
    cs = F32_CASES[i]
    assert ids_of(cs) == cs["ids"]
    assert flops(cs["ids"]) <= FLOP_CAP
    assert exact_ok(cs)             # the exact pass's sums stay fp32 integers


def test_kernel_list_is_the_instantiated_set():
    """k_gemm: 19 operand-mode lines x 6 tiles and IM2T's 3 split-grid tiles at
    32-deep K-tiles and 7 x 5 at 16-deep ones; k_gemm2; 10 fp32 patch forms;
    the weight pack, 2 GEMVs, 3 column-matrix kernels and 5 split-K reduces."""
    from rramsim import ops
    ids = ops.f32_kernel_list()
    assert len(ids) == len(set(ids)) == 19 * 6 + 3 + 7 * 5 + 1 + 10 + 1 + 2 + 3 + 5
    im2t = [f"gemm<NCHW,IM2T,ROWMAJOR,32;{t}>" for t in ("32x128", "64x64", "128x128")]
    assert [k for k in ids if ",IM2T," in k] == im2t       # the split-grid tiles alone
    for k in ids:
        assert re.fullmatch(r"gemm<[A-Z0-9]+,[A-Z0-9]+,(ROWMAJOR|NCHW),(16|32);\d+x\d+>|gemm2<KCV,KCV,ROWMAJOR,3>|"
                            r"patch_f32<\d,\d,\d,\d>|patch_pack|gemv|gemv_groups|im2col4?|col2im|"
                            r"reduce(_groups|_nchw|_dwdb|_wave)?", k), k


def test_every_instantiation_has_a_case_or_a_reason():
    from rramsim import ops
    ids = set(ops.f32_kernel_list())
    covered = {name(ln) for ln in _lines()}
    assert covered <= ids, sorted(covered - ids)              # no case names a kernel that is not built
    assert not covered & set(UNREACHED), sorted(covered & set(UNREACHED))
    assert set(UNREACHED) <= ids, sorted(set(UNREACHED) - ids)
    missing = sorted(ids - covered - set(UNREACHED))
    assert not missing, f"instantiations without a case in F32_CASES or a reason in UNREACHED: {missing}"
    for k, why in UNREACHED.items():
        if why.startswith("selected only above the 2 GFLOP cap"):
            assert re.search(r"at \d+\.\d+ GFLOP$", why), (k, why)    # its least FLOP count
        else:
            boxes = re.findall(r"SEARCH_BOX\['(\w+)'\]", why)
            assert why.startswith("never launched:") or \
                (why.startswith("not found in the search box: ") and boxes and set(boxes) <= set(SEARCH_BOX)), (k, why)


def test_every_reached_id_keeps_its_case():
    """Each (instantiation, split or not) the search reached is run by a case."""
    assert sorted({key(ln) for ln in _lines()}) == sorted(REACHED)


def _tiles():
    return sorted({tile(ln)[0] for ln in _lines() if tile(ln)})


def test_tile_shapes_present():
    """Every tile launch<>() can choose below the cap, k_gemm2's and both patch tiles."""
    assert set(_tiles()) >= {"32x128", "64x64", "64x128", "96x128", "128x128", "192x128", "gemm2:128x128",
                             "patch:128x128", "patch:192x128"}


@pytest.mark.parametrize("t", ["32x128", "64x64", "64x128", "96x128", "128x128", "192x128", "gemm2:128x128"])
def test_ragged_tiles_per_tile_shape(t):
    """k_gemm's and k_gemm2's tiles (the patch kernel's ragged tiles: test_conv_patch_shapes_vs_fp64)."""
    rag = [ragged(ln) for ln in _lines() if tile(ln) and tile(ln)[0] == t]
    assert rag, t
    assert t in NEVER_RAGGED_ROWS or any(r[0] for r in rag), f"{t}: no case with a ragged last row tile"
    assert any(r[1] for r in rag), f"{t}: no case with a ragged last column tile"
    assert any(r[2] for r in rag), f"{t}: no case whose K is no multiple of the K-tile"


def test_epilogues_on_split_and_unsplit_cases():
    """ReLU and both bias modes on a split-K and on an unsplit case: row-major
    output through the dense cases (epilogue(i)), NCHW output through the
    convolution forwards (row bias is the only mode conv2d_fwd has; every
    convolution case runs with bias, with and without ReLU)."""
    for split in (False, True):
        dense = [epilogue(i) for i, c in enumerate(F32_CASES)
                 if c["entry"] == "gemm" and any(key(ln).endswith("/split") for ln in c["ids"]) == split]
        assert {1, 2} <= {e[2] for e in dense if e[3]}, f"split={split}: ReLU with both bias modes"
        assert {0.0} < {e[1] for e in dense}, f"split={split}: beta != 0"
        conv = [c for c in F32_CASES if c["entry"] == "conv_fwd" and
                any("NCHW," in ln for ln in c["ids"]) and any(ln == "reduce_nchw" for ln in c["ids"]) == split]
        assert conv, f"split={split}: no NCHW-output case"
    # a case may be the only cover of its kernel: its products must reach the result
    assert all(epilogue(i)[0] != 0.0 for i in range(len(F32_CASES)))


@pytest.mark.parametrize("t", ["64x128", "96x128", "128x128", "192x128"])
def test_large_dense_tiles_walk_several_k_tiles(t):
    """An unsplit dense case per large tile whose K spans more than two K-tiles and ends in a partial one."""
    assert any(c["entry"] == "gemm" and c["K"] > 64 and c["K"] % 32 != 0 and
               c["ids"][0].split(" ")[0].endswith(f";{t}>/s1") for c in F32_CASES), t


def test_backward_forms_present():
    bw = [c for c in F32_CASES if c["entry"] == "conv_bwd"]
    assert any(c["dw"] and not c["db"] and not c["dx"] for c in bw), "dw alone"
    assert any(c["dx"] and not c["dw"] and not c["db"] for c in bw), "dx alone"
    assert any(c["dw"] and c["db"] and c["g"] == 1 and any(ln in ("reduce_dwdb", "reduce_wave") for ln in c["ids"])
               and not any(ln.startswith("aux:bias_bwd") for ln in c["ids"]) for c in bw), "dw + db folded"
    assert any(c["dw"] and c["db"] and c["g"] > 1 and any(ln.startswith("aux:bias_bwd") for ln in c["ids"])
               for c in bw), "dw + db with groups (no fold)"
    # (the matrix runs every w_flipped case a second time without it, with room for the flipped kernel)
    assert any(c["dx"] and c["wflip"] for c in bw) and any(c["dx"] and not c["wflip"] for c in bw)
    assert any(ln == "reduce_wave" for c in bw for ln in c["ids"])
    ipb = [c for c in F32_CASES if c["entry"] == "ip_bwd"]
    assert any(c["t"] for c in ipb) and any(not c["t"] for c in ipb)
