"""Which support-layer kernels (csrc/layers.hip) each case of
tests/_layer_cases.py launches, that the table reaches every kernel of the
file, and that it reaches the branches inside them (host logic, no GPU).

ops.pool_fwd_kernel_ids and its siblings call the entry points themselves with
the launches recorded instead of issued, so no threshold (kPlaneMax,
kPlaneTile, kBwdPlaneMax, kAccSmall, kAccFusedBlocks, kLossFusedMax, the 1024
classes of the register softmax, the 2048-block rule) is restated there; a
change of one moves a case to another id, or to another planes-per-block count,
and fails here.  tests/test_gpu_layer_kernel_matrix.py runs the same table
against float64."""
import pytest

from _layer_cases import LAYER_CASES, all_ids, geom, ids_of, label, name, ppb, want_ids

IDS = [label(i) for i in range(len(LAYER_CASES))]
POOLS = [c for c in LAYER_CASES if c["entry"] == "pool"]
STAGED = [c for c in POOLS if ppb(c) is not None]


def _hw(c):
    return c["x"][2] * c["x"][3]


def _planes(c):
    return c["x"][0] * c["x"][1]


@pytest.mark.parametrize("i", range(len(LAYER_CASES)), ids=IDS)
def test_case_selects_its_kernels(i):
    cs = LAYER_CASES[i]
    assert ids_of(cs) == want_ids(cs)


def test_labels_are_unique():
    assert len(set(IDS)) == len(IDS)


def test_every_kernel_has_a_case():
    """Nothing of this file is unreachable at a few MB, so there is no list of exceptions."""
    from rramsim import ops
    ids = ops.layer_kernel_list()
    assert len(ids) == len(set(ids)) == 35
    covered = {name(ln) for c in LAYER_CASES for ln in all_ids(c)}
    assert covered == set(ids), (sorted(set(ids) - covered), sorted(covered - set(ids)))


def test_queries_report_errors_and_measure():
    import ctypes as C
    from rramsim import _kernels as K
    from rramsim import ops
    lib = K.load()
    assert lib.rram_softmax_kernel_ids(2, 10, 1, None, 0) == len("softmax_reg<16>\n")      # snprintf: measures
    buf = C.create_string_buffer(8)
    assert lib.rram_softmax_kernel_ids(2, 10, 1, buf, 8) == 16 and buf.value == b"softmax"  # truncated, terminated
    assert lib.rram_softmax_kernel_ids(2, 0, 1, buf, 8) == K.RRAM_EINVAL
    assert lib.rram_layer_entry_kernel_ids(99, 10, buf, 8) == K.RRAM_EINVAL
    assert ops.softmax_kernel_ids(0, 10, 1) == []          # nothing to do: nothing launched
    # the one-block loss + gradient takes 65536 elements and refuses one more
    assert ops.softmax_loss_kernel_ids("fwd_bwd", 8192, 8, 1) == ["softmax_loss_fwd_bwd"]
    with pytest.raises(K.RramError, match="more than 65536"):
        ops.softmax_loss_kernel_ids("fwd_bwd", 65537, 1, 1)
    # the entry points launch again after a query (the scope is closed)
    assert lib.rram_relu_fwd(None, None, 0, 0.0, None) == K.RRAM_OK


# ------------------------------------------------------------- pool forward
def test_staged_pool_planes_per_block():
    """ppb is the query's; the block count and the last block's planes follow from it."""
    for want in (2, 3):
        cs = [c for c in STAGED if ppb(c) == want and name(c["ids"][0]).startswith("pool_planes<")]
        assert any(_planes(c) % want != 0 for c in cs), f"ppb={want}: no case with a partial last block"
        assert all(-(-_planes(c) // want) >= 2048 for c in cs)
    c = LAYER_CASES[0]
    assert (_planes(c), _hw(c), ppb(c), -(-_planes(c) // 2), _planes(c) % 2) == (4099, 25, 2, 2050, 1)
    assert any(ppb(c) > 1 and ppb(c) * _hw(c) == 4096 for c in STAGED), "ppb at the LDS tile's limit"
    assert any(ppb(c) > 1 and _hw(c) % 4 != 0 for c in STAGED), "p0 H W not 16-byte aligned"
    assert any(ppb(c) > 1 and (ppb(c) * _hw(c)) % 4 != 0 for c in STAGED), "a block's input ends inside a 16-byte load"
    assert any(4096 < _hw(c) < 16384 and ppb(c) == 1 for c in STAGED)
    assert any(_hw(c) == 16384 for c in STAGED)
    assert all(_hw(c) <= 16384 for c in STAGED) and all(_hw(c) > 16384 for c in POOLS if ppb(c) is None)
    assert min(_hw(c) for c in POOLS if ppb(c) is None) == 129 * 128


def test_staged_pool_forms():
    by = {}
    for c in STAGED:
        by.setdefault(name(c["ids"][0]), []).append(c)
    assert set(by) == {"pool_planes<0>", "pool_planes<2>", "pool_planes<3>", "pool_planes_sep3"}
    for k in ("pool_planes<0>", "pool_planes<2>", "pool_planes<3>"):
        assert {c["mask"] for c in by[k]} == {True, False}, k
        assert {c["relu"] for c in by[k]} == {True, False}, k
    k0 = by["pool_planes<0>"]
    assert any(c["method"] == 0 and c["k"][0] != c["k"][1] for c in k0), "MAX with a non-square window"
    assert any(c["method"] == 1 and ppb(c) > 1 for c in k0), "AVE with several planes per block"
    for f in ("s", "p"):
        assert any(c[f][0] != c[f][1] for c in k0), f
    assert any(c["x"][2] != c["x"][3] for c in k0)
    assert {c["off"] for c in STAGED if ppb(c) > 1} >= {0, 1, 2, 3}, "input base offsets of 0..3 floats"
    sep = by["pool_planes_sep3"]
    assert all(not c["mask"] and c["k"] == (3, 3) and c["s"] == (1, 1) and c["method"] == 0 for c in sep)
    assert any(ppb(c) > 1 and geom(c)[4] > 8 and geom(c)[4] % 8 != 0 and _planes(c) % ppb(c) for c in sep)
    assert any(_hw(c) == 4096 for c in sep)
    assert {c["relu"] for c in sep} == {True, False}


def test_direct_pool_forms():
    d = [c for c in POOLS if ppb(c) is None]
    f3 = [c for c in d if c["ids"] == ["pool_max_fixed<3>"]]
    assert {c["p"] == (0, 0) for c in f3} == {True, False}, "padded and unpadded"
    assert any(c["ids"] == ["pool_max_fixed<2>"] for c in d)
    gen = [c for c in d if c["ids"] == ["pool_fwd"]]
    assert any(c["method"] == 0 and c["k"] == (5, 3) for c in gen)
    assert any(c["method"] == 1 and c["p"] != (0, 0) for c in gen)
    assert {c["mask"] for c in d} == {True, False} and {c["relu"] for c in d} == {True, False}


def test_pool_backward_forms():
    b = [c for c in POOLS if c["bwd"]]
    pl = [c for c in b if c["bwd"] == ["pool_bwd_plane"]]
    el = [c for c in b if c["bwd"] == ["pool_bwd"]]
    assert any(_hw(c) == 4096 and geom(c)[4] * geom(c)[5] == 1024 for c in pl), "both limits of the plane form"
    assert any(c["method"] == 0 and _hw(c) > 4096 for c in el)
    assert any(c["method"] == 0 and _hw(c) <= 4096 and geom(c)[4] * geom(c)[5] > 1024 for c in el)
    assert any(c["method"] == 1 and c["p"] != (0, 0) and c["k"][0] != c["k"][1] and c["x"][2] != c["x"][3]
               for c in el)
    for grp in (pl, el):
        assert {c["relu"] for c in grp} == {True, False}


# ---------------------------------------------------------------------- LRN
def test_lrn_forms():
    lrn = [c for c in LAYER_CASES if c["entry"] == "lrn"]
    for size in (3, 5):
        sl = [c for c in lrn if c["ids"][0] == f"lrn_fwd_slide<{size}>"]
        assert {c["x"][1] for c in sl} == {1, 2, 4, 8, 9, 17}
        assert {c["scale"] for c in sl} == {True, False}
        assert any(c["x"][0] * c["x"][2] * c["x"][3] == 257 for c in sl), "a second block with one live thread"
        assert any(c["x"][0] > 1 for c in sl)
    gen = [c for c in lrn if c["ids"][0] == "lrn_fwd"]
    assert {c["size"] for c in gen} == {1, 7, 9}
    for size in (7, 9):
        assert {c["x"][1] < size for c in gen if c["size"] == size} == {True, False}
    assert {c["size"] for c in lrn if c["bwd"]} >= {1, 3, 5, 7, 9}
    w = [c for c in LAYER_CASES if c["entry"] == "within"]
    assert {c["size"] for c in w} == {1, 3, 5, 7}
    assert any(c["x"][2] < c["size"] and c["x"][3] < c["size"] for c in w)
    pl = [c for c in w if c["ids"][1] == "lrn_within_bwd_plane"]
    el = [c for c in w if c["ids"][1] == "lrn_within_bwd"]
    assert any(_hw(c) == 4096 for c in pl) and any(256 < _hw(c) < 512 for c in pl)
    assert min(_hw(c) for c in el) == 65 * 64
    for grp in (pl, el):
        assert {c["relu"] for c in grp} == {True, False}


# ------------------------------------------------------------------ softmax
def test_softmax_forms():
    sm = [c for c in LAYER_CASES if c["entry"] == "softmax"]
    reg = {c["C"] for c in sm if c["ids"] == ["softmax_reg<16>"]}
    col = {c["C"] for c in sm if c["ids"] == ["softmax"]}
    assert reg >= {1, 63, 64, 65, 1024} and max(reg) == 1024 and col >= {1025, 2049} and min(col) == 1025
    for grp in (reg, col):
        assert {c["inner"] for c in sm if c["C"] in grp} >= {1, 3}
    assert any((c["outer"] * c["inner"]) % 4 for c in sm)
    # 2048 blocks of 4 waves: above 8192 columns the grid-stride loop iterates, and its last pass is partial
    assert any(c["outer"] * c["inner"] > 8192 and c["inner"] == 1 for c in sm)
    assert any(c["outer"] * c["inner"] > 8192 and c["inner"] > 1 for c in sm)


def test_softmax_loss_forms():
    ls = [c for c in LAYER_CASES if c["entry"] == "loss"]
    for form in ("fwd", "fwd_bwd", "bwd"):
        f = [c for c in ls if c["form"] == form]
        assert any(c["outer"] * c["inner"] > 1024 and c["inner"] > 1 for c in f), form     # > 1 column per thread
        assert any(c["ignore"] >= 0 and c["inner"] > 1 and not c["data"] for c in f), form
        assert any(c["data"] == "all_ignored" for c in f), form
    assert any(c["data"] == "clamp" for c in ls)
    assert any(c["form"] == "fwd_bwd" and c["outer"] * c["C"] * c["inner"] == 65536 for c in ls)
    assert any(c["form"] == "fwd_groups" and c["fold"] and 0 < c["live"] < c["G"] for c in ls)
    assert {("count_valid" in c["ids"]) for c in ls if c["form"] == "bwd"} == {True, False}


def test_accuracy_plans():
    ac = [c for c in LAYER_CASES if c["entry"] == "acc"]
    plans = {tuple(c["ids"]) for c in ac}
    assert plans >= {("accuracy_small",), ("accuracy_fused",), ("accuracy", "accuracy_ratio"), ("accuracy",),
                     ("accuracy_small_groups", "fold_groups")}
    assert {c["C"] for c in ac if c["ids"] == ["accuracy_fused"]} >= {1024, 1025}


def test_flat_counts():
    for c in LAYER_CASES:
        if "n" in c:
            assert c["n"] % 256 != 0, c
    eu = [c["n"] for c in LAYER_CASES if c["entry"] == "euclidean"]
    assert min(eu) < 64 and max(eu) > 1024
