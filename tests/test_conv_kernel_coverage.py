"""Which bf16x6 convolution kernel each shape of tests/_x6_cases.py selects,
and that the table reaches every instantiation (host logic, no GPU).

ops.conv_fwd_kernel_id asks the launch paths' own plan functions, so a planner
change that moves a shape to another kernel, or a new instantiation that no
test shape runs, fails here; tests/test_gpu_conv_kernel_matrix.py then runs
every entry of the same table against fp64."""
import itertools
import re

import pytest

from _x6_cases import REACHED, SEARCH_BOX, UNREACHED, X6_CASES, desc, family, ragged, strip_kind

CB_KINDS = ("contig", "perimg", "rowalign", "whole")


def _ids():
    return [c["id"] for c in X6_CASES]


@pytest.mark.parametrize("cs", X6_CASES, ids=_ids())
def test_case_selects_its_kernel(cs):
    from rramsim import ops
    assert ops.get_f32_engine() == ops.ENGINE_BF16X6
    assert ops.conv_fwd_kernel_id(desc(cs), cs["align16"]) == cs["id"]
    prev = ops.set_f32_engine(ops.ENGINE_F32)
    try:
        assert ops.conv_fwd_kernel_id(desc(cs), cs["align16"]) == "f32"
    finally:
        ops.set_f32_engine(prev)


def test_kernel_list_is_the_instantiated_set():
    """10 + 3 x 2 channel-octet, 8 dma v4 + 8 ring v1 + 3 ring v4 1x1, 9 x 2 patch, 2 fixed."""
    from rramsim import ops
    ids = ops.conv_fwd_kernel_list()
    assert len(ids) == len(set(ids)) == 10 + 6 + 19 + 18 + 2
    for k in ids:
        assert re.fullmatch(r"(cb|cb16|c1x1|c1x1_dma|patch|conv1_ring|conv_s2)<[0-9,]+(;[kv][0-9])?>", k), k


def test_1x1_planner_selects_only_built_forms():
    """The 1x1 forms that are not built are the ones the host cannot select:
    the LDS-DMA form needs 16-byte loads (conv_1x1_dma), and with 16-byte loads
    the register ring is left num_output <= 64, for which conv_1x1_plan takes
    no tile of 32 MI WR >= 128 rows.  A sweep over num_output (every tile-row
    threshold and the DMA threshold included), HW % 4 both ways and both input
    alignments must never select a missing form (the id would read "f32")."""
    from rramsim import ops
    built = set(ops.conv_fwd_kernel_list())
    for (h, w), n, al in itertools.product([(7, 4), (7, 7), (15, 15), (14, 17)], (1, 8), (True, False)):
        for m in range(1, 521):
            kid = ops.conv_fwd_kernel_id(ops.conv_desc((n, 16, h, w), m, 1, 1, 0, 1, 1), al)
            where = (n, h, w, m, al, kid)
            assert kid.startswith("c1x1"), where
            assert strip_kind(kid) in built, where
            mi, _, wr = (int(v) for v in kid[kid.index("<") + 1:kid.index(";")].split(","))
            if family(kid) == "c1x1_dma":
                assert not kid.endswith("v1>"), where
            elif kid.endswith("v4>"):
                assert 32 * mi * wr <= 64, where


def test_every_instantiation_has_a_case_or_a_reason():
    from rramsim import ops
    ids = set(ops.conv_fwd_kernel_list())
    covered = {strip_kind(k) for k in _ids()}
    assert covered <= ids, sorted(covered - ids)                      # no case names a kernel that is not built
    assert not covered & set(UNREACHED), sorted(covered & set(UNREACHED))
    assert set(UNREACHED) <= ids, sorted(set(UNREACHED) - ids)
    missing = sorted(ids - covered - set(UNREACHED))
    assert not missing, f"instantiations without a case in X6_CASES or a reason in UNREACHED: {missing}"
    for k, why in UNREACHED.items():
        assert why.startswith(("never launched:", "selected only above the 2 GFLOP cap")) or \
            any(box in why for box in SEARCH_BOX.values()), (k, why)


def test_every_reached_id_keeps_its_case():
    """Each (instantiation, tiling kind, parity) the search reached is run by a case."""
    assert sorted(set(_ids())) == sorted(REACHED)


def test_every_case_is_needed():
    """One case per id (tiling kind included), plus the extra ragged / partial-octet shapes."""
    ids = _ids()
    dup = sorted({k for k in ids if ids.count(k) > 1})
    for k in dup:
        extra = [c for c in X6_CASES if c["id"] == k][1:]
        assert all((c["cout"] // c["g"]) % 8 != 0 or any(ragged(c, k)) for c in extra), k


def test_tiling_kinds_and_parities():
    ids = _ids()
    kinds = {(family(k), k.split("/")[1]) for k in ids if "/" in k}
    # the six tiling kinds of the channel-octet planner
    for want in [("cb", "contig"), ("cb", "perimg"), ("cb16", "contig"), ("cb16", "perimg"), ("cb16", "rowalign"),
                 ("cb16", "whole")]:
        assert want in kinds, want
    for form in ("5,4,4,8,2", "3,4,4,8,2", "3,2,2,8,2"):
        for par in ("k0", "k1"):
            assert any(k.startswith(f"cb16<{form};{par}>") for k in ids), (form, par)
        assert any(k.startswith(f"cb16<{form};") and k.endswith("/whole") for k in ids), form


@pytest.mark.parametrize("fam", ["cb", "cb16", "c1x1", "c1x1_dma", "patch"])
def test_ragged_tiles_per_family(fam):
    rag = [ragged(c, c["id"]) for c in X6_CASES if family(c["id"]) == fam]
    assert any(r[0] for r in rag), f"{fam}: no case with a ragged last row tile"
    assert any(r[1] for r in rag), f"{fam}: no case with a ragged last column tile"


def test_partial_octet_groups_present():
    """Channel-octet cases whose groups hold no whole number of octets (the
    companion is packed after the kernel) while num_output % 8 == 0."""
    for fam in ("cb", "cb16"):
        assert any(family(c["id"]) == fam and (c["cout"] // c["g"]) % 8 != 0 and c["cout"] % 8 == 0
                   for c in X6_CASES), fam
