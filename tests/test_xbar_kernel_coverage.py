"""Which crossbar kernels each case of tests/_xbar_matrix.py launches, and that
the table reaches every id of ops.xbar_kernel_list() and every named plan
branch of every read-out kernel (host logic, no GPU).

The *_kernel_ids queries run the entry points' own planning code with the
launches recorded instead of issued; tests/test_gpu_xbar_matrix.py then runs
every case of the same table against its numpy reference.  A case that is the
only cover of an id or of a branch cannot leave the table unnoticed: the
assertion that misses it names the kernel and the branch."""
import re

import numpy as np
import pytest

from _xbar_matrix import (LABELS, MNK_CAP, MNK_CAP_CHUNKED, XBAR_CASES, bf16_terms, compute, counts, conv_out, dims,
                          family_of, name, plan, query, readout, reference, workload)

FAMILIES = ["ip", "ip_t", "ip_bs;p4", "ip_bs;p7", "ip_ws", "ip_ss;d2", "ip_ss;d3", "conv"]
FP32 = ["ip", "ip_t", "ip_bs;p4", "ip_bs;p7", "conv"]
UNREACHED = {}      # id -> reason; none


def cases_of(fam):
    return [c for c in XBAR_CASES if family_of(c) == fam]


@pytest.mark.parametrize("label", LABELS)
def test_case_selects_its_kernels(label):
    c = XBAR_CASES[LABELS.index(label)]
    assert c["ids"] and query(c, "kernel_ids") == c["ids"]
    assert workload(c) <= (MNK_CAP_CHUNKED if plan(c)["chunks"] > 1 else MNK_CAP), workload(c)
    # a case may be the only cover of its kernel: it cannot pass on zeros (its conditions are asserted on the way)
    assert np.abs(reference(label)[3]).max() > 0


def test_kernel_list_is_the_recordable_set():
    from rramsim import ops
    ids = ops.xbar_kernel_list()
    assert len(ids) == len(set(ids)) == 24
    for k in ids:
        assert re.fullmatch(r"xbar:(pack(_codes|_i8|_sm8|_wslices)?<(vec|scalar)>|(ip|ip_t|conv)<(vec|scalar)>|"
                            r"ip_bs<(vec|scalar);p[47]>|ip_ws<p4>|ip_ss<d[23];p4>|finish)", k), k


def test_every_id_has_a_case_or_a_reason():
    from rramsim import ops
    ids = set(ops.xbar_kernel_list())
    covered = {name(ln) for c in XBAR_CASES for ln in c["ids"]}
    assert covered <= ids, sorted(covered - ids)
    assert set(UNREACHED) <= ids and not covered & set(UNREACHED)
    missing = sorted(ids - covered - set(UNREACHED))
    assert not missing, f"ids without a case in XBAR_CASES or a reason in UNREACHED: {missing}"


BRANCHES = {
    "more than one row tile, the last ragged": lambda c, p: p["rag_m"],
    "more than one column tile, the last ragged": lambda c, p: p["rag_n"],
    "K % 32 != 0": lambda c, p: p["k32"],
    "a short last crossbar tile": lambda c, p: p["short"] and p["ntiles"] > 1,
    "rows = 32": lambda c, p: p["R"] == 32,
    "rows >= 256": lambda c, p: p["R"] >= 256,
    "one slab": lambda c, p: p["split"] * p["chunks"] == 1,
    "several slabs, the last split of fewer tiles": lambda c, p: p["rag_split"],
    "fewer than 8 workgroups": lambda c, p: p["wgs"] < 8,
    "more than 8 workgroups, no multiple of 8": lambda c, p: p["wgs"] > 8 and p["wgs"] % 8 != 0,
}


@pytest.mark.parametrize("branch", list(BRANCHES))
@pytest.mark.parametrize("fam", FAMILIES)
def test_plan_branches_per_kernel(fam, branch):
    assert any(BRANCHES[branch](c, plan(c)) for c in cases_of(fam)), f"{fam}: no case with {branch}"


def test_rows_1024_on_an_fp32_kernel():
    assert any(c["cfg"][0] == 1024 for f in FP32 for c in cases_of(f)), "no fp32 read-out with rows = 1024"


def _vec(c, prefix):
    """Whether the case's id starting with prefix is the <vec> one."""
    return [ln for ln in c["ids"] if ln.startswith(prefix)][0].startswith(prefix + "<vec")


def _axes(c):
    """The case's two <vec|scalar> axes as (id prefix, aligned flag, row length) for the activations and the weights."""
    rows, cols, red, _ = dims(c)
    e = c["entry"]
    xid = {"ip": "xbar:pack", "bwd": "xbar:pack", "bs": "xbar:pack_codes", "ws": "xbar:pack_i8", "ss": "xbar:pack_sm8"}
    wid = {"ip": "xbar:ip", "bwd": "xbar:ip_t", "bs": "xbar:ip_bs", "ws": "xbar:pack_wslices", "ss": "xbar:pack_wslices",
           "conv": "xbar:conv"}
    axes = [] if e == "conv" else [(xid[e], c["xa"], red)]
    return axes + [(wid[e], c["wa"], cols if e == "bwd" else red)]


@pytest.mark.parametrize("fam", FAMILIES)
def test_alignment_pairs_per_kernel(fam):
    cs = cases_of(fam)
    pairs = {tuple(_vec(c, a[0]) for a in _axes(c)) for c in cs}
    want = {(True,), (False,)} if fam == "conv" else {(a, b) for a in (True, False) for b in (True, False)}
    assert pairs >= want, f"{fam}: (activation, weight) <vec> pairs missing: {sorted(want - pairs)}"
    for i in range(len(_axes(cs[0]))):
        ax = [_axes(c)[i] for c in cs]
        ids = [_vec(c, _axes(c)[i][0]) for c in cs]
        assert any(not v and not a[1] and a[2] % 4 == 0 for v, a in zip(ids, ax)), \
            f"{fam}: {ax[0][0]} never scalar through the pointer alone (row length % 4 == 0)"
        assert any(not v and a[1] and a[2] % 4 != 0 for v, a in zip(ids, ax)), \
            f"{fam}: {ax[0][0]} never scalar through the row length alone (aligned pointer)"


@pytest.mark.parametrize("fam", FP32)
def test_wide_operands_per_fp32_kernel(fam):
    """Each wide class on a <vec> read-out and on a <scalar> one with ragged tiles."""
    for kind in ("wide_w",) if fam.startswith("ip_bs") else ("wide_x", "wide_w"):
        cs = [c for c in cases_of(fam) if c["kind"] == kind]
        assert any(_vec(c, readout(c).split("<")[0]) for c in cs), f"{fam}: no {kind} case on <vec> loads"
        assert any(not _vec(c, readout(c).split("<")[0]) and all(not _vec(c, a[0]) for a in _axes(c)) and
                   (plan(c)["rag_m"] or plan(c)["rag_n"]) and plan(c)["k32"] and plan(c)["short"] for c in cs), \
            f"{fam}: no {kind} case on scalar loads with several tiles, the last ragged, and a K tail"


WIDE = [c["label"] for c in XBAR_CASES if c["kind"].startswith("wide")]


@pytest.mark.parametrize("label", WIDE)
def test_wide_cases_see_every_bf16_term(label):
    """From the reference alone: with the low (and, separately, the middle) bf16 term of the wide operand zeroed,
    most outputs of the case change, so a kernel that loses or misplaces that term cannot pass.  The signed
    round-to-nearest split covers 17 bits with h and m, so about a third of the elements carry a low term (at least
    a quarter is asserted); an output sums several pairs of them.  "Most" is more than half of the outputs that are
    non-zero before or after."""
    c = XBAR_CASES[LABELS.index(label)]
    x, w, bias, y = reference(label)
    for drop in (2, 1):
        ops_ = [np.array(x), np.array(w)]
        i = 0 if c["kind"] == "wide_x" else 1
        t = bf16_terms(ops_[i])
        assert all(np.count_nonzero(v) >= v.size // 4 for v in t), label
        ops_[i] = sum(t[j] for j in range(3) if j != drop)
        y2 = compute(c, ops_[0], ops_[1], bias)[0]
        live = (y != 0) | (y2 != 0)
        assert (y2 != y).sum() > 0.5 * live.sum() > 0, (label, "lmh"[2 - drop], int((y2 != y).sum()), int(live.sum()))


def test_chunk_states():
    planes = {counts(c)[0] for c in XBAR_CASES if c["entry"] == "bs"}
    assert planes >= {1, 4, 5, 7, 8, 14, 15} and planes & {2, 3}, f"bit-serial plane counts: {sorted(planes)}"
    ws = [c for c in XBAR_CASES if c["entry"] == "ws"]
    assert {counts(c)[0] for c in ws} >= set(range(1, 8)), "ws: a slice count in 1 .. 7 has no case"
    assert any(counts(c)[0] > 1 and (c["sl"][0] - 1) % c["sl"][1] for c in ws), "ws: no narrower top slice"
    ss = [c for c in XBAR_CASES if c["entry"] == "ss"]
    assert {counts(c)[1] for c in ss} >= set(range(1, 8)), "ss: a digit count in 1 .. 7 has no case"
    assert {c["db"] for c in ss if c["cfg"][3] == 8} >= set(range(1, 8)), "ss: a digit_bits in 1 .. 7 at 8 DAC bits"
    assert any(c["cfg"][3] < 8 and counts(c)[1] > 1 and (c["cfg"][3] - 1) % c["db"] for c in ss), \
        "ss: no case with fewer DAC bits, several digits and a narrower top digit"
    d3 = [counts(c) for c in cases_of("ip_ss;d3")]
    assert any(nd == 3 for _, nd in d3), "ss <d3;p4>: never one full chunk"
    assert any(nd % 3 == 2 for _, nd in d3), "ss <d3;p4>: never a last chunk of two digits"
    assert any(nd > 3 and nd % 3 and ns > 4 and ns % 4 for ns, nd in d3), \
        "ss: no case with several digit chunks x several slice chunks, the last of each unfull"
    assert any(nd == 4 for _, nd in [counts(c) for c in cases_of("ip_ss;d2")]), "ss <d2;p4>: never two chunks"
    assert sum(counts(c)[1] == 1 for c in ss) >= 3, "ss: one-digit cases (equal to ws) missing"


def test_convolution_geometries():
    cv = [c for c in XBAR_CASES if c["entry"] == "conv"]
    g = [c["geom"] for c in cv]
    assert any(x[13] > 1 and x[4] // x[13] > 128 for x in g), "conv: no groups > 1 with Ng > 128"
    assert any(x[5:7] == (11, 11) and x[9:11] == (4, 4) for x in g), "conv: no 11x11 stride-4 kernel"
    assert any(x[5:7] == (1, 1) for x in g), "conv: no 1x1 kernel"
    assert any(x[11] > 1 or x[12] > 1 for x in g), "conv: no dilation"
    def spans(x):                                       # some tile [128 t, 128 t + 128) holds an image boundary
        hw, m = conv_out(x)[0] * conv_out(x)[1], x[0] * conv_out(x)[0] * conv_out(x)[1]
        return any(t < b < min(t + 128, m) for t in range(0, m, 128) for b in range(hw, m, hw))
    assert any(spans(x) for x in g), "conv: no position tile that spans images"
    assert any(c["bias"] and c["geom"][13] > 1 for c in cv), "conv: no bias with groups"


def test_epilogues_and_clipping_per_kernel():
    for fam in FAMILIES:
        cs = cases_of(fam)
        assert any(c["clip"] for c in cs), f"{fam}: no case whose ADC clips"
        if fam != "ip_t":
            for split in (False, True):
                assert any(c["bias"] and c["relu"] and (plan(c)["split"] * plan(c)["chunks"] > 1) == split for c in cs), \
                    f"{fam}: no bias + ReLU case with {'several slabs' if split else 'one slab'}"
    for e in ("bs", "ws", "ss"):
        assert any(c["entry"] == e and c["kind"] == "odd_scale" for c in XBAR_CASES), f"{e}: no odd_scale case"


def test_empty_shapes_launch_nothing():
    from rramsim import ops
    cfg, sl = ops.xbar_cfg(32, 8, 4.0, 8, 1.0), ops.xbar_slices(8, 2, 1.0)
    for M, N in ((0, 16), (8, 0)):
        assert ops.ip_fwd_xbar_kernel_ids(M, N, 64, cfg) == []
        assert ops.ip_fwd_xbar_bs_kernel_ids(M, N, 64, cfg) == []
        assert ops.ip_fwd_xbar_ws_kernel_ids(M, N, 64, cfg, sl) == []
        assert ops.ip_fwd_xbar_ss_kernel_ids(M, N, 64, cfg, sl, 2) == []
        assert ops.ip_bwd_data_xbar_kernel_ids(M, 64, N, cfg) == []          # bwd: M = 0 and K = 0
    assert ops.conv_fwd_xbar_kernel_ids(ops.conv_desc((0, 3, 5, 5), 4, 3), cfg) == []    # (no zero-channel descriptor)
