#!/usr/bin/env python3
"""Search the boxes of tests/_f32_cases.py (SEARCH_BOX) through the fp32
engine's kernel-id queries and write the generated block of that file:
per (instantiation, split or not) the cheapest case, per tile shape the
cheapest ragged-row / ragged-column / ragged-K cases, and a reason for every
listed id no case runs.  Host only (no GPU).

    python scripts/find_f32_cases.py            # report
    python scripts/find_f32_cases.py --write    # rewrite tests/_f32_cases.py
    python scripts/find_f32_cases.py --dump F   # every planner answer per searched case (to diff two builds)
"""
import itertools
import pprint
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "rram-caffe-simulation_amd" / "python"), str(ROOT / "tests")]

import _f32_cases as F  # noqa: E402
from rramsim import _kernels as Kmod  # noqa: E402
from rramsim import ops  # noqa: E402

MiB = 1 << 20


def dense():
    Ms = (1, 20, 32, 33, 60, 64, 90, 96, 100, 128, 180, 192, 250, 256, 570)
    Ns = (5, 64, 65, 100, 500, 1000, 4097, 21761, 32641, 32768, 65409)
    Ks = (1, 8, 36, 68, 100, 256, 260, 800, 1027, 4096)
    for ta, tb, a16, b16, ws, K, N, M in itertools.product((0, 1), (0, 1), (True, False), (True, False), (0, 64 * MiB),
                                                           Ks, Ns, Ms):
        if 2 * M * N * K <= F.FLOP_CAP * 8:
            yield dict(entry="gemm", ta=ta, tb=tb, M=M, N=N, K=K, a16=a16, b16=b16, ws=ws)


def ip():
    Ms, Ns, Ks = (1, 2, 3, 8, 64, 128, 250), (5, 10, 100, 130, 500, 1000), (7, 50, 66, 256, 800, 4096)
    for t, ws, K, N, M in itertools.product((0, 1), (0, 64 * MiB), Ks, Ns, Ms):
        for bias, relu in ((True, False), (True, True), (False, True)):
            yield dict(entry="ip_fwd", M=M, N=N, K=K, t=t, bias=bias, relu=relu, ws=ws)
        if ws == 0:
            for dw, db, dx in ((1, 1, 1), (1, 0, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1)):
                yield dict(entry="ip_bwd", M=M, N=N, K=K, t=t, dw=dw, db=db, dx=dx)
        for G in (2, 3):
            yield dict(entry="ip_groups", G=G, M=M, N=N, K=K, t=t, ws=ws)


def conv():
    for n, c, h, cout, k, s, dil, g, w16 in itertools.product((1, 2, 8), (1, 3, 4, 16, 20, 128), (8, 12, 28, 32, 64, 128,
                                                                                                  256, 512),
                                                              (16, 20, 32, 64, 96, 128, 192, 256, 2560, 2592, 2880),
                                                              (1, 3, 5, 7, 9),
                                                              (1, 2), (1, 2), (1, 2), (True, False)):
        if c % g or cout % g:
            continue
        for p in sorted({0, k // 2}):
            if h + 2 * p < dil * (k - 1) + 1:
                continue
            base = dict(x=(n, c, h, h), cout=cout, k=k, s=s, p=p, d=dil, g=g, w16=w16)
            ho = (h + 2 * p - dil * (k - 1) - 1) // s + 1
            if 2 * n * cout * ho * ho * (c // g) * k * k > F.FLOP_CAP * 8 or n * c * h * h > 1 << 24:
                continue
            yield dict(entry="conv_fwd", **base)
            if not w16 or 3 * 2 * n * cout * ho * ho * (c // g) * k * k > F.FLOP_CAP:
                continue
            d = F.conv_desc(base)
            wt = c * (cout // g) * k * k * 4
            col1 = (c * k * k + 1) * d.out_h * d.out_w * 4        # one image's column matrix, no split-K partials
            for ws in sorted({ops.conv2d_bwd_workspace(d, 1), ops.conv2d_bwd_workspace(d, n), col1, wt}):
                for dw, db, dx in ((1, 0, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1)):
                    for wflip in (False, True):
                        if wflip and not dx:
                            continue
                        yield dict(entry="conv_bwd", **base, dw=dw, db=db, dx=dx, ws=ws, wflip=wflip)


def ws_sweep():
    """conv_bwd across every edge of the image-chunk plan: per group count the
    F32_CASES weight-gradient case with the most output positions, at batch 1,
    2 and 8, with the workspace of each chunk size 1..batch, those +-4 and
    +-256 bytes (the partials' 256-byte rounding) and halved."""
    for g in (1, 2):
        pick = max((c for c in F.F32_CASES if c["entry"] == "conv_bwd" and c["dw"] and c["g"] == g),
                   key=lambda c: F.conv_desc(c).out_h * F.conv_desc(c).out_w)
        for n in (1, 2, 8):
            base = dict({k: v for k, v in pick.items() if k != "ids"}, x=(n,) + tuple(pick["x"][1:]), wflip=False)
            d = F.conv_desc(base)
            full = [ops.conv2d_bwd_workspace(d, m) for m in range(1, n + 1)]
            for ws in sorted({w + e for w in full for e in (0, -4, 4, -256, 256)} | {w // 2 for w in full}):
                for dw, db, dx in ((1, 0, 0), (1, 1, 0), (1, 1, 1), (0, 0, 1)):
                    if ws >= 0:
                        yield dict(base, dw=dw, db=db, dx=dx, ws=ws)


def dump(path):
    """One line per searched case with the planner's whole answer (or its
    error text): two builds whose files are equal plan every case alike."""
    n = 0
    with open(path, "w") as f:
        for cs in itertools.chain(dense(), ip(), conv(), F.F32_CASES, ws_sweep()):
            cs = {k: v for k, v in cs.items() if k != "ids"}
            try:
                ans = " | ".join(F.ids_of(cs))
            except Kmod.RramError as e:
                ans = f"RramError: {e}"
            f.write(f"{cs!r}\t{ans}\n")
            n += 1
    print(f"# {n} cases dumped to {path}", file=sys.stderr)


def _aux(c, prefix):
    return any(ln.startswith(prefix) for ln in c["ids"])


# call forms the table must hold whatever the cheapest case per id looks like
FORMS = {
    "bwd dw alone": lambda c: c["entry"] == "conv_bwd" and c["dw"] and not c["db"] and not c["dx"],
    "bwd dx alone": lambda c: c["entry"] == "conv_bwd" and c["dx"] and not c["dw"] and not c["db"] and not c["wflip"],
    "bwd dx alone, w_flipped": lambda c: c["entry"] == "conv_bwd" and c["dx"] and not c["dw"] and c["wflip"],
    "bwd dw + db folded": lambda c: c["entry"] == "conv_bwd" and c["dw"] and c["db"] and c["g"] == 1 and
    not _aux(c, "aux:bias_bwd"),
    "bwd dw + db, groups": lambda c: c["entry"] == "conv_bwd" and c["dw"] and c["db"] and c["g"] > 1 and
    _aux(c, "aux:bias_bwd") and c["x"][0] > 1,
    "ip_bwd": lambda c: c["entry"] == "ip_bwd" and not c["t"] and c["dw"] and c["db"] and c["dx"] and c["M"] > 1,
    "ip_bwd transposed": lambda c: c["entry"] == "ip_bwd" and c["t"] and c["dw"] and c["db"] and c["dx"] and c["M"] > 1,
    **{f"dense {t}, unsplit, K over several K-tiles and ragged": (lambda c, t=t: c["entry"] == "gemm" and c["K"] > 64 and
       c["K"] % 32 != 0 and c["ids"][0].split(" ")[0].endswith(f";{t}>/s1"))
       for t in ("64x128", "96x128", "128x128", "192x128")},
    "ip_fwd gemv": lambda c: c["entry"] == "ip_fwd" and c["ids"][0] == "gemv" and c["bias"] and c["relu"] and c["K"] > 64,
}


def main():
    if "--dump" in sys.argv:
        return dump(sys.argv[sys.argv.index("--dump") + 1])
    listed = ops.f32_kernel_list()
    best, over, rag, forms = {}, {}, {}, {}
    n = 0
    for cs in itertools.chain(dense(), ip(), conv()):
        try:
            lines = F.ids_of(cs)
        except Kmod.RramError:
            continue                      # the entry point rejects the arguments (e.g. workspace too small)
        n += 1
        if not lines or any(ln.startswith("x6:") for ln in lines):
            continue
        fl = flops = F.flops(lines)
        cs = dict(cs, ids=lines)
        if fl <= F.FLOP_CAP and F.exact_ok(cs):
            for nm, pred in FORMS.items():
                if pred(cs) and (nm not in forms or fl < forms[nm][0]):
                    forms[nm] = (fl, cs)
        for ln in lines:
            if ln.startswith("aux:"):
                continue
            k = F.key(ln)
            if fl > F.FLOP_CAP or not F.exact_ok(cs):
                if k not in over or flops < over[k][0]:
                    over[k] = (flops, cs)
                continue
            if k not in best or (fl, len(lines)) < (best[k][0], len(best[k][1]["ids"])):
                best[k] = (fl, cs)
            t = F.tile(ln)
            if t:
                for j, r in enumerate(F.ragged(ln)):
                    if r and ((t[0], j) not in rag or fl < rag[(t[0], j)][0]):
                        rag[(t[0], j)] = (fl, cs)
    cases, seen = [], set()

    def add(cs):
        tag = repr(sorted((k, v) for k, v in cs.items() if k != "ids"))
        if tag not in seen:
            seen.add(tag)
            cases.append(cs)

    for k in sorted(best):
        if not any(k in map(F.key, c["ids"]) for c in cases):
            add(best[k][1])
    for tj in sorted(rag):
        if not any(F.tile(ln) and F.tile(ln)[0] == tj[0] and F.ragged(ln)[tj[1]] for c in cases for ln in c["ids"]):
            add(rag[tj][1])
    for nm in FORMS:
        add(forms[nm][1])
    reached = sorted({F.key(ln) for c in cases for ln in c["ids"] if not ln.startswith("aux:")})
    covered = {F.name(k.replace("/split", "").replace("/one", "")) for k in reached}
    unreached = {}
    for kid in listed:
        if kid in covered:
            continue
        ov = [(v[0], v[1]) for k, v in over.items() if F.name(k.replace("/split", "").replace("/one", "")) == kid]
        if ov:
            fl, cs = min(ov, key=lambda t: t[0])
            unreached[kid] = (f"selected only above the {F.FLOP_CAP / 1e9:g} GFLOP cap on a case: the least in the boxes "
                              f"(searched up to 8 x the cap) is { {k: v for k, v in cs.items() if k != 'ids'} } at "
                              f"{fl / 1e9:.2f} GFLOP")
        else:
            fam = "gemm" if "ROWMAJOR" in kid and "NCHW," not in kid and "NCHWT" not in kid else "conv"
            unreached[kid] = NEVER.get(kid) or ("not found in the search box: SEARCH_BOX[" +
                                                ("'gemm'] and SEARCH_BOX['ip']" if fam == "gemm" else "'conv']"))
    print(f"{n} queries; {len(listed)} listed ids, {len(covered & set(listed))} covered by {len(cases)} cases, "
          f"{len(unreached)} unreached ({sum(v.startswith('selected only') for v in unreached.values())} above the cap)")
    stray = covered - set(listed)
    assert not stray, stray
    if "--write" in sys.argv:
        path = ROOT / "tests" / "_f32_cases.py"
        text = path.read_text()
        a, b = text.index("# --- generated by"), text.index("# --- end generated ---")
        fmt = lambda v: pprint.pformat(v, width=118, sort_dicts=False)  # noqa: E731
        body = ("# --- generated by scripts/find_f32_cases.py --write ---\n"
                "# listed instantiations no case runs: id -> reason\n"
                f"UNREACHED = {fmt(unreached)}\n\n"
                "# every (instantiation, split or not) the search reached under the cap: each has its case below\n"
                f"REACHED = {fmt(reached)}\n\n"
                "F32_CASES = [\n" + "".join(f"    {c!r},\n" for c in cases) + "]\n")
        path.write_text(text[:a] + body + text[b:])
    else:
        for k, v in unreached.items():
            print(k, "|", v[:150])


# ids no public entry point launches: id -> the guard that excludes it
NEVER = {}
for _kb, _tiles in ((16, ("64x64", "64x128", "128x128", "192x128", "128x256")),
                    (32, ("32x128", "64x64", "64x128", "96x128", "128x128", "192x128"))):
    for _t in _tiles:
        NEVER[f"gemm<KC,CONVT,NCHW,{_kb};{_t}>"] = (
            "not found in the search box: SEARCH_BOX['conv'] (conv_fwd_core turns KC into KCU for every table gather, "
            "amode == KC && bmode == CONVT, whose weights are below 2 GiB; the box's weights stay below 64 MiB)")

if __name__ == "__main__":
    main()
