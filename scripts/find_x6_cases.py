#!/usr/bin/env python3
"""Finds, per bf16x6 convolution kernel instantiation, the cheapest shape
that makes the host planners select it (tests/_x6_cases.py).

Host only: every candidate descriptor is put to ops.conv_fwd_kernel_id, the
query built on the launch paths' own plan functions; nothing runs on a GPU.
Per id (tiling kind included) the shape with the fewest FLOPs is kept; then
per kernel family the cheapest shape with a ragged last row tile, with a
ragged last column tile and, for the channel-octet families, with a group
whose row count is no multiple of 8 (the companion is then packed after the
kernel) are added where the table has none.  Ids of
ops.conv_fwd_kernel_list() that no shape selected are listed as UNREACHED.

  python scripts/find_x6_cases.py            # print the table
  python scripts/find_x6_cases.py --write    # and rewrite tests/_x6_cases.py
  python scripts/find_x6_cases.py --dump F   # every planner answer per candidate (to diff two builds)

The boxes (SEARCH_BOX in tests/_x6_cases.py describes them):
"""
import argparse
import itertools
import pprint
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "tests", ROOT / "rram-caffe-simulation_amd" / "python"):
    sys.path.insert(0, str(p))

import _x6_cases as XC  # noqa: E402
from rramsim import ops  # noqa: E402

CAP = 2e9
BATCH = range(1, 9)
SIDES = range(6, 65)
ROWS = (8, 24, 32, 40, 52, 56, 64, 96, 100, 104, 128, 192)
# the fixed-shape kernels: the smallest batch of the shape they are written for
FIXED = [dict(x=(1, 3, 227, 227), cout=96, k=11, s=4, p=0, g=1, align16=True),      # AlexNet conv1
         dict(x=(1, 3, 176, 176), cout=64, k=7, s=2, p=3, g=1, align16=True)]       # GoogLeNet conv1's form


def planes(sides):
    for h in sides:
        for w in (h, h - 3, h + 3):
            yield h, w


def candidates():
    for n, (h, w), cg, g, m, k in itertools.product(BATCH, planes(SIDES), (16, 32, 48), (1, 2), ROWS, (3, 5)):
        for p in (0, (k - 1) // 2):
            yield dict(x=(n, cg * g, h, w), cout=m * g, k=k, s=1, p=p, g=g, align16=True)
    for n, (h, w), c, m, al in itertools.product(BATCH, planes(SIDES), (16, 32, 48, 64, 128, 256), ROWS + (256, 384),
                                                 (True, False)):
        yield dict(x=(n, c, h, w), cout=m, k=1, s=1, p=0, g=1, align16=al)
    for n, (h, w), cg, g, m, k in itertools.product(BATCH, planes(list(SIDES) + [96, 128]), (2, 4, 6, 8, 12, 24, 40),
                                                    (1, 2), ROWS + (88, 120), (3, 5)):
        for p in (0, (k - 1) // 2):
            yield dict(x=(n, cg * g, h, w), cout=m * g, k=k, s=1, p=p, g=g, align16=True)
    yield from FIXED


def search():
    best, extra, above = {}, {}, {}

    def keep(table, key, fl, cs, kid):
        if key not in table or fl < table[key][0]:
            table[key] = (fl, cs, kid)

    for cs in candidates():
        n, c, h, w = cs["x"]
        if min(h, w) + 2 * cs["p"] < cs["k"]:
            continue
        fl = XC.flops(cs)
        if fl > 2 * CAP:
            continue
        kid = ops.conv_fwd_kernel_id(XC.desc(cs), cs["align16"])
        if kid == "f32":
            continue
        if fl > CAP:            # too dear for the table: remembered for the UNREACHED reason
            keep(above, XC.strip_kind(kid), fl, cs, kid)
            continue
        keep(best, kid, fl, cs, kid)
        fam = XC.family(kid)
        rm, rn = XC.ragged(cs, kid)
        if rm:
            keep(extra, (fam, "ragged rows"), fl, cs, kid)
        if rn:
            keep(extra, (fam, "ragged columns"), fl, cs, kid)
        if fam in ("cb", "cb16") and (cs["cout"] // cs["g"]) % 8 != 0 and cs["cout"] % 8 == 0:
            keep(extra, (fam, "rows % 8 != 0"), fl, cs, kid)
    table = [dict(cs, id=kid) for _, cs, kid in sorted(best.values(), key=lambda t: (XC.family(t[2]), t[2]))]
    have = lambda fam, what: any(  # noqa: E731
        XC.family(e["id"]) == fam and
        {"ragged rows": XC.ragged(e, e["id"])[0], "ragged columns": XC.ragged(e, e["id"])[1],
         "rows % 8 != 0": (e["cout"] // e["g"]) % 8 != 0 and e["cout"] % 8 == 0}[what] for e in table)
    for (fam, what), (_, cs, kid) in sorted(extra.items()):
        if not have(fam, what):
            table.append(dict(cs, id=kid))
    reached = {XC.strip_kind(e["id"]) for e in table}
    return table, [k for k in ops.conv_fwd_kernel_list() if k not in reached], above


def reason(kid, above):
    fam = XC.family(kid)
    if kid in above:
        fl, cs, _ = above[kid]
        return (f"selected only above the 2 GFLOP cap on a case: cheapest in the box x={cs['x']} cout={cs['cout']} "
                f"k={cs['k']} p={cs['p']} g={cs['g']} at {fl / 1e9:.2f} GFLOP")
    box = XC.SEARCH_BOX["cb/cb16" if fam in ("cb", "cb16") else "c1x1" if fam.startswith("c1x1") else "patch"]
    return "the planner chose it for no shape of the box: " + box


# descriptors on either side of each family's 2 GB guard (ring, s2, cb packed input, 1x1, patch output)
GUARDS = [dict(x=(n, c, h, w), cout=m, k=k, s=s, p=p, g=1, align16=True)
          for (c, h, w, m, k, s, p), ns in [((3, 227, 227, 96, 11, 4, 0), (1848, 1849, 1850)),
                                            ((3, 224, 224, 64, 7, 2, 3), (668, 669)),
                                            ((256, 13, 13, 128, 3, 1, 1), (8272, 8273)),
                                            ((64, 56, 56, 64, 1, 1, 0), (2674, 2675)),
                                            ((8, 64, 64, 128, 3, 1, 1), (1023, 1024))] for n in ns]


def dump(path):
    """One line per descriptor with everything the host dispatch answers for
    it: two builds whose files are equal plan every shape alike."""
    def line(cs):
        d = XC.desc(cs)
        ids = [ops.conv_fwd_kernel_id(d, al) for al in (True, False)]
        nbytes, plan = ops.conv_weight_pack_bytes(d), ops.conv_octet_plan(d)
        assert (nbytes > 0) == (ids[0] != "f32"), (cs, ids, nbytes)
        return " ".join(map(str, [*cs["x"], cs["cout"], cs["k"], cs["s"], cs["p"], cs["g"], *ids, nbytes,
                                  ",".join(map(str, plan.values())) if plan else "-", ops.conv_output_octets_only(d),
                                  ops.conv_input_octets(d), ops.f32_engine_for_conv(d)])) + "\n"
    with open(path, "w") as f:
        n = sum(f.write(line(cs)) > 0 for cs in itertools.chain(candidates(), GUARDS, XC.X6_CASES)
                if min(cs["x"][2:]) + 2 * cs["p"] >= cs["k"])
        prev = ops.set_f32_engine(ops.ENGINE_F32)
        n += sum(f.write(line(cs)) > 0 for cs in XC.X6_CASES)
        ops.set_f32_engine(prev)
    print(f"# {n} descriptors dumped to {path}", file=sys.stderr)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", action="store_true", help="rewrite the generated block of tests/_x6_cases.py")
    ap.add_argument("--dump", metavar="FILE", help="write every planner answer per candidate descriptor and exit")
    a = ap.parse_args()
    if a.dump:
        return dump(a.dump)
    table, missing, above = search()
    body = "# instantiations no shape of the box selects: id -> reason\nUNREACHED = " + \
        pprint.pformat({k: reason(k, above) for k in missing}, width=118) + \
        "\n\n# every id the search reached, tiling kind included: each has its case below\nREACHED = " + \
        pprint.pformat(sorted({e["id"] for e in table}), width=118, compact=True) + "\n\nX6_CASES = [\n" + \
        "".join(f"    {e!r},\n" for e in table) + "]\n"
    print(body)
    print(f"# {len(table)} cases, {len(missing)} unreached, "
          f"{sum(XC.flops(e) for e in table) / 1e9:.2f} GFLOP in all", file=sys.stderr)
    if a.write:
        path = ROOT / "tests" / "_x6_cases.py"
        src = path.read_text()
        new = re.sub(r"(# --- generated by [^\n]*\n).*?(# --- end generated ---\n)",
                     lambda m: m.group(1) + body + m.group(2), src, flags=re.S)
        path.write_text(new)


if __name__ == "__main__":
    main()
