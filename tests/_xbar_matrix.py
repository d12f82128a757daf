"""The crossbar read-outs' case table (csrc/xbar.hip): XBAR_CASES, shared by
tests/test_xbar_kernel_coverage.py (host only: every case's recorded id lines,
and that the table reaches every id of ops.xbar_kernel_list() and every named
plan branch) and tests/test_gpu_xbar_matrix.py (every case against its numpy
reference of _xbar_cases.py, bit for bit, behind output and workspace guards).

A case: label, entry (ip | bs | ws | ss | bwd | conv), shape (M, N, K; bwd: dy
[M][N], w [N][K]) or geom (num, C, H, W, Cout, kh, kw, ph, pw, sh, sw, dh, dw,
group), cfg (rows, adc_bits, adc_range[, dac_bits, dac_range]), sl (weight_bits,
cell_bits, weight_range), db (digit bits), split (split_k; 0: the planner), xa /
wa (False: that operand is handed over 4 bytes past a 16-byte boundary), bias,
relu, kind (the operand class), seed, clip (the ADC saturates somewhere) and
ids, the lines the entry point's *_kernel_ids query prints for it (XBAR_IDS,
printed by `python tests/_xbar_matrix.py`).

Operand classes, all bit-exact:
  grid        integers in [-7, 7] times 2^-3 (with a DAC: [-64, 64] times 2^-6)
  half_codes  bs: x on half-code points, DAC ties and the clamp both occur
  gauss, max  ws / ss: standard normal operands; every code at +-max
  wide_x / wide_w  one operand n 2^-18 with |n| in [2^16, 2^19) (a non-zero high,
              middle and low bf16 term), the other from {0, +-1, +-1/2, +-1/4}
              (one term; bs: any code) on WIDE_PAIRS pairs of taps per crossbar
              tile and row, so every partial sum is an fp32 number in any order
              (wide_ok).  The taps of a pair are +t and -t on neighbouring k
              whose wide values differ by at most WIDE_DELTA quanta, so a
              tile's sum is a few thousand product quanta and the ADC runs at
              16 bits with the quantum as its step (2^-20; bs 2^-18) without
              clipping: every output carries the low term exactly
              (test_xbar_kernel_coverage.py proves it from the reference)
  odd_scale   bs / ws / ss: dac_range = cmax / 7 and weight_range = dmax / 7, so
              xs and ws are no powers of two; no x / xs or w / ws within 4 ulp
              of a rounding tie or of the clamp (tie_ok), by choice of seed
"""
import functools
import re

import numpy as np
from _xbar_cases import f32, grid, ref_bs, ref_bwd, ref_conv, ref_ss, ref_ws, ref_xbar

# rows of a workgroup tile per entry point; 128 columns everywhere
TILE_ROWS = {"ip": 128, "bwd": 128, "bs": 64, "ws": 64, "ss": 32, "conv": 128}
BN = 128
# A case's output rows x columns x reduction length stays at or below the largest exact
# case the per-read-out modules had (40 x 300 x 2068); a case whose reference loops over
# more than one chunk of planes, slices or digits stays at or below 40 x 130 x 1056.
MNK_CAP = 40 * 300 * 2068
MNK_CAP_CHUNKED = 40 * 130 * 1056
WIDE_PAIRS = 3       # 6 taps x |wide| < 2 x 1.02 < 16 = 2^24 x 2^-20, for any rows
WIDE_PAIRS_BS = 12   # bs: 24 taps (u = +-1) x 2 x 1.02 < 64 = 2^24 x 2^-18
WIDE_DELTA = 2 ** 11  # 3 pairs x |4 t| <= 4 x 2^11, and 12 pairs x 2^11, are 24576 <= 32767 ADC steps


def _adc(B, e):
    return (2 ** (B - 1) - 1) * 2.0 ** e


def _case(label, entry, shape, cfg, **kw):
    c = dict(label=label, entry=entry, cfg=tuple(cfg), sl=None, db=0, split=1, xa=True, wa=True, bias=False, relu=False,
             kind="grid", seed=1, clip=False)
    c["geom" if entry == "conv" else "shape"] = tuple(shape)
    c.update(kw)
    return c


def fp(label, entry, shape, R, B=None, e=None, dac=None, **kw):
    """ip / bwd / conv: step = 2^e, dac = (bits, log2 xs).  B and e not given: 8 bits at 2^-2; the wide classes take
    neither and run 16 bits at the products' quantum 2^-20."""
    if kw.get("kind", "grid").startswith("wide"):
        assert B is None and e is None and dac is None
        B, e = 16, -20
    B, e = B or 8, -2 if e is None else e
    return _case(label, entry, shape, (R, B, _adc(B, e)) + ((dac[0], _adc(dac[0], dac[1])) if dac else ()), **kw)


def bs(label, shape, R, b, B=None, e=None, **kw):
    """bs: xs = 2^-4 (odd_scale: 1 / 7), step = 2^e.  B and e not given: 8 bits (rows >= 256: 12, so that a plane's sum
    of up to R grid weights stays inside) at 2^-2; wide_w takes neither and runs 16 bits at the quantum 2^-18."""
    kind = kw.setdefault("kind", "half_codes")
    X = (2 ** (b - 1) - 1) / 7.0 if kind == "odd_scale" else _adc(b, -4)
    if kind == "wide_w":
        assert B is None and e is None
        B, e = 16, -18
    B, e = B or (12 if R >= 256 else 8), -2 if e is None else e
    return _case(label, "bs", shape, (R, B, _adc(B, e), b, X), **kw)


def sliced(label, entry, shape, R, b, wb, cb, db=0, B=None, h=None, **kw):
    """ws / ss: xs = ws = 2^-5 (odd_scale: 1 / 7) and kf = 2^h / 3; h: the largest at which the worst pair of codes
    stays inside the ADC (so only a 4-bit ADC, taken at the 8-bit h, clips)."""
    kw.setdefault("kind", "gauss")
    B = B or (16 if R >= 256 else 8)
    cmax, dmax = 2 ** (b - 1) - 1, 2 ** (wb - 1) - 1
    worst = R * min(cmax, 2 ** (db or 8) - 1) * min(dmax, 2 ** cb - 1)
    if h is None:
        h = int(np.floor(np.log2((2 ** (max(B, 8) - 1) - 1) * 3.0 / worst)))
    u = 1.0 / 7 if kw["kind"] == "odd_scale" else 2.0 ** -5
    cfg = (R, B, (2 ** (B - 1) - 1) * 3.0 * u * u * 2.0 ** -h, b, cmax * u)
    return _case(label, entry, shape, cfg, sl=(wb, cb, dmax * u), db=db, **kw)


def family(p, make, bm, wide, r1024=True):
    """The plan branches every InnerProduct-shaped read-out kernel has, for one kernel variant: make(label, (rows,
    columns, reduction), R, **kw) builds its case.  wide: the wide operand classes the kernel takes."""
    rag = (bm + 2, 130, 212)                              # 2 x 2 ragged tiles, 7 crossbar tiles, the last of 20 rows
    out = [make(p + "-one", (1, 1, 1), 32, bias=True, seed=13),                # one slab, one workgroup, scalar by K % 4
           make(p + "-rag-s3", rag, 32, split=3, bias=True, relu=True),   # splits of 3, 3, 1 tiles: 12 workgroups
           make(p + "-xs", (33, 40, 96), 32, xa=False),                   # scalar by the pointer alone, K % 4 == 0
           make(p + "-ws", (33, 40, 96), 32, wa=False, bias=True),
           make(p + "-xsws", (bm + 6, 200, 300), 128, xa=False, wa=False, relu=True),
           make(p + "-r256", (5, 10, 600), 256, bias=True, relu=True),    # 3 tiles, the last of 88 rows
           make(p + "-clip", (33, 130, 96), 32, B=4, clip=True, bias=True, relu=True)]
    if r1024:
        out.append(make(p + "-r1024", (5, 10, 1100), 1024, split=2))      # 2 tiles, the last of 76 rows
    for k in wide:
        out += [make(p + "-%s-v" % k, (33, 132, 96), 32, kind=k, bias=True),
                make(p + "-%s-s" % k, (bm + 2, 70, 213), 32, kind=k, split=3, relu=True),   # scalar loads, ragged
                make(p + "-%s-r256" % k, (5, 10, 600), 256, kind=k)]
    return out


def _ip(label, s, R, **kw):
    return fp(label, "ip", s, R, **kw)


def _bwd(label, s, R, **kw):                              # (rows, columns, reduction) -> dy [M][N], w [N][K]
    kw.pop("bias", 0), kw.pop("relu", 0)                  # the transposed read-out has neither
    return fp(label, "bwd", (s[0], s[2], s[1]), R, **kw)


def _bs(b):
    return lambda label, s, R, **kw: bs(label, s, R, b, **kw)


def _sl(entry, b, wb, cb, db=0):
    return lambda label, s, R, **kw: sliced(label, entry, s, R, b, wb, cb, db, **kw)


MID = (33, 130, 96)
# (num, C, H, W, Cout, kh, kw, ph, pw, sh, sw, dh, dw, group)
G_ONE = (1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1)
G_K45 = (3, 5, 7, 5, 33, 3, 3, 1, 1, 1, 1, 1, 1, 1)       # Kg = 45: a tile boundary inside a channel's taps
G_K36 = (2, 4, 6, 6, 33, 3, 3, 1, 1, 1, 1, 1, 1, 1)       # Kg = 36
G_GRP = (2, 8, 9, 11, 6, 5, 5, 2, 2, 2, 2, 1, 1, 2)       # two groups, stride 2, Kg = 100
G_NG130 = (2, 4, 6, 6, 260, 3, 3, 1, 1, 1, 1, 1, 1, 2)    # two groups of 130 channels: two channel tiles each
G_DIL = (2, 6, 10, 9, 10, 3, 2, 0, 1, 2, 1, 2, 2, 1)      # non-square, mixed stride / pad, dilation 2
G_PW = (5, 70, 3, 3, 20, 1, 1, 0, 0, 1, 1, 1, 1, 1)       # 1x1, a position tile spans images, Kg % 4 != 0
G_11 = (2, 3, 27, 27, 10, 11, 11, 0, 0, 4, 4, 1, 1, 1)    # CaffeNet conv1's kernel and stride: Kg = 363
G_T11 = (2, 36, 12, 12, 130, 3, 3, 1, 1, 1, 1, 1, 1, 1)   # 3 x 2 ragged tiles, Kg = 324: 11 tiles of 32, the last of 4
G_R256 = (1, 32, 5, 5, 10, 3, 3, 1, 1, 1, 1, 1, 1, 1)     # Kg = 288
G_R1024 = (1, 128, 4, 4, 6, 3, 3, 1, 1, 1, 1, 1, 1, 1)    # Kg = 1152
# the wide classes: stride = kernel and no pad, so the patches are disjoint and any column matrix is an image
G_W36 = (2, 4, 6, 6, 33, 3, 3, 0, 0, 3, 3, 1, 1, 1)       # Kg = 36, 8 positions
G_W45 = (4, 5, 18, 18, 33, 3, 3, 0, 0, 3, 3, 1, 1, 1)     # Kg = 45, 144 positions: two tiles, the last of 16
G_W288 = (1, 32, 6, 6, 10, 3, 3, 0, 0, 3, 3, 1, 1, 1)     # Kg = 288


def _cv(label, g, R, **kw):
    return fp(label, "conv", g, R, **kw)


XBAR_CASES = (
    family("ip", _ip, 128, ("wide_x", "wide_w")) +
    [_ip("ip-dac", MID, 32, e=-3, dac=(4, -3), bias=True),
     _ip("ip-fine", (70, 200, 300), 128, B=12, e=-6),
     _ip("ip-big", (40, 300, 2068), 64, split=0, bias=True, relu=True)] +      # the planner's split, the MNK cap
    family("bwd", _bwd, 128, ("wide_x", "wide_w")) +
    [_bwd("bwd-dac", MID, 32, e=-3, dac=(4, -3)),
     _bwd("bwd-big", (40, 300, 2068), 64, split=0)] +
    family("bs4", _bs(5), 64, ("wide_w",)) +                                   # 4 planes: <p4> full
    family("bs7", _bs(8), 64, ("wide_w",)) +                                   # 7 planes: <p7> full
    [bs("bs-p1", (5, 10, 50), 32, 2),
     bs("bs-p3", MID, 32, 4, bias=True),
     bs("bs-p5", MID, 32, 6, relu=True),
     bs("bs-p8", MID, 32, 9, bias=True),                                       # a last chunk of one plane
     bs("bs-p14", MID, 32, 15),                                                # two full chunks
     bs("bs-p15", MID, 32, 16, bias=True, relu=True),                          # three chunks, code bit 14
     bs("bs-p11-big", (40, 130, 1056), 32, 12, split=0, bias=True),
     bs("bs-odd", (9, 20, 70), 32, 8, kind="odd_scale", bias=True, seed=1)] +
    family("ws", _sl("ws", 8, 8, 2), 64, ()) +                                 # 4 slices: one full chunk
    [sliced("ws-n1", "ws", (5, 3, 32), 32, 4, 3, 2),
     sliced("ws-n2", "ws", MID, 32, 8, 8, 4, bias=True),                       # the top slice holds 3 bits
     sliced("ws-n3", "ws", MID, 32, 6, 8, 3, relu=True),                       # the top slice holds 1 bit
     sliced("ws-n5", "ws", MID, 32, 8, 6, 1, bias=True),
     sliced("ws-n6", "ws", MID, 32, 8, 7, 1),
     sliced("ws-n7", "ws", (40, 130, 212), 32, 8, 8, 1, split=3, bias=True, relu=True),
     sliced("ws-grid", "ws", (70, 130, 100), 32, 8, 8, 2, kind="grid", bias=True),
     sliced("ws-max", "ws", (33, 40, 1024), 1024, 8, 8, 7, B=16, h=-9, kind="max"),
     sliced("ws-n7-big", "ws", (40, 130, 1056), 32, 8, 8, 1, split=0, bias=True),
     sliced("ws-odd", "ws", (9, 20, 70), 32, 8, 8, 2, kind="odd_scale", bias=True, seed=1)] +
    family("ss2", _sl("ss", 8, 8, 2, 4), 32, ()) +                             # 2 digits (4 + 3 bits): <d2> full
    family("ss3", _sl("ss", 8, 8, 2, 3), 32, ()) +                             # 3 digits (3 + 3 + 1 bits): <d3> full
    [sliced("ss-d1-b4", "ss", (5, 3, 32), 32, 4, 3, 2, 3),                     # one digit: equals ws
     sliced("ss-d1", "ss", MID, 32, 8, 8, 2, 7, bias=True, relu=True),
     sliced("ss-d1-n7", "ss", MID, 32, 8, 8, 1, 7, bias=True),
     sliced("ss-max", "ss", (33, 40, 1024), 1024, 8, 8, 7, 7, B=16, h=-9, kind="max"),
     sliced("ss-db6", "ss", MID, 32, 8, 8, 2, 6),                              # digits of 6 + 1 bits
     sliced("ss-db5", "ss", MID, 32, 8, 8, 3, 5, bias=True),                   # digits of 5 + 2 bits
     sliced("ss-db2", "ss", MID, 32, 8, 8, 2, 2, relu=True),                   # 4 digits: two full chunks of <d2>
     sliced("ss-b6-db2", "ss", MID, 32, 6, 8, 2, 2, bias=True),                # 5 DAC bits as 2 + 2 + 1
     sliced("ss-nd5-n5", "ss", MID, 32, 6, 6, 1, 1, bias=True),                # chunks of 3 + 2 digits x 4 + 1 slices
     sliced("ss-nd6", "ss", MID, 32, 7, 8, 2, 1),                              # two full digit chunks of <d3>
     sliced("ss-nd7-n7", "ss", (40, 130, 212), 32, 8, 8, 1, 1, split=3, bias=True, relu=True),   # 3, 3, 1 x 4, 3
     sliced("ss-grid", "ss", (70, 130, 100), 32, 8, 8, 2, 2, kind="grid", bias=True),
     sliced("ss-nd7-big", "ss", (40, 130, 1056), 32, 8, 8, 1, 1, split=0, bias=True),
     sliced("ss-odd", "ss", (9, 20, 70), 32, 8, 8, 2, 3, kind="odd_scale", bias=True, seed=1)] +
    [_cv("cv-one", G_ONE, 32, bias=True),                                      # scalar by Kg % 4, one workgroup
     _cv("cv-k45", G_K45, 32, relu=True),
     _cv("cv-k45-clip", G_K45, 32, B=4, e=-3, clip=True, bias=True, relu=True),
     _cv("cv-k45-dac", G_K45, 32, dac=(4, -3), bias=True),
     _cv("cv-grp", G_GRP, 32, bias=True, xa=False, wa=False),
     _cv("cv-ng130", G_NG130, 32, bias=True, relu=True),
     _cv("cv-dil", G_DIL, 32),
     _cv("cv-pw", G_PW, 64, bias=True, relu=True),
     _cv("cv-11x11s4", G_11, 128, bias=True),
     _cv("cv-t11-s3", G_T11, 32, split=3, bias=True, relu=True),               # splits of 4, 4, 3 tiles: 18 workgroups
     _cv("cv-k36-ws", G_K36, 32, wa=False, bias=True),                         # scalar by the pointer, Kg % 4 == 0
     _cv("cv-r256", G_R256, 256, bias=True),
     _cv("cv-r1024", G_R1024, 1024, split=2, relu=True),
     _cv("cv-wide_x-v", G_W36, 32, kind="wide_x", bias=True),
     _cv("cv-wide_x-s", G_W45, 32, kind="wide_x", split=2, relu=True),
     _cv("cv-wide_w-v", G_W36, 32, kind="wide_w", bias=True),
     _cv("cv-wide_w-s", G_W45, 32, kind="wide_w", split=2, relu=True),
     _cv("cv-wide_w-r256", G_W288, 256, kind="wide_w")])

LABELS = [c["label"] for c in XBAR_CASES]
assert len(set(LABELS)) == len(LABELS)


# --- what the planner makes of a case, from the documented tile sizes and the recorded ids ---

def conv_out(g):
    num, C, H, W, Cout, kh, kw, ph, pw, sh, sw, dh, dw, group = g
    return (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1


def dims(c):
    """rows, cols (of one group), red (the reduction length), groups of the case's output."""
    if c["entry"] == "conv":
        g = c["geom"]
        ho, wo = conv_out(g)
        return g[0] * ho * wo, g[4] // g[13], g[1] // g[13] * g[5] * g[6], g[13]
    M, N, K = c["shape"]
    return (M, K, N, 1) if c["entry"] == "bwd" else (M, N, K, 1)


def name(line):
    """'xbar:ip_bs<vec;p7>/s3/c2' -> 'xbar:ip_bs<vec;p7>' (the id rram_xbar_kernel_list prints)."""
    return line.split("/")[0]


def readout(c):
    """The id of the case's read-out kernel."""
    return [name(ln) for ln in c["ids"] if re.match(r"xbar:(ip|conv)", ln)][0]


def family_of(c):
    """The read-out kernel without its <vec|scalar> axis: ip, ip_t, ip_bs;p4, ip_bs;p7, ip_ws, ip_ss;d2, ip_ss;d3, conv."""
    nm, args = re.match(r"xbar:(\w+)<(.*)>", readout(c)).groups()
    args = [a for a in args.split(";") if a not in ("vec", "scalar")]
    return nm + ";" + args[0] if nm in ("ip_bs", "ip_ss") else nm


def plan(c):
    """Tile counts, crossbar tiles, slabs and workgroups of the case (split and chunks are read off the ids)."""
    rows, cols, red, groups = dims(c)
    R = c["cfg"][0]
    line = [ln for ln in c["ids"] if re.match(r"xbar:(ip|conv)", ln)][0]
    split = int(re.search(r"/s(\d+)", line).group(1))
    m = re.search(r"/c(\d+)", line)
    chunks = int(m.group(1)) if m else 1
    bm = TILE_ROWS[c["entry"]]
    tm, tn, ntiles = -(-rows // bm), -(-cols // BN), -(-red // R)
    tc = -(-ntiles // split)
    return dict(rows=rows, cols=cols, red=red, R=R, tm=tm, tn=tn, ntiles=ntiles, split=split, chunks=chunks, tc=tc,
                rag_m=tm > 1 and rows % bm != 0, rag_n=tn > 1 and cols % BN != 0, k32=red % 32 != 0,
                short=red % R != 0, rag_split=split > 1 and ntiles % tc != 0, wgs=tm * tn * groups * split * chunks)


def counts(c):
    """(bit planes | weight slices, input digits) of the case (1 where the entry point has none)."""
    b = c["cfg"][3] if len(c["cfg"]) > 3 else 0
    ns = -(-(c["sl"][0] - 1) // c["sl"][1]) if c["sl"] else 1
    if c["entry"] == "bs":
        return b - 1, 1
    return ns, (-(-(b - 1) // c["db"]) if c["entry"] == "ss" else 1)


def workload(c):
    rows, cols, red, groups = dims(c)
    return rows * cols * red * groups


# --- the host queries ---

def _desc(g):
    from rramsim import ops
    num, C, H, W, Cout, kh, kw, ph, pw, sh, sw, dh, dw, group = g
    return ops.conv_desc((num, C, H, W), Cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw), group)


def query(c, what):
    """ops.<entry point>_<what> (what: "workspace" or "kernel_ids") with the case's arguments."""
    from rramsim import ops
    cfg = ops.xbar_cfg(*c["cfg"])
    e = c["entry"]
    fn = {"ip": "ip_fwd_xbar", "bs": "ip_fwd_xbar_bs", "ws": "ip_fwd_xbar_ws", "ss": "ip_fwd_xbar_ss",
          "bwd": "ip_bwd_data_xbar", "conv": "conv_fwd_xbar"}[e]
    args = (_desc(c["geom"]), cfg) if e == "conv" else c["shape"] + (cfg,)
    if e in ("ws", "ss"):
        args += (ops.xbar_slices(*c["sl"]),) + ((c["db"],) if e == "ss" else ())
    if what == "workspace":
        return getattr(ops, fn + "_workspace")(*args, c["split"])
    return getattr(ops, fn + "_kernel_ids")(*args, c["xa"], c["wa"], split_k=c["split"], ws_bytes=query(c, "workspace"))


# --- operands and references ---

def sig_bits(n):
    """Significant bits of the integers n: the bit length without the trailing zeros."""
    n = np.abs(n.astype(np.int64))
    low = n & -n
    return np.where(n == 0, 0, np.floor(np.log2(np.maximum(n, 1))) - np.floor(np.log2(np.maximum(low, 1))) + 1)


def wide(shape, seed, delta=WIDE_DELTA):
    """[rows][K] of n 2^-18, |n| in [2^16, 2^19): a non-zero high and middle bf16 term everywhere and a low one in
    about a third of the elements (the signed round-to-nearest split covers 17 bits with h and m).  Columns 2 i and
    2 i + 1 have one sign and differ by at most delta quanta, so taps +t and -t on them nearly cancel."""
    g = np.random.default_rng(seed)
    rows, K = shape
    half = (rows, (K + 1) // 2)
    n = np.empty((rows, 2 * half[1]), np.int64)
    n[:, 0::2] = g.integers(2 ** 16 + delta, 2 ** 19 - delta, half)
    n[:, 1::2] = n[:, 0::2] + g.integers(-delta, delta + 1, half)
    n *= np.repeat(g.choice([-1, 1], half), 2, axis=1)
    return (n[:, :K] * 2.0 ** -18).astype(f32)


def taps(shape, seed, R, vals=(1.0, 0.5, 0.25), pairs=WIDE_PAIRS):
    """[rows][K] with at most `pairs` pairs (+-v on 2 i, -+v on 2 i + 1; v from vals) per row and crossbar tile of R,
    zero elsewhere."""
    g = np.random.default_rng(seed)
    a = np.zeros(shape, f32)
    for r in range(shape[0]):
        for k0 in range(0, shape[1], R):
            n = min(R, shape[1] - k0) // 2
            i = k0 + 2 * g.choice(n, min(pairs, n), replace=False)
            v = g.choice(vals, len(i)) * g.choice([-1, 1], len(i))
            a[r, i], a[r, i + 1] = v, -v
    return a


def fold(cols, geom):
    """The image whose column matrix is cols [num Ho Wo][C kh kw], for a geometry of disjoint patches (G_W*)."""
    num, C, H, W, Cout, kh, kw, ph, pw, sh, sw, dh, dw, group = geom
    assert (ph, pw, dh, dw, group) == (0, 0, 1, 1, 1) and (sh, sw) == (kh, kw) and H % kh == 0 and W % kw == 0
    a = cols.reshape(num, H // kh, W // kw, C, kh, kw).transpose(0, 3, 1, 4, 2, 5)
    return np.ascontiguousarray(a.reshape(num, C, H, W))


def bf16_terms(a):
    """The round-to-nearest-even bf16 split a = h + m + l (split3.hpp), each as float32."""
    def rne(v):
        u = v.astype(f32).view(np.uint32).astype(np.uint64)
        return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(f32)
    h = rne(a)
    m = rne(a - h)
    return h, m, rne(a - h - m)


def wide_ok(a, b, R, q):
    """Condition 1 of the wide classes: per crossbar tile 1.02 (|a| @ |b|.T).max() <= 2^24 q (q: the products'
    common quantum), so every partial sum is an fp32 number in any order."""
    a, b = np.abs(a.astype(np.float64)), np.abs(b.astype(np.float64))
    return all(1.02 * (a[:, k:k + R] @ b[:, k:k + R].T).max() <= 2 ** 24 * q for k in range(0, a.shape[1], R))


def tie_ok(v, scale, cmax):
    """No v / scale within 4 ulp of a rounding tie (below the clamp) or of the clamp."""
    r = np.abs(v.astype(np.float64) / float(f32(scale)))
    ulp = np.spacing(r.astype(f32)).astype(np.float64)
    tie = (np.abs(r % 1.0 - 0.5) <= 4 * ulp) & (r < cmax + 1)
    return not tie.any() and not (np.abs(r - cmax) <= 4 * ulp).any() and not (np.abs(r - cmax - 0.5) <= 4 * ulp).any()


def operands(c):
    """(x | dy, w, bias or None) of the case, as the entry point takes them."""
    e, kind, seed = c["entry"], c["kind"], c["seed"]
    R, dacb = c["cfg"][0], (c["cfg"][3] if len(c["cfg"]) > 3 else 0)
    rows, cols, red, groups = dims(c)
    g = np.random.default_rng(seed)
    if e == "conv":
        geom = c["geom"]
        xs_, ws_ = geom[:4], (geom[4], geom[1] // geom[13], geom[5], geom[6])
        if kind == "wide_x":                              # built as the column matrix, folded into the image
            x, w = fold(wide((rows, red), seed), geom), taps((cols, red), seed + 1, R).reshape(ws_)
        elif kind == "wide_w":
            x, w = fold(taps((rows, red), seed, R), geom), wide((cols, red), seed + 1).reshape(ws_)
        else:
            x = grid(xs_, seed, -64, 64, 2.0 ** -6) if dacb else grid(xs_, seed)
            w = grid(ws_, seed + 1)
        return x, w, (grid((geom[4],), seed + 2) if c["bias"] else None)
    xshape, wshape = (rows, red), ((red, cols) if e == "bwd" else (cols, red))
    bias = grid((cols,), seed + 2) if c["bias"] else None

    def t(a):                                             # [cols][red] -> the entry point's weight layout
        return np.ascontiguousarray(a.T) if e == "bwd" else a

    if kind == "wide_x":
        return wide(xshape, seed), t(taps((cols, red), seed + 1, R)), bias
    if kind == "wide_w" and e == "bs":                    # any code: +c and -c have the same planes
        codes = tuple(v * 2.0 ** -4 for v in range(1, 2 ** (dacb - 1)))
        return taps(xshape, seed, R, codes, WIDE_PAIRS_BS), wide(wshape, seed + 1), bias
    if kind == "wide_w":
        return taps(xshape, seed, R), t(wide((cols, red), seed + 1)), bias
    if kind == "half_codes":                              # x on half-code points i xs / 2, past the clamp by 2
        n = 2 * (2 ** (dacb - 1) - 1) + 4
        return grid(xshape, seed, -n, n, 2.0 ** -5), grid(wshape, seed + 1), bias
    if kind == "odd_scale":
        x = (g.uniform(-1.05, 1.05, xshape) * c["cfg"][4]).astype(f32)
        w = (g.uniform(-1.05, 1.05, wshape) * c["sl"][2]).astype(f32) if c["sl"] else grid(wshape, seed + 1)
        return x, w, bias
    if kind == "gauss":
        return g.standard_normal(xshape).astype(f32), g.standard_normal(wshape).astype(f32), bias
    if kind == "max":
        x, w = np.where(g.random(xshape) < 0.5, f32(-8), f32(8)), np.where(g.random(wshape) < 0.5, f32(-8), f32(8))
        x[0], w[0] = 8, 8
        return x, w, bias
    if e in ("ws", "ss"):                                 # grid: half-code points of both quantisers and their clamps
        return grid(xshape, seed, -260, 260, 2.0 ** -6), grid(wshape, seed + 1, -260, 260, 2.0 ** -6), bias
    x = grid(xshape, seed, -64, 64, 2.0 ** -6) if dacb else grid(xshape, seed)
    return x, grid(wshape, seed + 1), bias


def conditions(c, x, w):
    """The case's conditions on its operands, from the reference side alone."""
    e, kind, cfg = c["entry"], c["kind"], c["cfg"]
    R = cfg[0]
    if kind.startswith("wide"):
        if e == "conv":
            from _xbar_cases import im2col
            Ng = c["geom"][4] // c["geom"][13]
            pairs = [(im2col(x, g, c["geom"])[0], w[g * Ng:(g + 1) * Ng].reshape(Ng, -1)) for g in range(c["geom"][13])]
        else:
            pairs = [(x, w.T if e == "bwd" else w)]
        q = 2.0 ** -18 if e == "bs" else 2.0 ** -20       # bs: a plane is +-1 or 0
        for a, b in pairs:
            a = (a != 0).astype(np.float64) if e == "bs" else a    # |u| of any plane
            assert wide_ok(a, b, R, q), c["label"]
        wd = x if kind == "wide_x" else w
        assert (sig_bits(np.rint(wd.astype(np.float64) * 2 ** 18)) > 16).mean() >= 0.5, c["label"]
    if kind == "odd_scale":
        cmax = 2 ** (cfg[3] - 1) - 1
        assert tie_ok(x, float(f32(cfg[4])) / cmax, cmax), c["label"]
        if c["sl"]:
            dmax = 2 ** (c["sl"][0] - 1) - 1
            assert tie_ok(w, float(f32(c["sl"][2])) / dmax, dmax), c["label"]


def compute(c, x, w, bias):
    """(y, clipped anywhere, max |p| or None) of the case's reference on the given operands."""
    e, cfg = c["entry"], c["cfg"]
    pmax = None
    dac = (cfg[3], cfg[4]) if len(cfg) > 3 else None
    if e == "ip":
        y, _, _, clipped = ref_xbar(x, w, bias, cfg[0], cfg[1], cfg[2], c["relu"], dac)
    elif e == "bwd":
        y, _, _, clipped = ref_bwd(x, w, cfg[0], cfg[1], cfg[2], dac)
    elif e == "conv":
        y, _, _, clipped, _ = ref_conv(x, w, bias, c["geom"] + (cfg[0],), cfg[1], cfg[2], c["relu"], dac)
    elif e == "bs":
        y, _, _, clipped = ref_bs(x, w, bias, cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], c["relu"])
    elif e == "ws":
        y, clipped, pmax = ref_ws(x, w, bias, cfg, c["sl"], c["relu"])
    else:
        y, clipped, pmax = ref_ss(x, w, bias, cfg, c["sl"], c["db"], c["relu"])
    return y, clipped, pmax


@functools.lru_cache(maxsize=None)
def reference(label):
    """(x, w, bias, y of the reference) of the case; its reference-side conditions are asserted on the way."""
    c = XBAR_CASES[LABELS.index(label)]
    x, w, bias = operands(c)
    conditions(c, x, w)
    y, clipped, pmax = compute(c, x, w, bias)
    assert clipped == c["clip"], (label, clipped)         # clipped where meant, and only there
    if c["kind"] == "max":
        assert pmax == 1024 * 127 * 127
    for a in (x, w, y):
        a.setflags(write=False)
    return x, w, bias, y


# --- generated by `python tests/_xbar_matrix.py`: the *_kernel_ids lines of every case ---
XBAR_IDS = {
    'ip-one': ['xbar:pack<scalar>', 'xbar:ip<scalar>/s1'],
    'ip-rag-s3': ['xbar:pack<vec>', 'xbar:ip<vec>/s3', 'xbar:finish'],
    'ip-xs': ['xbar:pack<scalar>', 'xbar:ip<vec>/s1'],
    'ip-ws': ['xbar:pack<vec>', 'xbar:ip<scalar>/s1'],
    'ip-xsws': ['xbar:pack<scalar>', 'xbar:ip<scalar>/s1'],
    'ip-r256': ['xbar:pack<vec>', 'xbar:ip<vec>/s1'],
    'ip-clip': ['xbar:pack<vec>', 'xbar:ip<vec>/s1'],
    'ip-r1024': ['xbar:pack<vec>', 'xbar:ip<vec>/s2', 'xbar:finish'],
    'ip-wide_x-v': ['xbar:pack<vec>', 'xbar:ip<vec>/s1'],
    'ip-wide_x-s': ['xbar:pack<scalar>', 'xbar:ip<scalar>/s3', 'xbar:finish'],
    'ip-wide_x-r256': ['xbar:pack<vec>', 'xbar:ip<vec>/s1'],
    'ip-wide_w-v': ['xbar:pack<vec>', 'xbar:ip<vec>/s1'],
    'ip-wide_w-s': ['xbar:pack<scalar>', 'xbar:ip<scalar>/s3', 'xbar:finish'],
    'ip-wide_w-r256': ['xbar:pack<vec>', 'xbar:ip<vec>/s1'],
    'ip-dac': ['xbar:pack<vec>', 'xbar:ip<vec>/s1'],
    'ip-fine': ['xbar:pack<vec>', 'xbar:ip<vec>/s1'],
    'ip-big': ['xbar:pack<vec>', 'xbar:ip<vec>/s33', 'xbar:finish'],
    'bwd-one': ['xbar:pack<scalar>', 'xbar:ip_t<scalar>/s1'],
    'bwd-rag-s3': ['xbar:pack<vec>', 'xbar:ip_t<scalar>/s3', 'xbar:finish'],
    'bwd-xs': ['xbar:pack<scalar>', 'xbar:ip_t<vec>/s1'],
    'bwd-ws': ['xbar:pack<vec>', 'xbar:ip_t<scalar>/s1'],
    'bwd-xsws': ['xbar:pack<scalar>', 'xbar:ip_t<scalar>/s1'],
    'bwd-r256': ['xbar:pack<vec>', 'xbar:ip_t<scalar>/s1'],
    'bwd-clip': ['xbar:pack<vec>', 'xbar:ip_t<scalar>/s1'],
    'bwd-r1024': ['xbar:pack<vec>', 'xbar:ip_t<scalar>/s2', 'xbar:finish'],
    'bwd-wide_x-v': ['xbar:pack<vec>', 'xbar:ip_t<vec>/s1'],
    'bwd-wide_x-s': ['xbar:pack<scalar>', 'xbar:ip_t<scalar>/s3', 'xbar:finish'],
    'bwd-wide_x-r256': ['xbar:pack<vec>', 'xbar:ip_t<scalar>/s1'],
    'bwd-wide_w-v': ['xbar:pack<vec>', 'xbar:ip_t<vec>/s1'],
    'bwd-wide_w-s': ['xbar:pack<scalar>', 'xbar:ip_t<scalar>/s3', 'xbar:finish'],
    'bwd-wide_w-r256': ['xbar:pack<vec>', 'xbar:ip_t<scalar>/s1'],
    'bwd-dac': ['xbar:pack<vec>', 'xbar:ip_t<scalar>/s1'],
    'bwd-big': ['xbar:pack<vec>', 'xbar:ip_t<vec>/s33', 'xbar:finish'],
    'bs4-one': ['xbar:pack_codes<scalar>', 'xbar:ip_bs<scalar;p4>/s1/c1'],
    'bs4-rag-s3': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p4>/s3/c1', 'xbar:finish'],
    'bs4-xs': ['xbar:pack_codes<scalar>', 'xbar:ip_bs<vec;p4>/s1/c1'],
    'bs4-ws': ['xbar:pack_codes<vec>', 'xbar:ip_bs<scalar;p4>/s1/c1'],
    'bs4-xsws': ['xbar:pack_codes<scalar>', 'xbar:ip_bs<scalar;p4>/s1/c1'],
    'bs4-r256': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p4>/s1/c1'],
    'bs4-clip': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p4>/s1/c1'],
    'bs4-r1024': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p4>/s2/c1', 'xbar:finish'],
    'bs4-wide_w-v': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p4>/s1/c1'],
    'bs4-wide_w-s': ['xbar:pack_codes<scalar>', 'xbar:ip_bs<scalar;p4>/s3/c1', 'xbar:finish'],
    'bs4-wide_w-r256': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p4>/s1/c1'],
    'bs7-one': ['xbar:pack_codes<scalar>', 'xbar:ip_bs<scalar;p7>/s1/c1'],
    'bs7-rag-s3': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p7>/s3/c1', 'xbar:finish'],
    'bs7-xs': ['xbar:pack_codes<scalar>', 'xbar:ip_bs<vec;p7>/s1/c1'],
    'bs7-ws': ['xbar:pack_codes<vec>', 'xbar:ip_bs<scalar;p7>/s1/c1'],
    'bs7-xsws': ['xbar:pack_codes<scalar>', 'xbar:ip_bs<scalar;p7>/s1/c1'],
    'bs7-r256': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p7>/s1/c1'],
    'bs7-clip': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p7>/s1/c1'],
    'bs7-r1024': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p7>/s2/c1', 'xbar:finish'],
    'bs7-wide_w-v': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p7>/s1/c1'],
    'bs7-wide_w-s': ['xbar:pack_codes<scalar>', 'xbar:ip_bs<scalar;p7>/s3/c1', 'xbar:finish'],
    'bs7-wide_w-r256': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p7>/s1/c1'],
    'bs-p1': ['xbar:pack_codes<scalar>', 'xbar:ip_bs<scalar;p4>/s1/c1'],
    'bs-p3': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p4>/s1/c1'],
    'bs-p5': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p7>/s1/c1'],
    'bs-p8': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p7>/s1/c2', 'xbar:finish'],
    'bs-p14': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p7>/s1/c2', 'xbar:finish'],
    'bs-p15': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p7>/s1/c3', 'xbar:finish'],
    'bs-p11-big': ['xbar:pack_codes<vec>', 'xbar:ip_bs<vec;p7>/s33/c2', 'xbar:finish'],
    'bs-odd': ['xbar:pack_codes<scalar>', 'xbar:ip_bs<scalar;p7>/s1/c1'],
    'ws-one': ['xbar:pack_i8<scalar>', 'xbar:pack_wslices<scalar>', 'xbar:ip_ws<p4>/s1/c1'],
    'ws-rag-s3': ['xbar:pack_i8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ws<p4>/s3/c1', 'xbar:finish'],
    'ws-xs': ['xbar:pack_i8<scalar>', 'xbar:pack_wslices<vec>', 'xbar:ip_ws<p4>/s1/c1'],
    'ws-ws': ['xbar:pack_i8<vec>', 'xbar:pack_wslices<scalar>', 'xbar:ip_ws<p4>/s1/c1'],
    'ws-xsws': ['xbar:pack_i8<scalar>', 'xbar:pack_wslices<scalar>', 'xbar:ip_ws<p4>/s1/c1'],
    'ws-r256': ['xbar:pack_i8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ws<p4>/s1/c1'],
    'ws-clip': ['xbar:pack_i8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ws<p4>/s1/c1'],
    'ws-r1024': ['xbar:pack_i8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ws<p4>/s2/c1', 'xbar:finish'],
    'ws-n1': ['xbar:pack_i8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ws<p4>/s1/c1'],
    'ws-n2': ['xbar:pack_i8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ws<p4>/s1/c1'],
    'ws-n3': ['xbar:pack_i8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ws<p4>/s1/c1'],
    'ws-n5': ['xbar:pack_i8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ws<p4>/s1/c2', 'xbar:finish'],
    'ws-n6': ['xbar:pack_i8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ws<p4>/s1/c2', 'xbar:finish'],
    'ws-n7': ['xbar:pack_i8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ws<p4>/s3/c2', 'xbar:finish'],
    'ws-grid': ['xbar:pack_i8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ws<p4>/s1/c1'],
    'ws-max': ['xbar:pack_i8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ws<p4>/s1/c1'],
    'ws-n7-big': ['xbar:pack_i8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ws<p4>/s33/c2', 'xbar:finish'],
    'ws-odd': ['xbar:pack_i8<scalar>', 'xbar:pack_wslices<scalar>', 'xbar:ip_ws<p4>/s1/c1'],
    'ss2-one': ['xbar:pack_sm8<scalar>', 'xbar:pack_wslices<scalar>', 'xbar:ip_ss<d2;p4>/s1/c1'],
    'ss2-rag-s3': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d2;p4>/s3/c1', 'xbar:finish'],
    'ss2-xs': ['xbar:pack_sm8<scalar>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d2;p4>/s1/c1'],
    'ss2-ws': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<scalar>', 'xbar:ip_ss<d2;p4>/s1/c1'],
    'ss2-xsws': ['xbar:pack_sm8<scalar>', 'xbar:pack_wslices<scalar>', 'xbar:ip_ss<d2;p4>/s1/c1'],
    'ss2-r256': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d2;p4>/s1/c1'],
    'ss2-clip': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d2;p4>/s1/c1'],
    'ss2-r1024': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d2;p4>/s2/c1', 'xbar:finish'],
    'ss3-one': ['xbar:pack_sm8<scalar>', 'xbar:pack_wslices<scalar>', 'xbar:ip_ss<d3;p4>/s1/c1'],
    'ss3-rag-s3': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d3;p4>/s3/c1', 'xbar:finish'],
    'ss3-xs': ['xbar:pack_sm8<scalar>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d3;p4>/s1/c1'],
    'ss3-ws': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<scalar>', 'xbar:ip_ss<d3;p4>/s1/c1'],
    'ss3-xsws': ['xbar:pack_sm8<scalar>', 'xbar:pack_wslices<scalar>', 'xbar:ip_ss<d3;p4>/s1/c1'],
    'ss3-r256': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d3;p4>/s1/c1'],
    'ss3-clip': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d3;p4>/s1/c1'],
    'ss3-r1024': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d3;p4>/s2/c1', 'xbar:finish'],
    'ss-d1-b4': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d2;p4>/s1/c1'],
    'ss-d1': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d2;p4>/s1/c1'],
    'ss-d1-n7': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d2;p4>/s1/c2', 'xbar:finish'],
    'ss-max': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d2;p4>/s1/c1'],
    'ss-db6': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d2;p4>/s1/c1'],
    'ss-db5': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d2;p4>/s1/c1'],
    'ss-db2': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d2;p4>/s1/c2', 'xbar:finish'],
    'ss-b6-db2': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d3;p4>/s1/c1'],
    'ss-nd5-n5': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d3;p4>/s1/c4', 'xbar:finish'],
    'ss-nd6': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d3;p4>/s1/c2', 'xbar:finish'],
    'ss-nd7-n7': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d3;p4>/s3/c6', 'xbar:finish'],
    'ss-grid': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d2;p4>/s1/c2', 'xbar:finish'],
    'ss-nd7-big': ['xbar:pack_sm8<vec>', 'xbar:pack_wslices<vec>', 'xbar:ip_ss<d3;p4>/s9/c6', 'xbar:finish'],
    'ss-odd': ['xbar:pack_sm8<scalar>', 'xbar:pack_wslices<scalar>', 'xbar:ip_ss<d3;p4>/s1/c1'],
    'cv-one': ['xbar:conv<scalar>/s1'],
    'cv-k45': ['xbar:conv<scalar>/s1'],
    'cv-k45-clip': ['xbar:conv<scalar>/s1'],
    'cv-k45-dac': ['xbar:conv<scalar>/s1'],
    'cv-grp': ['xbar:conv<scalar>/s1'],
    'cv-ng130': ['xbar:conv<scalar>/s1'],
    'cv-dil': ['xbar:conv<vec>/s1'],
    'cv-pw': ['xbar:conv<scalar>/s1'],
    'cv-11x11s4': ['xbar:conv<scalar>/s1'],
    'cv-t11-s3': ['xbar:conv<vec>/s3', 'xbar:finish'],
    'cv-k36-ws': ['xbar:conv<scalar>/s1'],
    'cv-r256': ['xbar:conv<vec>/s1'],
    'cv-r1024': ['xbar:conv<vec>/s2', 'xbar:finish'],
    'cv-wide_x-v': ['xbar:conv<vec>/s1'],
    'cv-wide_x-s': ['xbar:conv<scalar>/s2', 'xbar:finish'],
    'cv-wide_w-v': ['xbar:conv<vec>/s1'],
    'cv-wide_w-s': ['xbar:conv<scalar>/s2', 'xbar:finish'],
    'cv-wide_w-r256': ['xbar:conv<vec>/s1'],
}
# --- end of generated ---

for _c in XBAR_CASES:
    _c["ids"] = XBAR_IDS.get(_c["label"], [])


if __name__ == "__main__":
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    sys.path.insert(0, str(root / "rram-caffe-simulation_amd" / "python"))
    print("XBAR_IDS = {")
    for _c in XBAR_CASES:
        print("    %r: %r," % (_c["label"], query(_c, "kernel_ids")))
    print("}")
