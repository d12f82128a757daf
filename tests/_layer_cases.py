"""The support-layer cases (csrc/layers.hip) of tests/test_layer_kernel_coverage.py
and tests/test_gpu_layer_kernel_matrix.py, written by hand: per case the entry
point, its shape and the kernel ids the entry's own dispatch records for it
(ops.pool_fwd_kernel_ids and its siblings; host only).  A staged pool's id
carries the planes per block it chose (" ppb=N").  Each shape is the smallest
that still takes its branch; the coverage test asserts the branch conditions.
"""
from _ref64 import pool_shape

MAX, AVE = 0, 1


def _pool(x, k, s, p, method, ids, mask=True, relu=False, off=0, bwd=None):
    """x (N, C, H, W); k, s, p = (h, w) pairs; off: the input's base address in floats past a 16-byte boundary;
    bwd: the backward's ids when the case also runs it (MAX backward needs the mask)."""
    return dict(entry="pool", x=x, k=k, s=s, p=p, method=method, mask=mask, relu=relu, off=off, ids=ids,
                bwd=bwd or [])


def _lrn(x, size, ids, scale=True, bwd=False):
    return dict(entry="lrn", x=x, size=size, scale=scale, bwd=bwd, ids=ids + (["lrn_bwd"] if bwd else []))


def _within(x, size, bwd_id, relu=False):
    return dict(entry="within", x=x, size=size, relu=relu, ids=["lrn_within_fwd", bwd_id])


def _softmax(outer, C, inner, ids):
    return dict(entry="softmax", outer=outer, C=C, inner=inner, ids=ids)


def _loss(form, outer, C, inner, ids, ignore=-1, data="", G=1, live=None, fold=False):
    """data: '' | 'all_ignored' | 'clamp' (every label's probability is exactly 0)."""
    return dict(entry="loss", form=form, outer=outer, C=C, inner=inner, ignore=ignore, data=data, G=G,
                live=G if live is None else live, fold=fold, ids=ids)


def _acc(outer, C, inner, ids, top_k=1, ignore=-1, ratio=True, G=0, live=None, fold=False):
    return dict(entry="acc", outer=outer, C=C, inner=inner, top_k=top_k, ignore=ignore, ratio=ratio, G=G,
                live=G if live is None else live, fold=fold, ids=ids)


def _flat(entry, n, ids, **kw):
    return dict(entry=entry, n=n, ids=ids, **kw)


P3, P2, P0, SEP = "pool_planes<3> ppb=%d", "pool_planes<2> ppb=%d", "pool_planes<0> ppb=%d", "pool_planes_sep3 ppb=%d"

LAYER_CASES = [
    # ---- pool forward, staged planes (H W <= 16384) ----
    _pool((1, 4099, 5, 5), (3, 3), (2, 2), (0, 0), MAX, [P3 % 2], off=1),        # 2050 blocks, the last of 1 plane
    _pool((1, 4099, 5, 5), (3, 3), (2, 2), (1, 1), MAX, [P3 % 2], relu=True),
    _pool((1, 6145, 5, 5), (2, 2), (1, 1), (0, 0), MAX, [P2 % 3], off=2),        # 2049 blocks, the last of 1 plane
    _pool((2, 2048, 32, 64), (3, 2), (8, 16), (1, 0), MAX, [P0 % 2]),            # two planes fill the LDS tile
    _pool((1, 4101, 6, 7), (3, 3), (2, 2), (1, 1), AVE, [P0 % 2], off=3),        # H W = 42: no multiple of 4
    _pool((3, 1367, 6, 7), (2, 3), (1, 2), (0, 1), AVE, [P0 % 2], relu=True, off=1),
    _pool((1, 3, 70, 90), (5, 3), (2, 3), (2, 1), AVE, [P0 % 1], off=3),         # 4096 < H W < 16384
    _pool((1, 3, 70, 90), (5, 3), (2, 3), (2, 1), MAX, [P0 % 1], relu=True, off=2),
    _pool((1, 3, 128, 128), (3, 3), (2, 2), (0, 0), MAX, [P3 % 1]),              # H W = 16384 exactly
    _pool((2, 5, 13, 11), (2, 2), (2, 2), (0, 0), MAX, [P2 % 1], mask=False),
    _pool((2, 5, 13, 11), (2, 2), (2, 1), (1, 0), MAX, [P2 % 1], relu=True, off=1),
    _pool((2, 5, 13, 11), (5, 3), (2, 1), (2, 1), MAX, [P0 % 1], mask=False, off=2),
    _pool((1, 2, 70, 70), (3, 3), (1, 1), (1, 1), MAX, [P3 % 1], mask=False),    # no mask, but H W > 4096: not sep3
    _pool((1, 4097, 13, 11), (3, 3), (1, 1), (1, 1), MAX, [SEP % 2], mask=False, off=1),   # PH = 13: two row segments
    _pool((1, 4097, 13, 11), (3, 3), (1, 1), (0, 0), MAX, [SEP % 2], mask=False, relu=True, off=3),
    _pool((2, 3, 7, 9), (3, 3), (1, 1), (0, 0), MAX, [SEP % 1], mask=False),
    _pool((1, 2, 64, 64), (3, 3), (1, 1), (1, 1), MAX, [SEP % 1], mask=False),   # H W = 4096: still sep3
    # ---- pool forward, direct (H W > 16384) ----
    _pool((1, 2, 129, 128), (3, 3), (2, 2), (1, 1), MAX, ["pool_max_fixed<3>"]),
    _pool((1, 2, 129, 128), (3, 3), (2, 3), (0, 0), MAX, ["pool_max_fixed<3>"], mask=False, relu=True, off=1),
    _pool((1, 2, 129, 128), (2, 2), (2, 2), (0, 0), MAX, ["pool_max_fixed<2>"], relu=True),
    _pool((1, 2, 129, 128), (5, 3), (3, 2), (1, 0), MAX, ["pool_fwd"]),
    _pool((1, 2, 129, 128), (3, 3), (2, 2), (1, 1), AVE, ["pool_fwd"], relu=True, off=2),
    # ---- pool backward (with its forward) ----
    _pool((1, 3, 64, 64), (3, 3), (2, 2), (0, 0), MAX, [P3 % 1], bwd=["pool_bwd_plane"]),   # H W = 4096, PH PW = 1024
    _pool((2, 5, 13, 11), (3, 3), (2, 2), (1, 1), MAX, [P3 % 1], relu=True, bwd=["pool_bwd_plane"]),
    _pool((1, 2, 65, 64), (2, 2), (2, 2), (0, 0), MAX, [P2 % 1], bwd=["pool_bwd"]),         # H W = 4160
    _pool((1, 2, 40, 40), (3, 3), (1, 1), (1, 1), MAX, [P3 % 1], relu=True, bwd=["pool_bwd"]),   # PH PW = 1600
    _pool((2, 3, 13, 11), (5, 3), (2, 1), (2, 1), AVE, [P0 % 1], bwd=["pool_bwd"]),
    _pool((2, 3, 13, 11), (3, 2), (1, 2), (1, 0), AVE, [P0 % 1], relu=True, bwd=["pool_bwd"]),
    # ---- LRN across channels: the register window with C below, at and above SIZE and the prefetch depth 8 ----
    *[_lrn((1, C, 257, 1) if i % 2 else (2, C, 5, 7), size, ["lrn_fwd_slide<%d>" % size], scale=i % 2 == 0,
           bwd=C in (2, 9))
      for size in (3, 5) for i, C in enumerate((1, 2, 4, 8, 9, 17))],
    *[_lrn((1, C, 257, 1) if size == 7 else (2, C, 5, 7), size, ["lrn_fwd"], scale=C == 11, bwd=True)
      for size in (1, 7, 9) for C in (4, 11)],
    # ---- LRN within channel ----
    _within((2, 3, 2, 3), 5, "lrn_within_bwd_plane"),                 # the plane is smaller than the window
    _within((2, 3, 2, 3), 1, "lrn_within_bwd_plane", relu=True),
    _within((2, 3, 17, 19), 3, "lrn_within_bwd_plane", relu=True),    # 323 elements: more than one per thread
    _within((1, 2, 17, 19), 7, "lrn_within_bwd_plane"),
    _within((1, 2, 64, 64), 5, "lrn_within_bwd_plane"),               # H W = 4096
    _within((1, 2, 65, 64), 3, "lrn_within_bwd", relu=True),
    _within((1, 2, 65, 64), 7, "lrn_within_bwd"),
    # ---- softmax: the register column up to C = 1024, the strided one above; 8195 columns: the grid-stride loop ----
    *[_softmax(5, C, inner, ["softmax_reg<16>" if C <= 1024 else "softmax"])
      for C in (1, 63, 64, 65, 1024, 1025, 2049) for inner in (1, 3)],
    _softmax(8195, 3, 1, ["softmax_reg<16>"]),
    _softmax(1639, 3, 5, ["softmax_reg<16>"]),
    # ---- softmax loss ----
    _loss("fwd", 1030, 3, 2, ["softmax_loss_fwd"]),                   # 2060 columns: two per thread
    _loss("fwd", 7, 5, 3, ["softmax_loss_fwd"], ignore=1),
    _loss("fwd", 7, 5, 3, ["softmax_loss_fwd"], ignore=2, data="all_ignored"),
    _loss("fwd", 9, 4, 2, ["softmax_loss_fwd"], data="clamp"),
    _loss("fwd_groups", 5, 4, 2, ["softmax_loss_fwd_groups", "fold_groups"], ignore=1, G=3, live=2, fold=True),
    _loss("fwd_groups", 5, 4, 1, ["softmax_loss_fwd_groups"], G=2),
    _loss("fwd_bwd", 8192, 8, 1, ["softmax_loss_fwd_bwd"]),           # 65536 elements exactly
    _loss("fwd_bwd", 1030, 3, 2, ["softmax_loss_fwd_bwd"], ignore=0),
    _loss("fwd_bwd", 7, 5, 3, ["softmax_loss_fwd_bwd"], ignore=2, data="all_ignored"),
    _loss("bwd", 1030, 3, 2, ["softmax_loss_bwd"]),
    _loss("bwd", 7, 5, 3, ["count_valid", "softmax_loss_bwd"], ignore=1),
    _loss("bwd", 700, 3, 3, ["count_valid", "softmax_loss_bwd"], ignore=2, data="all_ignored"),
    # ---- accuracy: the three plans and the register path's boundary C = 1024 in label_hit ----
    _acc(100, 10, 1, ["accuracy_small"]),
    _acc(6, 1024, 2, ["accuracy_fused"], top_k=5),
    _acc(6, 1025, 2, ["accuracy_fused"], top_k=5, ignore=3),
    _acc(6, 1500, 2, ["accuracy_fused"]),
    _acc(16388, 4, 1, ["accuracy", "accuracy_ratio"], ignore=2),      # 4097 blocks
    _acc(16388, 4, 1, ["accuracy"], ratio=False),
    _acc(10, 10, 2, ["accuracy_small_groups", "fold_groups"], G=3, live=2, fold=True),
    _acc(5, 100, 1, ["accuracy_fused", "accuracy_fused"], G=2),
    # ---- elementwise, at counts that are no multiple of 256 ----
    _flat("relu", 1000, ["relu_fwd", "relu_bwd"]),
    _flat("concat", 3 * 35, ["concat", "concat"], num=3, sci=35, dci=100, off=45),
    _flat("i32_to_f32", 1000, ["i32_to_f32"]),
    _flat("euclidean", 1500, ["euclidean_fwd", "scale_copy"], num=6),
    _flat("euclidean", 50, ["euclidean_fwd", "scale_copy"], num=5),
]


def geom(cs):
    n, c, h, w = cs["x"]
    return (n, c, h, w) + pool_shape(h, w, *cs["k"], *cs["s"], *cs["p"]) + cs["k"] + cs["s"] + cs["p"]


def ids_of(cs):
    """The ids the entry points of this case record now, in the order the matrix calls them."""
    from rramsim import ops
    e = cs["entry"]
    if e == "pool":
        ids = ops.pool_fwd_kernel_ids(geom(cs), cs["method"], cs["mask"], cs["relu"])
        return ids, (ops.pool_bwd_kernel_ids(geom(cs), cs["method"], cs["relu"]) if cs["bwd"] else [])
    if e == "lrn":
        n = cs["x"][0] * cs["x"][1] * cs["x"][2] * cs["x"][3]
        return ops.lrn_fwd_kernel_ids(*cs["x"], cs["size"]) + (ops.layer_entry_kernel_ids("lrn_bwd", n) if cs["bwd"] else [])
    if e == "within":
        n = cs["x"][0] * cs["x"][1] * cs["x"][2] * cs["x"][3]
        return ops.layer_entry_kernel_ids("lrn_within_fwd", n) + ops.lrn_within_bwd_kernel_ids(*cs["x"], cs["size"], cs["relu"])
    if e == "softmax":
        return ops.softmax_kernel_ids(cs["outer"], cs["C"], cs["inner"])
    if e == "loss":
        return ops.softmax_loss_kernel_ids(cs["form"], cs["outer"], cs["C"], cs["inner"], cs["ignore"], cs["G"],
                                           cs["fold"], cs["live"])
    if e == "acc":
        if cs["G"]:
            return ops.accuracy_groups_kernel_ids(cs["G"], cs["outer"], cs["C"], cs["inner"], cs["fold"], cs["live"])
        return ops.accuracy_kernel_ids(cs["outer"], cs["C"], cs["inner"], cs["ratio"])
    if e == "relu":
        return ops.layer_entry_kernel_ids("relu_fwd", cs["n"]) + ops.layer_entry_kernel_ids("relu_bwd", cs["n"])
    if e == "concat":
        return ops.layer_entry_kernel_ids("concat", cs["n"]) * 2          # forward and backward copy
    if e == "i32_to_f32":
        return ops.layer_entry_kernel_ids("i32_to_f32", cs["n"])
    if e == "euclidean":
        return (ops.layer_entry_kernel_ids("euclidean_loss_fwd", cs["n"]) +
                ops.layer_entry_kernel_ids("euclidean_loss_bwd", cs["n"]))
    raise KeyError(e)


def want_ids(cs):
    return (cs["ids"], cs["bwd"]) if cs["entry"] == "pool" else cs["ids"]


def all_ids(cs):
    return cs["ids"] + (cs["bwd"] if cs["entry"] == "pool" else [])


def name(line):
    """'pool_planes<3> ppb=2' -> 'pool_planes<3>'."""
    return line.split(" ")[0]


def ppb(cs):
    """Planes per block of a staged pool forward, else None."""
    ln = cs["ids"][0]
    return int(ln.split("ppb=")[1]) if "ppb=" in ln else None


def label(i):
    cs = LAYER_CASES[i]
    e = cs["entry"]
    if e == "pool":
        d = "x".join(map(str, cs["x"])) + "-k%dx%d-s%dx%d-p%dx%d" % (cs["k"] + cs["s"] + cs["p"])
        d += ("-ave" if cs["method"] else "-max") + ("" if cs["mask"] else "-nomask") + ("-relu" if cs["relu"] else "")
        d += ("-off%d" % cs["off"] if cs["off"] else "") + ("-bwd" if cs["bwd"] else "")
    elif e in ("lrn", "within"):
        d = "x".join(map(str, cs["x"])) + "-size%d" % cs["size"]
    elif e in ("softmax", "loss", "acc"):
        d = "%dx%dx%d" % (cs["outer"], cs["C"], cs["inner"]) + ("-" + cs["form"] if e == "loss" else "")
    else:
        d = str(cs["n"])
    return "%02d-%s-%s" % (i, e, d)
