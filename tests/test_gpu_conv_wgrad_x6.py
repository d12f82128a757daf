"""wgrad_x6: the stride-1 3x3 / 5x5 convolution weight gradient on the bf16x6
engine (rram_set_bwd_weight_engine, conv_layer.cu:35-44's weight GEMM), each
case against float64 autograd at 1e-4 of Σ|a·b|, against the fp32-MFMA path on
the same data (the fp32-level guard of tests/_ref64.py) and against itself
(same call, same bits).  Every contraction is at most ~4096 positions."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# gr: positions per output row of an MFMA group of 8 is 8 / gr (the kernel id's second parameter)
CASES = [
    dict(x=(8, 16, 8, 8), cout=32, k=3, p=1, g=1, gr=1),       # aligned rows, 4-row blocks
    dict(x=(5, 8, 13, 13), cout=12, k=3, p=1, g=2, gr=1),      # padded row tail, groups, odd num
    dict(x=(7, 24, 4, 4), cout=40, k=3, p=1, g=1, gr=2),       # two rows per group, ragged 40 / 24 (VGG11 conv5-6)
    dict(x=(9, 8, 2, 2), cout=8, k=3, p=1, g=1, gr=4),         # four rows per group (VGG11 conv7-8)
    dict(x=(3, 5, 10, 7), cout=7, k=3, p=0, g=1, gr=1),        # pad 0, 8 x 5 outputs
    dict(x=(3, 5, 6, 6), cout=7, k=3, p=2, g=1, gr=1),         # pad 2 = k - 1
    dict(x=(4, 32, 16, 16), cout=16, k=5, p=2, g=1, gr=1),     # 5x5: kernel rows dealt to wave pairs
    dict(x=(6, 6, 4, 4), cout=10, k=5, p=2, g=1, gr=2),
    dict(x=(5, 4, 2, 2), cout=6, k=5, p=2, g=1, gr=4),
    dict(x=(4, 256, 8, 8), cout=256, k=3, p=1, g=1, gr=1),     # a VGG11-sized channel count, 4 x 4 tiles
    dict(x=(3, 3, 32, 32), cout=64, k=3, p=1, g=1, gr=1),      # Cin 3, one-row blocks
    dict(x=(1, 2, 5, 70), cout=3, k=3, p=1, g=1, gr=1),        # wider than 32: column chunks
    dict(x=(25, 128, 8, 8), cout=128, k=3, p=1, g=64, gr=1),   # 64 tiles: 7 steps per split, the last split short
    dict(x=(66, 128, 4, 4), cout=128, k=3, p=1, g=64, gr=2),   # two blocks (images) per step, 5 steps per split
]


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs, the float64 gradients (dw on top of its initial value) and their Σ|a·b| scales."""
    import torch
    cs = CASES[i]
    torch.manual_seed(i)
    x = torch.randn(cs["x"])
    w = torch.randn(cs["cout"], cs["x"][1] // cs["g"], cs["k"], cs["k"]) * 0.1
    b = torch.randn(cs["cout"])
    fwd = lambda xx, ww, bb: torch.nn.functional.conv2d(xx, ww, bb, 1, cs["p"], 1, cs["g"])  # noqa: E731
    dy = torch.randn_like(fwd(x, w, b))
    dw0 = torch.randn_like(w)
    xs = [t.double().clone().requires_grad_(True) for t in (x, w, b)]
    fwd(*xs).backward(dy.double())
    xa = [t.double().abs().clone().requires_grad_(True) for t in (x, w, b)]
    fwd(*xa).backward(dy.double().abs())
    ref = [xs[0].grad.numpy(), xs[1].grad.numpy() + dw0.double().numpy(), xs[2].grad.numpy()]
    scale = [xa[0].grad.numpy(), xa[1].grad.numpy() + dw0.abs().double().numpy(), xa[2].grad.numpy()]
    return x, w, dy, dw0, ref, scale


def _desc(cs):
    from rramsim import ops
    return ops.conv_desc(cs["x"], cs["cout"], cs["k"], 1, cs["p"], 1, cs["g"])


def _run(i, device, engine):
    """(dx, dw, db) of conv2d_bwd with the weight-gradient selector at engine
    (None: untouched), the engine reported for the call and its kernel ids."""
    import torch
    from rramsim import ops
    x, w, dy, dw0, _, _ = _case(i)
    d = _desc(CASES[i])
    prev = ops.get_bwd_weight_engine()
    try:
        if engine is not None:
            ops.set_bwd_weight_engine(engine)
        ws = torch.empty(ops.conv2d_bwd_workspace(d, CASES[i]["x"][0]) // 4 + 64, device=device)
        wsb = ws.numel() * 4
        dw, db, dx = dw0.to(device), torch.zeros(CASES[i]["cout"], device=device), torch.empty_like(x, device=device)
        ops.conv2d_bwd(d, x.to(device), w.to(device), dy.to(device), dw, db, dx, ws)
        torch.cuda.synchronize()
        return ([t.cpu().numpy() for t in (dx, dw, db)], ops.bwd_weight_engine_for_conv(d, wsb),
                ops.conv_bwd_kernel_ids(d, ws_bytes=wsb))
    finally:
        ops.set_bwd_weight_engine(prev)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_wgrad_x6_vs_fp64(device, i):
    from rramsim import ops
    import _ref64 as R
    cs = CASES[i]
    _, _, _, _, ref, scale = _case(i)
    off, eng_off, ids_off = _run(i, device, ops.ENGINE_F32)
    on, eng_on, ids_on = _run(i, device, ops.ENGINE_BF16X6)
    assert eng_off == ops.ENGINE_F32 and not [k for k in ids_off if k.startswith("wgrad_x6")]
    assert eng_on == ops.ENGINE_BF16X6
    assert [k.split("/")[0] for k in ids_on if k.startswith("wgrad_x6")] == [f"wgrad_x6<{cs['k']},{cs['gr']}>"], ids_on
    err = {}
    for name, got in (("f32", off), ("x6", on)):
        for g, r, s, nm in zip(got, ref, scale, ("dX", "dW", "db")):
            R.assert_scaled(g, r, s, f"{name} {nm}")
        e = np.abs(got[1].astype(np.float64) - ref[1]) / np.maximum(scale[1], 1e-300)
        err[name] = (float(e.max()), float(e.mean()))
    print(f"case {i}: dW err / sum|a*b| (max, mean)  f32 {err['f32']}  bf16x6 {err['x6']}  {ids_on}")
    bad = R.x6_guard_failures(err["x6"], err["f32"])
    assert not bad, "; ".join(bad)
    again, _, _ = _run(i, device, ops.ENGINE_BF16X6)
    assert np.array_equal(again[1].view(np.uint32), on[1].view(np.uint32)), "second run differs"


@pytest.mark.parametrize("i", [1, 6])
def test_default_selector_keeps_the_fp32_path(device, i):
    from rramsim import ops
    assert ops.get_bwd_weight_engine() == ops.ENGINE_F32
    default, eng, ids = _run(i, device, None)
    off, _, ids_off = _run(i, device, ops.ENGINE_F32)
    assert eng == ops.ENGINE_F32 and ids == ids_off and not [k for k in ids if k.startswith("wgrad_x6")]
    for a, b in zip(default, off):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
