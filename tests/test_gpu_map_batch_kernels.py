"""Kernels of the Monte-Carlo map batching (include/rram_kernels.h:
rram_inject_rng_maps, rram_ip_fwd_groups, rram_softmax_loss_fwd_groups,
rram_accuracy_groups).  Every entry is specified as bit-identical to a loop of
the existing entry over the groups; that loop is the oracle of each test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(t):
    import torch
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().view(np.uint32).copy()


def _cfgs():
    from rramsim import make_inject_cfg
    from rramsim import _kernels as K
    return {"stuck": make_inject_cfg(0.05, 5, 90, 5),
            "quant_lognormal": make_inject_cfg(0.05, quant_levels=16, g_max=0.5, var_sigma=0.1),
            "diffpair": make_inject_cfg(0.05, quant_levels=16, g_max=0.5, var_sigma=0.1,
                                        cell_mode=K.RRAM_CELL_DIFFPAIR)}


# ------------------------------------------------------------------ injection
@pytest.mark.parametrize("cfg_name", ["stuck", "quant_lognormal", "diffpair"])
@pytest.mark.parametrize("map_begin", [0, 7])
@pytest.mark.parametrize("n", [1, 1023, 4099])
def test_inject_maps_equals_batched_loop(device, cfg_name, map_begin, n):
    import torch
    from rramsim import ops
    cfg = _cfgs()[cfg_name]
    nmaps, seed = 3, 99
    g = torch.Generator(device="cpu").manual_seed(n)
    clean = [(torch.rand(n, generator=g) - 0.5).to(device), (torch.rand(2 * n + 5, generator=g) - 0.5).to(device)]
    ref = [torch.empty(nmaps, c.numel(), device=device) for c in clean]
    ref_cnt = ops.counters(2)
    for j in range(nmaps):
        ops.inject_batched([(clean[i], ref[i][j], 3 + i, cfg) for i in range(2)], seed, map_begin + j, ref_cnt)
    got = [torch.full((nmaps, c.numel()), float("nan"), device=device) for c in clean]
    got_cnt = ops.counters(2)
    ops.inject_maps([(clean[i], got[i], 3 + i, cfg) for i in range(2)], seed, map_begin, nmaps, got_cnt)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
        assert np.array_equal(bits(a), bits(b))
    torch.cuda.synchronize()
    assert got_cnt.tolist() == ref_cnt.tolist()
    if n > 1:
        assert sum(ref_cnt.tolist()) > 0                  # the maps do inject faults
        assert not torch.equal(got[1][0], got[1][1])       # and differ from each other


@pytest.mark.parametrize("cfg_name", ["stuck", "quant_lognormal", "diffpair"])
@pytest.mark.parametrize("n", [1023, 4099])
def test_inject_maps_padded_stride(device, cfg_name, n):
    """Copies strided past n by a multiple of four elements (a stack with
    padding between the copies): the 16-byte store path and its tail."""
    import torch
    from rramsim import ops
    cfg = _cfgs()[cfg_name]
    pad, nmaps = 9, 3
    assert (n + pad) % 4 == 0
    clean = (torch.rand(n) - 0.5).to(device)
    ref = torch.empty(nmaps, n, device=device)
    for j in range(nmaps):
        ops.inject_batched([(clean, ref[j], 1, cfg)], 5, 2 + j)
    buf = torch.zeros(nmaps, n + pad, device=device)
    ops.inject_maps([(clean, buf, 1, cfg)], 5, 2, nmaps)
    assert torch.equal(buf[:, :n], ref) and float(buf[:, n:].abs().sum()) == 0.0


# ------------------------------------------------------------------ grouped IP
def _ip_case(device, G, M, N, K, transpose=False, relu=False, bias="own", ws_floats=None, seed=0):
    """(got, ref): rram_ip_fwd_groups against the loop of rram_ip_fwd with the same workspace."""
    import torch
    from rramsim import ops
    g = torch.Generator(device="cpu").manual_seed(1000 * M + N + K + seed)
    x = (torch.rand(G * M, K, generator=g) - 0.5).to(device)
    w = (torch.rand(G, K, N, generator=g) - 0.5).to(device) if transpose else \
        (torch.rand(G, N, K, generator=g) - 0.5).to(device)
    b = None if bias is None else (torch.rand(G if bias == "own" else 1, N, generator=g) - 0.5).to(device)
    bstride = 0 if bias != "own" else N
    if ws_floats is None:
        ws_floats = G * 16 * M * N
    ws = torch.empty(max(ws_floats, 1), device=device) if ws_floats > 0 else None
    ref = torch.full((G * M, N), float("nan"), device=device)
    for i in range(G):
        bi = None if b is None else b[i if bias == "own" else 0]
        ops.ip_fwd(x[i * M:(i + 1) * M], w[i], bi, ref[i * M:(i + 1) * M], M, N, K, transpose, relu, ws)
    got = torch.full((G * M, N), float("nan"), device=device)
    ops.ip_fwd_groups(x, w, N * K, b, bstride, got, G, M, N, K, transpose, relu, ws)
    return got, ref


IP_CASES = {
    "c2_ip1_splitk": dict(G=3, M=100, N=64, K=1024),
    "c2_ip2": dict(G=3, M=100, N=10, K=64),
    "gemv": dict(G=2, M=1, N=10, K=64),
    "gemv_relu_shared_bias": dict(G=2, M=1, N=10, K=64, relu=True, bias="shared"),
    "unaligned": dict(G=2, M=37, N=19, K=53),
    "unaligned_transpose": dict(G=2, M=37, N=19, K=53, transpose=True),
    "unaligned_relu": dict(G=2, M=37, N=19, K=53, relu=True),
    "unaligned_no_bias": dict(G=2, M=37, N=19, K=53, bias=None),
    "unaligned_shared_bias": dict(G=2, M=37, N=19, K=53, bias="shared"),
    "lenet_ip1_splitk_relu": dict(G=4, M=20, N=500, K=800, relu=True),
    "gemm2_tile": dict(G=2, M=128, N=256, K=512),
    "transpose_splitk": dict(G=2, M=40, N=48, K=640, transpose=True),
}


@pytest.mark.parametrize("case", sorted(IP_CASES))
def test_ip_fwd_groups_equals_loop_f32_engine(device, case):
    import torch
    from rramsim import ops
    prev = ops.set_f32_engine(ops.ENGINE_F32)
    try:
        got, ref = _ip_case(device, **IP_CASES[case])
    finally:
        ops.set_f32_engine(prev)
    assert not torch.isnan(ref).any()
    assert np.array_equal(bits(got), bits(ref))


def test_ip_fwd_groups_fused_on_f32_engine(device):
    from rramsim import ops
    prev = ops.set_f32_engine(ops.ENGINE_F32)
    try:
        for name in ("c2_ip1_splitk", "c2_ip2", "gemv"):
            c = IP_CASES[name]
            assert ops.ip_fwd_groups_fused(c["G"], c["M"], c["N"], c["K"], False,
                                           c["G"] * 16 * c["M"] * c["N"] * 4) == 1, name
    finally:
        ops.set_f32_engine(prev)


def test_ip_fwd_groups_bf16x6_engine(device):
    """The bf16x6 engine's shapes may loop; the bits are the loop's either way."""
    import torch
    from rramsim import ops
    prev = ops.set_f32_engine(ops.ENGINE_BF16X6)
    try:
        got, ref = _ip_case(device, G=2, M=128, N=256, K=512)
        got2, ref2 = _ip_case(device, G=2, M=256, N=1024, K=1024, relu=True)   # a shape the engine serves
        got3, ref3 = _ip_case(device, **IP_CASES["c2_ip1_splitk"])             # one it leaves to fp32
    finally:
        ops.set_f32_engine(prev)
    assert np.array_equal(bits(got), bits(ref))
    assert np.array_equal(bits(got2), bits(ref2))
    assert np.array_equal(bits(got3), bits(ref3))


@pytest.mark.parametrize("ws_floats", [0, 8 * 100 * 64, 2 * 8 * 100 * 64])
def test_ip_fwd_groups_small_workspace(device, ws_floats):
    """A workspace too small for G groups of partials (none, one group's, two
    of three groups'): the call loops, the split is not changed, the bits are
    the loop's with that same workspace."""
    from rramsim import ops
    prev = ops.set_f32_engine(ops.ENGINE_F32)
    try:
        assert ops.ip_fwd_groups_fused(3, 100, 64, 1024, False, ws_floats * 4) == 0
        got, ref = _ip_case(device, G=3, M=100, N=64, K=1024, ws_floats=ws_floats)
    finally:
        ops.set_f32_engine(prev)
    assert np.array_equal(bits(got), bits(ref))


# -------------------------------------------------------- grouped loss / accuracy
@pytest.mark.parametrize("ignore", [-1, 3])
def test_loss_and_accuracy_groups_equal_slices(device, ignore):
    import torch
    from rramsim import ops
    G, outer, C = 3, 20, 10
    g = torch.Generator(device="cpu").manual_seed(11 + ignore)
    x = torch.randn(G * outer, C, generator=g).to(device)
    label = torch.randint(0, C, (G * outer,), generator=g).float()
    label[::4] = 3.0                                        # some rows carry the ignored label
    label = label.to(device)
    prob = torch.empty_like(x)
    ops.softmax_fwd(x, prob, G * outer, C, 1)

    ref_loss = torch.zeros(G, device=device)
    ref_acc = torch.zeros(G, device=device)
    ref_cc = torch.zeros(2, G, device=device)
    for i in range(G):
        sl = slice(i * outer, (i + 1) * outer)
        ops.softmax_loss_fwd(prob[sl], label[sl], ref_loss[i:i + 1], outer, C, 1, ignore)
        ops.accuracy(x[sl], label[sl], ref_cc[0, i:i + 1], ref_cc[1, i:i + 1], outer, C, 1, 1, ignore,
                     ratio=ref_acc[i:i + 1])

    live, stride = 2, 2
    for which in ("loss", "acc"):
        out = torch.full((G,), float("nan"), device=device)
        acc_sum = torch.full((1,), 0.1, device=device)
        rows = torch.full((G, stride), -7.0, device=device)
        if which == "loss":
            ops.softmax_loss_fwd_groups(prob, label, out, G, outer, C, 1, ignore, acc_sum, rows, stride, live)
            ref = ref_loss
        else:
            cc = torch.full((2, G), float("nan"), device=device)
            ops.accuracy_groups(x, label, cc[0], cc[1], out, G, outer, C, 1, 1, ignore, acc_sum, rows, stride, live)
            ref = ref_acc
            assert np.array_equal(bits(cc), bits(ref_cc))
        assert np.array_equal(bits(out), bits(ref)), which
        r = ref.cpu().numpy().astype(np.float32)
        want = np.float32(np.float32(np.float32(0.1) + r[0]) + r[1])
        assert bits(acc_sum)[0] == np.array([want], np.float32).view(np.uint32)[0], which
        rows_h = rows.cpu().numpy()
        assert np.array_equal(rows_h[:2, 0].view(np.uint32), r[:2].view(np.uint32))
        assert np.all(rows_h[2] == -7.0) and np.all(rows_h[:, 1] == -7.0)      # row 2 and the gaps untouched
    assert len(set(ref_loss.cpu().tolist())) == G                               # the slices do differ
