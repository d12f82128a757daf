"""Thin torch-tensor wrappers over the C-ABI (device memory via torch, calls
via ctypes).  Every op launches on torch's current HIP stream and raises
RramError on a non-zero status.  No CPU fallback: tensors must live on the GPU.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _kernels as K


def _lib():
    return K.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise K.RramError("rramsim ops take device tensors (no CPU fallback)")
    if t.dtype not in (torch.float32, torch.int32, torch.int64, torch.uint64, torch.uint8):
        raise K.RramError(f"unsupported dtype {t.dtype}")
    return C.c_void_p(t.data_ptr())


def _f32(t, name):
    if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
        raise K.RramError(f"{name} must be a contiguous float32 tensor")


def counters(n: int, device="cuda") -> torch.Tensor:
    return torch.zeros(n, dtype=torch.int64, device=device)


def fault_threshold(values, split1, split2):
    _f32(values, "values")
    K.check(_lib().rram_fault_threshold(_p(values), values.numel(), split1, split2, _stream()),
            "fault_threshold")


def fault_init(endurance, values, mean, std, thr_neg, thr_zero, seed, map_id=0, layer_id=0):
    _f32(endurance, "endurance")
    _f32(values, "values")
    K.check(_lib().rram_fault_init(_p(endurance), _p(values), endurance.numel(), mean, std,
                                   thr_neg, thr_zero, seed, map_id, layer_id, _stream()),
            "fault_init")


def fail_apply(dw, w, endurance, values, decrement=100.0, eps=1e-20, counter=None):
    for t, nm in ((dw, "dw"), (w, "w"), (endurance, "endurance"), (values, "values")):
        _f32(t, nm)
    K.check(_lib().rram_fail_apply(_p(dw), _p(w), _p(endurance), _p(values), w.numel(),
                                   decrement, eps, _p(counter), _stream()), "fail_apply")


def fail_apply_batched(segs, decrement=100.0, eps=1e-20, counters_t=None):
    arr = (K.FailSeg * len(segs))()
    for i, (dw, w, e, v) in enumerate(segs):
        arr[i] = K.FailSeg(dw.data_ptr(), w.data_ptr(), e.data_ptr(), v.data_ptr(), w.numel())
    K.check(_lib().rram_fail_apply_batched(arr, len(segs), decrement, eps, _p(counters_t),
                                           _stream()), "fail_apply_batched")


def inject(w_clean, w_out, cfg, seed, map_id, layer_id, counter=None):
    _f32(w_clean, "w_clean")
    _f32(w_out, "w_out")
    K.check(_lib().rram_inject_rng(_p(w_clean), _p(w_out), w_clean.numel(), C.byref(cfg), seed,
                                   map_id, layer_id, _p(counter), _stream()), "inject_rng")


def inject_batched(segs, seed, map_id, counters_t=None):
    """segs: list of (w_clean, w_out, layer_id, cfg)."""
    arr = (K.InjectSeg * len(segs))()
    for i, (src, dst, lid, cfg) in enumerate(segs):
        arr[i] = K.InjectSeg(src.data_ptr(), dst.data_ptr(), src.numel(), lid, 0, cfg)
    K.check(_lib().rram_inject_rng_batched(arr, len(segs), seed, map_id, _p(counters_t),
                                           _stream()), "inject_rng_batched")


def stuck_zero_counts(e, v, rows, cols, row_counts, col_counts):
    """row_counts[r] = #(e<0 & v==0) in row r; col_counts[c] += same per column (int32 tensors)."""
    _f32(e, "endurance")
    _f32(v, "values")
    K.check(_lib().rram_stuck_zero_counts(_p(e), _p(v), rows, cols, _p(row_counts), _p(col_counts), _stream()),
            "stuck_zero_counts")


def permute_rows(src, dst, row_len, to, frm):
    K.check(_lib().rram_permute_rows(_p(src), _p(dst), row_len, _p(to), _p(frm), to.numel(), _stream()),
            "permute_rows")


def permute_cols(src, dst, rows, cols, to, frm):
    K.check(_lib().rram_permute_cols(_p(src), _p(dst), rows, cols, _p(to), _p(frm), to.numel(), _stream()),
            "permute_cols")


def permute_elems(src, dst, to, frm):
    K.check(_lib().rram_permute_elems(_p(src), _p(dst), _p(to), _p(frm), to.numel(), _stream()), "permute_elems")


def threshold_strategy(dw, thr, counter=None):
    _f32(dw, "dw")
    K.check(_lib().rram_threshold_strategy(_p(dw), dw.numel(), thr, _p(counter), _stream()),
            "threshold_strategy")


def sgd_update(g, h, momentum, local_rate):
    K.check(_lib().rram_sgd_update(_p(g), _p(h), g.numel(), momentum, local_rate, _stream()),
            "sgd_update")


def axpy(alpha, x, y):
    """y = alpha*x + y (caffe_gpu_axpy, math_functions.cu:65-69)."""
    _f32(x, "x")
    _f32(y, "y")
    if x.numel() != y.numel():
        raise K.RramError("axpy: size mismatch")
    K.check(_lib().rram_axpy(x.numel(), alpha, _p(x), _p(y), _stream()), "axpy")


def fused_update_fail(w, g, h, e, v, decay, momentum, lr, apply_thr, thr, decrement=100.0,
                      eps=1e-20, counter=None):
    K.check(_lib().rram_fused_update_fail(_p(w), _p(g), _p(h), _p(e), _p(v), w.numel(), decay,
                                          momentum, lr, int(apply_thr), thr, decrement, eps,
                                          _p(counter), _stream()), "fused_update_fail")


def _tail_seg(cls, w, g, h, e, v, decay, lr, apply_thr, thr, counter, flip=None, *h2):
    """One K.UpdateSeg, or with h2 one K.OptSeg; flip: None or (w_flip, groups, cin, cout, taps)."""
    flip = flip or (None, 0, 0, 0, 0)
    for t, nm in ((w, "w"), (g, "g"), (h, "h"), (e, "endurance"), (v, "values"), (flip[0], "w_flip"),
                  *((t, "h2") for t in h2)):
        _f32(t, nm)
    return cls(_p(w), _p(g), _p(h), _p(e), _p(v), w.numel(), decay, lr, thr, int(apply_thr), _p(counter),
               _p(flip[0]), *flip[1:], *(_p(t) for t in h2))


def fused_update_fail_batched(segs, momentum, decrement=100.0, eps=1e-20):
    """segs: list of (w, g, h, e, v, decay, lr, apply_thr, thr, counter[, (w_flip, groups, cin, cout, taps)]);
    one launch."""
    arr = (K.UpdateSeg * len(segs))(*(_tail_seg(K.UpdateSeg, *sg) for sg in segs))
    K.check(_lib().rram_fused_update_fail_batched(arr, len(segs), momentum, decrement, eps, _stream()),
            "fused_update_fail_batched")


def nesterov_update(g, h, momentum, local_rate):
    K.check(_lib().rram_nesterov_update(_p(g), _p(h), g.numel(), momentum, local_rate, _stream()), "nesterov_update")


def adagrad_update(g, h, delta, local_rate):
    K.check(_lib().rram_adagrad_update(_p(g), _p(h), g.numel(), delta, local_rate, _stream()), "adagrad_update")


def rmsprop_update(g, h, rms_decay, delta, local_rate):
    K.check(_lib().rram_rmsprop_update(_p(g), _p(h), g.numel(), rms_decay, delta, local_rate, _stream()),
            "rmsprop_update")


def adadelta_update(g, h, h2, momentum, delta, local_rate):
    K.check(_lib().rram_adadelta_update(_p(g), _p(h), _p(h2), g.numel(), momentum, delta, local_rate, _stream()),
            "adadelta_update")


def adam_update(g, m, v, beta1, beta2, eps_hat, corrected_local_rate):
    K.check(_lib().rram_adam_update(_p(g), _p(m), _p(v), g.numel(), beta1, beta2, eps_hat, corrected_local_rate,
                                    _stream()), "adam_update")


def solver_hyper(momentum=0.0, momentum2=0.999, delta=1e-8):
    """rram_solver_hyper: momentum / beta1, momentum2 (beta2; rms_decay for RMSProp), delta / eps_hat."""
    return K.SolverHyper(momentum, momentum2, delta)


def fused_opt_update_fail(kind, hyper, w, g, h, h2, e, v, decay, lr, apply_thr, thr, decrement=100.0, eps=1e-20,
                          counter=None):
    """The fused tail of one blob for solver type `kind` (K.RRAM_SOLVER_*); h2 None for the one-history types."""
    K.check(_lib().rram_fused_opt_update_fail(_p(w), _p(g), _p(h), _p(h2), _p(e), _p(v), w.numel(), int(kind),
                                              C.byref(hyper), decay, lr, int(apply_thr), thr, decrement, eps,
                                              _p(counter), _stream()), "fused_opt_update_fail")


def fused_opt_update_fail_batched(kind, hyper, segs, decrement=100.0, eps=1e-20):
    """segs: list of (w, g, h, h2, e, v, decay, lr, apply_thr, thr, counter[, (w_flip, groups, cin, cout, taps)]);
    one launch."""
    arr = (K.OptSeg * len(segs))(*(_tail_seg(K.OptSeg, *sg[:3], *sg[4:11], sg[11] if len(sg) > 11 else None, sg[3])
                                   for sg in segs))
    K.check(_lib().rram_fused_opt_update_fail_batched(arr, len(segs), int(kind), C.byref(hyper), decrement, eps,
                                                      _stream()), "fused_opt_update_fail_batched")


def gemm(trans_a, trans_b, M, N, K_, alpha, A, B, beta, Cm):
    K.check(_lib().rram_gemm_f32(int(trans_a), int(trans_b), M, N, K_, alpha, _p(A), _p(B), beta,
                                 _p(Cm), _stream()), "gemm")


def gemm_ex(trans_a, trans_b, M, N, K_, alpha, A, lda, B, ldb, beta, Cm, ldc, bias=None,
            bias_mode=0, relu=False, workspace=None):
    ws = _p(workspace)
    wsb = workspace.numel() * workspace.element_size() if workspace is not None else 0
    K.check(_lib().rram_gemm_f32_ex(int(trans_a), int(trans_b), M, N, K_, alpha, _p(A), lda,
                                    _p(B), ldb, beta, _p(Cm), ldc, _p(bias), bias_mode, int(relu),
                                    ws, wsb, _stream()), "gemm_ex")


def gemv(trans_a, M, N, alpha, A, x, beta, y):
    """y = alpha * op(A) x + beta * y, A [M][N] row-major (caffe_gpu_gemv)."""
    K.check(_lib().rram_gemv_f32(int(trans_a), M, N, alpha, _p(A), _p(x), beta, _p(y), _stream()), "gemv")


def conv_desc(x_shape, num_output, kernel, stride=1, pad=0, dilation=1, group=1):
    kh, kw = (kernel, kernel) if isinstance(kernel, int) else kernel
    sh, sw = (stride, stride) if isinstance(stride, int) else stride
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    dh, dw = (dilation, dilation) if isinstance(dilation, int) else dilation
    n, c, h, w = x_shape
    d = K.ConvDesc(n, c, h, w, num_output, kh, kw, ph, pw, sh, sw, dh, dw, group, 0, 0)
    K.check(_lib().rram_conv_out_shape(C.byref(d)), "conv_out_shape")
    return d


ENGINE_F32, ENGINE_BF16X6 = 0, 1


def set_f32_engine(engine):
    """Matrix-core engine of the stride-1 3x3 / 5x5 convolution forward
    (rram_set_f32_engine); returns the previous one."""
    prev = _lib().rram_set_f32_engine(int(engine))
    if prev < 0:
        K.check(prev, "set_f32_engine")
    return prev


def get_f32_engine():
    return _lib().rram_get_f32_engine()


def f32_engine_for_conv(d):
    """Engine rram_conv2d_fwd would use for this descriptor now."""
    return _lib().rram_f32_engine_for_conv(C.byref(d))


def f32_engine_for_ip(M, N, K, ws_bytes=256 << 20):
    """Engine rram_ip_fwd (W [N][K], aligned operands) would use now."""
    return _lib().rram_f32_engine_for_ip(int(M), int(N), int(K), int(ws_bytes))


def conv2d_fwd(d, x, w, bias, y, relu=False):
    K.check(_lib().rram_conv2d_fwd(C.byref(d), _p(x), _p(w), _p(bias), _p(y), int(relu),
                                   _stream()), "conv2d_fwd")


def conv2d_fwd_octets(d, x, x_oct, w, bias, y, y_oct, relu=False):
    """rram_conv2d_fwd with channel-octet companions (x_oct / y_oct: uint8
    tensors of 6 bytes per element, or None)."""
    K.check(_lib().rram_conv2d_fwd_octets(C.byref(d), _p(x), _p(x_oct), _p(w), _p(bias), _p(y), _p(y_oct),
                                          int(relu), _stream()), "conv2d_fwd_octets")


def conv_weight_pack_bytes(d):
    """Bytes of the bf16x6 engine's packed-weight companion for d (0: no pack)."""
    return int(_lib().rram_conv_weight_pack_bytes(C.byref(d)))


def conv2d_fwd_cached(d, x, x_oct, w, w_pack, w_pack_valid, bias, y, y_oct=None, relu=False):
    """rram_conv2d_fwd_octets with a packed-weight companion w_pack (uint8
    tensor of conv_weight_pack_bytes(d) bytes): w_pack_valid False packs w
    into it first, True uses it as is."""
    K.check(_lib().rram_conv2d_fwd_cached(C.byref(d), _p(x), _p(x_oct), _p(w), _p(w_pack), int(bool(w_pack_valid)),
                                          _p(bias), _p(y), _p(y_oct), int(relu), _stream()), "conv2d_fwd_cached")


def conv2d_fwd_strided(d, x, w, bias, y, y_image_stride, relu=False, x_oct=None, w_pack=None, w_pack_valid=False):
    """rram_conv2d_fwd_strided: image n's output at y + n * y_image_stride
    floats (y may be a channel-offset view into a larger NCHW tensor)."""
    K.check(_lib().rram_conv2d_fwd_strided(C.byref(d), _p(x), _p(x_oct), _p(w), _p(w_pack), int(bool(w_pack_valid)),
                                           _p(bias), C.c_void_p(y.data_ptr()), int(y_image_stride), int(relu),
                                           _stream()), "conv2d_fwd_strided")


def conv_output_octets_only(d):
    """1 when rram_conv2d_fwd_octets accepts y = None with y_oct for d now
    (the channel-octet epilogue writes only the companion)."""
    return _lib().rram_conv_output_octets_only(C.byref(d))


def conv_input_octets(d):
    """1 when rram_conv2d_fwd_octets would read an input companion for d now."""
    return _lib().rram_conv_input_octets(C.byref(d))


def conv_octet_plan(d):
    """The channel-octet kernel's host plan for d: dict(rows, cols, per_cu,
    tiles_per_image, pieces), or None when that kernel does not take d."""
    plan = (C.c_int * 5)()
    if not _lib().rram_conv_octet_plan(C.byref(d), plan):
        return None
    return dict(rows=plan[0], cols=plan[1], per_cu=plan[2], tiles_per_image=plan[3], pieces=plan[4])


def conv_fwd_kernel_id(d, x_align16=True):
    """Text id of the forward kernel conv2d_fwd / conv2d_fwd_octets would
    launch for d now (rram_conv_fwd_kernel_id; host only): e.g.
    'cb16<3,2,2,8,2;k1>/rowalign', 'c1x1_dma<4,2,1;v4>', 'patch<3,4,3,8>', 'f32'."""
    buf = C.create_string_buffer(96)
    n = _lib().rram_conv_fwd_kernel_id(C.byref(d), int(bool(x_align16)), buf, len(buf))
    if n < 0:
        K.check(n, "conv_fwd_kernel_id")
    return buf.value.decode()


def conv_fwd_kernel_list():
    """Ids of every instantiated bf16x6 forward kernel (no tiling-kind suffix)."""
    n = _lib().rram_conv_fwd_kernel_list(None, 0)
    buf = C.create_string_buffer(n + 1)
    _lib().rram_conv_fwd_kernel_list(buf, len(buf))
    return buf.value.decode().split()


def _id_lines(fn, *args):
    """A kernel-id query of the fp32 engine (snprintf style) as a list of lines."""
    buf = C.create_string_buffer(4096)
    n = fn(*args, buf, len(buf))
    if n < 0:
        K.check(n, "kernel ids")
    return buf.value.decode().split("\n")[:-1] if n else []


def gemm_kernel_ids(trans_a, trans_b, M, N, K_, lda=None, ldb=None, a_align16=True, b_align16=True, beta_zero=True,
                    ws_bytes=0):
    """One id per kernel gemm_ex would launch now (rram_gemm_kernel_ids; host only)."""
    lda = (M if trans_a else K_) if lda is None else lda
    ldb = (K_ if trans_b else N) if ldb is None else ldb
    return _id_lines(_lib().rram_gemm_kernel_ids, int(trans_a), int(trans_b), M, N, K_, lda, ldb, int(a_align16),
                     int(b_align16), int(beta_zero), int(ws_bytes))


def ip_fwd_kernel_ids(M, N, K_, transpose=False, x_align16=True, w_align16=True, bias=True, relu=False, ws_bytes=0):
    return _id_lines(_lib().rram_ip_fwd_kernel_ids, M, N, K_, int(transpose), int(x_align16), int(w_align16),
                     int(bias), int(relu), int(ws_bytes))


def ip_bwd_kernel_ids(M, N, K_, transpose=False, dw=True, db=True, dx=True, align16=True):
    return _id_lines(_lib().rram_ip_bwd_kernel_ids, M, N, K_, int(transpose), int(dw), int(db), int(dx),
                     int(align16))


def ip_fwd_groups_kernel_ids(G, M, N, K_, transpose=False, w_stride=None, align16=True, ws_bytes=0):
    w_stride = N * K_ if w_stride is None else w_stride
    return _id_lines(_lib().rram_ip_fwd_groups_kernel_ids, G, M, N, K_, int(transpose), int(w_stride), int(align16),
                     int(ws_bytes))


def conv_fwd_kernel_ids(d, x_align16=True, w_align16=True):
    """One id per kernel conv2d_fwd would launch now: the fp32 engine's, or one 'x6:' line."""
    return _id_lines(_lib().rram_conv_fwd_kernel_ids, C.byref(d), int(x_align16), int(w_align16))


def conv_bwd_kernel_ids(d, dw=True, db=True, dx=True, ws_bytes=0, w_flipped=False, w_align16=True):
    return _id_lines(_lib().rram_conv_bwd_kernel_ids, C.byref(d), int(dw), int(db), int(dx), int(ws_bytes),
                     int(w_flipped), int(w_align16))


def f32_kernel_list():
    """Ids of every instantiated kernel of the fp32 engine (no /sS split suffix)."""
    n = _lib().rram_f32_kernel_list(None, 0)
    buf = C.create_string_buffer(n + 1)
    _lib().rram_f32_kernel_list(buf, len(buf))
    return buf.value.decode().split()


def conv2d_bwd_ex(d, x, w, w_flipped, dy, dw=None, db=None, dx=None, workspace=None):
    """rram_conv2d_bwd_ex: conv2d_bwd with the caller's flipped copy of w (or None)."""
    wsb = workspace.numel() * workspace.element_size() if workspace is not None else 0
    K.check(_lib().rram_conv2d_bwd_ex(C.byref(d), _p(x), _p(w), _p(w_flipped), _p(dy), _p(dw), _p(db), _p(dx),
                                      _p(workspace), wsb, _stream()), "conv2d_bwd_ex")


def pack_octets(x, oct_, n, c, h, w):
    K.check(_lib().rram_pack_octets(_p(x), _p(oct_), n, c, h, w, _stream()), "pack_octets")


def conv2d_bwd(d, x, w, dy, dw=None, db=None, dx=None, workspace=None):
    wsb = workspace.numel() * workspace.element_size() if workspace is not None else 0
    K.check(_lib().rram_conv2d_bwd(C.byref(d), _p(x), _p(w), _p(dy), _p(dw), _p(db), _p(dx),
                                   _p(workspace), wsb, _stream()), "conv2d_bwd")


def conv2d_bwd_workspace(d, images):
    return _lib().rram_conv2d_bwd_workspace(C.byref(d), images)


def im2col(im, C_, H, W, kh, kw, ph, pw, sh, sw, dh, dw, col):
    K.check(_lib().rram_im2col(_p(im), C_, H, W, kh, kw, ph, pw, sh, sw, dh, dw, _p(col),
                               _stream()), "im2col")


def col2im(col, C_, H, W, kh, kw, ph, pw, sh, sw, dh, dw, im):
    K.check(_lib().rram_col2im(_p(col), C_, H, W, kh, kw, ph, pw, sh, sw, dh, dw, _p(im),
                               _stream()), "col2im")


def ip_fwd(x, w, bias, y, M, N, K_, transpose=False, relu=False, workspace=None):
    wsb = workspace.numel() * workspace.element_size() if workspace is not None else 0
    K.check(_lib().rram_ip_fwd(_p(x), _p(w), _p(bias), _p(y), M, N, K_, int(transpose), int(relu),
                               _p(workspace), wsb, _stream()), "ip_fwd")


def ip_rows_pack_bytes(M, N, K_, ws_bytes):
    """(bytes, rows per tile) of the bf16x6 engine's packed-row input form (0, 0: not served)."""
    bmc = C.c_int(0)
    b = _lib().rram_ip_rows_pack_bytes(M, N, K_, ws_bytes, C.byref(bmc))
    return b, bmc.value


def ip_fwd_rows(x, x_rows, w, bias, y, y_rows, y_rows_per_tile, M, N, K_, relu=False, workspace=None):
    """rram_ip_fwd_rows: returns whether y_rows was written."""
    wsb = workspace.numel() * workspace.element_size() if workspace is not None else 0
    written = C.c_int(0)
    K.check(_lib().rram_ip_fwd_rows(_p(x), _p(x_rows), _p(w), _p(bias), _p(y), _p(y_rows), y_rows_per_tile, M, N,
                                    K_, int(relu), _p(workspace), wsb, C.byref(written), _stream()), "ip_fwd_rows")
    return bool(written.value)


def ip_bwd(x, w, dy, dw, db, dx, M, N, K_, transpose=False):
    K.check(_lib().rram_ip_bwd(_p(x), _p(w), _p(dy), _p(dw), _p(db), _p(dx), M, N, K_,
                               int(transpose), _stream()), "ip_bwd")


def pool_fwd(x, y, mask, geom, method):
    K.check(_lib().rram_pool_fwd(_p(x), _p(y), _p(mask), *geom, method, _stream()), "pool_fwd")


def pool_relu_bwd(dy, mask, dx, geom, method, relu_y, slope):
    """pool_bwd then the in-place ReLU's backward on dx (factor from relu_y), one launch."""
    K.check(_lib().rram_pool_relu_bwd(_p(dy), _p(mask), _p(dx), *geom, method, _p(relu_y), slope, _stream()),
            "pool_relu_bwd")


def pool_relu_fwd(x, y, mask, geom, method, slope):
    """pool_fwd then an in-place ReLU of y, one launch (rram_pool_relu_fwd)."""
    K.check(_lib().rram_pool_relu_fwd(_p(x), _p(y), _p(mask), *geom, method, slope, _stream()), "pool_relu_fwd")


def pool_bwd(dy, mask, dx, geom, method):
    K.check(_lib().rram_pool_bwd(_p(dy), _p(mask), _p(dx), *geom, method, _stream()), "pool_bwd")


def lrn_fwd(x, y, scale, n, c, h, w, size, alpha, beta, k):
    K.check(_lib().rram_lrn_fwd(_p(x), _p(y), _p(scale), n, c, h, w, size, alpha, beta, k,
                                _stream()), "lrn_fwd")


def lrn_bwd(x, y, scale, dy, dx, n, c, h, w, size, alpha, beta):
    K.check(_lib().rram_lrn_bwd(_p(x), _p(y), _p(scale), _p(dy), _p(dx), n, c, h, w, size, alpha,
                                beta, _stream()), "lrn_bwd")


def lrn_maxpool_fwd(x, y, n, c, h, w, ph, pw, kernel, stride, pad, size, alpha, beta, k=1.0):
    K.check(_lib().rram_lrn_maxpool_fwd(_p(x), _p(y), n, c, h, w, ph, pw, kernel, stride, stride, pad, pad,
                                        size, alpha, beta, k, _stream()), "lrn_maxpool_fwd")


def lrn_maxpool_fwd_octets(x, y, y_oct, n, c, h, w, ph, pw, kernel, stride, pad, size, alpha, beta, k=1.0):
    K.check(_lib().rram_lrn_maxpool_fwd_octets(_p(x), _p(y), _p(y_oct), n, c, h, w, ph, pw, kernel, stride, stride,
                                               pad, pad, size, alpha, beta, k, _stream()), "lrn_maxpool_fwd_octets")


def lrn_within_fwd(x, y, scale, n, c, h, w, size, alpha, beta):
    K.check(_lib().rram_lrn_within_fwd(_p(x), _p(y), _p(scale), n, c, h, w, size, alpha, beta,
                                       _stream()), "lrn_within_fwd")


def lrn_within_bwd(x, scale, dy, dx, n, c, h, w, size, alpha, beta):
    K.check(_lib().rram_lrn_within_bwd(_p(x), _p(scale), _p(dy), _p(dx), n, c, h, w, size, alpha,
                                       beta, _stream()), "lrn_within_bwd")


def lrn_within_relu_bwd(x, scale, dy, dx, n, c, h, w, size, alpha, beta, slope):
    """lrn_within_bwd then the in-place ReLU's backward on dx (factor from x), one launch."""
    K.check(_lib().rram_lrn_within_relu_bwd(_p(x), _p(scale), _p(dy), _p(dx), n, c, h, w, size, alpha, beta,
                                            slope, _stream()), "lrn_within_relu_bwd")


def relu_fwd(x, y, slope=0.0):
    K.check(_lib().rram_relu_fwd(_p(x), _p(y), x.numel(), slope, _stream()), "relu_fwd")


def relu_bwd(x, dy, dx, slope=0.0):
    K.check(_lib().rram_relu_bwd(_p(x), _p(dy), _p(dx), x.numel(), slope, _stream()), "relu_bwd")


def softmax_loss_fwd(prob, label, loss, outer, channels, inner, ignore=-1):
    K.check(_lib().rram_softmax_loss_fwd(_p(prob), _p(label), _p(loss), outer, channels, inner, ignore,
                                         _stream()), "softmax_loss_fwd")


def softmax_loss_bwd(prob, label, dx, outer, channels, inner, ignore=-1, loss_weight=1.0):
    K.check(_lib().rram_softmax_loss_bwd(_p(prob), _p(label), _p(dx), outer, channels, inner, ignore,
                                         loss_weight, _stream()), "softmax_loss_bwd")


def softmax_loss_fwd_bwd(prob, label, loss, dx, outer, channels, inner, ignore=-1, loss_weight=1.0):
    """softmax_loss_fwd + softmax_loss_bwd in one launch (<= 65536 elements)."""
    K.check(_lib().rram_softmax_loss_fwd_bwd(_p(prob), _p(label), _p(loss), _p(dx), outer, channels, inner, ignore,
                                             loss_weight, _stream()), "softmax_loss_fwd_bwd")


def concat_copy(src, dst, num, src_cxi, dst_cxi, off_xi, backward=False):
    K.check(_lib().rram_concat_copy(_p(src), _p(dst), num, src_cxi, dst_cxi, off_xi, int(backward),
                                    _stream()), "concat")


def dropout_fwd(x, y, mask, ratio, seed, layer_id=0, it=0):
    K.check(_lib().rram_dropout_fwd(_p(x), _p(y), _p(mask), x.numel(), ratio, seed, layer_id, it,
                                    _stream()), "dropout_fwd")


def dropout_bwd(dy, mask, dx, ratio):
    K.check(_lib().rram_dropout_bwd(_p(dy), _p(mask), _p(dx), dy.numel(), ratio, _stream()), "dropout_bwd")


def softmax_fwd(x, y, outer, channels, inner):
    K.check(_lib().rram_softmax_fwd(_p(x), _p(y), outer, channels, inner, _stream()), "softmax")


def accuracy(x, label, correct, count, outer, channels, inner, top_k=1, ignore=-1, ratio=None):
    K.check(_lib().rram_accuracy(_p(x), _p(label), _p(correct), _p(count), _p(ratio), outer,
                                 channels, inner, top_k, ignore, _stream()), "accuracy")


def euclidean_loss_fwd(a, b, diff, loss, num):
    """diff = a - b, loss[0] = sum(diff^2) / num / 2 (rram_euclidean_loss_fwd)."""
    K.check(_lib().rram_euclidean_loss_fwd(_p(a), _p(b), _p(diff), _p(loss), a.numel(), num, _stream()),
            "euclidean_loss_fwd")


def euclidean_loss_bwd(diff, dx, alpha):
    K.check(_lib().rram_euclidean_loss_bwd(_p(diff), _p(dx), diff.numel(), alpha, _stream()), "euclidean_loss_bwd")


def i32_to_f32(x, y):
    K.check(_lib().rram_i32_to_f32(_p(x), _p(y), x.numel(), _stream()), "i32_to_f32")


# ---- which kernels of the support layers a call would launch (host only; geom as pool_fwd's) ----
def pool_fwd_kernel_ids(geom, method, mask=True, relu=False):
    """e.g. ['pool_planes<3> ppb=2'] (rram_pool_fwd_kernel_ids)."""
    return _id_lines(_lib().rram_pool_fwd_kernel_ids, *geom, method, int(mask), int(relu))


def pool_bwd_kernel_ids(geom, method, relu=False):
    return _id_lines(_lib().rram_pool_bwd_kernel_ids, *geom, method, int(relu))


def lrn_fwd_kernel_ids(n, c, h, w, size):
    return _id_lines(_lib().rram_lrn_fwd_kernel_ids, n, c, h, w, size)


def lrn_within_bwd_kernel_ids(n, c, h, w, size, relu=False):
    return _id_lines(_lib().rram_lrn_within_bwd_kernel_ids, n, c, h, w, size, int(relu))


def softmax_kernel_ids(outer, channels, inner):
    return _id_lines(_lib().rram_softmax_kernel_ids, outer, channels, inner)


def softmax_loss_kernel_ids(form, outer, channels, inner, ignore=-1, G=1, fold=False, live=None):
    """form: 'fwd' | 'fwd_groups' | 'fwd_bwd' | 'bwd' (rram_softmax_loss_kernel_ids)."""
    form = {"fwd": K.RRAM_LOSS_FWD, "fwd_groups": K.RRAM_LOSS_FWD_GROUPS, "fwd_bwd": K.RRAM_LOSS_FWD_BWD,
            "bwd": K.RRAM_LOSS_BWD}[form]
    return _id_lines(_lib().rram_softmax_loss_kernel_ids, form, G, outer, channels, inner, ignore, int(fold),
                     G if live is None else live)


def accuracy_kernel_ids(outer, channels, inner, ratio=True):
    return _id_lines(_lib().rram_accuracy_kernel_ids, outer, channels, inner, int(ratio))


def accuracy_groups_kernel_ids(G, outer, channels, inner, fold=False, live=None):
    return _id_lines(_lib().rram_accuracy_groups_kernel_ids, G, outer, channels, inner, int(fold),
                     G if live is None else live)


def layer_entry_kernel_ids(entry, n):
    """entry: a key of K.LAYER_ENTRIES, the entries with a single launch form, on n elements."""
    return _id_lines(_lib().rram_layer_entry_kernel_ids, K.LAYER_ENTRIES[entry], n)


def layer_kernel_list():
    """Every id the support layers' launch sites can record (no ' ppb=N')."""
    n = _lib().rram_layer_kernel_list(None, 0)
    buf = C.create_string_buffer(n + 1)
    _lib().rram_layer_kernel_list(buf, len(buf))
    return buf.value.decode().split()


# ---- BatchNorm / Scale / Sigmoid (csrc/norm.hip); tensors are (num, channels, inner...) float32 ----
def _nci(x):
    num, ch = x.shape[0], x.shape[1]
    return num, ch, x.numel() // (num * ch)


def norm_workspace_floats(num, channels, inner):
    return int(_lib().rram_norm_workspace_floats(num, channels, inner))


def bn_stats_train(x, mean, rstd, ws, eps=1e-5, maf=0.999, run_mean=None, run_var=None, factor=None):
    """Per-channel mean and 1 / sqrt(biased var + eps) of x, plus the running update of the three
    BatchNorm blobs when they are given (rram_bn_stats_train)."""
    K.check(_lib().rram_bn_stats_train(_p(x), *_nci(x), eps, maf, _p(mean), _p(rstd), _p(run_mean), _p(run_var),
                                       _p(factor), _p(ws), ws.numel(), _stream()), "bn_stats_train")


def bn_stats_global(run_mean, run_var, factor, mean, rstd, eps=1e-5):
    K.check(_lib().rram_bn_stats_global(_p(run_mean), _p(run_var), _p(factor), run_mean.numel(), eps, _p(mean),
                                        _p(rstd), _stream()), "bn_stats_global")


def norm_apply(x, y, mean=None, rstd=None, gamma=None, beta=None, relu=False, xhat_out=None):
    """y = relu?(gamma * ((x - mean) * rstd) + beta), each stage optional; y may be x (rram_norm_apply)."""
    K.check(_lib().rram_norm_apply(_p(x), _p(y), _p(xhat_out), _p(mean), _p(rstd), _p(gamma), _p(beta), int(relu),
                                   *_nci(x), _stream()), "norm_apply")


def norm_bwd_reduce(dy, xhat, ws, relu_y=None, gamma=None, rstd=None, dgamma=None, dbeta=None, coef=None):
    """dbeta += sum g, dgamma += sum g * xhat per channel, coef = (gamma * rstd, sum g / m, sum g xhat / m)
    (rram_norm_bwd_reduce)."""
    K.check(_lib().rram_norm_bwd_reduce(_p(dy), _p(relu_y), _p(xhat), *_nci(dy), _p(gamma), _p(rstd), _p(dgamma),
                                        _p(dbeta), _p(coef), _p(ws), ws.numel(), _stream()), "norm_bwd_reduce")


def norm_bwd_apply(dy, dx, relu_y=None, xhat=None, coef=None, gamma=None, rstd=None):
    K.check(_lib().rram_norm_bwd_apply(_p(dy), _p(relu_y), _p(xhat), _p(coef), _p(gamma), _p(rstd), _p(dx),
                                       *_nci(dy), _stream()), "norm_bwd_apply")


def scale_fwd(x, y, gamma, beta=None):
    """The stand-alone Scale layer: y = x * gamma[c] (+ beta[c])."""
    norm_apply(x, y, gamma=gamma, beta=beta)


def scale_bwd(x, dy, gamma, ws, dgamma=None, dbeta=None, dx=None):
    """dgamma += sum dy * x, dbeta += sum dy, dx = dy * gamma (dx may be dy)."""
    if dgamma is not None or dbeta is not None:
        norm_bwd_reduce(dy, x, ws, dgamma=dgamma, dbeta=dbeta)
    if dx is not None:
        norm_bwd_apply(dy, dx, gamma=gamma)


def sigmoid_fwd(x, y):
    K.check(_lib().rram_sigmoid_fwd(_p(x), _p(y), x.numel(), _stream()), "sigmoid_fwd")


def sigmoid_bwd(y, dy, dx):
    K.check(_lib().rram_sigmoid_bwd(_p(y), _p(dy), _p(dx), y.numel(), _stream()), "sigmoid_bwd")


def bn_fwd_kernel_ids(num, channels, inner, global_stats=False, x_off=0, y_off=0):
    """e.g. ['bn_stats_plane<4>', 'bn_stats_finalize', 'norm_apply<4>']; *_off: floats past a 16-byte boundary."""
    return _id_lines(_lib().rram_bn_fwd_kernel_ids, num, channels, inner, int(global_stats), x_off, y_off)


def bn_bwd_kernel_ids(num, channels, inner, global_stats=False, scale=False, dy_off=0, dx_off=0):
    return _id_lines(_lib().rram_bn_bwd_kernel_ids, num, channels, inner, int(global_stats), int(scale), dy_off,
                     dx_off)


def scale_kernel_ids(num, channels, inner, backward=False, x_off=0, y_off=0):
    return _id_lines(_lib().rram_scale_kernel_ids, num, channels, inner, int(backward), x_off, y_off)


def sigmoid_kernel_ids(n, backward=False):
    return _id_lines(_lib().rram_sigmoid_kernel_ids, n, int(backward))


def norm_kernel_list():
    """Every id the launch sites of csrc/norm.hip can record."""
    n = _lib().rram_norm_kernel_list(None, 0)
    buf = C.create_string_buffer(n + 1)
    _lib().rram_norm_kernel_list(buf, len(buf))
    return buf.value.decode().split()


def fill_uniform(x, lo, hi, seed, sid=0):
    K.check(_lib().rram_fill_uniform(_p(x), x.numel(), lo, hi, seed, sid, _stream()), "fill")


def fill_gaussian(x, mean, std, seed, sid=0):
    K.check(_lib().rram_fill_gaussian(_p(x), x.numel(), mean, std, seed, sid, _stream()), "fill")


# ------------------------------------------------------------ map batching
def inject_maps(segs, seed, map_begin, nmaps, counters_t=None):
    """segs: list of (w_clean, w_out [nmaps, n], layer_id, cfg): nmaps faulted
    copies of every segment in one launch (rram_inject_rng_maps)."""
    arr = (K.InjectSeg * len(segs))()
    strides = (C.c_int64 * len(segs))()
    for i, (src, dst, lid, cfg) in enumerate(segs):
        arr[i] = K.InjectSeg(src.data_ptr(), dst.data_ptr(), src.numel(), lid, 0, cfg)
        strides[i] = dst.stride(0) if dst.dim() == 2 else src.numel()
    K.check(_lib().rram_inject_rng_maps(arr, len(segs), seed, map_begin, nmaps, strides, _p(counters_t),
                                        _stream()), "inject_rng_maps")


def ip_fwd_groups(x, w, w_stride, bias, bias_stride, y, G, M, N, K_, transpose=False, relu=False, workspace=None):
    """G InnerProduct forwards sharing launches (rram_ip_fwd_groups); strides in elements."""
    wsb = workspace.numel() * workspace.element_size() if workspace is not None else 0
    K.check(_lib().rram_ip_fwd_groups(_p(x), _p(w), w_stride, _p(bias), bias_stride, _p(y), G, M, N, K_,
                                      int(transpose), int(relu), _p(workspace), wsb, _stream()), "ip_fwd_groups")


def ip_fwd_groups_fused(G, M, N, K_, transpose=False, ws_bytes=0):
    return _lib().rram_ip_fwd_groups_fused(G, M, N, K_, int(transpose), ws_bytes)


def softmax_loss_fwd_groups(prob, label, out, G, outer, channels, inner, ignore=-1, acc_sum=None, acc_rows=None,
                            row_stride=1, live=None):
    K.check(_lib().rram_softmax_loss_fwd_groups(_p(prob), _p(label), _p(out), G, outer, channels, inner, ignore,
                                                _p(acc_sum), _p(acc_rows), row_stride, G if live is None else live,
                                                _stream()), "softmax_loss_fwd_groups")


def accuracy_groups(x, label, correct, count, ratio, G, outer, channels, inner, top_k=1, ignore=-1, acc_sum=None,
                    acc_rows=None, row_stride=1, live=None):
    K.check(_lib().rram_accuracy_groups(_p(x), _p(label), _p(correct), _p(count), _p(ratio), G, outer, channels,
                                        inner, top_k, ignore, _p(acc_sum), _p(acc_rows), row_stride,
                                        G if live is None else live, _stream()), "accuracy_groups")
