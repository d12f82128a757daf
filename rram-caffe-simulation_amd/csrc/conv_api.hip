// C-ABI entry points for GEMM / GEMV / convolution / InnerProduct.
// The heavy lifting is in gemm.hip (MFMA core) — this file validates
// arguments, computes Caffe's shape rules and sequences the backward passes.
#include <algorithm>
#include <atomic>

#include "rram_common.hpp"

namespace rram {
int gemm_core(int trans_a, int trans_b, int M, int N, int K, float alpha, const float* A, int lda,
              const float* B, int ldb, float beta, float* C, int ldc, const float* bias,
              int bias_mode, int relu, void* ws, size_t ws_bytes, hipStream_t s);
int conv_fwd_core(const rram_conv_desc* d, const float* x, const float* w, const float* bias,
                  float* y, int relu, hipStream_t s, int64_t y_img = 0);
int conv_bwd_weight_core(const rram_conv_desc* d, int nimg, const float* dy, const float* col,
                         int64_t ldcol, float* dw, void* part, size_t part_bytes, hipStream_t s,
                         float* db = nullptr);
int bwd_weight_split(int M, int N, int64_t K);
bool conv_bwd_weight_im2t_ok(const rram_conv_desc* d, size_t part_bytes);
int conv_bwd_weight_im2t(const rram_conv_desc* d, const float* x, const float* dy, float* dw, float* db, void* part,
                         size_t part_bytes, hipStream_t s);
int conv_bwd_data_col_core(const rram_conv_desc* d, int nimg, const float* w, const float* dy,
                           float* col, int64_t ldcol, hipStream_t s);
int im2col_core(const float* im, int64_t im_img, int nimg, const rram_conv_desc* d, float* col,
                int64_t ldcol, hipStream_t s, int ones_row = 0);
int col2im_core(const float* col, int64_t ldcol, int nimg, const rram_conv_desc* d, float* im,
                int64_t im_img, int accumulate, hipStream_t s);
int gemv_core(int trans, int M, int N, float alpha, const float* A, const float* x, float beta,
              float* y, hipStream_t s);
std::atomic<int>& conv_plan_num();
int gemm_groups_fused(int G, int M, int N, int K, bool have_ws, size_t ws_bytes);
int gemm_groups_core(int G, int trans_b, int M, int N, int K, const float* A, int64_t grp_a, const float* B, int ldb,
                     int64_t grp_b, float* C, int64_t grp_c, const float* bias, int64_t grp_bias, int relu, void* ws,
                     size_t ws_bytes, hipStream_t s);
int gemv_groups_core(int G, int N, int K, const float* W, int64_t grp_w, const float* x, const float* bias,
                     int64_t grp_bias, int relu, float* y, hipStream_t s);
int release_conv_tables();
std::atomic<uint64_t>& scratch_gen();
int pack_octets(const float* x, void* oct, int num, int C, int HWi, hipStream_t s);
std::atomic<int>& f32_engine();
std::string f32_kernel_list();

namespace {

__global__ void __launch_bounds__(256) k_bias_add(float* __restrict__ y, const float* __restrict__ b,
                                                  int num, int C, int inner) {
  const int64_t total = (int64_t)num * C * inner;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int c = static_cast<int>((i / inner) % C);
    y[i] += b[c];
  }
}

// db[c] += sum over (n, inner) of dy; one block per channel, deterministic
// (fixed per-thread order, fixed tree); image-major walk, no divisions.
__global__ void __launch_bounds__(256) k_bias_bwd(const float* __restrict__ dy, float* __restrict__ db,
                                                  int num, int C, int inner) {
  __shared__ float part[4];
  const int c = blockIdx.x;
  float s = 0.0f;
  if (inner >= 128) {
    for (int n = 0; n < num; ++n) {
      const float* row = dy + ((int64_t)n * C + c) * inner;
      for (int q = threadIdx.x; q < inner; q += blockDim.x) s += row[q];
    }
  } else {
    // short rows (InnerProduct: inner = 1): the threads walk (n, q) jointly so
    // every thread has work instead of `inner` of them walking all n
    const int total = num * inner;
    for (int t = threadIdx.x; t < total; t += blockDim.x) {
      const int n = t / inner, q = t - n * inner;
      s += dy[((int64_t)n * C + c) * inner + q];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) db[c] += part[0] + part[1] + part[2] + part[3];
}

// Two-stage deterministic bias gradient when a workspace is at hand: block
// (c, j) sums images [j*per, (j+1)*per) of channel c into part[c][j]; then
// db[c] += part[c][0] + ... + part[c][S-1] in order.
__global__ void __launch_bounds__(256) k_bias_bwd_part(const float* __restrict__ dy, float* __restrict__ part,
                                                       int num, int C, int inner, int per) {
  __shared__ float red[4];
  const int c = blockIdx.x, j = blockIdx.y;
  const int n1 = min(num, (j + 1) * per);
  float s = 0.0f;
  for (int n = j * per; n < n1; ++n) {
    const float* row = dy + ((int64_t)n * C + c) * inner;
    for (int q = threadIdx.x; q < inner; q += blockDim.x) s += row[q];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[(int64_t)c * gridDim.y + j] = red[0] + red[1] + red[2] + red[3];
}
// one wave per channel: lane l sums partials l, l + 64, ...; fixed xor tree
__global__ void __launch_bounds__(64) k_bias_bwd_reduce(const float* __restrict__ part, float* __restrict__ db,
                                                        int C, int S) {
  const int c = blockIdx.x;
  float s = 0.0f;
  for (int j = threadIdx.x; j < S; j += 64) s += part[(int64_t)c * S + j];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (threadIdx.x == 0) db[c] += s;
}

// wt[g*cin_g + c][co][tap] = w[g*cout_g + co][c][T-1-tap]: each group's kernel
// transposed (in <-> out channels) and rotated 180 degrees (taps reversed), the
// weights of the stride-1 data gradient as a forward convolution
__global__ void __launch_bounds__(256) k_flip_kernel(const float* __restrict__ w, float* __restrict__ wt,
                                                     int G, int cin_g, int cout_g, int T) {
  const int total = G * cin_g * cout_g * T;  // < 2^31 (checked by the caller)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    int t = i;
    const int tap = t % T;
    t /= T;
    const int co = t % cout_g;
    t /= cout_g;
    const int c = t % cin_g;
    const int g = t / cin_g;
    wt[i] = w[((g * cout_g + co) * cin_g + c) * T + (T - 1 - tap)];
  }
}

// the stride-1 data gradient as a forward convolution with the flipped
// kernel: padding dil (k - 1) - pad >= 0 per axis, 32-bit sizes (d: shape
// filled by rram_conv_out_shape)
bool flip_geometry_ok(const rram_conv_desc& d) {
  const int eph = d.dilation_h * (d.kernel_h - 1) - d.pad_h, epw = d.dilation_w * (d.kernel_w - 1) - d.pad_w;
  const size_t wt_bytes = (size_t)d.channels * (d.num_output / d.group) * d.kernel_h * d.kernel_w * sizeof(float);
  return d.stride_h == 1 && d.stride_w == 1 && eph >= 0 && epw >= 0 && wt_bytes < (1ull << 31) &&
         (int64_t)d.num * d.height * d.width < (1ll << 31) &&
         (int64_t)d.num * d.num_output * d.out_h * d.out_w * 4 < (1ll << 31);
}

int check_desc(const rram_conv_desc* d) {
  RRAM_REQUIRE(d != nullptr, "conv: desc is NULL");
  RRAM_REQUIRE(d->num >= 0 && d->channels > 0 && d->height > 0 && d->width > 0 &&
                   d->num_output > 0,
               "conv: bad input/output sizes");
  RRAM_REQUIRE(d->kernel_h > 0 && d->kernel_w > 0 && d->stride_h > 0 && d->stride_w > 0 &&
                   d->dilation_h > 0 && d->dilation_w > 0 && d->pad_h >= 0 && d->pad_w >= 0,
               "conv: bad kernel/stride/pad/dilation");
  RRAM_REQUIRE(d->group > 0 && d->channels % d->group == 0 && d->num_output % d->group == 0,
               "conv: channels and num_output must be divisible by group");
  return RRAM_OK;
}

}  // namespace
}  // namespace rram

using namespace rram;

extern "C" {

int rram_release_caches(void) { return rram::release_conv_tables(); }

uint64_t rram_scratch_generation(void) { return rram::scratch_gen().load(); }

int rram_set_f32_engine(int engine) {
  RRAM_REQUIRE(engine == RRAM_ENGINE_F32 || engine == RRAM_ENGINE_BF16X6, "conv engine: unknown engine");
  return rram::f32_engine().exchange(engine);
}

int rram_get_f32_engine(void) { return rram::f32_engine().load(); }

int rram_gemm_f32_ex(int trans_a, int trans_b, int M, int N, int K, float alpha, const float* A,
                     int lda, const float* B, int ldb, float beta, float* C, int ldc,
                     const float* bias, int bias_mode, int relu, void* ws, size_t ws_bytes,
                     rram_stream_t s) {
  RRAM_REQUIRE(bias_mode >= RRAM_BIAS_NONE && bias_mode <= RRAM_BIAS_COL, "gemm: bad bias_mode");
  return gemm_core(trans_a != 0, trans_b != 0, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, bias,
                   bias_mode, relu, ws, ws_bytes, as_stream(s));
}

int rram_gemm_f32(int trans_a, int trans_b, int M, int N, int K, float alpha, const float* A,
                  const float* B, float beta, float* C, rram_stream_t s) {
  const int lda = trans_a ? M : K;
  const int ldb = trans_b ? K : N;
  return gemm_core(trans_a != 0, trans_b != 0, M, N, K, alpha, A, lda, B, ldb, beta, C, N, nullptr,
                   RRAM_BIAS_NONE, 0, nullptr, 0, as_stream(s));
}

int rram_gemv_f32(int trans_a, int M, int N, float alpha, const float* A, const float* x,
                  float beta, float* y, rram_stream_t s) {
  return gemv_core(trans_a != 0, M, N, alpha, A, x, beta, y, as_stream(s));
}

int rram_conv_out_shape(rram_conv_desc* d) {
  const int rc = check_desc(d);
  if (rc) return rc;
  const int ekh = d->dilation_h * (d->kernel_h - 1) + 1;
  const int ekw = d->dilation_w * (d->kernel_w - 1) + 1;
  RRAM_REQUIRE(d->height + 2 * d->pad_h >= ekh && d->width + 2 * d->pad_w >= ekw,
               "conv: kernel larger than padded input");
  d->out_h = (d->height + 2 * d->pad_h - ekh) / d->stride_h + 1;
  d->out_w = (d->width + 2 * d->pad_w - ekw) / d->stride_w + 1;
  return RRAM_OK;
}

int rram_conv2d_fwd(const rram_conv_desc* d_in, const float* x, const float* w, const float* bias,
                    float* y, int relu, rram_stream_t s) {
  rram_conv_desc d = *d_in;
  int rc = rram_conv_out_shape(&d);
  if (rc) return rc;
  if (d.num == 0) return RRAM_OK;
  RRAM_REQUIRE(x && w && y, "conv2d_fwd: NULL pointer");
  RRAM_REQUIRE((int64_t)d.num * d.out_h * d.out_w < (1ll << 31), "conv2d_fwd: too many output positions");
  return conv_fwd_core(&d, x, w, bias, y, relu, as_stream(s));
}

int rram_conv2d_fwd_octets(const rram_conv_desc* d_in, const float* x, const void* x_oct, const float* w,
                           const float* bias, float* y, void* y_oct, int relu, rram_stream_t s) {
  rram_conv_desc d = *d_in;
  int rc = rram_conv_out_shape(&d);
  if (rc) return rc;
  if (d.num == 0) return RRAM_OK;
  RRAM_REQUIRE(x && w && (y || y_oct), "conv2d_fwd_octets: NULL pointer");
  RRAM_REQUIRE((int64_t)d.num * d.out_h * d.out_w < (1ll << 31), "conv2d_fwd_octets: too many output positions");
  RRAM_REQUIRE(x_oct == nullptr || d.channels % 8 == 0, "conv2d_fwd_octets: input octets need channels %% 8 == 0");
  RRAM_REQUIRE(y_oct == nullptr || d.num_output % 8 == 0, "conv2d_fwd_octets: output octets need num_output %% 8 == 0");
  rc = conv_x6_fwd(&d, x, x_oct, w, bias, y, y_oct, relu, as_stream(s));
  if (rc < 0) return rc;
  if (rc > 0) return RRAM_OK;
  RRAM_REQUIRE(y != nullptr, "conv2d_fwd_octets: y = NULL needs rram_conv_output_octets_only(d) == 1");
  rc = conv_fwd_core(&d, x, w, bias, y, relu, as_stream(s));
  if (rc == 0 && y_oct != nullptr) rc = pack_octets(y, y_oct, d.num, d.num_output, d.out_h * d.out_w, as_stream(s));
  return rc;
}

size_t rram_conv_weight_pack_bytes(const rram_conv_desc* d_in) {
  if (d_in == nullptr) return 0;
  rram_conv_desc d = *d_in;
  if (rram_conv_out_shape(&d) != RRAM_OK || d.num == 0) return 0;
  size_t bytes = 0;
  WPack q;
  q.query = &bytes;
  return conv_x6_fwd(&d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, q) > 0 ? bytes : 0;
}

int rram_conv2d_fwd_cached(const rram_conv_desc* d_in, const float* x, const void* x_oct, const float* w,
                           void* w_pack, int w_pack_valid, const float* bias, float* y, void* y_oct, int relu,
                           rram_stream_t s) {
  RRAM_REQUIRE(w_pack != nullptr || !w_pack_valid, "conv2d_fwd_cached: w_pack_valid without a w_pack buffer");
  if (w_pack == nullptr) return rram_conv2d_fwd_octets(d_in, x, x_oct, w, bias, y, y_oct, relu, s);
  rram_conv_desc d = *d_in;
  int rc = rram_conv_out_shape(&d);
  if (rc) return rc;
  if (d.num == 0) return RRAM_OK;
  RRAM_REQUIRE(x && w && (y || y_oct), "conv2d_fwd_cached: NULL pointer");
  RRAM_REQUIRE((int64_t)d.num * d.out_h * d.out_w < (1ll << 31), "conv2d_fwd_cached: too many output positions");
  RRAM_REQUIRE(x_oct == nullptr || d.channels % 8 == 0, "conv2d_fwd_cached: input octets need channels %% 8 == 0");
  RRAM_REQUIRE(y_oct == nullptr || d.num_output % 8 == 0, "conv2d_fwd_cached: output octets need num_output %% 8 == 0");
  RRAM_REQUIRE(rram_conv_weight_pack_bytes(&d) > 0, "conv2d_fwd_cached: this shape's engine takes no weight pack");
  RRAM_REQUIRE((reinterpret_cast<uintptr_t>(w_pack) & 15u) == 0, "conv2d_fwd_cached: w_pack must be 16-byte aligned");
  WPack wk;
  wk.p = w_pack;
  wk.valid = w_pack_valid != 0;
  rc = conv_x6_fwd(&d, x, x_oct, w, bias, y, y_oct, relu, as_stream(s), wk);
  if (rc < 0) return rc;
  RRAM_REQUIRE(rc > 0, "conv2d_fwd_cached: the packed-weight engine did not run (w misaligned?)");
  return RRAM_OK;
}

int rram_conv2d_fwd_strided(const rram_conv_desc* d_in, const float* x, const void* x_oct, const float* w,
                            void* w_pack, int w_pack_valid, const float* bias, float* y, int64_t y_image_stride,
                            int relu, rram_stream_t s) {
  RRAM_REQUIRE(w_pack != nullptr || !w_pack_valid, "conv2d_fwd_strided: w_pack_valid without a w_pack buffer");
  rram_conv_desc d = *d_in;
  int rc = rram_conv_out_shape(&d);
  if (rc) return rc;
  if (d.num == 0) return RRAM_OK;
  RRAM_REQUIRE(x && w && y, "conv2d_fwd_strided: NULL pointer");
  const int64_t dense = (int64_t)d.num_output * d.out_h * d.out_w;
  RRAM_REQUIRE(y_image_stride >= dense, "conv2d_fwd_strided: image stride %lld < num_output * Ho * Wo = %lld",
               (long long)y_image_stride, (long long)dense);
  RRAM_REQUIRE(((int64_t)d.num - 1) * y_image_stride + dense < (1ll << 31) &&
                   (int64_t)d.num * d.out_h * d.out_w < (1ll << 31),
               "conv2d_fwd_strided: output span >= 2^31 floats");
  RRAM_REQUIRE(x_oct == nullptr || d.channels % 8 == 0, "conv2d_fwd_strided: input octets need channels %% 8 == 0");
  WPack wk;
  wk.y_img = y_image_stride;
  if (w_pack != nullptr) {
    RRAM_REQUIRE(rram_conv_weight_pack_bytes(&d) > 0, "conv2d_fwd_strided: this shape's engine takes no weight pack");
    RRAM_REQUIRE((reinterpret_cast<uintptr_t>(w_pack) & 15u) == 0, "conv2d_fwd_strided: w_pack must be 16-byte aligned");
    wk.p = w_pack;
    wk.valid = w_pack_valid != 0;
  }
  rc = conv_x6_fwd(&d, x, x_oct, w, bias, y, nullptr, relu, as_stream(s), wk);
  if (rc < 0) return rc;
  if (rc > 0) return RRAM_OK;
  RRAM_REQUIRE(w_pack == nullptr, "conv2d_fwd_strided: the packed-weight engine did not run (w misaligned?)");
  return conv_fwd_core(&d, x, w, bias, y, relu, as_stream(s), y_image_stride);
}

namespace {
// split-K partial buffer of the weight gradient (conv_bwd_weight_core) for
// chunks of `imgs` images
// (N = K + 1: room for the folded bias column, see rram_conv2d_bwd)
size_t bwd_part_bytes(const rram_conv_desc& d, int imgs) {
  const int M = d.num_output / d.group;
  const int N = d.channels / d.group * d.kernel_h * d.kernel_w + 1;
  const int sp = bwd_weight_split(M, N, (int64_t)imgs * d.out_h * d.out_w);
  return sp > 1 ? (size_t)sp * M * N * sizeof(float) : 0;
}
// the K column rows + the ones row of the folded bias gradient
size_t col_bytes(const rram_conv_desc& d, int imgs) {
  return ((size_t)d.channels * d.kernel_h * d.kernel_w + 1) * (size_t)imgs * d.out_h * d.out_w * sizeof(float);
}
// The column path's share of ws_bytes: the largest image chunk (0: not even one
// image fits) whose column buffer + weight-gradient partials (want_dw) fit, the
// partials' offset (256-byte aligned) and bytes (0: no split-K, none wanted or no room)
struct BwdColPlan { int chunk; size_t col_bytes_rounded, part_bytes; };
static BwdColPlan bwd_col_plan(const rram_conv_desc& d, size_t ws_bytes, bool want_dw) {
  const size_t per_img = col_bytes(d, 1);
  int chunk = static_cast<int>(std::min<size_t>(ws_bytes / per_img, d.num));
  if (chunk < 1) return {0, 0, 0};
  size_t part = want_dw ? bwd_part_bytes(d, chunk) : 0;
  while (chunk > 1 && col_bytes(d, chunk) + part > ws_bytes) {
    --chunk;
    part = bwd_part_bytes(d, chunk);
  }
  const size_t col = (col_bytes(d, chunk) + 255) / 256 * 256;
  return {chunk, col, col + part <= ws_bytes ? part : 0};
}
}  // namespace

size_t rram_conv2d_bwd_workspace(const rram_conv_desc* d_in, int images_per_chunk) {
  rram_conv_desc d = *d_in;
  if (rram_conv_out_shape(&d) != RRAM_OK || images_per_chunk < 1) return 0;
  return col_bytes(d, images_per_chunk) + bwd_part_bytes(d, images_per_chunk);
}

int rram_conv2d_bwd(const rram_conv_desc* d_in, const float* x, const float* w, const float* dy,
                    float* dw, float* db, float* dx, void* ws, size_t ws_bytes, rram_stream_t st) {
  return rram_conv2d_bwd_ex(d_in, x, w, nullptr, dy, dw, db, dx, ws, ws_bytes, st);
}

int rram_conv2d_flip_applies(const rram_conv_desc* d_in) {
  if (d_in == nullptr) return 0;
  rram_conv_desc d = *d_in;
  if (rram_conv_out_shape(&d) != RRAM_OK) return 0;
  return flip_geometry_ok(d) ? 1 : 0;
}

int rram_conv2d_bwd_ex(const rram_conv_desc* d_in, const float* x, const float* w, const float* w_flipped,
                       const float* dy, float* dw, float* db, float* dx, void* ws, size_t ws_bytes,
                       rram_stream_t st) {
  rram_conv_desc d = *d_in;
  int rc = rram_conv_out_shape(&d);
  if (rc) return rc;
  if (d.num == 0) return RRAM_OK;
  RRAM_REQUIRE(dy != nullptr, "conv2d_bwd: dy is NULL");
  hipStream_t s = as_stream(st);
  const int HoWo = d.out_h * d.out_w;
  // The bias gradient folded into the weight-gradient GEMM (one more output
  // column against a ones row of the column matrix, summed by the split-K
  // reduce): no bias kernels.  Ungrouped layers whose weight GEMM is split
  // (partials in the workspace) and whose every image chunk has >= 2 K-tiles.
  // The weight gradient gathers its column matrix inside the GEMM
  // (conv_bwd_weight_im2t: no im2col pass, all images in one split GEMM) when
  // the workspace holds its split-K partials; else the column path below.
  const bool im2t = dw && x && w && ws && conv_bwd_weight_im2t_ok(&d, ws_bytes);
  bool fold_db = im2t && db && d.group == 1;
  if (!im2t && db && dw && x && w && ws && d.group == 1 && HoWo >= 2 * 32)
    fold_db = bwd_col_plan(d, ws_bytes, true).part_bytes > 0;
  if (db && !fold_db) {
    const int S = d.num < 64 ? d.num : 64;
    if (ws && S > 1 && ws_bytes >= (size_t)d.num_output * S * sizeof(float)) {
      // the workspace head holds the partials; the passes below reuse it after
      // this reduction (same stream)
      float* part = static_cast<float*>(ws);
      const int per = (d.num + S - 1) / S;
      const int Sx = (d.num + per - 1) / per;
      if (!plan_note("aux:bias_bwd_part\naux:bias_bwd_reduce")) {
        hipLaunchKernelGGL(k_bias_bwd_part, dim3(d.num_output, Sx), dim3(256), 0, s, dy, part, d.num, d.num_output,
                           HoWo, per);
        hipLaunchKernelGGL(k_bias_bwd_reduce, dim3(d.num_output), dim3(64), 0, s, part, db,
                           d.num_output, Sx);
      }
    } else if (!plan_note("aux:bias_bwd")) {
      hipLaunchKernelGGL(k_bias_bwd, dim3(d.num_output), dim3(256), 0, s, dy, db, d.num, d.num_output, HoWo);
    }
    rc = launch_status("conv bias bwd");
    if (rc) return rc;
  }
  if (!dw && !dx) return RRAM_OK;
  RRAM_REQUIRE(x && w, "conv2d_bwd: x/w NULL");
  // Stride 1: dX = dY (*) rot180(W^T), a forward convolution with padding
  // dil*(k-1) - pad (>= 0 needed), so no column matrix is written and
  // gathered back (conv_layer.cu:47-52's data GEMM + col2im); the flipped
  // kernel lives in the workspace head after the weight-gradient passes
  const int G = d.group, cin_g = d.channels / G, cout_g = d.num_output / G;
  const int T = d.kernel_h * d.kernel_w;
  const int eph = d.dilation_h * (d.kernel_h - 1) - d.pad_h, epw = d.dilation_w * (d.kernel_w - 1) - d.pad_w;
  const size_t wt_bytes = (size_t)d.channels * cout_g * T * sizeof(float);
  // (round 4 kept the data GEMM + col2im for grids below 128 tiles of 32
  // channels x 128 positions, 1.4-1.6x faster then, profiles/r04_ab_dx_fwd.txt;
  // since the thin convolution forwards split K, the flipped-kernel forward
  // wins there too: CIFAR-10 full training 0.419-0.421 -> 0.408-0.411 ms per
  // iteration, profiles/r05_ab_occ2_plans.txt)
  // (w_flipped: the caller's copy, rram_update_seg.w_flip, no flip pass)
  const bool dx_fwd = dx && flip_geometry_ok(d) && (w_flipped != nullptr || (ws != nullptr && ws_bytes >= wt_bytes));
  auto dx_as_fwd = [&]() -> int {
    const float* wt = w_flipped;
    int r = 0;
    if (wt == nullptr) {
      float* wf = static_cast<float*>(ws);
      const int64_t n = (int64_t)d.channels * cout_g * T;
      if (!plan_note("aux:flip_kernel"))
        hipLaunchKernelGGL(k_flip_kernel, dim3(stream_blocks(n)), dim3(256), 0, s, w, wf, G, cin_g, cout_g, T);
      r = launch_status("conv bwd kernel flip");
      if (r) return r;
      wt = wf;
    }
    rram_conv_desc t{d.num, d.num_output, d.out_h, d.out_w, d.channels, d.kernel_h, d.kernel_w,
                     eph, epw, 1, 1, d.dilation_h, d.dilation_w, G, 0, 0};
    r = rram_conv_out_shape(&t);
    if (r) return r;
    RRAM_REQUIRE(t.out_h == d.height && t.out_w == d.width, "conv2d_bwd: flipped-kernel output %dx%d != input %dx%d",
                 t.out_h, t.out_w, d.height, d.width);
    return conv_fwd_core(&t, dy, wt, nullptr, dx, 0, s);
  };
  if (im2t) {
    rc = conv_bwd_weight_im2t(&d, x, dy, dw, fold_db ? db : nullptr, ws, ws_bytes, s);
    if (rc) return rc;
    dw = nullptr;  // done
  }
  if (!dw && !dx) return RRAM_OK;
  if (dx_fwd && !dw) return dx_as_fwd();
  const size_t per_img = col_bytes(d, 1);
  RRAM_REQUIRE(ws != nullptr && ws_bytes >= per_img, "conv2d_bwd: workspace needs >= %zu bytes", per_img);
  const BwdColPlan plan = bwd_col_plan(d, ws_bytes, dw != nullptr);
  float* col = static_cast<float*>(ws);
  void* part = plan.part_bytes ? static_cast<char*>(ws) + plan.col_bytes_rounded : nullptr;
  const int64_t chw = (int64_t)d.channels * d.height * d.width;
  const int64_t ohw = (int64_t)d.num_output * HoWo;
  for (int n0 = 0; n0 < d.num; n0 += plan.chunk) {
    const int nimg = std::min(d.num - n0, plan.chunk);
    const int64_t ldcol = (int64_t)nimg * HoWo;
    if (dw) {
      rc = im2col_core(x + n0 * chw, chw, nimg, &d, col, ldcol, s, fold_db ? 1 : 0);
      if (rc) return rc;
      rc = conv_bwd_weight_core(&d, nimg, dy + n0 * ohw, col, ldcol, dw, part, plan.part_bytes, s,
                                fold_db ? db : nullptr);
      if (rc) return rc;
    }
    if (dx && !dx_fwd) {
      rc = conv_bwd_data_col_core(&d, nimg, w, dy + n0 * ohw, col, ldcol, s);
      if (rc) return rc;
      rc = col2im_core(col, ldcol, nimg, &d, dx + n0 * chw, chw, 0, s);
      if (rc) return rc;
    }
  }
  return dx_fwd ? dx_as_fwd() : RRAM_OK;
}

int rram_im2col(const float* im, int C, int H, int W, int kh, int kw, int ph, int pw, int sh,
                int sw, int dh, int dwl, float* col, rram_stream_t s) {
  rram_conv_desc d{1, C, H, W, 1, kh, kw, ph, pw, sh, sw, dh, dwl, 1, 0, 0};
  int rc = rram_conv_out_shape(&d);
  if (rc) return rc;
  RRAM_REQUIRE(im && col, "im2col: NULL");
  return im2col_core(im, 0, 1, &d, col, (int64_t)d.out_h * d.out_w, as_stream(s));
}

int rram_col2im(const float* col, int C, int H, int W, int kh, int kw, int ph, int pw, int sh,
                int sw, int dh, int dwl, float* im, rram_stream_t s) {
  rram_conv_desc d{1, C, H, W, 1, kh, kw, ph, pw, sh, sw, dh, dwl, 1, 0, 0};
  int rc = rram_conv_out_shape(&d);
  if (rc) return rc;
  RRAM_REQUIRE(im && col, "col2im: NULL");
  return col2im_core(col, (int64_t)d.out_h * d.out_w, 1, &d, im, 0, 0, as_stream(s));
}

int rram_ip_fwd(const float* x, const float* w, const float* bias, float* y, int M, int N, int K,
                int transpose, int relu, void* ws, size_t ws_bytes, rram_stream_t s) {
  // top = bottom * W^T (W [N][K]) or bottom * W (W [K][N], transpose)
  if (M == 1 && !transpose) {
    // one row: the reference's GPU path is caffe_gpu_gemv(NoTrans, N, K, W, x)
    // then caffe_gpu_axpy(N, 1, bias, top) (inner_product_layer.cu:15-20).
    // (With transpose it still calls gemv(NoTrans) on the [K][N] weights,
    // i.e. reads them as [N][K]; its CPU path, inner_product_layer.cpp:83-96,
    // does the transposed product, which this build follows: Appendix Q15.)
    int rc = gemv_core(0, N, K, 1.0f, w, x, 0.0f, y, as_stream(s));
    if (rc) return rc;
    if (planning()) {  // the two elementwise passes launch outside the engine's files
      if (bias && N > 0) plan_note("aux:bias_add");
      if (relu && N > 0) plan_note("aux:relu");
      return RRAM_OK;
    }
    if (bias) {
      rc = rram_bias_add(y, bias, 1, N, 1, s);
      if (rc) return rc;
    }
    return relu ? rram_relu_fwd(y, y, N, 0.0f, s) : RRAM_OK;
  }
  if (transpose)
    return gemm_core(0, 0, M, N, K, 1.0f, x, K, w, N, 0.0f, y, N, bias, RRAM_BIAS_COL, relu, ws,
                     ws_bytes, as_stream(s));
  return gemm_core(0, 1, M, N, K, 1.0f, x, K, w, K, 0.0f, y, N, bias, RRAM_BIAS_COL, relu, ws,
                   ws_bytes, as_stream(s));
}

int rram_set_conv_plan_num(int num) {
  RRAM_REQUIRE(num >= 0, "set_conv_plan_num: negative batch");
  return conv_plan_num().exchange(num);
}

int rram_ip_fwd_groups_fused(int G, int M, int N, int K, int transpose, size_t ws_bytes) {
  RRAM_REQUIRE(G >= 0 && M >= 0 && N >= 0 && K >= 0, "ip_fwd_groups: negative size");
  if (M == 1 && !transpose) return 1;  // the GEMV plan: one launch over G
  if (!transpose && rram_f32_engine_for_ip(M, N, K, ws_bytes) == RRAM_ENGINE_BF16X6) return 0;
  return gemm_groups_fused(G, M, N, K, ws_bytes > 0, ws_bytes);
}

int rram_ip_fwd_groups(const float* x, const float* w, int64_t w_group_stride, const float* bias,
                       int64_t bias_group_stride, float* y, int G, int M, int N, int K, int transpose, int relu,
                       void* ws, size_t ws_bytes, rram_stream_t s) {
  RRAM_REQUIRE(G >= 0 && M >= 0 && N >= 0 && K >= 0, "ip_fwd_groups: negative size");
  RRAM_REQUIRE(w_group_stride >= 0 && bias_group_stride >= 0, "ip_fwd_groups: negative group stride");
  if (G == 0 || M == 0 || N == 0) return RRAM_OK;
  RRAM_REQUIRE(x && w && y, "ip_fwd_groups: NULL");
  const size_t wsb = ws != nullptr ? ws_bytes : 0;
  if (M == 1 && !transpose)
    return gemv_groups_core(G, N, K, w, w_group_stride, x, bias, bias_group_stride, relu, y, as_stream(s));
  // the bf16x6 engine's shapes loop (its packed operands and partials are per call)
  if (transpose || rram_f32_engine_for_ip(M, N, K, wsb) != RRAM_ENGINE_BF16X6) {
    const int rc = gemm_groups_core(G, transpose ? 0 : 1, M, N, K, x, (int64_t)M * K, w, transpose ? N : K,
                                    w_group_stride, y, (int64_t)M * N, bias, bias_group_stride, relu, ws, wsb,
                                    as_stream(s));
    if (rc != 0) return rc < 0 ? rc : RRAM_OK;
  }
  for (int g = 0; g < G; ++g) {
    const int rc = rram_ip_fwd(x + (int64_t)g * M * K, w + g * w_group_stride,
                               bias ? bias + g * bias_group_stride : nullptr, y + (int64_t)g * M * N, M, N, K,
                               transpose, relu, ws, ws_bytes, s);
    if (rc) return rc;
  }
  return RRAM_OK;
}

int rram_ip_bwd(const float* x, const float* w, const float* dy, float* dw, float* db, float* dx,
                int M, int N, int K, int transpose, rram_stream_t st) {
  hipStream_t s = as_stream(st);
  int rc;
  if (dw) {
    if (transpose)  // dW[K][N] += X^T dY
      rc = gemm_core(1, 0, K, N, M, 1.0f, x, K, dy, N, 1.0f, dw, N, nullptr, 0, 0, nullptr, 0, s);
    else  // dW[N][K] += dY^T X
      rc = gemm_core(1, 0, N, K, M, 1.0f, dy, N, x, K, 1.0f, dw, K, nullptr, 0, 0, nullptr, 0, s);
    if (rc) return rc;
  }
  if (db) {
    // db[n] += sum_m dY[m][n]  (the reference's gemv against bias_multiplier_)
    if (M > 0 && N > 0) {
      if (!plan_note("aux:bias_bwd")) hipLaunchKernelGGL(k_bias_bwd, dim3(N), dim3(256), 0, s, dy, db, M, N, 1);
      rc = launch_status("ip bias bwd");
      if (rc) return rc;
    }
  }
  if (dx) {
    if (transpose)  // dX[M][K] = dY W^T
      rc = gemm_core(0, 1, M, K, N, 1.0f, dy, N, w, N, 0.0f, dx, K, nullptr, 0, 0, nullptr, 0, s);
    else  // dX = dY W
      rc = gemm_core(0, 0, M, K, N, 1.0f, dy, N, w, K, 0.0f, dx, K, nullptr, 0, 0, nullptr, 0, s);
    if (rc) return rc;
  }
  return RRAM_OK;
}

int rram_bias_add(float* y, const float* b, int num, int C, int inner, rram_stream_t s) {
  RRAM_REQUIRE(num >= 0 && C >= 0 && inner >= 0, "bias_add: negative size");
  const int64_t total = (int64_t)num * C * inner;
  if (total == 0) return RRAM_OK;
  RRAM_REQUIRE(y && b, "bias_add: NULL");
  hipLaunchKernelGGL(k_bias_add, dim3(stream_blocks(total)), dim3(256), 0, as_stream(s), y, b, num,
                     C, inner);
  return launch_status("bias_add");
}

int rram_bias_bwd(const float* dy, float* db, int num, int C, int inner, rram_stream_t s) {
  RRAM_REQUIRE(num >= 0 && C >= 0 && inner >= 0, "bias_bwd: negative size");
  if (C == 0) return RRAM_OK;
  RRAM_REQUIRE(dy && db, "bias_bwd: NULL");
  hipLaunchKernelGGL(k_bias_bwd, dim3(C), dim3(256), 0, as_stream(s), dy, db, num, C, inner);
  return launch_status("bias_bwd");
}

// ---- which kernels the fp32 engine's entry points launch (host only) ----
// Each query opens a PlanScope and calls the entry point itself with operand
// pointers that carry only the stated alignment, so the ids come from the
// launch paths' own planning code.
namespace {
// a 256-byte aligned address (the allocators' alignment), or 4 bytes past one
float* plan_ptr(int align16) { return reinterpret_cast<float*>(uintptr_t{1} << 20 | (align16 ? 0u : 4u)); }
int plan_result(int rc, const PlanScope& sc, char* out, size_t cap) { return rc ? rc : copy_text(sc.text, out, cap); }
}  // namespace

int rram_gemm_kernel_ids(int trans_a, int trans_b, int M, int N, int K, int lda, int ldb, int a_align16,
                         int b_align16, int beta_zero, size_t ws_bytes, char* out, size_t cap) {
  PlanScope sc;
  const int ldc = N > 0 ? N : 1;
  const int rc = rram_gemm_f32_ex(trans_a, trans_b, M, N, K, 1.0f, plan_ptr(a_align16), lda, plan_ptr(b_align16), ldb,
                                  beta_zero ? 0.0f : 1.0f, plan_ptr(1), ldc, nullptr, RRAM_BIAS_NONE, 0,
                                  ws_bytes ? plan_ptr(1) : nullptr, ws_bytes, nullptr);
  return plan_result(rc, sc, out, cap);
}

int rram_ip_fwd_kernel_ids(int M, int N, int K, int transpose, int x_align16, int w_align16, int bias, int relu,
                           size_t ws_bytes, char* out, size_t cap) {
  PlanScope sc;
  const int rc = rram_ip_fwd(plan_ptr(x_align16), plan_ptr(w_align16), bias ? plan_ptr(1) : nullptr, plan_ptr(1), M, N,
                             K, transpose, relu, ws_bytes ? plan_ptr(1) : nullptr, ws_bytes, nullptr);
  return plan_result(rc, sc, out, cap);
}

int rram_ip_bwd_kernel_ids(int M, int N, int K, int transpose, int want_dw, int want_db, int want_dx, int align16,
                           char* out, size_t cap) {
  PlanScope sc;
  float* p = plan_ptr(align16);
  const int rc = rram_ip_bwd(p, p, p, want_dw ? p : nullptr, want_db ? p : nullptr, want_dx ? p : nullptr, M, N, K,
                             transpose, nullptr);
  return plan_result(rc, sc, out, cap);
}

int rram_ip_fwd_groups_kernel_ids(int G, int M, int N, int K, int transpose, int64_t w_group_stride, int align16,
                                  size_t ws_bytes, char* out, size_t cap) {
  PlanScope sc;
  float* p = plan_ptr(align16);
  const int rc = rram_ip_fwd_groups(p, p, w_group_stride, nullptr, 0, p, G, M, N, K, transpose, 0,
                                    ws_bytes ? plan_ptr(1) : nullptr, ws_bytes, nullptr);
  return plan_result(rc, sc, out, cap);
}

int rram_conv_fwd_kernel_ids(const rram_conv_desc* d, int x_align16, int w_align16, char* out, size_t cap) {
  RRAM_REQUIRE(d != nullptr, "kernel id query: desc is NULL");
  PlanScope sc;
  const int rc = rram_conv2d_fwd(d, plan_ptr(x_align16), plan_ptr(w_align16), nullptr, plan_ptr(1), 0, nullptr);
  return plan_result(rc, sc, out, cap);
}

int rram_conv_bwd_kernel_ids(const rram_conv_desc* d, int want_dw, int want_db, int want_dx, size_t ws_bytes,
                             int have_w_flipped, int w_align16, char* out, size_t cap) {
  RRAM_REQUIRE(d != nullptr, "kernel id query: desc is NULL");
  PlanScope sc;
  float* p = plan_ptr(1);
  const int rc = rram_conv2d_bwd_ex(d, p, plan_ptr(w_align16), have_w_flipped ? p : nullptr, p, want_dw ? p : nullptr,
                                    want_db ? p : nullptr, want_dx ? p : nullptr, ws_bytes ? p : nullptr, ws_bytes,
                                    nullptr);
  return plan_result(rc, sc, out, cap);
}

int rram_f32_kernel_list(char* out, size_t cap) { return copy_text(rram::f32_kernel_list(), out, cap); }

}  // extern "C"
