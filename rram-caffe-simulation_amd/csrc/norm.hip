// BatchNorm, Scale and Sigmoid for gfx950 (batch_norm_layer.cpp, scale_layer.cpp,
// sigmoid_layer.cu).  The reference runs BatchNorm as ~20 gemv / gemm /
// elementwise launches per direction, a Scale layer and an in-place ReLU after
// it; here each direction is one per-channel reduction (split over slices so a
// channel is not confined to one workgroup), a finalize over the slices in a
// fixed order, and one streaming pass that also carries the Scale layer's
// gamma / beta and the ReLU.  No floating-point atomics: every result is
// bit-identical from run to run.
//
// Layout: fp32 NC(inner), channels = shape(1), inner = count / (num channels);
// inner == 1 is the fully-connected case, whose channel elements are `channels`
// floats apart (the *_cols reductions put neighbouring lanes on neighbouring
// channels).
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "rram_common.hpp"

namespace rram {
namespace {

struct FastDiv {
  uint32_t d, m, s;
};
FastDiv make_fastdiv(uint32_t d) {
  FastDiv f{d, 0, 0};
  if (d <= 1) return f;
  uint32_t sh = 0;
  while ((1ull << sh) < d) ++sh;
  f.s = sh;
  f.m = static_cast<uint32_t>(((1ull << 32) * ((1ull << sh) - d)) / d + 1);
  return f;
}
// x / f.d for x < 2^31
__device__ __forceinline__ uint32_t fdiv(uint32_t x, const FastDiv& f) {
  return f.d <= 1 ? x : (__umulhi(x, f.m) + x) >> f.s;
}

constexpr int kMaxSlices = 64;   // slices of one channel (the finalize sums them in order)
constexpr int kColsLanes = 64;   // channels per block of the *_cols reductions (one wave wide)
constexpr int kColsRows = kThreads / kColsLanes;

// ---- running moments (count, mean, M2 = sum (x - mean)^2), merged by Chan et al.'s formula ----
struct Moments {
  float n, mean, m2;
};
__device__ __forceinline__ Moments merge(const Moments& a, const Moments& b) {
  if (b.n == 0.0f) return a;
  if (a.n == 0.0f) return b;
  const float n = a.n + b.n;
  const float d = b.mean - a.mean;
  const float fb = b.n / n;
  return Moments{n, fmaf(d, fb, a.mean), a.m2 + b.m2 + d * d * a.n * fb};
}
// One thread's elements: sums shifted by the thread's first element, so the
// subtraction s2 - s1^2/n cancels only against the thread's own spread (the
// one-pass E[x^2] - E[x]^2 cancels against the mean).
struct Shifted {
  float k = 0.0f, s1 = 0.0f, s2 = 0.0f, n = 0.0f;
  __device__ __forceinline__ void add(float x) {
    if (n == 0.0f) k = x;
    const float d = x - k;
    s1 += d;
    s2 = fmaf(d, d, s2);
    n += 1.0f;
  }
  __device__ __forceinline__ Moments done() const {
    if (n == 0.0f) return Moments{0.0f, 0.0f, 0.0f};
    const float dm = s1 / n;
    return Moments{n, k + dm, fmaxf(fmaf(-s1, dm, s2), 0.0f)};
  }
};
__device__ __forceinline__ Moments wave_merge(Moments v) {
  for (int off = 32; off > 0; off >>= 1) {
    Moments o{__shfl_down(v.n, off, 64), __shfl_down(v.mean, off, 64), __shfl_down(v.m2, off, 64)};
    v = merge(v, o);   // lane 0 ends with lanes 0..63 merged in a fixed tree
  }
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// V floats at p (16-byte aligned when V == 4)
template <int V>
struct Vec;
template <>
struct Vec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = p[0]; }
  __device__ __forceinline__ void store(float* p) const { p[0] = v[0]; }
};
template <>
struct Vec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  }
  __device__ __forceinline__ void store(float* p) const {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};

// the part [lo, hi) of `total` work items that slice s of S takes
__device__ __forceinline__ void slice_range(int total, int s, int S, int& lo, int& hi) {
  const int per = (total + S - 1) / S;
  lo = min(total, s * per);
  hi = min(total, lo + per);
}

// ---- training statistics, pass over x (batch_norm_layer.cpp:107-135) ----
// grid (C, S): block (c, s) reduces slice s of channel c's m = num * inner
// elements (V at a time; V == 4 needs inner % 4 == 0 and x 16-byte aligned) to
// part[(s * C + c) * 3 .. +2] = {count, mean, M2}.
template <int V>
__global__ void __launch_bounds__(kThreads) k_bn_stats_plane(const float* __restrict__ x, int C, int inner,
                                                             FastDiv dinner, int m, float* __restrict__ part) {
  const int c = blockIdx.x, s = blockIdx.y, S = gridDim.y;
  int lo, hi;
  slice_range(m / V, s, S, lo, hi);
  Shifted acc;
  for (int j = lo + threadIdx.x; j < hi; j += kThreads) {
    const uint32_t e = static_cast<uint32_t>(j) * V;
    const uint32_t n = fdiv(e, dinner);
    Vec<V> t;
    t.load(x + (static_cast<int64_t>(n) * C + c) * inner + (e - n * inner));
#pragma unroll
    for (int k = 0; k < V; ++k) acc.add(t.v[k]);
  }
  __shared__ Moments sh[kThreads / 64];
  const Moments w = wave_merge(acc.done());
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    Moments t = sh[0];
    for (int i = 1; i < kThreads / 64; ++i) t = merge(t, sh[i]);
    float* o = part + (static_cast<int64_t>(s) * C + c) * 3;
    o[0] = t.n, o[1] = t.mean, o[2] = t.m2;
  }
}
// inner == 1: grid (ceil(C / 64), S); lane l of a block takes channel
// blockIdx.x * 64 + l, its 4 waves take rows s * 4 + w, + 4 S, ... of x[num][C]
__global__ void __launch_bounds__(kThreads) k_bn_stats_cols(const float* __restrict__ x, int num, int C,
                                                            float* __restrict__ part) {
  const int lane = threadIdx.x & (kColsLanes - 1), row = threadIdx.x / kColsLanes;
  const int c = blockIdx.x * kColsLanes + lane, s = blockIdx.y, S = gridDim.y;
  Shifted acc;
  if (c < C)
    for (int n = s * kColsRows + row; n < num; n += S * kColsRows) acc.add(x[static_cast<int64_t>(n) * C + c]);
  __shared__ Moments sh[kColsRows][kColsLanes];
  sh[row][lane] = acc.done();
  __syncthreads();
  if (row == 0 && c < C) {
    Moments t = sh[0][lane];
    for (int i = 1; i < kColsRows; ++i) t = merge(t, sh[i][lane]);
    float* o = part + (static_cast<int64_t>(s) * C + c) * 3;
    o[0] = t.n, o[1] = t.mean, o[2] = t.m2;
  }
}
// The slices of one channel in slice order, then batch_norm_layer.cpp:138-146
// on the device: factor = factor maf + 1, run_mean = mean + maf run_mean,
// run_var = (m > 1 ? m / (m - 1) : 1) var + maf run_var (run_* nullable).
__global__ void k_bn_stats_finalize(const float* __restrict__ part, int S, int C, int m, float eps, float maf,
                                    float* __restrict__ mean, float* __restrict__ rstd, float* run_mean,
                                    float* run_var, float* factor) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && factor != nullptr) factor[0] = fmaf(factor[0], maf, 1.0f);
  if (c >= C) return;
  Moments t{0.0f, 0.0f, 0.0f};
  for (int s = 0; s < S; ++s) {
    const float* p = part + (static_cast<int64_t>(s) * C + c) * 3;
    t = merge(t, Moments{p[0], p[1], p[2]});
  }
  const float var = t.m2 / static_cast<float>(m);
  mean[c] = t.mean;
  rstd[c] = 1.0f / sqrtf(var + eps);
  if (run_mean != nullptr) run_mean[c] = fmaf(maf, run_mean[c], t.mean);
  if (run_var != nullptr) {
    const float corr = m > 1 ? static_cast<float>(m) / static_cast<float>(m - 1) : 1.0f;
    run_var[c] = fmaf(maf, run_var[c], corr * var);
  }
}
// batch_norm_layer.cpp:98-105: s = factor == 0 ? 0 : 1 / factor
__global__ void k_bn_global_stats(const float* __restrict__ run_mean, const float* __restrict__ run_var,
                                  const float* __restrict__ factor, int C, float eps, float* __restrict__ mean,
                                  float* __restrict__ rstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float f = factor[0];
  const float s = f == 0.0f ? 0.0f : 1.0f / f;
  mean[c] = s * run_mean[c];
  rstd[c] = 1.0f / sqrtf(s * run_var[c] + eps);
}

// ---- the streaming passes ----
// The tensor as one flat run of n floats, V at a time.  V == 4: every operand
// starts `head` floats past a 16-byte boundary (the host checks that they all
// share it), vector j covers the elements [4 j - head, 4 j - head + 4), and the
// first and last vectors fall back to their live elements one by one.  The
// channel of element e is (e / inner) % C; `uniform` (head == 0 and inner % 4
// == 0): one channel per vector.
struct Flat {
  int n, head, C;
  FastDiv dinner, dC;
  int uniform;
};
__device__ __forceinline__ int channel_of(uint32_t e, const Flat& f) {
  const uint32_t q = fdiv(e, f.dinner);
  return static_cast<int>(q - fdiv(q, f.dC) * f.C);
}

// x^ = (x - mean[c]) rstd[c] (mean NULL: x^ = x, the stand-alone Scale);
// y = gamma ? (beta ? fmaf(x^, gamma[c], beta[c]) : x^ gamma[c]) : x^; relu: y = max(y, 0);
// xhat_out (nullable) = x^.  y may be x.  (batch_norm_layer.cpp:148-166 +
// scale_layer.cpp Forward + relu_layer.cu:9-15)
struct ApplyArgs {
  const float *mean, *rstd, *gamma, *beta;
  int relu;
};
__device__ __forceinline__ float apply_one(float x, int c, const ApplyArgs& a, float& xh) {
  xh = a.mean != nullptr ? (x - a.mean[c]) * a.rstd[c] : x;
  float y = xh;
  if (a.gamma != nullptr) y = a.beta != nullptr ? fmaf(xh, a.gamma[c], a.beta[c]) : xh * a.gamma[c];
  if (a.relu) y = y > 0.0f ? y : y * 0.0f;   // k_relu_fwd's expression at slope 0, bit for bit
  return y;
}
template <int V>
__global__ void __launch_bounds__(kThreads) k_norm_apply(const float* x, float* y, float* xhat_out, Flat f,
                                                         ApplyArgs a) {
  const int nvec = (f.n + f.head + V - 1) / V;
  for (int j = blockIdx.x * kThreads + threadIdx.x; j < nvec; j += gridDim.x * kThreads) {
    const int e0 = j * V - f.head;
    if (V > 1 && (e0 < 0 || e0 + V > f.n)) {
      for (int k = 0; k < V; ++k) {
        const int e = e0 + k;
        if (e < 0 || e >= f.n) continue;
        float xh;
        const float r = apply_one(x[e], channel_of(e, f), a, xh);
        if (xhat_out != nullptr) xhat_out[e] = xh;
        y[e] = r;
      }
      continue;
    }
    Vec<V> t, h;
    t.load(x + e0);
    const int c0 = channel_of(e0, f);
#pragma unroll
    for (int k = 0; k < V; ++k)
      t.v[k] = apply_one(t.v[k], (k == 0 || f.uniform) ? c0 : channel_of(e0 + k, f), a, h.v[k]);
    if (xhat_out != nullptr) h.store(xhat_out + e0);
    t.store(y + e0);
  }
}

// g = relu_y ? dy [relu_y > 0] : dy
// coef (3 per channel: a, b, d; the backward reduction's finalize wrote them):
//   dx = a (g - b - xhat d)          (batch_norm_layer.cpp:187-241, a = gamma rstd, b = sum g / m, d = sum g x^ / m)
// else dx = g (gamma ? gamma[c] : 1) (rstd ? rstd[c] : 1)     (:180-183, scale_layer.cpp Backward)
// dx may be dy.
struct BwdArgs {
  const float *coef, *gamma, *rstd;
};
__device__ __forceinline__ float bwd_one(float dy, float yr, float xh, int c, const BwdArgs& a, bool masked) {
  const float g = (masked && !(yr > 0.0f)) ? 0.0f : dy;
  if (a.coef != nullptr) {
    const float* k = a.coef + 3 * c;
    return k[0] * (g - k[1] - xh * k[2]);
  }
  float r = g;
  if (a.gamma != nullptr) r *= a.gamma[c];
  if (a.rstd != nullptr) r *= a.rstd[c];
  return r;
}
template <int V>
__global__ void __launch_bounds__(kThreads) k_norm_bwd(const float* dy, const float* __restrict__ relu_y,
                                                       const float* __restrict__ xhat, float* dx, Flat f,
                                                       BwdArgs a) {
  const int nvec = (f.n + f.head + V - 1) / V;
  const bool masked = relu_y != nullptr, centred = a.coef != nullptr;
  for (int j = blockIdx.x * kThreads + threadIdx.x; j < nvec; j += gridDim.x * kThreads) {
    const int e0 = j * V - f.head;
    if (V > 1 && (e0 < 0 || e0 + V > f.n)) {
      for (int k = 0; k < V; ++k) {
        const int e = e0 + k;
        if (e < 0 || e >= f.n) continue;
        dx[e] = bwd_one(dy[e], masked ? relu_y[e] : 1.0f, centred ? xhat[e] : 0.0f, channel_of(e, f), a, masked);
      }
      continue;
    }
    Vec<V> g, yr, xh;
    g.load(dy + e0);
    if (masked) yr.load(relu_y + e0);
    if (centred) xh.load(xhat + e0);
    const int c0 = channel_of(e0, f);
#pragma unroll
    for (int k = 0; k < V; ++k)
      g.v[k] = bwd_one(g.v[k], masked ? yr.v[k] : 1.0f, centred ? xh.v[k] : 0.0f,
                       (k == 0 || f.uniform) ? c0 : channel_of(e0 + k, f), a, masked);
    g.store(dx + e0);
  }
}

// ---- backward reduction: part[(s * C + c) * 2 .. +1] = {sum g, sum g x^} over slice s of channel c ----
template <int V>
__global__ void __launch_bounds__(kThreads) k_norm_bwd_reduce_plane(const float* __restrict__ dy,
                                                                    const float* __restrict__ relu_y,
                                                                    const float* __restrict__ xhat, int C,
                                                                    int inner, FastDiv dinner, int m,
                                                                    float* __restrict__ part) {
  const int c = blockIdx.x, s = blockIdx.y, S = gridDim.y;
  int lo, hi;
  slice_range(m / V, s, S, lo, hi);
  float sg = 0.0f, sgx = 0.0f;
  for (int j = lo + threadIdx.x; j < hi; j += kThreads) {
    const uint32_t e = static_cast<uint32_t>(j) * V;
    const uint32_t n = fdiv(e, dinner);
    const int64_t at = (static_cast<int64_t>(n) * C + c) * inner + (e - n * inner);
    Vec<V> g, yr, xh;
    g.load(dy + at);
    xh.load(xhat + at);
    if (relu_y != nullptr) yr.load(relu_y + at);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float gv = (relu_y != nullptr && !(yr.v[k] > 0.0f)) ? 0.0f : g.v[k];
      sg += gv;
      sgx = fmaf(gv, xh.v[k], sgx);
    }
  }
  __shared__ float sh[2][kThreads / 64];
  sg = wave_sum(sg);
  sgx = wave_sum(sgx);
  if ((threadIdx.x & 63) == 0) sh[0][threadIdx.x >> 6] = sg, sh[1][threadIdx.x >> 6] = sgx;
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = sh[0][0], b = sh[1][0];
    for (int i = 1; i < kThreads / 64; ++i) a += sh[0][i], b += sh[1][i];
    float* o = part + (static_cast<int64_t>(s) * C + c) * 2;
    o[0] = a, o[1] = b;
  }
}
__global__ void __launch_bounds__(kThreads) k_norm_bwd_reduce_cols(const float* __restrict__ dy,
                                                                   const float* __restrict__ relu_y,
                                                                   const float* __restrict__ xhat, int num, int C,
                                                                   float* __restrict__ part) {
  const int lane = threadIdx.x & (kColsLanes - 1), row = threadIdx.x / kColsLanes;
  const int c = blockIdx.x * kColsLanes + lane, s = blockIdx.y, S = gridDim.y;
  float sg = 0.0f, sgx = 0.0f;
  if (c < C)
    for (int n = s * kColsRows + row; n < num; n += S * kColsRows) {
      const int64_t at = static_cast<int64_t>(n) * C + c;
      const float gv = (relu_y != nullptr && !(relu_y[at] > 0.0f)) ? 0.0f : dy[at];
      sg += gv;
      sgx = fmaf(gv, xhat[at], sgx);
    }
  __shared__ float sh[2][kColsRows][kColsLanes];
  sh[0][row][lane] = sg;
  sh[1][row][lane] = sgx;
  __syncthreads();
  if (row == 0 && c < C) {
    float a = sh[0][0][lane], b = sh[1][0][lane];
    for (int i = 1; i < kColsRows; ++i) a += sh[0][i][lane], b += sh[1][i][lane];
    float* o = part + (static_cast<int64_t>(s) * C + c) * 2;
    o[0] = a, o[1] = b;
  }
}
// dbeta[c] += sum g, dgamma[c] += sum g x^ (each nullable: the Scale layer's
// parameter gradients, accumulated like InnerProduct's dW); coef (nullable) =
// {gamma rstd, sum g / m, sum g x^ / m} for k_norm_bwd
__global__ void k_norm_bwd_finalize(const float* __restrict__ part, int S, int C, int m,
                                    const float* __restrict__ gamma, const float* __restrict__ rstd,
                                    float* dgamma, float* dbeta, float* __restrict__ coef) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float sg = 0.0f, sgx = 0.0f;
  for (int s = 0; s < S; ++s) {
    const float* p = part + (static_cast<int64_t>(s) * C + c) * 2;
    sg += p[0];
    sgx += p[1];
  }
  if (dbeta != nullptr) dbeta[c] += sg;
  if (dgamma != nullptr) dgamma[c] += sgx;
  if (coef != nullptr) {
    const float fm = static_cast<float>(m);
    coef[3 * c] = (gamma != nullptr ? gamma[c] : 1.0f) * (rstd != nullptr ? rstd[c] : 1.0f);
    coef[3 * c + 1] = sg / fm;
    coef[3 * c + 2] = sgx / fm;
  }
}

// sigmoid_layer.cu: y = 1 / (1 + exp(-x)); dx = dy y (1 - y)
__global__ void k_sigmoid_fwd(const float* x, float* y, int n) {
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) y[i] = 1.0f / (1.0f + expf(-x[i]));
}
__global__ void k_sigmoid_bwd(const float* __restrict__ y, const float* dy, float* dx, int n) {
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
    const float v = y[i];
    dx[i] = dy[i] * v * (1.0f - v);
  }
}

// ---- host-side geometry ----
struct Geom {
  int num, C, inner, m, n;
};
int geom_of(int num, int C, int64_t inner, Geom* g, const char* what) {
  RRAM_REQUIRE(num > 0 && C > 0 && inner > 0, "%s: num, channels and inner must be > 0", what);
  // (8 below 2^31: the streaming kernels round n + head up to whole vectors in int)
  RRAM_REQUIRE(static_cast<int64_t>(num) * C < (2147483647ll - 8) / inner,
               "%s: more than 2^31 - 8 elements is not supported", what);
  // the per-channel counts are carried as floats: exact up to 2^24
  RRAM_REQUIRE(static_cast<int64_t>(num) * inner <= (1ll << 24), "%s: more than 2^24 elements per channel is not supported",
               what);
  *g = Geom{num, C, static_cast<int>(inner), static_cast<int>(num * inner), static_cast<int>(num * C * inner)};
  return RRAM_OK;
}
int misalign(const void* p) { return static_cast<int>((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }
// slices per channel: about four vector loads per thread, at most 2048 blocks
// in all (stream_blocks' cap) and kMaxSlices; a function of the shape alone
int plane_slices(const Geom& g, int V) {
  int S = (g.m / V + kThreads * 4 - 1) / (kThreads * 4);
  S = std::min(S, std::max(1, kMaxStreamBlocks / g.C));
  return std::max(1, std::min(S, kMaxSlices));
}
int cols_slices(const Geom& g) {
  const int gy = (g.C + kColsLanes - 1) / kColsLanes;
  int S = (g.num + kColsRows * 4 - 1) / (kColsRows * 4);
  S = std::min(S, std::max(1, kMaxStreamBlocks / gy));
  return std::max(1, std::min(S, kMaxSlices));
}
size_t partial_floats(const Geom& g) {
  const int S = g.inner == 1 ? cols_slices(g) : std::max(plane_slices(g, 1), plane_slices(g, 4));
  return static_cast<size_t>(3) * S * g.C;
}
// the flat streaming geometry: vectors when every operand shares one offset to a 16-byte boundary
template <typename... P>
Flat flat_of(const Geom& g, int* V, const void* first, P... rest) {
  const int a = misalign(first);
  bool same = true;
  for (const void* p : {static_cast<const void*>(rest)...})
    if (p != nullptr && misalign(p) != a) same = false;
  *V = same ? 4 : 1;
  const int head = same ? a : 0;
  return Flat{g.n, head, g.C, make_fastdiv(g.inner), make_fastdiv(g.C), (head == 0 && g.inner % 4 == 0) ? 1 : 0};
}
int finalize_blocks(int C) { return (C + kThreads - 1) / kThreads; }

}  // namespace
}  // namespace rram

using namespace rram;

extern "C" {

size_t rram_norm_workspace_floats(int num, int channels, int64_t inner) {
  Geom g;
  if (geom_of(num, channels, inner, &g, "norm_workspace_floats") != RRAM_OK) return 0;
  return partial_floats(g) + static_cast<size_t>(3) * g.C;
}

int rram_bn_stats_train(const float* x, int num, int channels, int64_t inner, float eps, float maf, float* mean,
                        float* rstd, float* run_mean, float* run_var, float* factor, float* ws, size_t ws_floats,
                        rram_stream_t s) {
  Geom g;
  if (int rc = geom_of(num, channels, inner, &g, "bn_stats_train")) return rc;
  RRAM_REQUIRE(x && mean && rstd && ws, "bn_stats_train: NULL");
  RRAM_REQUIRE(ws_floats >= partial_floats(g), "bn_stats_train: workspace of %zu floats, %zu needed", ws_floats,
               partial_floats(g));
  int S;
  if (g.inner == 1) {
    S = cols_slices(g);
    if (!plan_note("bn_stats_cols"))
      hipLaunchKernelGGL(k_bn_stats_cols, dim3((g.C + kColsLanes - 1) / kColsLanes, S), dim3(kThreads), 0,
                         as_stream(s), x, g.num, g.C, ws);
  } else if (g.inner % 4 == 0 && misalign(x) == 0) {
    S = plane_slices(g, 4);
    if (!plan_note("bn_stats_plane<4>"))
      hipLaunchKernelGGL(k_bn_stats_plane<4>, dim3(g.C, S), dim3(kThreads), 0, as_stream(s), x, g.C, g.inner,
                         make_fastdiv(g.inner), g.m, ws);
  } else {
    S = plane_slices(g, 1);
    if (!plan_note("bn_stats_plane<1>"))
      hipLaunchKernelGGL(k_bn_stats_plane<1>, dim3(g.C, S), dim3(kThreads), 0, as_stream(s), x, g.C, g.inner,
                         make_fastdiv(g.inner), g.m, ws);
  }
  if (!plan_note("bn_stats_finalize"))
    hipLaunchKernelGGL(k_bn_stats_finalize, dim3(finalize_blocks(g.C)), dim3(kThreads), 0, as_stream(s), ws, S, g.C,
                       g.m, eps, maf, mean, rstd, run_mean, run_var, factor);
  return launch_status("bn_stats_train");
}

int rram_bn_stats_global(const float* run_mean, const float* run_var, const float* factor, int channels, float eps,
                         float* mean, float* rstd, rram_stream_t s) {
  RRAM_REQUIRE(channels > 0, "bn_stats_global: channels must be > 0");
  RRAM_REQUIRE(run_mean && run_var && factor && mean && rstd, "bn_stats_global: NULL");
  if (!plan_note("bn_global_stats"))
    hipLaunchKernelGGL(k_bn_global_stats, dim3(finalize_blocks(channels)), dim3(kThreads), 0, as_stream(s), run_mean,
                       run_var, factor, channels, eps, mean, rstd);
  return launch_status("bn_stats_global");
}

int rram_norm_apply(const float* x, float* y, float* xhat_out, const float* mean, const float* rstd,
                    const float* gamma, const float* beta, int relu, int num, int channels, int64_t inner,
                    rram_stream_t s) {
  Geom g;
  if (int rc = geom_of(num, channels, inner, &g, "norm_apply")) return rc;
  RRAM_REQUIRE(x && y, "norm_apply: NULL");
  RRAM_REQUIRE((mean == nullptr) == (rstd == nullptr), "norm_apply: mean and rstd go together");
  RRAM_REQUIRE(beta == nullptr || gamma != nullptr, "norm_apply: beta without gamma");
  RRAM_REQUIRE(xhat_out != x && (xhat_out == nullptr || xhat_out != y), "norm_apply: xhat_out aliases x or y");
  int V;
  const Flat f = flat_of(g, &V, x, y, xhat_out);
  const ApplyArgs a{mean, rstd, gamma, beta, relu};
  const int blocks = stream_blocks((static_cast<int64_t>(g.n) + f.head + V - 1) / V);
  if (V == 4) {
    if (!plan_note("norm_apply<4>"))
      hipLaunchKernelGGL(k_norm_apply<4>, dim3(blocks), dim3(kThreads), 0, as_stream(s), x, y, xhat_out, f, a);
  } else if (!plan_note("norm_apply<1>")) {
    hipLaunchKernelGGL(k_norm_apply<1>, dim3(blocks), dim3(kThreads), 0, as_stream(s), x, y, xhat_out, f, a);
  }
  return launch_status("norm_apply");
}

int rram_norm_bwd_reduce(const float* dy, const float* relu_y, const float* xhat, int num, int channels,
                         int64_t inner, const float* gamma, const float* rstd, float* dgamma, float* dbeta,
                         float* coef, float* ws, size_t ws_floats, rram_stream_t s) {
  Geom g;
  if (int rc = geom_of(num, channels, inner, &g, "norm_bwd_reduce")) return rc;
  RRAM_REQUIRE(dy && xhat && ws, "norm_bwd_reduce: NULL");
  RRAM_REQUIRE(ws_floats >= partial_floats(g), "norm_bwd_reduce: workspace of %zu floats, %zu needed", ws_floats,
               partial_floats(g));
  int S;
  const bool al = misalign(dy) == 0 && misalign(xhat) == 0 && (relu_y == nullptr || misalign(relu_y) == 0);
  if (g.inner == 1) {
    S = cols_slices(g);
    if (!plan_note("norm_bwd_reduce_cols"))
      hipLaunchKernelGGL(k_norm_bwd_reduce_cols, dim3((g.C + kColsLanes - 1) / kColsLanes, S), dim3(kThreads), 0,
                         as_stream(s), dy, relu_y, xhat, g.num, g.C, ws);
  } else if (g.inner % 4 == 0 && al) {
    S = plane_slices(g, 4);
    if (!plan_note("norm_bwd_reduce_plane<4>"))
      hipLaunchKernelGGL(k_norm_bwd_reduce_plane<4>, dim3(g.C, S), dim3(kThreads), 0, as_stream(s), dy, relu_y, xhat,
                         g.C, g.inner, make_fastdiv(g.inner), g.m, ws);
  } else {
    S = plane_slices(g, 1);
    if (!plan_note("norm_bwd_reduce_plane<1>"))
      hipLaunchKernelGGL(k_norm_bwd_reduce_plane<1>, dim3(g.C, S), dim3(kThreads), 0, as_stream(s), dy, relu_y, xhat,
                         g.C, g.inner, make_fastdiv(g.inner), g.m, ws);
  }
  if (!plan_note("norm_bwd_finalize"))
    hipLaunchKernelGGL(k_norm_bwd_finalize, dim3(finalize_blocks(g.C)), dim3(kThreads), 0, as_stream(s), ws, S, g.C,
                       g.m, gamma, rstd, dgamma, dbeta, coef);
  return launch_status("norm_bwd_reduce");
}

int rram_norm_bwd_apply(const float* dy, const float* relu_y, const float* xhat, const float* coef,
                        const float* gamma, const float* rstd, float* dx, int num, int channels, int64_t inner,
                        rram_stream_t s) {
  Geom g;
  if (int rc = geom_of(num, channels, inner, &g, "norm_bwd_apply")) return rc;
  RRAM_REQUIRE(dy && dx, "norm_bwd_apply: NULL");
  RRAM_REQUIRE(coef == nullptr || xhat != nullptr, "norm_bwd_apply: coef without xhat");
  RRAM_REQUIRE(dx != relu_y && dx != xhat, "norm_bwd_apply: dx aliases relu_y or xhat");
  int V;
  const Flat f = flat_of(g, &V, dy, dx, relu_y, coef != nullptr ? xhat : nullptr);
  const BwdArgs a{coef, gamma, rstd};
  const int blocks = stream_blocks((static_cast<int64_t>(g.n) + f.head + V - 1) / V);
  if (V == 4) {
    if (!plan_note("norm_bwd<4>"))
      hipLaunchKernelGGL(k_norm_bwd<4>, dim3(blocks), dim3(kThreads), 0, as_stream(s), dy, relu_y, xhat, dx, f, a);
  } else if (!plan_note("norm_bwd<1>")) {
    hipLaunchKernelGGL(k_norm_bwd<1>, dim3(blocks), dim3(kThreads), 0, as_stream(s), dy, relu_y, xhat, dx, f, a);
  }
  return launch_status("norm_bwd_apply");
}

int rram_sigmoid_fwd(const float* x, float* y, int64_t n, rram_stream_t s) {
  RRAM_REQUIRE(n >= 0 && n < 2147483647ll, "sigmoid: n outside [0, 2^31)");
  if (n == 0) return RRAM_OK;
  RRAM_REQUIRE(x && y, "sigmoid: NULL");
  if (!plan_note("sigmoid_fwd"))
    hipLaunchKernelGGL(k_sigmoid_fwd, dim3(stream_blocks(n)), dim3(kThreads), 0, as_stream(s), x, y,
                       static_cast<int>(n));
  return launch_status("sigmoid_fwd");
}
int rram_sigmoid_bwd(const float* y, const float* dy, float* dx, int64_t n, rram_stream_t s) {
  RRAM_REQUIRE(n >= 0 && n < 2147483647ll, "sigmoid: n outside [0, 2^31)");
  if (n == 0) return RRAM_OK;
  RRAM_REQUIRE(y && dy && dx, "sigmoid: NULL");
  RRAM_REQUIRE(dx != y, "sigmoid_bwd: dx aliases y");
  if (!plan_note("sigmoid_bwd"))
    hipLaunchKernelGGL(k_sigmoid_bwd, dim3(stream_blocks(n)), dim3(kThreads), 0, as_stream(s), y, dy, dx,
                       static_cast<int>(n));
  return launch_status("sigmoid_bwd");
}

// ---- which kernels of this file an entry point would launch (host only) ----
namespace {
// an address `off` floats past a 16-byte boundary; never dereferenced
float* norm_ptr(int off) { return reinterpret_cast<float*>((uintptr_t{1} << 20) + 4 * static_cast<uintptr_t>(off & 3)); }
int norm_result(int rc, const PlanScope& sc, char* out, size_t cap) { return rc ? rc : copy_text(sc.text, out, cap); }
}  // namespace

int rram_bn_fwd_kernel_ids(int num, int channels, int64_t inner, int global_stats, int x_off, int y_off, char* out,
                           size_t cap) {
  PlanScope sc;
  float *x = norm_ptr(x_off), *y = norm_ptr(y_off), *p = norm_ptr(0);
  int rc = global_stats ? rram_bn_stats_global(p, p, p, channels, 1e-5f, p, p, nullptr)
                        : rram_bn_stats_train(x, num, channels, inner, 1e-5f, 0.999f, p, p, p, p, p, p, ~size_t{0},
                                              nullptr);
  if (rc == RRAM_OK)
    rc = rram_norm_apply(x, y, global_stats ? nullptr : norm_ptr(y_off) + 4, p, p, nullptr, nullptr, 0, num, channels,
                         inner, nullptr);
  return norm_result(rc, sc, out, cap);
}
int rram_bn_bwd_kernel_ids(int num, int channels, int64_t inner, int global_stats, int with_scale, int dy_off,
                           int dx_off, char* out, size_t cap) {
  PlanScope sc;
  float *dy = norm_ptr(dy_off), *dx = norm_ptr(dx_off), *p = norm_ptr(0);
  float* xh = norm_ptr(dy_off) + 4;
  float* yr = with_scale ? norm_ptr(dy_off) + 8 : nullptr;
  int rc = RRAM_OK;
  if (!global_stats || with_scale)
    rc = rram_norm_bwd_reduce(dy, yr, xh, num, channels, inner, with_scale ? p : nullptr, p, with_scale ? p : nullptr,
                              with_scale ? p : nullptr, global_stats ? nullptr : p, p, ~size_t{0}, nullptr);
  if (rc == RRAM_OK)
    rc = rram_norm_bwd_apply(dy, yr, xh, global_stats ? nullptr : p, with_scale ? p : nullptr, p, dx, num, channels,
                             inner, nullptr);
  return norm_result(rc, sc, out, cap);
}
int rram_scale_kernel_ids(int num, int channels, int64_t inner, int backward, int x_off, int y_off, char* out,
                          size_t cap) {
  PlanScope sc;
  float *x = norm_ptr(x_off), *y = norm_ptr(y_off), *p = norm_ptr(0);
  int rc;
  if (!backward) {
    rc = rram_norm_apply(x, y, nullptr, nullptr, nullptr, p, p, 0, num, channels, inner, nullptr);
  } else {
    rc = rram_norm_bwd_reduce(x, nullptr, norm_ptr(x_off) + 4, num, channels, inner, nullptr, nullptr, p, p, nullptr,
                              p, ~size_t{0}, nullptr);
    if (rc == RRAM_OK) rc = rram_norm_bwd_apply(x, nullptr, nullptr, nullptr, p, nullptr, y, num, channels, inner, nullptr);
  }
  return norm_result(rc, sc, out, cap);
}
int rram_sigmoid_kernel_ids(int64_t n, int backward, char* out, size_t cap) {
  PlanScope sc;
  float* p = norm_ptr(0);
  return norm_result(backward ? rram_sigmoid_bwd(p, p + 4, p + 4, n, nullptr) : rram_sigmoid_fwd(p, p, n, nullptr), sc,
                     out, cap);
}
// every id a launch site of this file can record
int rram_norm_kernel_list(char* out, size_t cap) {
  return copy_text(
      "bn_stats_plane<1>\nbn_stats_plane<4>\nbn_stats_cols\nbn_stats_finalize\nbn_global_stats\n"
      "norm_apply<1>\nnorm_apply<4>\n"
      "norm_bwd_reduce_plane<1>\nnorm_bwd_reduce_plane<4>\nnorm_bwd_reduce_cols\nnorm_bwd_finalize\n"
      "norm_bwd<1>\nnorm_bwd<4>\nsigmoid_fwd\nsigmoid_bwd\n",
      out, cap);
}

}  // extern "C"
