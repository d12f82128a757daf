// The crossbar-tiled InnerProduct forward (no reference
// counterpart): y[M][N] = read-out of x[M][K] . W[N][K]^T from arrays of R rows.
// The K axis is cut into crossbar tiles of R rows; every tile's partial sum is
// formed in fp32 with the bf16x6 product order (x6::mfma6), digitised by an
// ADC of B bits (q = clamp(rint(p / step), +-qmax), step = range / qmax) and
// only the integer codes are summed:
//   S[m][n] = sum_t q_t[m][n] (int32),   y = float(S) * step + bias, ReLU.
// S is an integer, so the result does not depend on how the tiles are spread
// over workgroups: every split over K gives the same bits.
//
// Work split.  A workgroup (4 waves) owns 128 rows x 128 columns of y for a
// range of whole crossbar tiles (split-K in tiles).  Wave w owns all 128 rows
// x columns 32 w .. 32 w + 31: four 32 x 32 blocks, each with one fp32
// accumulator (the current tile's partial sum) and one int32 accumulator (S).
// At a tile boundary the ADC runs on the fp32 set in registers, the codes are
// added to S and the fp32 set is cleared; a partial sum never leaves the
// registers.  With one split the epilogue writes y; otherwise each split writes
// its int32 slab [z][M][N] to the workspace and k_xbar_finish sums the slabs.
//
// Staging.  The activations are split once into bf16 terms by k_xbar_pack
// (the DAC is applied there), laid out as the LDS image of a K-step: [row tile]
// [K-step of 32][128 rows][208 B], a row = [group g][half h][term][8 bf16] +
// 16 B pad (13 16-byte units: conflict-free ds_read_b128), lane half h of MFMA
// group g holding k = 16 h + 8 g + j.  The weights are read from HBM once as
// fp32 (16-byte loads, or 4-byte loads for unaligned rows / K % 4 != 0) and
// split in registers after the LDS read, each wave only its own 32 columns.
// Two LDS stages: the global loads of K-step s + 1 are issued before the MFMAs
// of step s and land in LDS after them, one barrier per step.
#include <algorithm>
#include <cmath>

#include "gemm_common.hpp"
#include "split3.hpp"

namespace rram {
float* pack_buffer(size_t floats, hipStream_t s);  // gemm.hip

namespace {
namespace xb {

constexpr int KS = 32;                // k per K-step: two MFMA groups of 16
constexpr int MI = 4;                 // 32-row blocks per wave
constexpr int BM = 32 * MI, BN = 128;
constexpr int RLB = 2 * 96 + 16;      // packed activation row bytes per K-step
constexpr int A_B = BM * RLB;         // activation bytes per K-step and row tile
constexpr int A_U = A_B / 16;         // ... in 16-byte units
constexpr int A_LD = (A_U + 255) / 256;
constexpr int B_B = BN * KS * 4;      // weight bytes per K-step (fp32)
constexpr int B_LD = BN * (KS / 4) / 256;
constexpr int STAGE = A_B + B_B;
static_assert(2 * STAGE <= 160 * 1024, "LDS");

struct Plan {
  const char* apack;
  const float* w;
  const float* bias;
  float* y;
  int32_t* part;       // int32 slabs [split][M][N] (split > 1)
  int M, N, K;
  int tiles_m, tiles_n;
  int ksteps;          // ceil(K / 32)
  int spt;             // K-steps per crossbar tile (R / 32)
  int ntiles;          // crossbar tiles ceil(K / R)
  int tc, split;       // tiles per split, splits
  float step, inv_step, qmax;
  int relu;
};

// y of one output: float(S) * step, + bias when there is one, ReLU
__device__ __forceinline__ float xbar_out(int32_t S, float step, const float* bias, int n, int relu) {
  float o = __fmul_rn(static_cast<float>(S), step);
  if (bias != nullptr) o = __fadd_rn(o, bias[n]);
  return relu ? fmaxf(o, 0.0f) : o;
}

// x [M][K] fp32 -> DAC -> bf16 terms in the K-step slabs k_ip_xbar copies to
// LDS (zero past M and K).  One thread per (row, K-step, group, half): 8
// activations in, 48 bytes out.  dac_qmax = 0: no DAC.
template <bool VEC>
__global__ void __launch_bounds__(256) k_xbar_pack(const float* __restrict__ x, int M, int K, char* __restrict__ out,
                                                   int ksteps, int64_t units, float dac_xs, float dac_qmax) {
  for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
    const int h = static_cast<int>(u & 1), g = static_cast<int>((u >> 1) & 1);
    const int64_t r = u >> 2;
    const int ks = static_cast<int>(r % ksteps);
    const int64_t mrow = r / ksteps;  // tm * BM + row
    const int k = ks * KS + 16 * h + 8 * g;
    float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (mrow < M) {
      const float* src = x + mrow * K + k;
      if (VEC) {  // K % 4 == 0, x 16-byte aligned
#pragma unroll
        for (int q = 0; q < 2; ++q)
          if (k + 4 * q < K) {
            const float4 f = *reinterpret_cast<const float4*>(src + 4 * q);
            v[4 * q] = f.x, v[4 * q + 1] = f.y, v[4 * q + 2] = f.z, v[4 * q + 3] = f.w;
          }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (k + j < K) v[j] = src[j];
      }
    }
    if (dac_qmax > 0.0f) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = __fmul_rn(__builtin_amdgcn_fmed3f(__builtin_rintf(v[j] / dac_xs), -dac_qmax, dac_qmax), dac_xs);
    }
    const int64_t tm = mrow / BM;
    const int row = static_cast<int>(mrow - tm * BM);
    char* rowp = out + ((tm * ksteps + ks) * BM + row) * RLB;
    x6::store_terms8(v, rowp + (g * 2 + h) * 48);
    if (g == 1 && h == 1) *reinterpret_cast<uint4*>(rowp + 192) = make_uint4(0, 0, 0, 0);
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) k_ip_xbar(Plan P) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63, lr = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int id = xcd_tile_id(blockIdx.x, gridDim.x);
  const int tm = __builtin_amdgcn_readfirstlane(id % P.tiles_m);
  const int tn = __builtin_amdgcn_readfirstlane((id / P.tiles_m) % P.tiles_n);
  const int z = __builtin_amdgcn_readfirstlane(id / (P.tiles_m * P.tiles_n));
  const int m0 = tm * BM, n0 = tn * BN;
  // whole crossbar tiles [t0, t1) = K-steps [s0, s1); the last tile may be short
  const int t0 = z * P.tc, t1 = min(P.ntiles, t0 + P.tc);
  const int s0 = t0 * P.spt, s1 = min(P.ksteps, t1 * P.spt);

  // this thread's pieces of a K-step: A_LD 16-byte units of the packed
  // activations, B_LD quads (row, 4 k) of the weights
  const char* asrc = P.apack + (int64_t)tm * P.ksteps * A_B + tid * 16;
  const float* bsrc[B_LD];
  int bq[B_LD], blds[B_LD];
#pragma unroll
  for (int i = 0; i < B_LD; ++i) {
    const int idx = tid + 256 * i, row = idx >> 3, q = idx & 7;
    bsrc[i] = n0 + row < P.N ? P.w + (int64_t)(n0 + row) * P.K + 4 * q : nullptr;
    bq[i] = 4 * q;
    blds[i] = A_B + row * (KS * 4) + ((q ^ ((row >> 1) & 7)) << 4);
  }
  uint4 ra[A_LD];
  float4 rb[B_LD];
  auto gload = [&](int s) {
    const char* a = asrc + (int64_t)s * A_B;
#pragma unroll
    for (int i = 0; i < A_LD; ++i)
      if (tid + 256 * i < A_U) ra[i] = *reinterpret_cast<const uint4*>(a + 4096 * i);
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
      const int k = s * KS + bq[i];
      float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (bsrc[i] != nullptr) {
        const float* p = bsrc[i] + s * KS;
        if (VEC) {  // K % 4 == 0, w 16-byte aligned
          if (k < P.K) f = *reinterpret_cast<const float4*>(p);
        } else {
          if (k < P.K) f.x = p[0];
          if (k + 1 < P.K) f.y = p[1];
          if (k + 2 < P.K) f.z = p[2];
          if (k + 3 < P.K) f.w = p[3];
        }
      }
      rb[i] = f;
    }
  };
  auto lstore = [&](char* st) {
#pragma unroll
    for (int i = 0; i < A_LD; ++i)
      if (tid + 256 * i < A_U) *reinterpret_cast<uint4*>(st + tid * 16 + 4096 * i) = ra[i];
#pragma unroll
    for (int i = 0; i < B_LD; ++i) *reinterpret_cast<float4*>(st + blds[i]) = rb[i];
  };

  floatx16 acc[MI];   // the current crossbar tile's partial sums
  int32_t S[MI][16];  // the digital sum of the ADC codes
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[i][r] = 0.0f;
      S[i][r] = 0;
    }

  const int nw = 32 * wave + lr;  // this lane's weight row (output column) inside the tile
  auto compute = [&](const char* st) {
    const float* sb = reinterpret_cast<const float*>(st + A_B) + nw * KS;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      float b[8];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float4 q = *reinterpret_cast<const float4*>(sb + (((4 * lh + 2 * g + u) ^ ((nw >> 1) & 7)) << 2));
        b[4 * u] = q.x, b[4 * u + 1] = q.y, b[4 * u + 2] = q.z, b[4 * u + 3] = q.w;
      }
      x6::Parts bp;
      x6::split8_safe(b, bp);
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const char* p = st + (i * 32 + lr) * RLB + (g * 2 + lh) * 48;
        const x6::Parts a{*reinterpret_cast<const x6::bf16x8*>(p), *reinterpret_cast<const x6::bf16x8*>(p + 16),
                          *reinterpret_cast<const x6::bf16x8*>(p + 32)};
        acc[i] = x6::mfma6(a, bp, acc[i]);
      }
    }
  };
  // the ADC at a tile boundary: codes into S, the partial sums cleared
  auto adc = [&]() {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float q = __builtin_amdgcn_fmed3f(__builtin_rintf(__fmul_rn(acc[i][r], P.inv_step)), -P.qmax, P.qmax);
        S[i][r] += static_cast<int32_t>(q);
        acc[i][r] = 0.0f;
      }
  };

  gload(s0);
  lstore(smem);
  __syncthreads();
  int in_tile = 0;
  for (int s = s0; s < s1; ++s) {
    const int cur = (s - s0) & 1;
    const bool more = s + 1 < s1;
    if (more) gload(s + 1);
    compute(smem + cur * STAGE);
    if (++in_tile == P.spt) {
      adc();
      in_tile = 0;
    }
    if (more) lstore(smem + (cur ^ 1) * STAGE);
    __syncthreads();
  }
  if (in_tile != 0) adc();  // the short last tile

  // lane (lr, lh) holds column lr, rows 32 i + 8 (r >> 2) + 4 lh + (r & 3)
  const int n = n0 + nw;
  if (n >= P.N) return;
  int32_t* part = P.split > 1 ? P.part + (int64_t)z * P.M * P.N : nullptr;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + 32 * i + 8 * (r >> 2) + 4 * lh + (r & 3);
      if (m >= P.M) continue;
      if (part != nullptr)
        part[(int64_t)m * P.N + n] = S[i][r];
      else
        P.y[(int64_t)m * P.N + n] = xbar_out(S[i][r], P.step, P.bias, n, P.relu);
    }
}

// y = the read-out of the summed int32 slabs [split][M][N]
__global__ void __launch_bounds__(256) k_xbar_finish(const int32_t* __restrict__ part, int split, int M, int N,
                                                     float step, const float* __restrict__ bias, int relu,
                                                     float* __restrict__ y) {
  const int64_t total = (int64_t)M * N;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int32_t S = 0;
    for (int z = 0; z < split; ++z) S += part[z * total + idx];
    y[idx] = xbar_out(S, step, bias, static_cast<int>(idx % N), relu);
  }
}

// The configuration's checks (host only) and the plan of a shape.
int check(int M, int N, int K, const rram_xbar_cfg* c, int transpose) {
  RRAM_REQUIRE(c != nullptr, "ip_fwd_xbar: cfg is NULL");
  RRAM_REQUIRE(M >= 0 && N >= 0 && K >= 1, "ip_fwd_xbar: bad shape %d x %d x %d", M, N, K);
  RRAM_REQUIRE(!transpose, "ip_fwd_xbar: transposed weights are not served");
  RRAM_REQUIRE(c->rows >= 32 && c->rows <= 1024 && c->rows % 32 == 0,
               "ip_fwd_xbar: rows %d not a multiple of 32 in [32, 1024]", c->rows);
  RRAM_REQUIRE(c->adc_bits >= 2 && c->adc_bits <= 16, "ip_fwd_xbar: adc_bits %d outside [2, 16]", c->adc_bits);
  RRAM_REQUIRE(std::isfinite(c->adc_range) && c->adc_range > 0.0f, "ip_fwd_xbar: adc_range must be finite and > 0");
  RRAM_REQUIRE(c->dac_bits == 0 || (c->dac_bits >= 2 && c->dac_bits <= 16),
               "ip_fwd_xbar: dac_bits %d neither 0 nor in [2, 16]", c->dac_bits);
  RRAM_REQUIRE(c->dac_bits == 0 || (std::isfinite(c->dac_range) && c->dac_range > 0.0f),
               "ip_fwd_xbar: dac_range must be finite and > 0");
  RRAM_REQUIRE((int64_t)M * N < (1ll << 31), "ip_fwd_xbar: more than 2^31 outputs");
  return RRAM_OK;
}

// split_k = 0: toward 256 workgroups, whole tiles, partials within ws_bytes;
// else the caller's split clamped to the tile count
void make_plan(int M, int N, int K, const rram_xbar_cfg& c, int split_k, size_t ws_bytes, Plan& P) {
  P = Plan{};
  P.M = M, P.N = N, P.K = K;
  P.tiles_m = (M + BM - 1) / BM;
  P.tiles_n = (N + BN - 1) / BN;
  P.ksteps = (K + KS - 1) / KS;
  P.spt = c.rows / KS;
  P.ntiles = (K + c.rows - 1) / c.rows;
  int split = split_k;
  if (split_k <= 0) {
    const int64_t tiles = (int64_t)P.tiles_m * P.tiles_n;
    split = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(64, 256 / tiles)));
    while (split > 1 && (size_t)split * M * N * sizeof(int32_t) > ws_bytes) --split;
  }
  split = std::max(1, std::min(split, P.ntiles));
  P.tc = (P.ntiles + split - 1) / split;
  P.split = (P.ntiles + P.tc - 1) / P.tc;
  const int qmax = (1 << (c.adc_bits - 1)) - 1;
  const double step = static_cast<double>(c.adc_range) / qmax;
  P.step = static_cast<float>(step);
  P.inv_step = static_cast<float>(1.0 / step);
  P.qmax = static_cast<float>(qmax);
}

size_t part_bytes(const Plan& P) { return P.split > 1 ? (size_t)P.split * P.M * P.N * sizeof(int32_t) : 0; }

}  // namespace xb
}  // namespace
}  // namespace rram

extern "C" {

size_t rram_ip_fwd_xbar_workspace(int M, int N, int K, const rram_xbar_cfg* cfg, int split_k) {
  if (rram::xb::check(M, N, K, cfg, 0) != RRAM_OK || M == 0 || N == 0 || split_k < 0) return 0;
  rram::xb::Plan P;
  rram::xb::make_plan(M, N, K, *cfg, split_k, ~static_cast<size_t>(0), P);
  return rram::xb::part_bytes(P);
}

int rram_ip_fwd_xbar(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int transpose,
                     const rram_xbar_cfg* cfg, int relu, int split_k, void* ws, size_t ws_bytes, rram_stream_t st) {
  using namespace rram;
  const int rc0 = xb::check(M, N, K, cfg, transpose);
  if (rc0) return rc0;
  RRAM_REQUIRE(split_k >= 0, "ip_fwd_xbar: negative split_k");
  if (M == 0 || N == 0) return RRAM_OK;
  RRAM_REQUIRE(x && w && y, "ip_fwd_xbar: NULL");
  xb::Plan P;
  xb::make_plan(M, N, K, *cfg, split_k, ws != nullptr ? ws_bytes : 0, P);
  RRAM_REQUIRE(P.split == 1 || (ws != nullptr && ws_bytes >= xb::part_bytes(P)),
               "ip_fwd_xbar: workspace of %zu bytes below the %zu of %d splits", ws_bytes, xb::part_bytes(P), P.split);
  RRAM_REQUIRE((int64_t)P.tiles_m * P.tiles_n * P.split < (1ll << 31), "ip_fwd_xbar: grid too large");
  hipStream_t s = as_stream(st);
  auto al16 = [&](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && K % 4 == 0; };
  const bool xv = al16(x), wv = al16(w);

  const int64_t pack_b = (int64_t)P.tiles_m * P.ksteps * xb::A_B;
  float dac_xs = 1.0f, dac_qmax = 0.0f;
  if (cfg->dac_bits > 0) {
    dac_qmax = static_cast<float>((1 << (cfg->dac_bits - 1)) - 1);
    dac_xs = static_cast<float>(static_cast<double>(cfg->dac_range) / dac_qmax);
  }
  if (!plan_note("xbar:pack<%s>", xv ? "vec" : "scalar")) {
    char* pb = reinterpret_cast<char*>(pack_buffer(static_cast<size_t>(pack_b / 4), s));
    RRAM_REQUIRE(pb != nullptr, "ip_fwd_xbar: packed-activation buffer allocation failed");
    P.apack = pb;
    const int64_t units = (int64_t)P.tiles_m * xb::BM * P.ksteps * 4;
    if (xv)
      hipLaunchKernelGGL(xb::k_xbar_pack<true>, dim3(stream_blocks(units)), dim3(256), 0, s, x, M, K, pb, P.ksteps,
                         units, dac_xs, dac_qmax);
    else
      hipLaunchKernelGGL(xb::k_xbar_pack<false>, dim3(stream_blocks(units)), dim3(256), 0, s, x, M, K, pb, P.ksteps,
                         units, dac_xs, dac_qmax);
    const int rc = launch_status("ip_fwd_xbar pack");
    if (rc) return rc;
  }
  P.w = w;
  P.bias = bias;
  P.y = y;
  P.part = P.split > 1 ? static_cast<int32_t*>(ws) : nullptr;
  P.relu = relu;
  if (!plan_note("xbar:ip<%s>/s%d", wv ? "vec" : "scalar", P.split)) {
    const dim3 grid(static_cast<unsigned>(P.tiles_m * P.tiles_n * P.split));
    if (wv)
      hipLaunchKernelGGL(xb::k_ip_xbar<true>, grid, dim3(256), 0, s, P);
    else
      hipLaunchKernelGGL(xb::k_ip_xbar<false>, grid, dim3(256), 0, s, P);
    const int rc = launch_status("ip_fwd_xbar");
    if (rc) return rc;
  }
  if (P.split == 1 || plan_note("xbar:finish")) return RRAM_OK;
  hipLaunchKernelGGL(xb::k_xbar_finish, dim3(stream_blocks((int64_t)M * N)), dim3(256), 0, s, P.part, P.split, M, N,
                     P.step, bias, relu, y);
  return launch_status("ip_fwd_xbar finish");
}

int rram_ip_fwd_xbar_kernel_ids(int M, int N, int K, const rram_xbar_cfg* cfg, int x_align16, int w_align16,
                                int split_k, size_t ws_bytes, char* out, size_t cap) {
  rram::PlanScope sc;
  auto ptr = [](int align16) { return reinterpret_cast<float*>(uintptr_t{1} << 20 | (align16 ? 0u : 4u)); };
  const int rc = rram_ip_fwd_xbar(ptr(x_align16), ptr(w_align16), nullptr, ptr(1), M, N, K, 0, cfg, 0, split_k,
                                  ws_bytes ? ptr(1) : nullptr, ws_bytes, nullptr);
  return rc ? rc : rram::copy_text(sc.text, out, cap);
}

}  // extern "C"
