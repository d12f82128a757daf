// The stride-1 3x3 / 5x5 convolution weight gradient on the bf16x6 engine
// (conv_layer.cu:35-44's weight GEMM):
//   dW_g[co][ci][kh][kw] += sum_{n,oh,ow} dY[n][co][oh][ow] X[n][ci][oh+kh-ph][ow+kw-pw]
// on v_mfma_f32_32x32x16_bf16 with both operands split in the kernel
// (x6::split8_safe) and the six products of x6::mfma6.
//
// Work split.  The contraction runs over blocks: SR output rows (1, 2 or 4)
// of one image, and for planes wider than 32 one chunk of 32 output columns
// of them.  A workgroup owns 32 WM output channels x 32 WN input channels x
// all taps of one group for one range of blocks (split-K), walks the range in
// steps of BS blocks and writes one fp32 partial slab [split][Cout][N]; the
// slabs are summed in split order into dw (beta = 1) by the fp32 engine's
// k_splitk_reduce / k_splitk_reduce_wave.  No atomics: the result is a pure
// function of the inputs and the plan.
//   3x3: 2 x 2 waves, each 32 co x 32 ci x 9 taps (144 accumulator registers)
//   5x5: 2 co tiles x 2 kernel-row halves (rows 0-2 | 3-4), 32 ci: 240 registers
//
// Staging.  Per step the 256 threads read the dY rows of the co tile and, for
// each block, its SR + K - 1 input rows of the ci tile (halo columns and rows
// written as zeros), split each run of 8 floats once and write three planes of
// plain bf16 rows to LDS (two stages: step t + 1 is staged before the MFMAs of
// step t, one barrier per step).  dY rows are padded with zeros to a multiple
// of 8 positions; a zero dY kills the products of the padding.
//
// Fragments.  The MFMA K index is a group of 8 output positions, lane half h
// taking group 2 s + h of MFMA step s.  GR = 1: 8 consecutive positions of one
// output row; GR = 2 | 4 (planes at most 4 | 2 wide): 4 | 2 positions of 2 | 4
// consecutive rows.  An A fragment term is one 16-byte LDS read of dY, held
// across every (kh, kw).  For a kernel row the lane reads the aligned window of
// the X row once (16 elements, or GR sub-rows of 8) and derives every kw shift
// in registers with v_alignbit_b32: one window read per kernel row, no
// 2-byte-misaligned LDS access.
#include <algorithm>
#include <atomic>
#include <string>

#include "gemm_common.hpp"
#include "split3.hpp"

namespace rram {
namespace {
namespace wg6 {

constexpr int kLdsMax = 160 * 1024;
constexpr int kColChunk = 32;  // output columns of a block when the plane is wider

struct Plan {
  const float* x;
  const float* dy;
  float* part;
  int cin, cout, cin_g, cout_g, H, W, Ho, Wo, ph, pw;
  int sr_log, SR, BS, GR, RP, RP8, XW8, NXR, NG, NS;  // NS: MFMA steps per step = ceil(NG / 2)
  int pitch_a, pitch_x, plane_a, plane_x;              // bytes
  int nblk, chunk, split;                              // blocks, blocks per split, splits
  int tiles_m, tiles_n, G;
  FastDiv bpi, ncc, rp8, xw8, nxr_xw8, rows_in, npos8;
};

// the image, first output row and first output column of block blk
struct Block {
  int n, oh0, c0;
};
__device__ __forceinline__ Block decode(const Plan& P, int blk) {
  const uint32_t n = fdiv(static_cast<uint32_t>(blk), P.bpi);
  const uint32_t rem = static_cast<uint32_t>(blk) - n * P.bpi.d;
  const uint32_t rb = fdiv(rem, P.ncc);
  return Block{static_cast<int>(n), static_cast<int>(rb) << P.sr_log, static_cast<int>(rem - rb * P.ncc.d) * kColChunk};
}

template <int KS, int WM, int WN, int NKG, int GR>
__global__ void __launch_bounds__(256) k_wgrad_x6(Plan P) {
  constexpr int NKR = (KS + NKG - 1) / NKG;  // kernel rows per wave
  constexpr int CP = 8 / GR;                 // positions per row of a group
  constexpr int NW = GR == 1 ? 8 : 4 * GR;   // 32-bit words of a window term
  constexpr int T = KS * KS;
  constexpr int COT = 32 * WM, CIT = 32 * WN;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

  const int tid = threadIdx.x;
  const int lane = tid & 63, lr = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave % WM, wn = (wave / WM) % WN, kg = wave / (WM * WN);
  const int kh0 = kg * NKR;

  int bid = blockIdx.x;
  const int tm = bid % P.tiles_m;
  bid /= P.tiles_m;
  const int tn = bid % P.tiles_n;
  bid /= P.tiles_n;
  const int g = bid % P.G;
  const int z = bid / P.G;
  const int co0 = tm * COT, ci0 = tn * CIT;
  const int blk_lo = z * P.chunk, blk_hi = min(blk_lo + P.chunk, P.nblk);
  const int nsteps = (blk_hi - blk_lo + P.BS - 1) / P.BS;
  const int stage_bytes = 3 * (P.plane_a + P.plane_x);
  const int rows_in = P.SR + KS - 1;

  // one step's operands into stage st: every byte of the stage is written
  auto stage = [&](int step, int st) {
    char* sa = smem + st * stage_bytes;
    char* sx = sa + 3 * P.plane_a;
    const int blk0 = blk_lo + step * P.BS;
    const int ua = COT * static_cast<int>(P.npos8.d);
    for (int u = tid; u < ua; u += 256) {
      const int col = static_cast<int>(fdiv(static_cast<uint32_t>(u), P.npos8));
      const int p8 = u - col * static_cast<int>(P.npos8.d);
      int rs, ow0;  // first row slot and column of the 8 positions
      if (GR == 1) {
        rs = static_cast<int>(fdiv(static_cast<uint32_t>(p8), P.rp8));
        ow0 = (p8 - rs * P.RP8) * 8;
      } else {
        rs = p8 * GR;
        ow0 = 0;
      }
      const int blk = blk0 + (rs >> P.sr_log);
      const int co = co0 + col;
      float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (p8 < P.NG && blk < blk_hi && co < P.cout_g) {
        const Block b = decode(P, blk);
        const int row0 = b.oh0 + (rs & (P.SR - 1));
        const float* src = P.dy + ((int64_t)b.n * P.cout + g * P.cout_g + co) * (P.Ho * P.Wo);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const int oh = row0 + t / CP, ow = b.c0 + ow0 + t % CP;
          if (oh < P.Ho && ow < P.Wo && ow0 + t % CP < P.RP) v[t] = src[oh * P.Wo + ow];
        }
      }
      x6::Parts s;
      x6::split8_safe(v, s);
      char* dst = sa + col * P.pitch_a + p8 * 16;
      *reinterpret_cast<x6::bf16x8*>(dst) = s.h;
      *reinterpret_cast<x6::bf16x8*>(dst + P.plane_a) = s.m;
      *reinterpret_cast<x6::bf16x8*>(dst + 2 * P.plane_a) = s.l;
    }
    const int ux = CIT * static_cast<int>(P.nxr_xw8.d);
    for (int u = tid; u < ux; u += 256) {
      const int cil = static_cast<int>(fdiv(static_cast<uint32_t>(u), P.nxr_xw8));
      const int rem = u - cil * static_cast<int>(P.nxr_xw8.d);
      const int xr = static_cast<int>(fdiv(static_cast<uint32_t>(rem), P.xw8));
      const int e8 = rem - xr * P.XW8;
      const int bs = static_cast<int>(fdiv(static_cast<uint32_t>(xr), P.rows_in));
      const int i = xr - bs * rows_in;
      const int blk = blk0 + bs;
      const int ci = ci0 + cil;
      float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (blk < blk_hi && ci < P.cin_g) {
        const Block b = decode(P, blk);
        const int ih = b.oh0 - P.ph + i;
        if (ih >= 0 && ih < P.H) {
          const float* src = P.x + (((int64_t)b.n * P.cin + g * P.cin_g + ci) * P.H + ih) * P.W;
          const int iw0 = b.c0 + e8 * 8 - P.pw;
#pragma unroll
          for (int t = 0; t < 8; ++t)
            if (iw0 + t >= 0 && iw0 + t < P.W) v[t] = src[iw0 + t];
        }
      }
      x6::Parts s;
      x6::split8_safe(v, s);
      char* dst = sx + cil * P.pitch_x + (xr * P.XW8 + e8) * 16;
      *reinterpret_cast<x6::bf16x8*>(dst) = s.h;
      *reinterpret_cast<x6::bf16x8*>(dst + P.plane_x) = s.m;
      *reinterpret_cast<x6::bf16x8*>(dst + 2 * P.plane_x) = s.l;
    }
  };

  floatx16 acc[NKR][KS];
#pragma unroll
  for (int i = 0; i < NKR; ++i)
#pragma unroll
    for (int j = 0; j < KS; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  // a wave whose co or ci tile lies past the group's channels only stages
  const bool active = co0 + wm * 32 < P.cout_g && ci0 + wn * 32 < P.cin_g;

  auto compute = [&](int st) {
    const char* sa = smem + st * stage_bytes + (wm * 32 + lr) * P.pitch_a;
    const char* sx = smem + st * stage_bytes + 3 * P.plane_a + (wn * 32 + lr) * P.pitch_x;
    for (int s = 0; s < P.NS; ++s) {
      const int gi = 2 * s + lh;
      x6::Parts a;
      a.h = *reinterpret_cast<const x6::bf16x8*>(sa + gi * 16);
      a.m = *reinterpret_cast<const x6::bf16x8*>(sa + P.plane_a + gi * 16);
      a.l = *reinterpret_cast<const x6::bf16x8*>(sa + 2 * P.plane_a + gi * 16);
      // the window of group gi at kernel row 0 (the odd count's last group
      // has zero dY: it rereads the group before it)
      const int gx = min(gi, P.NG - 1);
      int xoff, khs;
      if (GR == 1) {
        const int rs = static_cast<int>(fdiv(static_cast<uint32_t>(gx), P.rp8));
        const int gc = gx - rs * P.RP8;
        const int xr = (rs >> P.sr_log) * rows_in + (rs & (P.SR - 1));
        khs = P.XW8 * 16;
        xoff = xr * khs + gc * 16;
      } else {
        const int rs = gx * GR;
        const int xr = (rs >> P.sr_log) * rows_in + (rs & (P.SR - 1));
        khs = 16;
        xoff = xr * 16;
      }
#pragma unroll
      for (int i = 0; i < NKR; ++i) {
        if (kh0 + i >= KS) continue;
        uint32_t w[3][NW];
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
          for (int q = 0; q < NW / 4; ++q) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(sx + t * P.plane_x + xoff + (kh0 + i) * khs + q * 16);
            w[t][4 * q] = v[0];
            w[t][4 * q + 1] = v[1];
            w[t][4 * q + 2] = v[2];
            w[t][4 * q + 3] = v[3];
          }
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {
          u32x4 f[3];
#pragma unroll
          for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int sub = GR == 1 ? 0 : (2 * j) / CP, c = GR == 1 ? 2 * j : (2 * j) % CP;
              const int wi = sub * 4 + (c + kw) / 2;
              f[t][j] = (c + kw) % 2 ? __builtin_amdgcn_alignbit(w[t][wi + 1], w[t][wi], 16) : w[t][wi];
            }
          const x6::Parts b{__builtin_bit_cast(x6::bf16x8, f[0]), __builtin_bit_cast(x6::bf16x8, f[1]),
                            __builtin_bit_cast(x6::bf16x8, f[2])};
          acc[i][kw] = x6::mfma6(a, b, acc[i][kw]);
        }
      }
    }
  };

  stage(0, 0);
  __syncthreads();
  for (int t = 0; t < nsteps; ++t) {
    if (t + 1 < nsteps) stage(t + 1, (t + 1) & 1);
    if (active) compute(t & 1);
    __syncthreads();
  }

  // the partial slab: [z][g * cout_g + co][ci * T + kh * KS + kw]
  if (!active) return;
  const int N = P.cin_g * T;
  const int ci = ci0 + wn * 32 + lr;
  if (ci >= P.cin_g) return;
  float* out = P.part + ((int64_t)z * P.cout + g * P.cout_g) * N + ci * T;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = co0 + wm * 32 + 4 * lh + (r & 3) + 8 * (r >> 2);
    if (co >= P.cout_g) continue;
#pragma unroll
    for (int i = 0; i < NKR; ++i) {
      if (kh0 + i >= KS) continue;
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) out[(int64_t)co * N + (kh0 + i) * KS + kw] = acc[i][kw][r];
    }
  }
}

int pitch16(int bytes) {  // rows 16-byte aligned, an odd count of 16-byte units apart
  const int u = (bytes + 15) / 16;
  return (u | 1) * 16;
}

// The plan of d (shape filled by rram_conv_out_shape), or false: not served.
bool make_plan(const rram_conv_desc& d, Plan& P) {
  const int KS = d.kernel_h;
  if (d.kernel_w != KS || (KS != 3 && KS != 5) || d.stride_h != 1 || d.stride_w != 1 || d.dilation_h != 1 ||
      d.dilation_w != 1 || d.pad_h > KS - 1 || d.pad_w > KS - 1 || d.num < 1)
    return false;
  const int G = d.group, cin_g = d.channels / G, cout_g = d.num_output / G;
  const int64_t N = (int64_t)cin_g * KS * KS;
  // 32-bit offsets: a larger shape keeps the fp32 path
  if ((int64_t)d.num * d.channels * d.height * d.width >= (1ll << 31) ||
      (int64_t)d.num * d.num_output * d.out_h * d.out_w >= (1ll << 31) || (int64_t)d.num_output * N >= (1ll << 31))
    return false;
  P = Plan{};
  P.cin = d.channels, P.cout = d.num_output, P.cin_g = cin_g, P.cout_g = cout_g, P.G = G;
  P.H = d.height, P.W = d.width, P.Ho = d.out_h, P.Wo = d.out_w, P.ph = d.pad_h, P.pw = d.pad_w;
  const int COT = 64, CIT = KS == 3 ? 64 : 32;
  P.tiles_m = (cout_g + COT - 1) / COT;
  P.tiles_n = (cin_g + CIT - 1) / CIT;
  P.GR = d.out_w > 4 ? 1 : d.out_w > 2 ? 2 : 4;
  int ncc = 1;
  if (P.GR == 1) {
    ncc = (d.out_w + kColChunk - 1) / kColChunk;
    P.RP = ncc > 1 ? kColChunk : (d.out_w + 7) / 8 * 8;
    P.SR = P.RP <= 8 ? 4 : P.RP <= 16 ? 2 : 1;
    while (P.SR > 1 && P.SR / 2 >= d.out_h) P.SR /= 2;
  } else {
    P.RP = 8 / P.GR;
    P.SR = 4;
  }
  P.sr_log = P.SR == 4 ? 2 : P.SR == 2 ? 1 : 0;
  P.RP8 = P.GR == 1 ? P.RP / 8 : 1;
  P.XW8 = P.GR == 1 ? P.RP8 + 1 : 1;
  const int rows_blk = (d.out_h + P.SR - 1) / P.SR;
  const int64_t nblk = (int64_t)d.num * rows_blk * ncc;
  if (nblk >= (1 << 30)) return false;
  P.nblk = static_cast<int>(nblk);
  const int gpb = P.GR == 1 ? P.SR * P.RP8 : P.SR / P.GR;  // groups per block
  // splits toward 512 workgroups, each at least one step
  const int tiles = P.tiles_m * P.tiles_n * G;
  int want = std::max(1, std::min(256, 512 / tiles));
  P.BS = std::max(1, std::min({16 / gpb, 16, P.nblk}));
  while (P.BS > 1 && (P.nblk + P.BS - 1) / P.BS < want) P.BS /= 2;
  for (;; P.BS /= 2) {
    P.NG = P.BS * gpb;
    P.NS = (P.NG + 1) / 2;
    P.NXR = P.BS * (P.SR + KS - 1);
    P.pitch_a = pitch16(P.NS * 32);
    P.pitch_x = pitch16(P.NXR * P.XW8 * 16);
    P.plane_a = COT * P.pitch_a;
    P.plane_x = CIT * P.pitch_x;
    if (2 * 3 * (P.plane_a + P.plane_x) <= kLdsMax) break;
    if (P.BS == 1) return false;
  }
  const int steps = (P.nblk + P.BS - 1) / P.BS;
  want = std::min(want, steps);
  while (want > 1 && (int64_t)want * d.num_output * N * 4 > (256ll << 20)) --want;
  P.chunk = (steps + want - 1) / want * P.BS;
  P.split = (P.nblk + P.chunk - 1) / P.chunk;
  if ((int64_t)P.split * d.num_output * N >= (1ll << 31) || (int64_t)tiles * P.split >= (1ll << 31)) return false;
  P.bpi = make_fastdiv(rows_blk * ncc);
  P.ncc = make_fastdiv(ncc);
  P.rp8 = make_fastdiv(P.RP8);
  P.xw8 = make_fastdiv(P.XW8);
  P.nxr_xw8 = make_fastdiv(P.NXR * P.XW8);
  P.rows_in = make_fastdiv(P.SR + KS - 1);
  P.npos8 = make_fastdiv(2 * P.NS);
  return true;
}

size_t part_bytes(const rram_conv_desc& d, const Plan& P) {
  return (size_t)P.split * d.num_output * (d.channels / d.group) * d.kernel_h * d.kernel_w * sizeof(float);
}

#define RRAM_WGRAD_LIST(X) X(3, 2, 2, 1, 1) X(3, 2, 2, 1, 2) X(3, 2, 2, 1, 4) X(5, 2, 1, 2, 1) X(5, 2, 1, 2, 2) X(5, 2, 1, 2, 4)

// raised: the instantiation's flag, its dynamic-LDS limit is raised once
template <typename Kern>
int launch(Kern kern, std::atomic<bool>& raised, const Plan& P, hipStream_t s) {
  const int lds = 2 * 3 * (P.plane_a + P.plane_x);
  if (!raised.exchange(true))
    RRAM_HIP_RET(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     kLdsMax));
  hipLaunchKernelGGL(kern, dim3(P.tiles_m * P.tiles_n * P.G * P.split), dim3(256), lds, s, P);
  return launch_status("conv bwd weight (bf16x6)");
}

}  // namespace wg6
}  // namespace

std::atomic<int>& bwd_weight_engine() {
  static std::atomic<int> e{RRAM_ENGINE_F32};
  return e;
}

// partial bytes of the bf16x6 weight gradient of d, 0 when it does not serve d
size_t conv_bwd_weight_x6_bytes(const rram_conv_desc* d) {
  wg6::Plan P;
  return wg6::make_plan(*d, P) ? wg6::part_bytes(*d, P) : 0;
}

// dw += the weight gradient of all groups; part: conv_bwd_weight_x6_bytes(d) bytes
int conv_bwd_weight_x6(const rram_conv_desc* d, const float* x, const float* dy, float* dw, void* part,
                       size_t part_bytes, hipStream_t s) {
  wg6::Plan P;
  RRAM_REQUIRE(wg6::make_plan(*d, P) && part != nullptr && part_bytes >= wg6::part_bytes(*d, P),
               "conv bwd weight (bf16x6): shape or workspace not covered");
  P.x = x;
  P.dy = dy;
  P.part = static_cast<float*>(part);
  const int KS = d->kernel_h, N = P.cin_g * KS * KS;
  if (!plan_note("wgrad_x6<%d,%d>/s%d", KS, P.GR, P.split)) {
    int rc = RRAM_EINVAL;
#define RRAM_X(ks, wm, wn, nkg, gr)                                     \
  if (KS == ks && P.GR == gr) {                                         \
    static std::atomic<bool> raised{false};                             \
    rc = wg6::launch(wg6::k_wgrad_x6<ks, wm, wn, nkg, gr>, raised, P, s); \
  }
    RRAM_WGRAD_LIST(RRAM_X)
#undef RRAM_X
    if (rc) return rc;
  }
  const bool wave = P.split >= 32;
  if (plan_note(wave ? "reduce_wave" : "reduce")) return RRAM_OK;
  const int64_t outs = (int64_t)d->num_output * N;
  if (wave)
    hipLaunchKernelGGL(k_splitk_reduce_wave, dim3(static_cast<unsigned>((outs + 3) / 4)), dim3(256), 0, s, P.part,
                       P.split, d->num_output, N, N, dw, static_cast<float*>(nullptr));
  else
    hipLaunchKernelGGL(k_splitk_reduce, dim3(stream_blocks(outs)), dim3(256), 0, s, P.part, P.split, d->num_output, N,
                       make_epi(dw, N, 1.0f, 1.0f, nullptr, 0, 0));
  return launch_status("conv bwd weight (bf16x6) split-K reduce");
}

std::string conv_wgrad_kernel_list() {
  std::string out;
  char b[32];
#define RRAM_X(ks, wm, wn, nkg, gr)                     \
  snprintf(b, sizeof b, "wgrad_x6<%d,%d>\n", ks, gr); \
  out += b;
  RRAM_WGRAD_LIST(RRAM_X)
#undef RRAM_X
  return out;
}

}  // namespace rram
