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
//
// The crossbar-tiled Convolution forward (k_conv_xbar) is the same
// array with the unrolled kernel as its rows: see the comment above the kernel.
// The bit-serial read-out of the InnerProduct array (k_ip_xbar_bs)
// converts every input bit plane on its own: see the comment above that kernel.
// The bit-sliced-weight read-out (k_ip_xbar_ws) converts every
// weight slice's column sum on its own, on int8 codes and the int32 MFMA.
// Its digit-serial form (k_ip_xbar_ss) streams the input code a few
// bits per cycle against those slices, one conversion per (digit, slice) pair.
// The transposed read-out (k_ip_xbar_t) is the input gradient read
// from the same array the other way, the weights staged transposed.
// The kernels are built from the shared pieces below; which kernel uses which,
// and why k_conv_xbar keeps some text of its own, is above k_conv_xbar.
#include <algorithm>
#include <cmath>
#include <type_traits>

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
// bounds the two stages the source declares; the size the compiler reports for
// the InnerProduct kernels is larger ("LDS")
static_assert(2 * STAGE <= 160 * 1024, "LDS");

// What every read-out's plan holds: the operands, the K axis in K-steps and
// crossbar tiles with its split, and the ADC.
struct Core {
  const float* w;
  const float* bias;
  float* y;
  int32_t* part;       // int32 slabs [slab][y's layout] (more than one slab)
  int ksteps;          // ceil(K / 32)
  int spt;             // K-steps per crossbar tile (R / 32)
  int ntiles;          // crossbar tiles ceil(K / R)
  int tc, split;       // tiles per split, splits
  float step, inv_step, qmax;
  int relu;
};

struct Plan : Core {
  const char* apack;
  int M, N, K;
  int tiles_m, tiles_n;
};

// split z's whole crossbar tiles [z tc, (z + 1) tc) as K-steps [s0, s1); the last tile may be short
struct Span {
  int s0, s1;
};
template <class PlanT>  // Plan, BsPlan (through Core) or ConvPlan
__device__ __forceinline__ Span tile_span(int z, const PlanT& P) {
  const int t0 = z * P.tc, t1 = min(P.ntiles, t0 + P.tc);
  return {t0 * P.spt, min(P.ksteps, t1 * P.spt)};
}

// y of one output: float(S) * step, + bias when there is one, ReLU
__device__ __forceinline__ float xbar_out(int32_t S, float step, const float* bias, int n, int relu) {
  float o = __fmul_rn(static_cast<float>(S), step);
  if (bias != nullptr) o = __fadd_rn(o, bias[n]);
  return relu ? fmaxf(o, 0.0f) : o;
}

// the DAC on a run of 8 inputs: clamp(rint(v / xs), +-qmax) * xs (qmax = 0: none); 0 stays 0
__device__ __forceinline__ void dac8(float (&v)[8], float xs, float qmax) {
  if (qmax > 0.0f) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = __fmul_rn(__builtin_amdgcn_fmed3f(__builtin_rintf(v[j] / xs), -qmax, qmax), xs);
  }
}

// the ADC code of one partial sum: clamp(rint(p / step), +-qmax), half to even
__device__ __forceinline__ int32_t adc_code(float p, float inv_step, float qmax) {
  return static_cast<int32_t>(__builtin_amdgcn_fmed3f(__builtin_rintf(__fmul_rn(p, inv_step)), -qmax, qmax));
}

// Unit u of a pack kernel, one per (row, K-step, group g, half h): v = the 8
// activations k = 32 ks + 16 h + 8 g + j of row mrow = tm * bm + row (zero past
// M and K); returns where that row's row_bytes of K-step ks lie in the slabs
// [row tile][K-step][bm rows][row_bytes].
struct PackUnit {
  int g, h;
  char* row;
  int64_t slab;  // tm * ksteps + ks: which [row tile][K-step] slab
  int r;         // the row inside it
};
template <bool VEC>
__device__ __forceinline__ PackUnit pack_unit(int64_t u, const float* __restrict__ x, int M, int K, int ksteps,
                                              char* out, int bm, int row_bytes, float (&v)[8]) {
  const int h = static_cast<int>(u & 1), g = static_cast<int>((u >> 1) & 1);
  const int64_t r = u >> 2;
  const int ks = static_cast<int>(r % ksteps);
  const int64_t mrow = r / ksteps;
  const int k = ks * KS + 16 * h + 8 * g;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.0f;
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
  const int64_t tm = mrow / bm;
  const int row = static_cast<int>(mrow - tm * bm);
  return {g, h, out + ((tm * ksteps + ks) * bm + row) * row_bytes, tm * ksteps + ks, row};
}

// x [M][K] fp32 -> DAC -> bf16 terms in the K-step slabs k_ip_xbar copies to
// LDS (zero past M and K).  One thread per unit: 8 activations in, 48 bytes
// out.  dac_qmax = 0: no DAC.
template <bool VEC>
__global__ void __launch_bounds__(256) k_xbar_pack(const float* __restrict__ x, int M, int K, char* __restrict__ out,
                                                   int ksteps, int64_t units, float dac_xs, float dac_qmax) {
  for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
    float v[8];
    const PackUnit U = pack_unit<VEC>(u, x, M, K, ksteps, out, BM, RLB, v);
    dac8(v, dac_xs, dac_qmax);
    x6::store_terms8(v, U.row + (U.g * 2 + U.h) * 48);
    if (U.g == 1 && U.h == 1) *reinterpret_cast<uint4*>(U.row + 192) = make_uint4(0, 0, 0, 0);
  }
}

// Where quad q (4 k) of weight row `row` lies in a stage's weight region
// [128 rows][32 fp32], in bytes: the quad index is XOR-swizzled with the row so
// that the fragment reads are conflict-free.  WStage writes through this and
// wfrag, right below it, reads: the two must agree.
__device__ __forceinline__ int wquad_lds(int row, int q) { return row * (KS * 4) + ((q ^ ((row >> 1) & 7)) << 4); }

// the split fragment of weight row nw for MFMA group g, lane half lh (k = 16 lh
// + 8 g + j), from a stage's weight region: quads 4 lh + 2 g + u of wquad_lds,
// addressed in floats (written through wquad_lds itself, k_ip_xbar_bs<vec, PC 7>
// spills one register more)
__device__ __forceinline__ x6::Parts wfrag(const char* stage_b, int nw, int lh, int g) {
  const float* sb = reinterpret_cast<const float*>(stage_b) + nw * KS;
  float b[8];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const float4 q = *reinterpret_cast<const float4*>(sb + (((4 * lh + 2 * g + u) ^ ((nw >> 1) & 7)) << 2));
    b[4 * u] = q.x, b[4 * u + 1] = q.y, b[4 * u + 2] = q.z, b[4 * u + 3] = q.w;
  }
  x6::Parts p;
  x6::split8_safe(b, p);
  return p;
}

// One K-step of the weights, register-staged: B_LD quads per thread of the 128
// rows from w0 (row pitch K floats), zero for the rows at and past `rows` and
// for k past K, stored to the weight region at lds_off of a stage.
template <bool VEC>
struct WStage {
  const float* src[B_LD];  // the quad's first element at K-step 0; nullptr: a row past the matrix
  int k4[B_LD], lds[B_LD];
  int K;
  float4 r[B_LD];
  __device__ __forceinline__ WStage(const float* w0, int rows, int K_, int lds_off, int tid) : K(K_) {
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
      const int idx = tid + 256 * i, row = idx >> 3, q = idx & 7;
      src[i] = row < rows ? w0 + (int64_t)row * K + 4 * q : nullptr;
      k4[i] = 4 * q;
      lds[i] = lds_off + wquad_lds(row, q);
    }
  }
  __device__ __forceinline__ void load(int s) {
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
      const int k = s * KS + k4[i];
      float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (src[i] != nullptr) {
        const float* p = src[i] + s * KS;
        if (VEC) {  // K % 4 == 0, w 16-byte aligned
          if (k < K) f = *reinterpret_cast<const float4*>(p);
        } else {
          if (k < K) f.x = p[0];
          if (k + 1 < K) f.y = p[1];
          if (k + 2 < K) f.z = p[2];
          if (k + 3 < K) f.w = p[3];
        }
      }
      r[i] = f;
    }
  }
  __device__ __forceinline__ void store(char* st) const {
#pragma unroll
    for (int i = 0; i < B_LD; ++i) *reinterpret_cast<float4*>(st + lds[i]) = r[i];
  }
};

// the three 8-term runs (h, m, l) of one (group, half) of a packed 208-byte row
__device__ __forceinline__ x6::Parts term_parts(const char* p) {
  return {*reinterpret_cast<const x6::bf16x8*>(p), *reinterpret_cast<const x6::bf16x8*>(p + 16),
          *reinterpret_cast<const x6::bf16x8*>(p + 32)};
}

// The two-stage pipeline of the two InnerProduct kernels (k_conv_xbar keeps its
// own single loop) over K-steps [s0, s1), spt of them per crossbar tile:
// load(s + 1) is issued before compute(stage of s) and store(other stage) comes
// after it, one barrier per step; adc() after every tile's last step, the
// short last tile included.  Two levels, crossbar tiles then their K-steps, so
// that the ADC sits between loops and the accumulator sets stay in place (with
// one loop and a counter inside, k_ip_xbar_bs's sets become merges of "cleared"
// and "kept" and spill: DESIGN §7.6).
template <class Load, class Compute, class Store, class Adc>
__device__ __forceinline__ void pipeline(char* smem, int stage_bytes, Span k, int spt, Load load, Compute compute,
                                         Store store, Adc adc) {
  load(k.s0);
  store(smem);
  __syncthreads();
  for (int s = k.s0; s < k.s1;) {
    const int se = min(k.s1, s + spt);
    for (; s < se; ++s) {
      const int cur = (s - k.s0) & 1;
      const bool more = s + 1 < k.s1;
      if (more) load(s + 1);
      compute(smem + cur * stage_bytes);
      if (more) store(smem + (cur ^ 1) * stage_bytes);
      __syncthreads();
    }
    adc();
  }
}

// The InnerProduct epilogue of MI_ 32 x 32 blocks: lane (lr, lh) holds column
// n, rows m0 + 32 i + 8 (r >> 2) + 4 lh + (r & 3).  part: the workgroup's
// int32 slab, or nullptr to write y.
template <int MI_>
__device__ __forceinline__ void ip_store(const int32_t (&S)[MI_][16], const Plan& P, int32_t* part, int m0, int n,
                                         int lh) {
  if (n >= P.N) return;
#pragma unroll
  for (int i = 0; i < MI_; ++i)
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

  // this thread's pieces of a K-step: A_LD 16-byte units of the packed
  // activations, copied as they lie, and the weight stager's quads.  The copy
  // is written here and in k_ip_xbar_bs, not shared: through a function over
  // ra, k_ip_xbar_bs<PC 7> measured 0.9 % slower, and with ra inside a stager
  // object it spills 19 registers or more instead of 16 (DESIGN §7.4 "LDS").
  const char* asrc = P.apack + (int64_t)tm * P.ksteps * A_B + tid * 16;
  uint4 ra[A_LD];
  WStage<VEC> ws(P.w + (int64_t)n0 * P.K, P.N - n0, P.K, A_B, tid);
  auto gload = [&](int s) {
    const char* a = asrc + (int64_t)s * A_B;
#pragma unroll
    for (int i = 0; i < A_LD; ++i)
      if (tid + 256 * i < A_U) ra[i] = *reinterpret_cast<const uint4*>(a + 4096 * i);
    ws.load(s);
  };
  auto lstore = [&](char* st) {
#pragma unroll
    for (int i = 0; i < A_LD; ++i)
      if (tid + 256 * i < A_U) *reinterpret_cast<uint4*>(st + tid * 16 + 4096 * i) = ra[i];
    ws.store(st);
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
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const x6::Parts bp = wfrag(st + A_B, nw, lh, g);
#pragma unroll
      for (int i = 0; i < MI; ++i)
        acc[i] = x6::mfma6(term_parts(st + (i * 32 + lr) * RLB + (g * 2 + lh) * 48), bp, acc[i]);
    }
  };
  // the ADC at a tile boundary: codes into S, the partial sums cleared
  auto adc = [&]() {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        S[i][r] += adc_code(acc[i][r], P.inv_step, P.qmax);
        acc[i][r] = 0.0f;
      }
  };
  pipeline(smem, STAGE, tile_span(z, P), P.spt, gload, compute, lstore, adc);

  ip_store(S, P, P.split > 1 ? P.part + (int64_t)z * P.M * P.N : nullptr, m0, n0 + nw, lh);
}

// The transposed read-out: the input gradient of the same array,
// dx[m][k] = read-out of dy[m][n] . W[n][k], the voltages on the columns and the
// currents summed along the rows.  The reduction runs over the ROW index n of
// W [N][K], cut into crossbar tiles of C columns; everything but the weight
// operand is k_ip_xbar's: dy is packed by k_xbar_pack (the DAC there), the
// accumulator sets, the ADC between the loops, the pipeline and ip_store with
// the output columns k in N's place.  In the kernel's Plan, N is the output
// count (the caller's K, the pitch of a weight row) and K the reduction length
// (the caller's N).
//
// Weight operand.  A K-step needs the block W[32 n][128 k]: read along k (a
// weight row's contiguous floats), read back by the MFMA lanes along n (8
// consecutive n of one k).  WStageT transposes on the way: thread (kq, nq)
// loads the four quads W[32 s + 4 nq + i][k0 + 4 kq .. + 3], i = 0 .. 3 (the
// transpose of the 4 x 4 block is a renaming of its 16 registers) and stores
// four quads, output column 4 kq + c, n-quad nq.
//
// Placement.  wquad_lds would take these stores 4-way conflicted: a store
// instruction's rows 4 kq + c all have the parity of c, so its XOR swizzle
// reaches 4 of the 16 16-byte bank units.  The transposed region therefore has
// a placement and a reader of its own (tquad_lds, tfrag) and wquad_lds stays as
// it is: rows of 32 fp32 + 16 B pad, 9 units, so unit (9 row + q) mod 16.
// Reads: a ds_read_b128 lane group holds 16 rows distinct mod 16 at one q, 16
// distinct units.  Writes: lane l of wave v is kq = (l & 3) | (l >> 4) << 2 |
// (v & 1) << 4, nq = (l >> 2 & 3) | (v >> 1) << 2, so a group of 16 lanes
// (consecutive, or the read groups) holds all four kq mod 4 against four nq
// distinct mod 4: unit (4 kq + nq + 9 c) mod 16, all 16.  A wave's load
// instruction still covers 4 weight rows x 256 contiguous bytes.
constexpr int TRB = KS * 4 + 16;     // transposed weight row bytes per K-step: 32 n of one k + 16 B pad
constexpr int STAGE_T = A_B + BN * TRB;
static_assert(2 * STAGE_T <= 160 * 1024, "LDS");

__device__ __forceinline__ int tquad_lds(int row, int q) { return row * TRB + (q << 4); }

// wfrag for the transposed region: output column kw's n = 16 lh + 8 g + j
__device__ __forceinline__ x6::Parts tfrag(const char* stage_b, int kw, int lh, int g) {
  const float4* sb = reinterpret_cast<const float4*>(stage_b + tquad_lds(kw, 4 * lh + 2 * g));
  float b[8];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const float4 q = sb[u];
    b[4 * u] = q.x, b[4 * u + 1] = q.y, b[4 * u + 2] = q.z, b[4 * u + 3] = q.w;
  }
  x6::Parts p;
  x6::split8_safe(b, p);
  return p;
}

// One K-step of the weights, transposed through registers: the block of 32
// reduction rows n x 128 output columns from column k0 of w (row pitch `pitch`
// floats), zero for n at and past nred and for the columns at and past `cols`
// from k0, stored to the transposed region at lds_off of a stage.
//
// The loads carry no branch: a quad outside the matrix reads the matrix's first
// element(s) instead and is zeroed by select in store(), after the loads have
// landed.  With the zeros as the other arm of a branch around each load, the
// compiler resolved the transpose's renaming right behind the load, a wait for
// the load inside load(): the four loads of a step in series, and before the
// MFMAs they were to hide behind.
template <bool VEC>
struct WStageT {
  const float* w;    // the matrix: always readable, the stand-in address
  const float* src;  // W[0][k0 + 4 kq]: this thread's column quad
  int64_t pitch;
  int n4, cols, nred, lds;  // cols: valid columns from this thread's first
  int ok;                   // bit i: row i of the loaded step lies inside the matrix (and cols > 0)
  float4 r[4];
  __device__ __forceinline__ WStageT(const float* w_, int k0, int cols_, int nred_, int pitch_, int lds_off, int tid)
      : w(w_), pitch(pitch_), nred(nred_), ok(0) {
    const int l = tid & 63, v = tid >> 6;
    const int kq = (l & 3) | ((l >> 4) << 2) | ((v & 1) << 4), nq = ((l >> 2) & 3) | ((v >> 1) << 2);
    n4 = 4 * nq;
    cols = cols_ - 4 * kq;
    src = w_ + k0 + 4 * kq;
    lds = lds_off + tquad_lds(4 * kq, nq);
  }
  __device__ __forceinline__ void load(int s) {
    ok = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = s * KS + n4 + i;
      const bool in = n < nred && cols > 0;
      ok |= static_cast<int>(in) << i;
      const float* p = in ? src + n * pitch : w;
      if (VEC) {  // pitch % 4 == 0, w 16-byte aligned
        r[i] = *reinterpret_cast<const float4*>(p);
      } else {
        r[i].x = *p;
        r[i].y = *(in && cols > 1 ? p + 1 : w);
        r[i].z = *(in && cols > 2 ? p + 2 : w);
        r[i].w = *(in && cols > 3 ? p + 3 : w);
      }
    }
  }
  // element c of loaded row i, zero outside the matrix
  __device__ __forceinline__ float at(int i, float v, int c) const {
    return ((ok >> i) & 1) && (VEC || cols > c) ? v : 0.0f;
  }
  __device__ __forceinline__ void store(char* st) const {
    float4* d = reinterpret_cast<float4*>(st + lds);
    d[0 * (TRB / 16)] = make_float4(at(0, r[0].x, 0), at(1, r[1].x, 0), at(2, r[2].x, 0), at(3, r[3].x, 0));
    d[1 * (TRB / 16)] = make_float4(at(0, r[0].y, 1), at(1, r[1].y, 1), at(2, r[2].y, 1), at(3, r[3].y, 1));
    d[2 * (TRB / 16)] = make_float4(at(0, r[0].z, 2), at(1, r[1].z, 2), at(2, r[2].z, 2), at(3, r[3].z, 2));
    d[3 * (TRB / 16)] = make_float4(at(0, r[0].w, 3), at(1, r[1].w, 3), at(2, r[2].w, 3), at(3, r[3].w, 3));
  }
};

template <bool VEC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) k_ip_xbar_t(Plan P) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_T];
  const int tid = threadIdx.x;
  const int lane = tid & 63, lr = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int id = xcd_tile_id(blockIdx.x, gridDim.x);
  const int tm = __builtin_amdgcn_readfirstlane(id % P.tiles_m);
  const int tn = __builtin_amdgcn_readfirstlane((id / P.tiles_m) % P.tiles_n);
  const int z = __builtin_amdgcn_readfirstlane(id / (P.tiles_m * P.tiles_n));
  const int m0 = tm * BM, n0 = tn * BN;  // n0: the tile's first output column

  // this thread's pieces of a K-step: the packed dy as in k_ip_xbar (why the
  // copy is written in each kernel: there) and the transposing stager's quads
  const char* asrc = P.apack + (int64_t)tm * P.ksteps * A_B + tid * 16;
  uint4 ra[A_LD];
  WStageT<VEC> ws(P.w, n0, P.N - n0, P.K, P.N, A_B, tid);
  auto gload = [&](int s) {
    const char* a = asrc + (int64_t)s * A_B;
#pragma unroll
    for (int i = 0; i < A_LD; ++i)
      if (tid + 256 * i < A_U) ra[i] = *reinterpret_cast<const uint4*>(a + 4096 * i);
    ws.load(s);
  };
  auto lstore = [&](char* st) {
#pragma unroll
    for (int i = 0; i < A_LD; ++i)
      if (tid + 256 * i < A_U) *reinterpret_cast<uint4*>(st + tid * 16 + 4096 * i) = ra[i];
    ws.store(st);
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

  const int kw = 32 * wave + lr;  // this lane's output column inside the tile
  auto compute = [&](const char* st) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const x6::Parts bp = tfrag(st + A_B, kw, lh, g);
#pragma unroll
      for (int i = 0; i < MI; ++i)
        acc[i] = x6::mfma6(term_parts(st + (i * 32 + lr) * RLB + (g * 2 + lh) * 48), bp, acc[i]);
    }
  };
  auto adc = [&]() {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        S[i][r] += adc_code(acc[i][r], P.inv_step, P.qmax);
        acc[i][r] = 0.0f;
      }
  };
  pipeline(smem, STAGE_T, tile_span(z, P), P.spt, gload, compute, lstore, adc);

  ip_store(S, P, P.split > 1 ? P.part + (int64_t)z * P.M * P.N : nullptr, m0, n0 + kw, lh);
}

// The bit-serial read-out: the DAC code c of every activation is
// streamed one magnitude bit per cycle, plane j holding u_j = sign(c) *
// ((|c| >> j) & 1) in {-1, 0, +1}; the ADC converts every plane's column sum of
// every crossbar tile on its own and a shift-and-add combines the codes:
//   S[m][n] = sum_t sum_j 2^j q_{t,j}[m][n] (int32),  y = float(S) * out_scale + bias.
// A plane is one exact bf16 term, so a product with a weight is three MFMAs
// (u * w_l, u * w_m, u * w_h), and one split weight fragment serves every plane.
//
// Activations.  k_xbar_pack_codes writes the 16-bit sign-magnitude code (bit 15
// the sign, bits 0..14 |c|) of every activation, in the LDS image of a K-step:
// [row tile][K-step of 32][bm rows][80 B], a row = four 16-byte units (group g,
// half h: the 8 codes k = 16 h + 8 g + j) + 16 B pad (5 units: conflict-free
// ds_read_b128).  No plane exists in memory: a lane forms plane j of its 8
// codes in registers from the one 16-byte read.
//
// Work split.  A workgroup (4 waves) owns 32 MI rows x 128 columns for a range
// of whole crossbar tiles and one chunk of up to PC planes; wave w owns all
// rows x columns 32 w .. 32 w + 31: MI blocks, each with PC fp32 sets (one per
// plane of the chunk) and one int32 set S.  At a tile boundary the ADC runs on
// every plane's set in registers, the code shifted by the plane index goes to
// S and the sets are cleared.  <PC 7, MI 2> serves up to 7 planes in one pass
// (dac_bits <= 8), <PC 4, MI 2> up to 4 planes in half the registers (MI 4
// spills: DESIGN §7.6); more than 7 planes are cut into chunks of 7, a further factor of
// the grid beside the K splits (the sum is an integer, so chunks combine like
// splits: slabs [chunk][split][M][N] and k_xbar_finish).  The weight staging
// and the two-stage pipeline are k_ip_xbar's.
constexpr int CRB = 64 + 16;  // code row bytes per K-step

template <int MI_>
struct Bs {
  static constexpr int BM = 32 * MI_;
  static constexpr int A_B = BM * CRB;  // code bytes per K-step and row tile
  static constexpr int A_U = A_B / 16;
  static constexpr int A_LD = (A_U + 255) / 256;
  static constexpr int STAGE = A_B + B_B;
};

// The host plans both InnerProduct read-outs in a BsPlan (make_ip_plan); for
// the parallel one chunks = 1, bm = 128, planes and pc stay 0 and mean
// nothing, and only its Plan part reaches k_ip_xbar.
struct BsPlan : Plan {  // bit-serial: Core::step is out_scale = step * xs
  int planes;           // dac_bits - 1
  int pc, chunks;       // planes per chunk, ceil(planes / pc)
  int bm;               // rows of a workgroup tile
};

// x [M][K] fp32 -> 16-bit sign-magnitude DAC codes clamp(rint(x / xs), +-cmax)
// in the K-step slabs k_ip_xbar_bs copies to LDS (zero past M and K, zero
// pad).  One thread per unit: 8 activations in, 16 bytes out.
template <bool VEC>
__global__ void __launch_bounds__(256) k_xbar_pack_codes(const float* __restrict__ x, int M, int K,
                                                         char* __restrict__ out, int ksteps, int bm, int64_t units,
                                                         float xs, float cmax) {
  for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
    float v[8];
    const PackUnit U = pack_unit<VEC>(u, x, M, K, ksteps, out, bm, CRB, v);
    uint32_t cw[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      uint32_t c2[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const float c = __builtin_amdgcn_fmed3f(__builtin_rintf(v[2 * p + e] / xs), -cmax, cmax);
        c2[e] = static_cast<uint32_t>(__builtin_fabsf(c)) | (c < 0.0f ? 0x8000u : 0u);
      }
      cw[p] = c2[0] | c2[1] << 16;
    }
    *reinterpret_cast<uint4*>(U.row + (U.g * 2 + U.h) * 16) = make_uint4(cw[0], cw[1], cw[2], cw[3]);
    if (U.g == 1 && U.h == 1) *reinterpret_cast<uint4*>(U.row + 64) = make_uint4(0, 0, 0, 0);
  }
}

template <bool VEC, int PC, int MI_>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) k_ip_xbar_bs(BsPlan P) {
  typedef Bs<MI_> T;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) char smem[2 * T::STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63, lr = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int id = xcd_tile_id(blockIdx.x, gridDim.x);
  const int tm = __builtin_amdgcn_readfirstlane(id % P.tiles_m);
  const int tn = __builtin_amdgcn_readfirstlane((id / P.tiles_m) % P.tiles_n);
  const int zc = __builtin_amdgcn_readfirstlane(id / (P.tiles_m * P.tiles_n));  // chunk * split + z: the slab
  const int z = zc % P.split;
  const int j0 = (zc / P.split) * PC;          // the chunk's first plane
  const int np = min(PC, P.planes - j0);       // ... and how many it has
  const int m0 = tm * T::BM, n0 = tn * BN;

  // this thread's pieces of a K-step: A_LD 16-byte units of the codes, copied as
  // they lie (as in k_ip_xbar, and why it is written twice: there), and the
  // weight stager's quads
  const char* asrc = P.apack + (int64_t)tm * P.ksteps * T::A_B + tid * 16;
  uint4 ra[T::A_LD];
  WStage<VEC> ws(P.w + (int64_t)n0 * P.K, P.N - n0, P.K, T::A_B, tid);
  auto gload = [&](int s) {
    const char* a = asrc + (int64_t)s * T::A_B;
#pragma unroll
    for (int i = 0; i < T::A_LD; ++i)
      if (tid + 256 * i < T::A_U) ra[i] = *reinterpret_cast<const uint4*>(a + 4096 * i);
    ws.load(s);
  };
  auto lstore = [&](char* st) {
#pragma unroll
    for (int i = 0; i < T::A_LD; ++i)
      if (tid + 256 * i < T::A_U) *reinterpret_cast<uint4*>(st + tid * 16 + 4096 * i) = ra[i];
    ws.store(st);
  };

  // a cleared set comes out of the matrix pipe (0 * 0 + 0, the addend an inline
  // constant): zeros written as vector registers would be copied in set by set,
  // PC * MI * 16 more registers live at every tile boundary
  auto zero_set = [&]() {
    const x6::bf16x8 z = __builtin_bit_cast(x6::bf16x8, u32x4{0u, 0u, 0u, 0u});
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(z, z, floatx16{}, 0, 0, 0);
  };
  floatx16 acc[MI_][PC];  // the current crossbar tile's partial sums, one set per plane
  int32_t S[MI_][16];     // the shift-and-add of the ADC codes
#pragma unroll
  for (int i = 0; i < MI_; ++i) {
#pragma unroll
    for (int j = 0; j < PC; ++j) acc[i][j] = zero_set();
#pragma unroll
    for (int r = 0; r < 16; ++r) S[i][r] = 0;
  }

  const int nw = 32 * wave + lr;  // this lane's weight row (output column) inside the tile
  auto compute = [&](const char* st) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const x6::Parts wp = wfrag(st + T::A_B, nw, lh, g);
#pragma unroll
      for (int i = 0; i < MI_; ++i) {
        // 8 codes as 4 packed pairs; plane j of a pair is bit j of each half as the
        // bf16 1.0 (0x3F80 = (1 << 14) - (1 << 7)) under the pair's sign bits
        const u32x4 cw = *reinterpret_cast<const u32x4*>(st + (i * 32 + lr) * CRB + (g * 2 + lh) * 16);
        const u32x4 sg = cw & 0x80008000u;
#pragma unroll
        for (int j = 0; j < PC; ++j)
          if (j < np) {
            const u32x4 bits = (cw >> static_cast<uint32_t>(j0 + j)) & 0x00010001u;
            const x6::bf16x8 u = __builtin_bit_cast(x6::bf16x8, ((bits << 14) - (bits << 7)) | sg);
            floatx16 c = acc[i][j];
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u, wp.l, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u, wp.m, c, 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(u, wp.h, c, 0, 0, 0);
          }
      }
    }
  };
  // the ADC at a tile boundary, per plane: codes shifted by the plane index into S, the sets cleared
  auto adc = [&]() {
#pragma unroll
    for (int i = 0; i < MI_; ++i)
#pragma unroll
      for (int j = 0; j < PC; ++j) {
        // every set of the pass is converted (a plane past np has stayed 0 and adds
        // 0): per-plane branches here make the sets merge values, copied out all at once
#pragma unroll
        for (int r = 0; r < 16; ++r) S[i][r] += adc_code(acc[i][j][r], P.inv_step, P.qmax) * (1 << (j0 + j));
        acc[i][j] = zero_set();
      }
  };
  pipeline(smem, T::STAGE, tile_span(z, P), P.spt, gload, compute, lstore, adc);

  ip_store(S, P, P.split * P.chunks > 1 ? P.part + (int64_t)zc * P.M * P.N : nullptr, m0, n0 + nw, lh);
}

// The bit-sliced-weight read-out: a cell stores cb bits, the
// code d of a weight is spread over Ns columns, slice s holding d_s = sign(d) *
// ((|d| >> s cb) & (2^cb - 1)); the ADC converts every slice's column sum of
// every crossbar tile on its own and a shift-and-add combines the codes:
//   S[m][n] = sum_t sum_s q_{t,s}[m][n] << (s cb) (int32),  y = float(S) * out_scale + bias.
// The activations are their DAC codes c (dac_bits <= 8), so both operands are
// int8 and a tile's column sum is an exact int32 on v_mfma_i32_32x32x32_i8: one
// MFMA per product and K-step of 32, no split, no term order.
//
// Operands.  Lane (lr, lh) of either MFMA operand holds 16 bytes: the codes
// k = 16 lh + j, j = 0 .. 15, of its row (which k of the step the matrix pipe
// pairs with which does not matter as long as both operands agree, and a
// tile's sum does not depend on the order).  k_xbar_pack_i8 writes the
// activation codes as the LDS image of a K-step: [row tile][K-step][64 rows]
// [48 B], a row = its two 16-byte halves + 16 B pad (3 units: coprime with the
// 16 units of an LDS bank row, conflict-free ds_read_b128).  k_xbar_pack_wslices
// reads the weights once per forward as fp32 and writes the Ns slice planes:
// [column tile][K-step][slice][128 rows][32 B], the half h of row n at unit
// h ^ ((n >> 3) & 1) (wslice_lds: 16 consecutive rows then cover the 16 bank
// units once, without a pad, so a plane costs one byte per weight).  The
// slices of a chunk lie next to each other, so a stage's weight fill is one
// run of np * 4096 bytes.
//
// Work split.  A workgroup (4 waves) owns 64 rows x 128 columns for a range of
// whole crossbar tiles and one chunk of up to PC slices; wave w owns all rows
// x columns 32 w .. 32 w + 31: two 32 x 32 blocks, each with PC int32 sets
// (one per slice of the chunk) and the int32 set S.  One activation fragment
// serves all PC slices, one slice fragment both row blocks; the K loop has no
// VALU work on operands.  The ADC at a tile boundary: convert, multiply by kf,
// round, clamp, convert, shift-add by s cb into S; the sets are cleared through
// the matrix pipe (zero_set, as in k_ip_xbar_bs).  More than PC slices are
// chunks, a grid factor combined like K splits.  Both operands are copied as
// they lie through registers into two LDS stages (pipeline).
constexpr int QRB = 32 + 16;  // int8 code row bytes per K-step
struct Wsl {
  static constexpr int MI = 2, BM = 32 * MI;
  static constexpr int A_B = BM * QRB;   // code bytes per K-step and row tile
  static constexpr int A_U = A_B / 16;   // ... in 16-byte units, below the 256 threads
  static constexpr int P_B = BN * KS;    // bytes of one slice plane per K-step and column tile
  static_assert(A_U <= 256 && P_B == 256 * 16, "one unit per thread");
};

struct WsPlan : Plan {  // Core::step is out_scale; Plan::w is not read by the read-out kernel
  const char* wplanes;  // the slice planes (the head of the caller's workspace)
  int ns, cb;           // slices of a weight, bits of a cell
  int chunks;           // ceil(ns / PC)
  float kf;             // partial sum -> ADC steps
};

// x [M][K] fp32 -> two's-complement int8 DAC codes clamp(rint(x / xs), +-cmax)
// in the K-step slabs k_ip_xbar_ws copies to LDS (zero past M and K, zero pad).
// One thread per unit: 8 activations in, 8 bytes out.
template <bool VEC>
__global__ void __launch_bounds__(256) k_xbar_pack_i8(const float* __restrict__ x, int M, int K, char* __restrict__ out,
                                                      int ksteps, int64_t units, float xs, float cmax) {
  for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
    float v[8];
    const PackUnit U = pack_unit<VEC>(u, x, M, K, ksteps, out, Wsl::BM, QRB, v);
    uint32_t cw[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = static_cast<int>(__builtin_amdgcn_fmed3f(__builtin_rintf(v[j] / xs), -cmax, cmax));
      cw[j >> 2] |= (static_cast<uint32_t>(c) & 0xFFu) << (8 * (j & 3));
    }
    *reinterpret_cast<uint2*>(U.row + U.h * 16 + U.g * 8) = make_uint2(cw[0], cw[1]);
    if (U.g == 1 && U.h == 1) *reinterpret_cast<uint4*>(U.row + 32) = make_uint4(0, 0, 0, 0);
  }
}

// where half h (16 k) of weight row `row` lies in a slice plane [128 rows][32 B]:
// k_xbar_pack_wslices writes through this and k_ip_xbar_ws reads through it
__device__ __forceinline__ int wslice_lds(int row, int h) { return row * KS + ((h ^ ((row >> 3) & 1)) << 4); }

// w [N][K] fp32 -> codes d = clamp(rint(w / ws), +-dmax) -> the ns sign-magnitude
// slices of cb bits as int8 planes [column tile][K-step][slice][128 rows][32 B]
// (zero past N and K).  One thread per unit: 8 weights in, 8 bytes out per slice.
template <bool VEC>
__global__ void __launch_bounds__(256) k_xbar_pack_wslices(const float* __restrict__ w, int N, int K,
                                                           char* __restrict__ out, int ksteps, int64_t units, float ws,
                                                           float dmax, int ns, int cb) {
  const int mask = (1 << cb) - 1;
  for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
    float v[8];
    const PackUnit U = pack_unit<VEC>(u, w, N, K, ksteps, out, BN, KS, v);
    int mag[8];
    bool neg[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = __builtin_amdgcn_fmed3f(__builtin_rintf(v[j] / ws), -dmax, dmax);
      mag[j] = static_cast<int>(__builtin_fabsf(d));
      neg[j] = d < 0.0f;
    }
    char* dst = out + U.slab * ns * Wsl::P_B + wslice_lds(U.r, U.h) + U.g * 8;
    for (int s = 0; s < ns; ++s) {
      uint32_t dw[2] = {0u, 0u};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int m = (mag[j] >> (s * cb)) & mask;
        dw[j >> 2] |= (static_cast<uint32_t>(neg[j] ? -m : m) & 0xFFu) << (8 * (j & 3));
      }
      *reinterpret_cast<uint2*>(dst + s * Wsl::P_B) = make_uint2(dw[0], dw[1]);
    }
  }
}

template <int PC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) k_ip_xbar_ws(WsPlan P) {
  typedef Wsl T;
  typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
  typedef int32_t i32x16 __attribute__((ext_vector_type(16)));
  constexpr int STAGE_B = T::A_B + PC * T::P_B;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_B];
  const int tid = threadIdx.x;
  const int lane = tid & 63, lr = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int id = xcd_tile_id(blockIdx.x, gridDim.x);
  const int tm = __builtin_amdgcn_readfirstlane(id % P.tiles_m);
  const int tn = __builtin_amdgcn_readfirstlane((id / P.tiles_m) % P.tiles_n);
  const int zc = __builtin_amdgcn_readfirstlane(id / (P.tiles_m * P.tiles_n));  // chunk * split + z: the slab
  const int z = zc % P.split;
  const int j0 = (zc / P.split) * PC;      // the chunk's first slice
  const int np = min(PC, P.ns - j0);       // ... and how many it has
  const int m0 = tm * T::BM, n0 = tn * BN;

  // this thread's pieces of a K-step, copied as they lie: one 16-byte unit of the
  // codes (the first A_U threads) and one of each of the chunk's np slice planes
  const char* asrc = P.apack + (int64_t)tm * P.ksteps * T::A_B + tid * 16;
  const char* bsrc = P.wplanes + ((int64_t)tn * P.ksteps * P.ns + j0) * T::P_B + tid * 16;
  uint4 ra, rb[PC];
  auto gload = [&](int s) {
    if (tid < T::A_U) ra = *reinterpret_cast<const uint4*>(asrc + (int64_t)s * T::A_B);
#pragma unroll
    for (int j = 0; j < PC; ++j)
      if (j < np) rb[j] = *reinterpret_cast<const uint4*>(bsrc + ((int64_t)s * P.ns + j) * T::P_B);
  };
  auto lstore = [&](char* st) {
    if (tid < T::A_U) *reinterpret_cast<uint4*>(st + tid * 16) = ra;
#pragma unroll
    for (int j = 0; j < PC; ++j)
      if (j < np) *reinterpret_cast<uint4*>(st + T::A_B + j * T::P_B + tid * 16) = rb[j];
  };

  // a cleared set comes out of the matrix pipe (0 * 0 + 0, the addend an inline
  // constant), as in k_ip_xbar_bs: no zeros are written as vector registers
  auto zero_set = [&]() {
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(i32x4{0, 0, 0, 0}, i32x4{0, 0, 0, 0}, i32x16{}, 0, 0, 0);
  };
  i32x16 acc[T::MI][PC];  // the current crossbar tile's column sums, one set per slice
  int32_t S[T::MI][16];   // the shift-and-add of the ADC codes
#pragma unroll
  for (int i = 0; i < T::MI; ++i) {
#pragma unroll
    for (int j = 0; j < PC; ++j) acc[i][j] = zero_set();
#pragma unroll
    for (int r = 0; r < 16; ++r) S[i][r] = 0;
  }

  const int nw = 32 * wave + lr;  // this lane's weight row (output column) inside the tile
  const int boff = T::A_B + wslice_lds(nw, lh);
  auto compute = [&](const char* st) {
    i32x4 a[T::MI];
#pragma unroll
    for (int i = 0; i < T::MI; ++i) a[i] = *reinterpret_cast<const i32x4*>(st + (i * 32 + lr) * QRB + lh * 16);
#pragma unroll
    for (int j = 0; j < PC; ++j)
      if (j < np) {
        const i32x4 b = *reinterpret_cast<const i32x4*>(st + boff + j * T::P_B);
#pragma unroll
        for (int i = 0; i < T::MI; ++i) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b, acc[i][j], 0, 0, 0);
      }
  };
  // the ADC at a tile boundary, per slice: codes shifted by the slice's position into S, the sets cleared
  // (every set of the pass is converted; a slice past np has stayed 0 and adds 0)
  auto adc = [&]() {
#pragma unroll
    for (int i = 0; i < T::MI; ++i)
#pragma unroll
      for (int j = 0; j < PC; ++j) {
        const int sh = (j0 + j) * P.cb;
#pragma unroll
        for (int r = 0; r < 16; ++r) S[i][r] += adc_code(static_cast<float>(acc[i][j][r]), P.kf, P.qmax) * (1 << sh);
        acc[i][j] = zero_set();
      }
  };
  pipeline(smem, STAGE_B, tile_span(z, P), P.spt, gload, compute, lstore, adc);

  ip_store(S, P, P.split * P.chunks > 1 ? P.part + (int64_t)zc * P.M * P.N : nullptr, m0, n0 + nw, lh);
}

// The digit-serial read-out of the bit-sliced array: the input
// code c is streamed db bits per cycle, digit j holding c_j = sign(c) *
// ((|c| >> j db) & (2^db - 1)), against the weight slices d_s of §7.7; the ADC
// converts the column sum of every (digit, slice) pair of every crossbar tile
// on its own and a shift-and-add combines the codes:
//   S[m][n] = sum_t sum_j sum_s q_{t,j,s}[m][n] << (j db + s cb) (int32).
// Both operands of a pair are int8, so its column sum is one exact int32 MFMA
// per K-step, Nd Ns of them per product.
//
// Activations.  k_xbar_pack_sm8 writes the sign-magnitude byte of every code
// (bit 7 the sign, bits 0..6 |c|) in k_xbar_pack_i8's LDS image on 32-row
// tiles.  No digit exists in memory: a lane forms digit j of its 16 codes in
// registers from the one 16-byte fragment, four bytes to a word.  With the
// sign bits s (0x80 per negative byte) taken off, d = (mag >> j db) & mask has
// at most 7 bits per byte (the mask of the top digit stops at bit 6, so that no
// bit of the next byte comes in), and the two's-complement byte of -d is
//   ((d ^ 0x7F) + 1) ^ 0x80:  127 - d + 1 = 128 - d in [1, 128] never carries
// out of its byte, and flipping bit 7 makes it 256 - d mod 256, 0 for d = 0
// (~d + 1 carries into the next byte exactly there).  Under the byte's sign:
//   a = ((d ^ m7) + s1) ^ s,  s1 = s >> 7, m7 = s - s1 (0x7F per negative byte),
// three operations per word and digit after the shift and the mask.
//
// Work split.  A workgroup (4 waves) owns 32 rows x 128 columns for a range of
// whole crossbar tiles and one chunk of up to PD digits x PS slices; wave w
// owns columns 32 w .. 32 w + 31: one 32 x 32 block with PD PS int32 sets (one
// per pair) and the int32 set S.  Per K-step a lane reads one activation
// fragment and PS slice fragments and issues PD PS MFMAs: one digit fragment
// serves every slice, one slice fragment every digit.  The ADC, the clearing
// through the matrix pipe, the stage copies and the pipeline are
// k_ip_xbar_ws's.  Digit chunks and slice chunks are grid factors combined
// like K splits: slabs [slice chunk][digit chunk][split][M][N], k_xbar_finish.
struct Ssl {
  static constexpr int BM = 32;
  static constexpr int A_B = BM * QRB;  // code bytes per K-step and row tile
  static constexpr int A_U = A_B / 16;  // ... in 16-byte units, below the 256 threads
  static_assert(A_U <= 256, "one unit per thread");
};

struct SsPlan : WsPlan {  // WsPlan::chunks = cd * cs
  int nd, db;             // digits of an input code, bits of a digit
  int pd;                 // digits per chunk: which instantiation (host only)
  int cd, cs;             // digit chunks ceil(nd / PD), slice chunks ceil(ns / PS)
};

// x [M][K] fp32 -> sign-magnitude int8 DAC codes (bit 7: c < 0, bits 0..6: |c|,
// c = clamp(rint(x / xs), +-cmax)) in the K-step slabs k_ip_xbar_ss copies to
// LDS (zero past M and K, zero pad).  One thread per unit: 8 activations in, 8
// bytes out.
template <bool VEC>
__global__ void __launch_bounds__(256) k_xbar_pack_sm8(const float* __restrict__ x, int M, int K,
                                                       char* __restrict__ out, int ksteps, int64_t units, float xs,
                                                       float cmax) {
  for (int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; u < units; u += (int64_t)gridDim.x * blockDim.x) {
    float v[8];
    const PackUnit U = pack_unit<VEC>(u, x, M, K, ksteps, out, Ssl::BM, QRB, v);
    uint32_t cw[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float c = __builtin_amdgcn_fmed3f(__builtin_rintf(v[j] / xs), -cmax, cmax);
      cw[j >> 2] |= (static_cast<uint32_t>(__builtin_fabsf(c)) | (c < 0.0f ? 0x80u : 0u)) << (8 * (j & 3));
    }
    *reinterpret_cast<uint2*>(U.row + U.h * 16 + U.g * 8) = make_uint2(cw[0], cw[1]);
    if (U.g == 1 && U.h == 1) *reinterpret_cast<uint4*>(U.row + 32) = make_uint4(0, 0, 0, 0);
  }
}

template <int PD, int PS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) k_ip_xbar_ss(SsPlan P) {
  typedef Ssl T;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
  typedef int32_t i32x16 __attribute__((ext_vector_type(16)));
  constexpr int STAGE_B = T::A_B + PS * Wsl::P_B;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_B];
  const int tid = threadIdx.x;
  const int lane = tid & 63, lr = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int id = xcd_tile_id(blockIdx.x, gridDim.x);
  const int tm = __builtin_amdgcn_readfirstlane(id % P.tiles_m);
  const int tn = __builtin_amdgcn_readfirstlane((id / P.tiles_m) % P.tiles_n);
  const int zc = __builtin_amdgcn_readfirstlane(id / (P.tiles_m * P.tiles_n));  // chunk * split + z: the slab
  const int z = zc % P.split, ch = zc / P.split;
  const int jd0 = (ch % P.cd) * PD, js0 = (ch / P.cd) * PS;  // the chunk's first digit and slice
  const int npd = min(PD, P.nd - jd0), nps = min(PS, P.ns - js0);  // ... and how many it has
  const int m0 = tm * T::BM, n0 = tn * BN;

  // this thread's pieces of a K-step, copied as they lie: one 16-byte unit of the
  // codes (the first A_U threads) and one of each of the chunk's nps slice planes
  const char* asrc = P.apack + (int64_t)tm * P.ksteps * T::A_B + tid * 16;
  const char* bsrc = P.wplanes + ((int64_t)tn * P.ksteps * P.ns + js0) * Wsl::P_B + tid * 16;
  uint4 ra, rb[PS];
  auto gload = [&](int s) {
    if (tid < T::A_U) ra = *reinterpret_cast<const uint4*>(asrc + (int64_t)s * T::A_B);
#pragma unroll
    for (int j = 0; j < PS; ++j)
      if (j < nps) rb[j] = *reinterpret_cast<const uint4*>(bsrc + ((int64_t)s * P.ns + j) * Wsl::P_B);
  };
  auto lstore = [&](char* st) {
    if (tid < T::A_U) *reinterpret_cast<uint4*>(st + tid * 16) = ra;
#pragma unroll
    for (int j = 0; j < PS; ++j)
      if (j < nps) *reinterpret_cast<uint4*>(st + T::A_B + j * Wsl::P_B + tid * 16) = rb[j];
  };

  // a cleared set comes out of the matrix pipe, as in k_ip_xbar_bs and k_ip_xbar_ws
  auto zero_set = [&]() {
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(i32x4{0, 0, 0, 0}, i32x4{0, 0, 0, 0}, i32x16{}, 0, 0, 0);
  };
  i32x16 acc[PD][PS];  // the current crossbar tile's column sums, one set per (digit, slice) pair
  int32_t S[1][16];    // the shift-and-add of the ADC codes
#pragma unroll
  for (int jd = 0; jd < PD; ++jd)
#pragma unroll
    for (int js = 0; js < PS; ++js) acc[jd][js] = zero_set();
#pragma unroll
  for (int r = 0; r < 16; ++r) S[0][r] = 0;

  // digit jd of the chunk: its shift and its per-byte mask, which stops at bit 6
  uint32_t dsh[PD], dmk[PD];
#pragma unroll
  for (int jd = 0; jd < PD; ++jd) {
    dsh[jd] = static_cast<uint32_t>(min((jd0 + jd) * P.db, 6));
    dmk[jd] = ((1u << min(P.db, 7 - static_cast<int>(dsh[jd]))) - 1u) * 0x01010101u;
  }

  const int nw = 32 * wave + lr;  // this lane's weight row (output column) inside the tile
  const int aoff = lr * QRB + lh * 16, boff = T::A_B + wslice_lds(nw, lh);
  auto compute = [&](const char* st) {
    const u32x4 cw = *reinterpret_cast<const u32x4*>(st + aoff);
    const u32x4 sg = cw & 0x80808080u, s1 = sg >> 7u, m7 = sg - s1, mag = cw ^ sg;
    i32x4 b[PS];
#pragma unroll
    for (int js = 0; js < PS; ++js)
      if (js < nps) b[js] = *reinterpret_cast<const i32x4*>(st + boff + js * Wsl::P_B);
#pragma unroll
    for (int jd = 0; jd < PD; ++jd)
      if (jd < npd) {
        const u32x4 d = (mag >> dsh[jd]) & dmk[jd];
        const i32x4 a = __builtin_bit_cast(i32x4, ((d ^ m7) + s1) ^ sg);
#pragma unroll
        for (int js = 0; js < PS; ++js)
          if (js < nps) acc[jd][js] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[js], acc[jd][js], 0, 0, 0);
      }
  };
  // the ADC at a tile boundary, per pair: codes shifted by the pair's position into S, the sets cleared
  // (every set of the pass is converted; a pair past the chunk's counts has stayed 0 and adds 0)
  auto adc = [&]() {
#pragma unroll
    for (int jd = 0; jd < PD; ++jd)
#pragma unroll
      for (int js = 0; js < PS; ++js) {
        const int sh = ((jd0 + jd) * P.db + (js0 + js) * P.cb) & 31;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          S[0][r] += adc_code(static_cast<float>(acc[jd][js][r]), P.kf, P.qmax) * (1 << sh);
        acc[jd][js] = zero_set();
      }
  };
  pipeline(smem, STAGE_B, tile_span(z, P), P.spt, gload, compute, lstore, adc);

  ip_store(S, P, P.split * P.chunks > 1 ? P.part + (int64_t)zc * P.M * P.N : nullptr, m0, n0 + nw, lh);
}

// The crossbar-tiled Convolution forward.  The array of group g
// has the unrolled kernel as its rows, k = (ci * kh + i) * kw + j (the row order
// of Caffe's im2col and of the weight blob), Kg = C/group * kh * kw of them,
// against the group's output channels; crossbar tile t holds rows [t R, (t + 1) R),
// the last may be short, and a tile boundary falls wherever t R falls in that
// order.  There is no im2col buffer: the gather is the LDS fill.
//
// Roles.  An output position is a flattened (n, oh, ow), so a tile of 128
// positions runs across rows and images.  The positions are the MFMA column
// operand and the output channels the row operand (k_ip_xbar's roles swapped):
// a lane of the 32 x 32 accumulator then holds one position and 16 channels,
// and a store instruction writes 32 consecutive positions (consecutive ow) of
// a channel plane.  With k_ip_xbar's roles the lanes would run along the
// channels, a stride of Ho * Wo floats between lanes.
//
// Work split.  A workgroup (4 waves) owns 128 positions x 128 output channels
// of one group for a range of whole crossbar tiles.  Wave v owns channels
// 32 v .. 32 v + 31 for all 128 positions: four 32 x 32 blocks, each with the
// fp32 set of the current tile and the int32 set S, the ADC in registers at
// the tile boundary as in k_ip_xbar.
//
// Staging, per K-step of 32 k.  Thread (p = tid & 127, h = tid >> 7) gathers
// the 16 values k = 32 s + 16 h .. + 15 of position p straight from x: k is
// decomposed into (ci, i, j) once (FastDiv) and advanced incrementally, a
// padding tap, a position past M and k past Kg are zeros by predicate (the
// load then reads the group's first element, never an out-of-range address).
// Consecutive lanes take consecutive positions, so a stride-1 row is one
// coalesced request.  When the loads have landed (after the MFMAs of the
// current step) the thread applies the DAC, splits each run of 8 once and
// writes the two 48-byte term groups (MFMA group g = 0, 1, lane half h) of
// k_ip_xbar's 208-byte row.  The weights of the group are the [Cout/group][Kg]
// matrix k_ip_xbar streams: fp32 from HBM, split after the LDS read.
//
// What is shared with k_ip_xbar here: tile_span, wfrag, term_parts, adc_code and
// wquad_lds.  The weight staging, the accumulator clear / ADC loops and the
// single-level K loop are this kernel's own text: through WStage the <vec>
// kernel spills 5 scalar registers instead of 3, and through shared functions
// over acc / S or the two-level pipeline it compiles to 255 VGPRs + 84 AGPRs or
// measured up to 1.5 % slower (profiles/xbar_refactor.txt).  As written the
// kernel's ISA is the same as before the pieces were shared.
//
// ConvPlan has Core's members by name, in the order it always had (the order
// of the kernel's arguments is part of that ISA), so tile_span, plan_core and
// launch_finish are templates over the plan.
struct ConvPlan {
  const float* x;
  const float* w;
  const float* bias;
  float* y;
  int32_t* part;       // int32 slabs [split][num][Cout][Ho][Wo] (split > 1)
  int H, W, KH, KW, ph, pw, sh, sw, dh, dw, Wo;
  int HW, HoWo;
  int Cin, Cout;       // all groups
  int Cg, Ng;          // input / output channels of one group
  int M, Kg;           // positions num * Ho * Wo, rows of one group's array
  FastDiv khkw, kw_div, howo, wo_div;
  int tiles_p, tiles_c, groups;
  int ksteps, spt, ntiles, tc, split;
  int64_t total;       // num * Cout * Ho * Wo
  float step, inv_step, qmax, dac_xs, dac_qmax;
  int relu;
};

template <bool VEC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) k_conv_xbar(ConvPlan P) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63, lr = lane & 31, lh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  int id = xcd_tile_id(blockIdx.x, gridDim.x);
  const int tp = __builtin_amdgcn_readfirstlane(id % P.tiles_p);
  id /= P.tiles_p;
  const int tn = __builtin_amdgcn_readfirstlane(id % P.tiles_c);
  id /= P.tiles_c;
  const int grp = __builtin_amdgcn_readfirstlane(id % P.groups);
  const int z = __builtin_amdgcn_readfirstlane(id / P.groups);
  const int p0 = tp * BM, c0 = tn * BN;
  const Span ks = tile_span(z, P);
  const int s0 = ks.s0, s1 = ks.s1;

  // the gather: this thread's position and its corner (oh sh - ph, ow sw - pw)
  const int gp = tid & (BM - 1), gh = tid >> 7;
  const bool pvalid = p0 + gp < P.M;
  const uint32_t gpos = pvalid ? static_cast<uint32_t>(p0 + gp) : 0u;
  const uint32_t gn = fdiv(gpos, P.howo), gsp = gpos - gn * P.HoWo;
  const uint32_t goh = fdiv(gsp, P.wo_div), gow = gsp - goh * P.Wo;
  const int hb = static_cast<int>(goh) * P.sh - P.ph, wb = static_cast<int>(gow) * P.sw - P.pw;
  const float* xg = P.x + ((int64_t)gn * P.Cin + (int64_t)grp * P.Cg) * P.HW;  // image gn, first channel of the group
  const int corner = hb * P.W + wb;
  const int row_step = P.dh * P.W - P.KW * P.dw;        // offset step from tap (i, kw) to (i + 1, 0)
  const int chan_step = P.HW - P.KH * P.dh * P.W;       // ... from tap (kh, 0) of ci to (0, 0) of ci + 1

  // the weights: B_LD quads (row, 4 k) of the group's [Ng][Kg] matrix.  This is
  // WStage's text (and must agree with wquad_lds), kept here: through WStage
  // k_conv_xbar<vec> spills 5 scalar registers instead of 3.
  const float* bsrc[B_LD];
  int bq[B_LD], blds[B_LD];
#pragma unroll
  for (int i = 0; i < B_LD; ++i) {
    const int idx = tid + 256 * i, row = idx >> 3, q = idx & 7;
    bsrc[i] = c0 + row < P.Ng ? P.w + ((int64_t)grp * P.Ng + c0 + row) * P.Kg + 4 * q : nullptr;
    bq[i] = 4 * q;
    blds[i] = A_B + wquad_lds(row, q);
  }
  float rx[16];
  float4 rb[B_LD];
  auto gload = [&](int s) {
    const int k0 = s * KS + 16 * gh;
    const uint32_t ci = fdiv(static_cast<uint32_t>(k0), P.khkw), rem = static_cast<uint32_t>(k0) - ci * P.khkw.d;
    int ki = static_cast<int>(fdiv(rem, P.kw_div));
    int kj = static_cast<int>(rem) - ki * P.KW;
    int ih = hb + ki * P.dh, iw = wb + kj * P.dw;
    int off = static_cast<int>(ci) * P.HW + ki * P.dh * P.W + kj * P.dw;  // of tap (ci, ki, kj) from the corner
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const bool ok = pvalid && k0 + u < P.Kg && static_cast<uint32_t>(ih) < static_cast<uint32_t>(P.H) &&
                      static_cast<uint32_t>(iw) < static_cast<uint32_t>(P.W);
      const float v = xg[ok ? corner + off : 0];
      rx[u] = ok ? v : 0.0f;
      ++kj, iw += P.dw, off += P.dw;
      if (kj == P.KW) {
        kj = 0, iw = wb, ++ki, ih += P.dh, off += row_step;
        if (ki == P.KH) ki = 0, ih = hb, off += chan_step;
      }
    }
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
      const int k = s * KS + bq[i];
      float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (bsrc[i] != nullptr) {
        const float* p = bsrc[i] + s * KS;
        if (VEC) {  // Kg % 4 == 0, w 16-byte aligned
          if (k < P.Kg) f = *reinterpret_cast<const float4*>(p);
        } else {
          if (k < P.Kg) f.x = p[0];
          if (k + 1 < P.Kg) f.y = p[1];
          if (k + 2 < P.Kg) f.z = p[2];
          if (k + 3 < P.Kg) f.w = p[3];
        }
      }
      rb[i] = f;
    }
  };
  auto lstore = [&](char* st) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = rx[8 * g + j];
      dac8(v, P.dac_xs, P.dac_qmax);
      x6::store_terms8(v, st + gp * RLB + (g * 2 + gh) * 48);
    }
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

  const int nw = 32 * wave + lr;  // this lane's weight row (output channel) inside the tile
  auto compute = [&](const char* st) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const x6::Parts wp = wfrag(st + A_B, nw, lh, g);
#pragma unroll
      for (int i = 0; i < MI; ++i)  // rows = channels, columns = positions
        acc[i] = x6::mfma6(wp, term_parts(st + (i * 32 + lr) * RLB + (g * 2 + lh) * 48), acc[i]);
    }
  };
  auto adc = [&]() {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        S[i][r] += adc_code(acc[i][r], P.inv_step, P.qmax);
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

  // lane (lr, lh) holds position 32 i + lr, channels 32 wave + 8 (r >> 2) + 4 lh + (r & 3)
  int32_t* part = P.split > 1 ? P.part + (int64_t)z * P.total : nullptr;
  const float* bias = P.bias != nullptr ? P.bias + grp * P.Ng : nullptr;
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int pos = p0 + 32 * i + lr;
    if (pos >= P.M) continue;
    const uint32_t n = fdiv(static_cast<uint32_t>(pos), P.howo), sp = static_cast<uint32_t>(pos) - n * P.HoWo;
    const int64_t base = ((int64_t)n * P.Cout + (int64_t)grp * P.Ng) * P.HoWo + sp;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = c0 + 32 * wave + 8 * (r >> 2) + 4 * lh + (r & 3);
      if (co >= P.Ng) continue;
      const int64_t o = base + (int64_t)co * P.HoWo;
      if (part != nullptr)
        part[o] = S[i][r];
      else
        P.y[o] = xbar_out(S[i][r], P.step, bias, co, P.relu);
    }
  }
}

// y = the read-out of the summed int32 slabs [split][M][N][inner] (inner = 1:
// InnerProduct; Ho * Wo: a convolution's NCHW output with M = num, N = Cout)
__global__ void __launch_bounds__(256) k_xbar_finish(const int32_t* __restrict__ part, int split, int M, int N,
                                                     int inner, float step, const float* __restrict__ bias, int relu,
                                                     float* __restrict__ y) {
  const int64_t total = (int64_t)M * N * inner;
  for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int32_t S = 0;
    for (int z = 0; z < split; ++z) S += part[z * total + idx];
    y[idx] = xbar_out(S, step, bias, static_cast<int>((idx / inner) % N), relu);
  }
}

// The configuration's checks (host only) and the plan of a shape.
int check_cfg(const rram_xbar_cfg* c, const char* who) {
  RRAM_REQUIRE(c != nullptr, "%s: cfg is NULL", who);
  RRAM_REQUIRE(c->rows >= 32 && c->rows <= 1024 && c->rows % 32 == 0,
               "%s: rows %d not a multiple of 32 in [32, 1024]", who, c->rows);
  RRAM_REQUIRE(c->adc_bits >= 2 && c->adc_bits <= 16, "%s: adc_bits %d outside [2, 16]", who, c->adc_bits);
  RRAM_REQUIRE(std::isfinite(c->adc_range) && c->adc_range > 0.0f, "%s: adc_range must be finite and > 0", who);
  RRAM_REQUIRE(c->dac_bits == 0 || (c->dac_bits >= 2 && c->dac_bits <= 16),
               "%s: dac_bits %d neither 0 nor in [2, 16]", who, c->dac_bits);
  RRAM_REQUIRE(c->dac_bits == 0 || (std::isfinite(c->dac_range) && c->dac_range > 0.0f),
               "%s: dac_range must be finite and > 0", who);
  return RRAM_OK;
}

int check(int M, int N, int K, const rram_xbar_cfg* c, int transpose) {
  RRAM_REQUIRE(c != nullptr, "ip_fwd_xbar: cfg is NULL");
  RRAM_REQUIRE(M >= 0 && N >= 0 && K >= 1, "ip_fwd_xbar: bad shape %d x %d x %d", M, N, K);
  RRAM_REQUIRE(!transpose, "ip_fwd_xbar: transposed weights are not served");
  const int rc = check_cfg(c, "ip_fwd_xbar");
  if (rc) return rc;
  RRAM_REQUIRE((int64_t)M * N < (1ll << 31), "ip_fwd_xbar: more than 2^31 outputs");
  return RRAM_OK;
}

// ADC step and DAC step of a configuration: computed in double, cast to float
struct Steps {
  float step, inv_step, qmax, dac_xs, dac_qmax;  // dac_qmax = 0: no DAC
};
Steps steps_of(const rram_xbar_cfg& c) {
  Steps r{};
  const int qmax = (1 << (c.adc_bits - 1)) - 1;
  const double step = static_cast<double>(c.adc_range) / qmax;
  r.step = static_cast<float>(step);
  r.inv_step = static_cast<float>(1.0 / step);
  r.qmax = static_cast<float>(qmax);
  r.dac_xs = 1.0f;
  if (c.dac_bits > 0) {
    r.dac_qmax = static_cast<float>((1 << (c.dac_bits - 1)) - 1);
    r.dac_xs = static_cast<float>(static_cast<double>(c.dac_range) / r.dac_qmax);
  }
  return r;
}

// splits of ntiles crossbar tiles: split_k = 0 toward 256 workgroups from
// `tiles` output tiles with slabs of slab_bytes inside ws_bytes, else the
// caller's split clamped to the tile count; whole tiles per split
void plan_split(int ntiles, int64_t tiles, size_t slab_bytes, int split_k, size_t ws_bytes, int& tc, int& split) {
  int s = split_k;
  if (split_k <= 0) {
    s = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(64, 256 / tiles)));
    while (s > 1 && (size_t)s * slab_bytes > ws_bytes) --s;
  }
  s = std::max(1, std::min(s, ntiles));
  tc = (ntiles + s - 1) / s;
  split = (ntiles + tc - 1) / tc;
}

// The core of a plan over K array rows: `tiles` workgroups per split, each
// split writing slab_bytes when there is more than one (plan_split), the ADC
// of the configuration.  The operands are the entry point's to fill.
template <class PlanT>
void plan_core(PlanT& P, int K, const rram_xbar_cfg& c, int64_t tiles, size_t slab_bytes, int split_k,
               size_t ws_bytes) {
  P.ksteps = (K + KS - 1) / KS;
  P.spt = c.rows / KS;
  P.ntiles = (K + c.rows - 1) / c.rows;
  plan_split(P.ntiles, tiles, slab_bytes, split_k, ws_bytes, P.tc, P.split);
  const Steps st = steps_of(c);
  P.step = st.step, P.inv_step = st.inv_step, P.qmax = st.qmax;
}

// the workspace of `slabs` int32 slabs of `outputs` each: none for one slab, which is y
size_t part_bytes(int slabs, int64_t outputs) { return slabs > 1 ? (size_t)slabs * outputs * sizeof(int32_t) : 0; }

// The bit-serial read-out's checks (host only).  The DAC is mandatory, and S
// (so every partial slab too) must fit int32: |S| <= ntiles * qmax * cmax.
int bs_check(int M, int N, int K, const rram_xbar_cfg* c, int transpose) {
  const int rc = check(M, N, K, c, transpose);
  if (rc) return rc;
  RRAM_REQUIRE(c->dac_bits != 0, "ip_fwd_xbar_bs: bit-serial inputs need a DAC (dac_bits in [2, 16])");
  const int64_t ntiles = (K + c->rows - 1) / c->rows;
  const int64_t qmax = (1 << (c->adc_bits - 1)) - 1, cmax = (1 << (c->dac_bits - 1)) - 1;
  RRAM_REQUIRE(ntiles * qmax * cmax < (1ll << 31), "ip_fwd_xbar_bs: %lld tiles x qmax %lld x cmax %lld overflows int32",
               (long long)ntiles, (long long)qmax, (long long)cmax);
  return RRAM_OK;
}

// The plan of either InnerProduct read-out; the parallel one is a BsPlan of one
// chunk on 128-row tiles whose Plan part goes to k_ip_xbar.  Bit-serial: up to
// 4 planes on <PC 4, MI 2>, else chunks of 7 planes on <PC 7, MI 2> (both
// 64-row tiles).  The chunk count is folded into the planner's workgroup count
// and slab size, so a multi-chunk problem asks for fewer K splits.
// split_k = 0: toward 256 workgroups, whole tiles, partials within ws_bytes;
// else the caller's split clamped to the tile count.
void make_ip_plan(int M, int N, int K, const rram_xbar_cfg& c, bool serial, int split_k, size_t ws_bytes, BsPlan& P) {
  P = BsPlan{};
  P.M = M, P.N = N, P.K = K;
  P.chunks = 1;
  P.bm = BM;
  if (serial) {
    P.planes = c.dac_bits - 1;
    P.pc = P.planes <= 4 ? 4 : 7;
    P.chunks = (P.planes + P.pc - 1) / P.pc;
    P.bm = Bs<2>::BM;
  }
  P.tiles_m = (M + P.bm - 1) / P.bm;
  P.tiles_n = (N + BN - 1) / BN;
  plan_core(P, K, c, (int64_t)P.tiles_m * P.tiles_n * P.chunks, (size_t)M * N * sizeof(int32_t) * P.chunks, split_k,
            ws_bytes);
  if (serial) {  // out_scale
    const Steps st = steps_of(c);
    P.step = static_cast<float>(static_cast<double>(c.adc_range) / st.qmax *
                                (static_cast<double>(c.dac_range) / st.dac_qmax));
  }
}

// The convolution's checks (host only; d gets its output shape) and plan.
int conv_check(rram_conv_desc& d, const rram_xbar_cfg* c, int split_k) {
  const int rc0 = check_cfg(c, "conv2d_fwd_xbar");
  if (rc0) return rc0;
  const int rc = rram_conv_out_shape(&d);
  if (rc) return rc;
  RRAM_REQUIRE(d.num >= 0, "conv2d_fwd_xbar: negative num");
  RRAM_REQUIRE(split_k >= 0, "conv2d_fwd_xbar: negative split_k");
  RRAM_REQUIRE((int64_t)d.num * d.num_output * d.out_h * d.out_w < (1ll << 31), "conv2d_fwd_xbar: more than 2^31 outputs");
  RRAM_REQUIRE((int64_t)d.channels * d.height * d.width < (1ll << 30) &&
                   (int64_t)d.channels / d.group * d.kernel_h * d.kernel_w < (1ll << 30),
               "conv2d_fwd_xbar: an image or a kernel of 2^30 elements or more");
  return RRAM_OK;
}

void make_conv_plan(const rram_conv_desc& d, const rram_xbar_cfg& c, int split_k, size_t ws_bytes, ConvPlan& P) {
  P = ConvPlan{};
  P.H = d.height, P.W = d.width, P.KH = d.kernel_h, P.KW = d.kernel_w;
  P.ph = d.pad_h, P.pw = d.pad_w, P.sh = d.stride_h, P.sw = d.stride_w, P.dh = d.dilation_h, P.dw = d.dilation_w;
  P.Wo = d.out_w;
  P.HW = d.height * d.width, P.HoWo = d.out_h * d.out_w;
  P.Cin = d.channels, P.Cout = d.num_output, P.groups = d.group;
  P.Cg = d.channels / d.group, P.Ng = d.num_output / d.group;
  P.M = d.num * P.HoWo;
  P.Kg = P.Cg * d.kernel_h * d.kernel_w;
  P.khkw = make_fastdiv(static_cast<uint32_t>(d.kernel_h * d.kernel_w));
  P.kw_div = make_fastdiv(static_cast<uint32_t>(d.kernel_w));
  P.howo = make_fastdiv(static_cast<uint32_t>(P.HoWo));
  P.wo_div = make_fastdiv(static_cast<uint32_t>(d.out_w));
  P.tiles_p = (P.M + BM - 1) / BM;
  P.tiles_c = (P.Ng + BN - 1) / BN;
  P.total = (int64_t)d.num * d.num_output * P.HoWo;
  plan_core(P, P.Kg, c, (int64_t)P.tiles_p * P.tiles_c * P.groups, (size_t)P.total * sizeof(int32_t), split_k,
            ws_bytes);
  const Steps st = steps_of(c);
  P.dac_xs = st.dac_xs, P.dac_qmax = st.dac_qmax;
}

// The pieces every entry point ends with or passes through.

// whether an operand with rows of K floats takes the 16-byte loads
bool al16(const void* p, int K) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0 && K % 4 == 0; }

// f(std::true_type) or f(std::false_type): a kernel's VEC instantiation chosen at run time
template <class F>
void by_vec(bool vec, F f) {
  if (vec)
    f(std::true_type{});
  else
    f(std::false_type{});
}

// the caller's workspace must hold the `need` bytes of the plan's slabs; tail: what multiplies the splits
int require_ws(const char* who, const void* ws, size_t ws_bytes, size_t need, int split, int chunks) {
  if (need == 0 || (ws != nullptr && ws_bytes >= need)) return RRAM_OK;
  RRAM_REQUIRE(chunks == 0, "%s: workspace of %zu bytes below the %zu of %d splits x %d plane chunks", who, ws_bytes,
               need, split, chunks);
  RRAM_REQUIRE(false, "%s: workspace of %zu bytes below the %zu of %d splits", who, ws_bytes, need, split);
  return RRAM_OK;
}

// the slabs summed into y [M][N][inner], unless y was written by the one slab's epilogue
template <class PlanT>
int launch_finish(const char* what, const PlanT& P, int slabs, int M, int N, int inner, hipStream_t s) {
  if (slabs == 1 || plan_note("xbar:finish")) return RRAM_OK;
  hipLaunchKernelGGL(xb::k_xbar_finish, dim3(stream_blocks((int64_t)M * N * inner)), dim3(256), 0, s, P.part, slabs, M,
                     N, inner, P.step, P.bias, P.relu, P.y);
  return launch_status(what);
}

// an operand for the host-only id queries: never dereferenced, only its alignment is read
float* fake_ptr(int align16) { return reinterpret_cast<float*>(uintptr_t{1} << 20 | (align16 ? 0u : 4u)); }

size_t ip_workspace(bool serial, int M, int N, int K, const rram_xbar_cfg* cfg, int split_k) {
  if ((serial ? bs_check(M, N, K, cfg, 0) : check(M, N, K, cfg, 0)) != RRAM_OK || M == 0 || N == 0 || split_k < 0)
    return 0;
  BsPlan P;
  make_ip_plan(M, N, K, *cfg, serial, split_k, ~static_cast<size_t>(0), P);
  return part_bytes(P.split * P.chunks, (int64_t)M * N);
}

// rram_ip_fwd_xbar and, with serial, rram_ip_fwd_xbar_bs: the checks, the plan
// and the pack kernel, the read-out kernel and its id differ, the rest is one
int ip_fwd(bool serial, const float* x, const float* w, const float* bias, float* y, int M, int N, int K,
           int transpose, const rram_xbar_cfg* cfg, int relu, int split_k, void* ws, size_t ws_bytes,
           rram_stream_t st) {
  const char* who = serial ? "ip_fwd_xbar_bs" : "ip_fwd_xbar";
  const int rc0 = serial ? bs_check(M, N, K, cfg, transpose) : check(M, N, K, cfg, transpose);
  if (rc0) return rc0;
  RRAM_REQUIRE(split_k >= 0, "%s: negative split_k", who);
  if (M == 0 || N == 0) return RRAM_OK;
  RRAM_REQUIRE(x && w && y, "%s: NULL", who);
  BsPlan P;
  make_ip_plan(M, N, K, *cfg, serial, split_k, ws != nullptr ? ws_bytes : 0, P);
  const int slabs = P.split * P.chunks;
  const int rcw = require_ws(who, ws, ws_bytes, part_bytes(slabs, (int64_t)M * N), P.split, serial ? P.chunks : 0);
  if (rcw) return rcw;
  RRAM_REQUIRE((int64_t)P.tiles_m * P.tiles_n * slabs < (1ll << 31), "%s: grid too large", who);
  hipStream_t s = as_stream(st);
  const bool xv = al16(x, K), wv = al16(w, K);

  const Steps dac = steps_of(*cfg);
  if (!plan_note(serial ? "xbar:pack_codes<%s>" : "xbar:pack<%s>", xv ? "vec" : "scalar")) {
    const int64_t pack_b = (int64_t)P.tiles_m * P.ksteps * P.bm * (serial ? CRB : RLB);
    char* pb = reinterpret_cast<char*>(pack_buffer(static_cast<size_t>(pack_b / 4), s));
    RRAM_REQUIRE(pb != nullptr, "%s: packed-%s buffer allocation failed", who, serial ? "code" : "activation");
    P.apack = pb;
    const int64_t units = (int64_t)P.tiles_m * P.bm * P.ksteps * 4;
    const dim3 grid(stream_blocks(units));
    by_vec(xv, [&](auto V) {
      if (serial)
        hipLaunchKernelGGL(k_xbar_pack_codes<decltype(V)::value>, grid, dim3(256), 0, s, x, M, K, pb, P.ksteps, P.bm,
                           units, dac.dac_xs, dac.dac_qmax);
      else
        hipLaunchKernelGGL(k_xbar_pack<decltype(V)::value>, grid, dim3(256), 0, s, x, M, K, pb, P.ksteps, units,
                           dac.dac_xs, dac.dac_qmax);
    });
    const int rc = launch_status(serial ? "ip_fwd_xbar_bs pack" : "ip_fwd_xbar pack");
    if (rc) return rc;
  }
  P.w = w;
  P.bias = bias;
  P.y = y;
  P.part = slabs > 1 ? static_cast<int32_t*>(ws) : nullptr;
  P.relu = relu;
  const char* wl = wv ? "vec" : "scalar";
  if (!(serial ? plan_note("xbar:ip_bs<%s;p%d>/s%d/c%d", wl, P.pc, P.split, P.chunks)
               : plan_note("xbar:ip<%s>/s%d", wl, P.split))) {
    const dim3 grid(static_cast<unsigned>(P.tiles_m * P.tiles_n * slabs));
    by_vec(wv, [&](auto V) {
      constexpr bool VEC = decltype(V)::value;
      if (!serial)
        hipLaunchKernelGGL(k_ip_xbar<VEC>, grid, dim3(256), 0, s, static_cast<const Plan&>(P));
      else if (P.pc == 4)
        hipLaunchKernelGGL((k_ip_xbar_bs<VEC, 4, 2>), grid, dim3(256), 0, s, P);
      else
        hipLaunchKernelGGL((k_ip_xbar_bs<VEC, 7, 2>), grid, dim3(256), 0, s, P);
    });
    const int rc = launch_status(who);
    if (rc) return rc;
  }
  return launch_finish(serial ? "ip_fwd_xbar_bs finish" : "ip_fwd_xbar finish", P, slabs, M, N, 1, s);
}

// The transposed read-out's checks (host only): cfg->rows is the number of array
// columns C one read sums over, N the reduction length, K the output count.
int bwd_check(int M, int N, int K, const rram_xbar_cfg* c, int split_k) {
  const char* who = "ip_bwd_data_xbar";
  RRAM_REQUIRE(M >= 0 && N >= 1 && K >= 0, "%s: bad shape %d x %d x %d", who, M, N, K);
  const int rc = check_cfg(c, who);
  if (rc) return rc;
  RRAM_REQUIRE(split_k >= 0, "%s: negative split_k", who);
  const int64_t ntiles = (N + c->rows - 1) / c->rows, qmax = (1 << (c->adc_bits - 1)) - 1;
  RRAM_REQUIRE(ntiles * qmax < (1ll << 31), "%s: %lld tiles x qmax %lld overflows int32", who, (long long)ntiles,
               (long long)qmax);
  RRAM_REQUIRE((int64_t)M * K < (1ll << 31), "%s: more than 2^31 outputs", who);
  return RRAM_OK;
}

// the kernel's Plan: N is the output count (the caller's K), K the reduction length (the caller's N)
void make_bwd_plan(int M, int N, int K, const rram_xbar_cfg& c, int split_k, size_t ws_bytes, Plan& P) {
  P = Plan{};
  P.M = M, P.N = K, P.K = N;
  P.tiles_m = (M + BM - 1) / BM;
  P.tiles_n = (K + BN - 1) / BN;
  plan_core(P, N, c, (int64_t)P.tiles_m * P.tiles_n, (size_t)M * K * sizeof(int32_t), split_k, ws_bytes);
}

int bwd_data(const float* dy, const float* w, float* dx, int M, int N, int K, const rram_xbar_cfg* cfg, int split_k,
             void* ws, size_t ws_bytes, rram_stream_t st) {
  const char* who = "ip_bwd_data_xbar";
  const int rc0 = bwd_check(M, N, K, cfg, split_k);
  if (rc0) return rc0;
  if (M == 0 || K == 0) return RRAM_OK;
  RRAM_REQUIRE(dy && w && dx, "%s: NULL", who);
  Plan P;
  make_bwd_plan(M, N, K, *cfg, split_k, ws != nullptr ? ws_bytes : 0, P);
  const int rcw = require_ws(who, ws, ws_bytes, part_bytes(P.split, (int64_t)M * K), P.split, 0);
  if (rcw) return rcw;
  RRAM_REQUIRE((int64_t)P.tiles_m * P.tiles_n * P.split < (1ll << 31), "%s: grid too large", who);
  hipStream_t s = as_stream(st);
  const bool yv = al16(dy, N), wv = al16(w, K);

  if (!plan_note("xbar:pack<%s>", yv ? "vec" : "scalar")) {  // dy through the forward's pack, N as its K
    const Steps dac = steps_of(*cfg);
    const int64_t pack_b = (int64_t)P.tiles_m * P.ksteps * A_B;
    char* pb = reinterpret_cast<char*>(pack_buffer(static_cast<size_t>(pack_b / 4), s));
    RRAM_REQUIRE(pb != nullptr, "%s: packed-gradient buffer allocation failed", who);
    P.apack = pb;
    const int64_t units = (int64_t)P.tiles_m * BM * P.ksteps * 4;
    by_vec(yv, [&](auto V) {
      hipLaunchKernelGGL(k_xbar_pack<decltype(V)::value>, dim3(stream_blocks(units)), dim3(256), 0, s, dy, M, N, pb,
                         P.ksteps, units, dac.dac_xs, dac.dac_qmax);
    });
    const int rc = launch_status("ip_bwd_data_xbar pack");
    if (rc) return rc;
  }
  P.w = w;
  P.y = dx;
  P.part = P.split > 1 ? static_cast<int32_t*>(ws) : nullptr;
  if (!plan_note("xbar:ip_t<%s>/s%d", wv ? "vec" : "scalar", P.split)) {
    const dim3 grid(static_cast<unsigned>(P.tiles_m * P.tiles_n * P.split));
    by_vec(wv, [&](auto V) { hipLaunchKernelGGL(k_ip_xbar_t<decltype(V)::value>, grid, dim3(256), 0, s, P); });
    const int rc = launch_status(who);
    if (rc) return rc;
  }
  return launch_finish("ip_bwd_data_xbar finish", P, P.split, M, K, 1, s);
}

// The bit-sliced-weight read-outs' checks (host only): rram_ip_fwd_xbar_ws and,
// with serial, the digit-serial rram_ip_fwd_xbar_ss of db bits per digit.  Both
// operands must fit int8, and S (so every partial slab too) int32:
// |S| <= ntiles * qmax * sum_s 2^(s cb) (* sum_j 2^(j db)).
constexpr int WS_PC = 4;             // slices per chunk: the one k_ip_xbar_ws instantiation
constexpr int SS_PS = 4;             // slices per chunk of k_ip_xbar_ss<PD 3 | 2, PS 4>
int slices_of(const rram_xbar_slices& sl) { return (sl.weight_bits - 1 + sl.cell_bits - 1) / sl.cell_bits; }
const char* ws_who(bool serial) { return serial ? "ip_fwd_xbar_ss" : "ip_fwd_xbar_ws"; }

int ws_check(bool serial, int M, int N, int K, const rram_xbar_cfg* c, const rram_xbar_slices* sl, int db,
             int transpose) {
  const char* who = ws_who(serial);
  const int rc = check(M, N, K, c, transpose);
  if (rc) return rc;
  RRAM_REQUIRE(c->dac_bits >= 2 && c->dac_bits <= 8, "%s: dac_bits %d outside [2, 8]", who, c->dac_bits);
  RRAM_REQUIRE(sl != nullptr, "%s: slices is NULL", who);
  RRAM_REQUIRE(sl->weight_bits >= 2 && sl->weight_bits <= 8, "%s: weight_bits %d outside [2, 8]", who,
               sl->weight_bits);
  RRAM_REQUIRE(sl->cell_bits >= 1 && sl->cell_bits <= sl->weight_bits - 1,
               "%s: cell_bits %d outside [1, weight_bits - 1]", who, sl->cell_bits);
  RRAM_REQUIRE(std::isfinite(sl->weight_range) && sl->weight_range > 0.0f,
               "%s: weight_range must be finite and > 0", who);
  const int64_t ntiles = (K + c->rows - 1) / c->rows, qmax = (1 << (c->adc_bits - 1)) - 1;
  int64_t weight = 0;
  for (int s = 0; s < slices_of(*sl); ++s) weight += 1ll << (s * sl->cell_bits);
  if (!serial) {
    RRAM_REQUIRE(ntiles * qmax * weight < (1ll << 31), "%s: %lld tiles x qmax %lld x slice weights %lld overflows int32",
                 who, (long long)ntiles, (long long)qmax, (long long)weight);
    return RRAM_OK;
  }
  RRAM_REQUIRE(db >= 1 && db <= c->dac_bits - 1, "%s: digit_bits %d outside [1, dac_bits - 1]", who, db);
  int64_t digit = 0;
  for (int j = 0; j * db < c->dac_bits - 1; ++j) digit += 1ll << (j * db);
  RRAM_REQUIRE(ntiles * qmax * digit * weight < (1ll << 31),
               "%s: %lld tiles x qmax %lld x digit weights %lld x slice weights %lld overflows int32", who,
               (long long)ntiles, (long long)qmax, (long long)digit, (long long)weight);
  return RRAM_OK;
}

// The plan of a shape; ws_bytes is the caller's whole workspace, of which the
// slice planes take plane_bytes first and the planner's slabs the rest.  The
// chunk count is folded into the planner's workgroup count and slab size.
// serial: digits of db bits on k_ip_xbar_ss's 32-row tiles, chunks on both axes
// (3 digits x 4 slices, or 2 x 4 where that takes no more chunks: 1, 2 and 4 digits).
size_t make_ws_plan(bool serial, int M, int N, int K, const rram_xbar_cfg& c, const rram_xbar_slices& sl, int db,
                    int split_k, size_t ws_bytes, SsPlan& P) {
  P = SsPlan{};
  P.M = M, P.N = N, P.K = K;
  P.ns = slices_of(sl), P.cb = sl.cell_bits;
  P.chunks = (P.ns + WS_PC - 1) / WS_PC;
  if (serial) {
    P.db = db, P.nd = (c.dac_bits - 1 + db - 1) / db;
    P.pd = (P.nd + 2) / 3 < (P.nd + 1) / 2 ? 3 : 2;  // the fewer digit chunks, a tie to the fewer idle sets
    P.cd = (P.nd + P.pd - 1) / P.pd, P.cs = (P.ns + SS_PS - 1) / SS_PS;
    P.chunks = P.cd * P.cs;
  }
  const int bm = serial ? Ssl::BM : Wsl::BM;
  P.tiles_m = (M + bm - 1) / bm;
  P.tiles_n = (N + BN - 1) / BN;
  const size_t plane_bytes = (size_t)P.tiles_n * ((K + KS - 1) / KS) * P.ns * Wsl::P_B;
  plan_core(P, K, c, (int64_t)P.tiles_m * P.tiles_n * P.chunks, (size_t)M * N * sizeof(int32_t) * P.chunks, split_k,
            ws_bytes > plane_bytes ? ws_bytes - plane_bytes : 0);
  const double cmax = (1 << (c.dac_bits - 1)) - 1, dmax = (1 << (sl.weight_bits - 1)) - 1;
  P.kf = static_cast<float>(static_cast<double>(c.dac_range) / cmax * (static_cast<double>(sl.weight_range) / dmax) /
                            (static_cast<double>(c.adc_range) / P.qmax));
  return plane_bytes;
}

size_t ws_workspace(bool serial, int M, int N, int K, const rram_xbar_cfg* cfg, const rram_xbar_slices* sl, int db,
                    int split_k) {
  if (ws_check(serial, M, N, K, cfg, sl, db, 0) != RRAM_OK || M == 0 || N == 0 || split_k < 0) return 0;
  SsPlan P;
  const size_t plane_bytes = make_ws_plan(serial, M, N, K, *cfg, *sl, db, split_k, ~static_cast<size_t>(0), P);
  return plane_bytes + part_bytes(P.split * P.chunks, (int64_t)M * N);
}

// rram_ip_fwd_xbar_ws and, with serial, rram_ip_fwd_xbar_ss: the checks, the
// plan, the activation pack, the read-out kernel and its id differ, the rest
// (the weight pack among it) is one
int ws_fwd(bool serial, const float* x, const float* w, const float* bias, float* y, int M, int N, int K,
           int transpose, const rram_xbar_cfg* cfg, const rram_xbar_slices* sl, int db, int relu, int split_k, void* ws,
           size_t ws_bytes, rram_stream_t st) {
  const char* who = ws_who(serial);
  const int rc0 = ws_check(serial, M, N, K, cfg, sl, db, transpose);
  if (rc0) return rc0;
  RRAM_REQUIRE(split_k >= 0, "%s: negative split_k", who);
  if (M == 0 || N == 0) return RRAM_OK;
  RRAM_REQUIRE(x && w && y, "%s: NULL", who);
  RRAM_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15u) == 0, "%s: workspace not 16-byte aligned", who);
  SsPlan P;
  const size_t plane_bytes = make_ws_plan(serial, M, N, K, *cfg, *sl, db, split_k, ws != nullptr ? ws_bytes : 0, P);
  const int slabs = P.split * P.chunks;
  const int rcw = require_ws(who, ws, ws_bytes, plane_bytes + part_bytes(slabs, (int64_t)M * N), P.split, P.chunks);
  if (rcw) return rcw;
  RRAM_REQUIRE((int64_t)P.tiles_m * P.tiles_n * slabs < (1ll << 31), "%s: grid too large", who);
  hipStream_t s = as_stream(st);
  const Steps dac = steps_of(*cfg);

  if (!plan_note(serial ? "xbar:pack_sm8<%s>" : "xbar:pack_i8<%s>", al16(x, K) ? "vec" : "scalar")) {
    const int bm = serial ? Ssl::BM : Wsl::BM;
    const int64_t pack_b = (int64_t)P.tiles_m * P.ksteps * bm * QRB;
    char* pb = reinterpret_cast<char*>(pack_buffer(static_cast<size_t>(pack_b / 4), s));
    RRAM_REQUIRE(pb != nullptr, "%s: packed-code buffer allocation failed", who);
    P.apack = pb;
    const int64_t units = (int64_t)P.tiles_m * bm * P.ksteps * 4;
    by_vec(al16(x, K), [&](auto V) {
      const auto pack = serial ? k_xbar_pack_sm8<decltype(V)::value> : k_xbar_pack_i8<decltype(V)::value>;
      hipLaunchKernelGGL(pack, dim3(stream_blocks(units)), dim3(256), 0, s, x, M, K, pb, P.ksteps, units, dac.dac_xs,
                         dac.dac_qmax);
    });
    const int rc = launch_status(serial ? "ip_fwd_xbar_ss pack" : "ip_fwd_xbar_ws pack");
    if (rc) return rc;
  }
  P.wplanes = static_cast<const char*>(ws);
  if (!plan_note("xbar:pack_wslices<%s>", al16(w, K) ? "vec" : "scalar")) {
    const float dmax = static_cast<float>((1 << (sl->weight_bits - 1)) - 1);
    const float wsc = static_cast<float>(static_cast<double>(sl->weight_range) / dmax);
    const int64_t units = (int64_t)P.tiles_n * BN * P.ksteps * 4;
    by_vec(al16(w, K), [&](auto V) {
      hipLaunchKernelGGL(k_xbar_pack_wslices<decltype(V)::value>, dim3(stream_blocks(units)), dim3(256), 0, s, w, N, K,
                         static_cast<char*>(ws), P.ksteps, units, wsc, dmax, P.ns, P.cb);
    });
    const int rc = launch_status(serial ? "ip_fwd_xbar_ss weight pack" : "ip_fwd_xbar_ws weight pack");
    if (rc) return rc;
  }
  P.w = w;
  P.bias = bias;
  P.y = y;
  P.part = slabs > 1 ? reinterpret_cast<int32_t*>(static_cast<char*>(ws) + plane_bytes) : nullptr;
  P.relu = relu;
  if (!(serial ? plan_note("xbar:ip_ss<d%d;p%d>/s%d/c%d", P.pd, SS_PS, P.split, P.chunks)
               : plan_note("xbar:ip_ws<p%d>/s%d/c%d", WS_PC, P.split, P.chunks))) {
    const dim3 grid(static_cast<unsigned>(P.tiles_m * P.tiles_n * slabs));
    if (serial && P.pd == 3)
      hipLaunchKernelGGL((k_ip_xbar_ss<3, SS_PS>), grid, dim3(256), 0, s, P);
    else if (serial)
      hipLaunchKernelGGL((k_ip_xbar_ss<2, SS_PS>), grid, dim3(256), 0, s, P);
    else
      hipLaunchKernelGGL(k_ip_xbar_ws<WS_PC>, grid, dim3(256), 0, s, static_cast<const WsPlan&>(P));
    const int rc = launch_status(who);
    if (rc) return rc;
  }
  return launch_finish(serial ? "ip_fwd_xbar_ss finish" : "ip_fwd_xbar_ws finish", P, slabs, M, N, 1, s);
}

}  // namespace xb
}  // namespace
}  // namespace rram

extern "C" {

size_t rram_ip_fwd_xbar_workspace(int M, int N, int K, const rram_xbar_cfg* cfg, int split_k) {
  return rram::xb::ip_workspace(false, M, N, K, cfg, split_k);
}

int rram_ip_fwd_xbar(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, int transpose,
                     const rram_xbar_cfg* cfg, int relu, int split_k, void* ws, size_t ws_bytes, rram_stream_t st) {
  return rram::xb::ip_fwd(false, x, w, bias, y, M, N, K, transpose, cfg, relu, split_k, ws, ws_bytes, st);
}

int rram_ip_fwd_xbar_kernel_ids(int M, int N, int K, const rram_xbar_cfg* cfg, int x_align16, int w_align16,
                                int split_k, size_t ws_bytes, char* out, size_t cap) {
  using rram::xb::fake_ptr;
  rram::PlanScope sc;
  const int rc = rram_ip_fwd_xbar(fake_ptr(x_align16), fake_ptr(w_align16), nullptr, fake_ptr(1), M, N, K, 0, cfg, 0,
                                  split_k, ws_bytes ? fake_ptr(1) : nullptr, ws_bytes, nullptr);
  return rc ? rc : rram::copy_text(sc.text, out, cap);
}

size_t rram_ip_fwd_xbar_bs_workspace(int M, int N, int K, const rram_xbar_cfg* cfg, int split_k) {
  return rram::xb::ip_workspace(true, M, N, K, cfg, split_k);
}

int rram_ip_fwd_xbar_bs(const float* x, const float* w, const float* bias, float* y, int M, int N, int K,
                        int transpose, const rram_xbar_cfg* cfg, int relu, int split_k, void* ws, size_t ws_bytes,
                        rram_stream_t st) {
  return rram::xb::ip_fwd(true, x, w, bias, y, M, N, K, transpose, cfg, relu, split_k, ws, ws_bytes, st);
}

int rram_ip_fwd_xbar_bs_kernel_ids(int M, int N, int K, const rram_xbar_cfg* cfg, int x_align16, int w_align16,
                                   int split_k, size_t ws_bytes, char* out, size_t cap) {
  using rram::xb::fake_ptr;
  rram::PlanScope sc;
  const int rc = rram_ip_fwd_xbar_bs(fake_ptr(x_align16), fake_ptr(w_align16), nullptr, fake_ptr(1), M, N, K, 0, cfg,
                                     0, split_k, ws_bytes ? fake_ptr(1) : nullptr, ws_bytes, nullptr);
  return rc ? rc : rram::copy_text(sc.text, out, cap);
}

size_t rram_ip_fwd_xbar_ws_workspace(int M, int N, int K, const rram_xbar_cfg* cfg, const rram_xbar_slices* slices,
                                     int split_k) {
  return rram::xb::ws_workspace(false, M, N, K, cfg, slices, 0, split_k);
}

int rram_ip_fwd_xbar_ws(const float* x, const float* w, const float* bias, float* y, int M, int N, int K,
                        int transpose, const rram_xbar_cfg* cfg, const rram_xbar_slices* slices, int relu,
                        int split_k, void* ws, size_t ws_bytes, rram_stream_t st) {
  return rram::xb::ws_fwd(false, x, w, bias, y, M, N, K, transpose, cfg, slices, 0, relu, split_k, ws, ws_bytes,
                          st);
}

int rram_ip_fwd_xbar_ws_kernel_ids(int M, int N, int K, const rram_xbar_cfg* cfg, const rram_xbar_slices* slices,
                                   int x_align16, int w_align16, int split_k, size_t ws_bytes, char* out,
                                   size_t cap) {
  using rram::xb::fake_ptr;
  rram::PlanScope sc;
  const int rc = rram_ip_fwd_xbar_ws(fake_ptr(x_align16), fake_ptr(w_align16), nullptr, fake_ptr(1), M, N, K, 0, cfg,
                                     slices, 0, split_k, ws_bytes ? fake_ptr(1) : nullptr, ws_bytes, nullptr);
  return rc ? rc : rram::copy_text(sc.text, out, cap);
}

size_t rram_ip_fwd_xbar_ss_workspace(int M, int N, int K, const rram_xbar_cfg* cfg, const rram_xbar_slices* slices,
                                     int digit_bits, int split_k) {
  return rram::xb::ws_workspace(true, M, N, K, cfg, slices, digit_bits, split_k);
}

int rram_ip_fwd_xbar_ss(const float* x, const float* w, const float* bias, float* y, int M, int N, int K,
                        int transpose, const rram_xbar_cfg* cfg, const rram_xbar_slices* slices, int digit_bits,
                        int relu, int split_k, void* ws, size_t ws_bytes, rram_stream_t st) {
  return rram::xb::ws_fwd(true, x, w, bias, y, M, N, K, transpose, cfg, slices, digit_bits, relu, split_k, ws,
                          ws_bytes, st);
}

int rram_ip_fwd_xbar_ss_kernel_ids(int M, int N, int K, const rram_xbar_cfg* cfg, const rram_xbar_slices* slices,
                                   int digit_bits, int x_align16, int w_align16, int split_k, size_t ws_bytes,
                                   char* out, size_t cap) {
  using rram::xb::fake_ptr;
  rram::PlanScope sc;
  const int rc = rram_ip_fwd_xbar_ss(fake_ptr(x_align16), fake_ptr(w_align16), nullptr, fake_ptr(1), M, N, K, 0, cfg,
                                     slices, digit_bits, 0, split_k, ws_bytes ? fake_ptr(1) : nullptr, ws_bytes,
                                     nullptr);
  return rc ? rc : rram::copy_text(sc.text, out, cap);
}

size_t rram_ip_bwd_data_xbar_workspace(int M, int N, int K, const rram_xbar_cfg* cfg, int split_k) {
  if (rram::xb::bwd_check(M, N, K, cfg, split_k) != RRAM_OK || M == 0 || K == 0) return 0;
  rram::xb::Plan P;
  rram::xb::make_bwd_plan(M, N, K, *cfg, split_k, ~static_cast<size_t>(0), P);
  return rram::xb::part_bytes(P.split, (int64_t)M * K);
}

int rram_ip_bwd_data_xbar(const float* dy, const float* w, float* dx, int M, int N, int K, const rram_xbar_cfg* cfg,
                          int split_k, void* ws, size_t ws_bytes, rram_stream_t st) {
  return rram::xb::bwd_data(dy, w, dx, M, N, K, cfg, split_k, ws, ws_bytes, st);
}

int rram_ip_bwd_data_xbar_kernel_ids(int M, int N, int K, const rram_xbar_cfg* cfg, int dy_align16, int w_align16,
                                     int split_k, size_t ws_bytes, char* out, size_t cap) {
  using rram::xb::fake_ptr;
  rram::PlanScope sc;
  const int rc = rram_ip_bwd_data_xbar(fake_ptr(dy_align16), fake_ptr(w_align16), fake_ptr(1), M, N, K, cfg, split_k,
                                       ws_bytes ? fake_ptr(1) : nullptr, ws_bytes, nullptr);
  return rc ? rc : rram::copy_text(sc.text, out, cap);
}

size_t rram_conv2d_fwd_xbar_workspace(const rram_conv_desc* d_in, const rram_xbar_cfg* cfg, int split_k) {
  if (d_in == nullptr) return 0;
  rram_conv_desc d = *d_in;
  if (rram::xb::conv_check(d, cfg, split_k) != RRAM_OK || d.num == 0) return 0;
  rram::xb::ConvPlan P;
  rram::xb::make_conv_plan(d, *cfg, split_k, ~static_cast<size_t>(0), P);
  return rram::xb::part_bytes(P.split, P.total);
}

int rram_conv2d_fwd_xbar(const rram_conv_desc* d_in, const float* x, const float* w, const float* bias, float* y,
                         const rram_xbar_cfg* cfg, int relu, int split_k, void* ws, size_t ws_bytes,
                         rram_stream_t st) {
  using namespace rram;
  RRAM_REQUIRE(d_in != nullptr, "conv2d_fwd_xbar: descriptor is NULL");
  rram_conv_desc d = *d_in;
  const int rc0 = xb::conv_check(d, cfg, split_k);
  if (rc0) return rc0;
  if (d.num == 0) return RRAM_OK;
  RRAM_REQUIRE(x && w && y, "conv2d_fwd_xbar: NULL pointer");
  xb::ConvPlan P;
  xb::make_conv_plan(d, *cfg, split_k, ws != nullptr ? ws_bytes : 0, P);
  const int rcw = xb::require_ws("conv2d_fwd_xbar", ws, ws_bytes, xb::part_bytes(P.split, P.total), P.split, 0);
  if (rcw) return rcw;
  const int64_t wgs = (int64_t)P.tiles_p * P.tiles_c * P.groups * P.split;
  RRAM_REQUIRE(wgs < (1ll << 31) && (int64_t)P.tiles_p * xb::BM < (1ll << 31), "conv2d_fwd_xbar: grid too large");
  hipStream_t s = as_stream(st);
  const bool wv = xb::al16(w, P.Kg);
  P.x = x, P.w = w, P.bias = bias, P.y = y;
  P.part = P.split > 1 ? static_cast<int32_t*>(ws) : nullptr;
  P.relu = relu;
  if (!plan_note("xbar:conv<%s>/s%d", wv ? "vec" : "scalar", P.split)) {
    const dim3 grid(static_cast<unsigned>(wgs));
    xb::by_vec(wv, [&](auto V) {
      hipLaunchKernelGGL(xb::k_conv_xbar<decltype(V)::value>, grid, dim3(256), 0, s, P);
    });
    const int rc = launch_status("conv2d_fwd_xbar");
    if (rc) return rc;
  }
  return xb::launch_finish("conv2d_fwd_xbar finish", P, P.split, d.num, d.num_output, P.HoWo, s);
}

int rram_conv2d_fwd_xbar_kernel_ids(const rram_conv_desc* d, const rram_xbar_cfg* cfg, int x_align16, int w_align16,
                                    int split_k, size_t ws_bytes, char* out, size_t cap) {
  using rram::xb::fake_ptr;
  rram::PlanScope sc;
  const int rc = rram_conv2d_fwd_xbar(d, fake_ptr(x_align16), fake_ptr(w_align16), nullptr, fake_ptr(1), cfg, 0,
                                      split_k, ws_bytes ? fake_ptr(1) : nullptr, ws_bytes, nullptr);
  return rc ? rc : rram::copy_text(sc.text, out, cap);
}

// every id a launch site of this file can record, without the /sS and /cC tails
int rram_xbar_kernel_list(char* out, size_t cap) {
  return rram::copy_text(
      "xbar:pack<vec>\nxbar:pack<scalar>\nxbar:pack_codes<vec>\nxbar:pack_codes<scalar>\n"
      "xbar:pack_i8<vec>\nxbar:pack_i8<scalar>\nxbar:pack_sm8<vec>\nxbar:pack_sm8<scalar>\n"
      "xbar:pack_wslices<vec>\nxbar:pack_wslices<scalar>\n"
      "xbar:ip<vec>\nxbar:ip<scalar>\nxbar:ip_t<vec>\nxbar:ip_t<scalar>\n"
      "xbar:ip_bs<vec;p4>\nxbar:ip_bs<scalar;p4>\nxbar:ip_bs<vec;p7>\nxbar:ip_bs<scalar;p7>\n"
      "xbar:ip_ws<p4>\nxbar:ip_ss<d3;p4>\nxbar:ip_ss<d2;p4>\n"
      "xbar:conv<vec>\nxbar:conv<scalar>\nxbar:finish\n",
      out, cap);
}

}  // extern "C"
