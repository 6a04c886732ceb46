// sf_policy_gemm.hpp — the matrix kernels of the policy network (HIP only; sf_policy.hip includes it and launches them):
//   k_gemm<WM, WN, BKT, MODE>  C[M][N] = A[M][K] * W[N][K]^T (+ bias) on the f32 matrix pipe, stream-K runs
//   k_gemm_fixup               finishes the row tiles whose K range a run boundary cut
//   k_gemm_b3<MODE>            the large-M products on the bf16 matrix pipe at f32-level accuracy (hi + mid + lo)
//   k_split_weights            W -> k_gemm_b3's image, on the device (sf_policy_gemm_split)
// and the constants and the argument block (Gemm) that the other policy kernels and the host side share.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/strikeforce_policy.h"

namespace sfp {

constexpr int HID = SF_POLICY_HIDDEN;    // 160
constexpr int ACT = SF_POLICY_ACTIONS;   // 9
constexpr int G3 = 3 * HID;              // 480 gate rows r,z,n
constexpr int OBS_C = SF_OBS_CHANNELS;   // 32
constexpr int OBS_W = SF_OBS_WINDOW;     // 31
constexpr int OBS_F = SF_OBS_FLOATS;     // 30752
constexpr int POV = SF_POLICY_POV;       // 169
constexpr int COMB = 2 * HID + ACT;      // 329 inputs of combined_processor
constexpr int COMB_PAD = 352;            // padded to a multiple of the GEMM's K tiles (16 and 32)

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { MODE_DENSE = 0, MODE_NHWC = 1, MODE_NCHW = 2 };

struct Gemm {
  const float *A;
  const float *W;     // [N][K] row-major
  const float *bias;  // [N] or null
  float *C;           // [M][ldc]
  int M, N, K;        // K % 32 == 0, N % 160 == 0
  int lda, ldc;
  int S, Cin, So;     // convolution modes: input side, input channels, output side
  // work split: the (row tile, K tile) units of one 160-column strip, numbered tile-major, are dealt to the
  // gridDim.x blocks in contiguous runs of unit_base (+1 for the first unit_rem blocks) units
  int ntiles, unit_base, unit_rem;
  float *part;        // [gridDim.y][gridDim.x][2][BM*160] partial tiles of runs that start or end inside a tile
  // an independent second product of the same shape, computed by the blocks with blockIdx.z == 1 (one launch for
  // the two gate products of a GRU cell, or for the same layer of the two heads)
  const float *A2, *W2, *bias2;
  float *C2;
  const void *W3;     // k_gemm_b3: W split into bf16 hi / mid / lo parts (split_weights)
};

constexpr int BN = 160;

__device__ inline f32x4 ldg4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }

__device__ inline int run_start(const Gemm &g, int b) { return b * g.unit_base + (b < g.unit_rem ? b : g.unit_rem); }
__device__ inline int run_owner(const Gemm &g, int u) {
  const int big = g.unit_rem * (g.unit_base + 1);
  return u < big ? u / (g.unit_base + 1) : g.unit_rem + (u - big) / g.unit_base;
}

// Block tile (WM*32) x 160, K tile BKT.  WN = 1: a wave owns 32 rows x 160 columns (5 accumulator tiles; the
// large-M shape).  WN = 5: the five 32-column tiles of the same 32 rows go to five waves (the small-M shape: five
// times the waves for the same work, each with a fifth of the dependent MFMA chain).
//
// A block walks a contiguous run of (row tile, K tile) units ("stream-K"): with one tile per run this is the
// classic one-block-per-tile GEMM; with gridDim.x = the number of resident blocks the chip holds, every block gets
// the same number of MFMAs whatever M is, the global->LDS->MFMA pipeline never drains between row tiles, and a tile
// whose K range is cut by a run boundary is finished by k_gemm_fixup, which adds the partial tiles in K order
// (deterministic: no atomics).
template <int WM, int WN, int BKT, int MODE>
__global__ __launch_bounds__(WM *WN * 64, 2) void k_gemm(Gemm g) {
  if (blockIdx.z) g.A = g.A2, g.W = g.W2, g.bias = g.bias2, g.C = g.C2;
  constexpr int T = WM * WN * 64, BM = WM * 32, LD = BKT + 1;
  constexpr int NT = 5 / WN;                    // 32-column tiles per wave
  constexpr int Q = BKT / 4;                    // float4 per tile row
  constexpr int AJ = (BM * Q + T - 1) / T;      // float4 loads of A per thread
  constexpr int BJ = (BN * Q + T - 1) / T;      // float4 loads of W per thread
  constexpr int SJ = (BM * BKT + T - 1) / T;    // scalar loads of A per thread (NCHW gather)
  constexpr int KS = BKT / 2;                   // 32x32x2 products per tile
  constexpr int GS = KS / 2;                    // groups of two products
  __shared__ float As[2][BM * LD];
  __shared__ float Bs[2][BN * LD];

  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int wm = w / WN, wn = w - wm * WN;
  const int n0 = blockIdx.y * BN;
  const int KT = g.K / BKT;
  const int u0 = run_start(g, blockIdx.x);
  const int nu = g.unit_base + ((int)blockIdx.x < g.unit_rem ? 1 : 0);
  if (nu == 0) return;

  // ---- where this thread's share of an A tile comes from (recomputed when the load cursor enters a new row tile) ----
  const float *arow[AJ];
  // NCHW: consecutive threads walk consecutive rows, one row per thread.  The address is split into a wave-uniform
  // part (the tile's first agent + the (cin, ky, kx) offset of the k being loaded: SALU, lands in the load's saddr)
  // and a 32-bit per-lane part (this row's pixel relative to that agent), so a gathered element costs no VALU.
  const float *abase = nullptr;
  uint32_t avoff = 0;
  auto setrow = [&](int tile) {
    const int m0 = tile * BM;
    if (MODE == MODE_NCHW) {
      int m = m0 + (t % BM);
      if (m >= g.M) m = g.M - 1;
      const int so2 = g.So * g.So;
      const int b0 = m0 / so2;
      const int b = m / so2, r = m - b * so2, oy = r / g.So, ox = r - oy * g.So;
      abase = g.A + (size_t)b0 * g.Cin * g.S * g.S;
      avoff = (uint32_t)(((b - b0) * g.Cin * g.S * g.S + (2 * oy) * g.S + 2 * ox) * 4);
    } else {
#pragma unroll
      for (int j = 0; j < AJ; ++j) {
        const int f = t + j * T;
        int m = m0 + ((f / Q < BM) ? f / Q : BM - 1);
        if (m >= g.M) m = g.M - 1;
        if (MODE == MODE_DENSE) {
          arow[j] = g.A + (size_t)m * g.lda + (f % Q) * 4;
        } else {
          const int so2 = g.So * g.So;
          const int b = m / so2, r = m - b * so2, oy = r / g.So, ox = r - oy * g.So;
          arow[j] = g.A + ((size_t)(b * g.S + 2 * oy) * g.S + 2 * ox) * g.Cin + (f % Q) * 4;
        }
      }
    }
  };
  const float *brow[BJ];
#pragma unroll
  for (int j = 0; j < BJ; ++j) {
    const int f = t + j * T;
    const int n = (f / Q < BN) ? f / Q : BN - 1;
    brow[j] = g.W + (size_t)(n0 + n) * g.K + (f % Q) * 4;
  }

  f32x4 ra[AJ], rb[BJ];
  float rs[SJ];

  auto gload = [&](int kt) {
    const int k0 = kt * BKT;
    if (MODE == MODE_NCHW) {
      const int ss = g.S * g.S;
#pragma unroll
      for (int j = 0; j < SJ; ++j) {
        const int e = t + j * T;
        int kl = (e / BM < BKT) ? e / BM : BKT - 1;
        if (BM % 64 == 0) kl = __builtin_amdgcn_readfirstlane(kl);  // a wave's 64 rows share k
        const int k = k0 + kl;
        const int cin = k / 9, tap = k - cin * 9, ky = tap / 3, kx = tap - ky * 3;
        const char *sb = reinterpret_cast<const char *>(abase + ((size_t)cin * ss + ky * g.S + kx));
        rs[j] = *reinterpret_cast<const float *>(sb + avoff);
      }
    } else {
      int off = k0;
      if (MODE == MODE_NHWC) {
        const int tap = k0 / g.Cin, c0 = k0 - tap * g.Cin, ky = tap / 3, kx = tap - ky * 3;
        off = (ky * g.S + kx) * g.Cin + c0;
      }
#pragma unroll
      for (int j = 0; j < AJ; ++j) ra[j] = ldg4(arow[j] + off);
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j) rb[j] = ldg4(brow[j] + k0);
  };
  auto lstore = [&](int buf) {
    if (MODE == MODE_NCHW) {
#pragma unroll
      for (int j = 0; j < SJ; ++j) {
        const int e = t + j * T;
        if ((BM * BKT) % T == 0 || e < BM * BKT) As[buf][(e % BM) * LD + e / BM] = rs[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < AJ; ++j) {
        const int f = t + j * T;
        if ((BM * Q) % T == 0 || f < BM * Q) {
          float *d = &As[buf][(f / Q) * LD + (f % Q) * 4];
          d[0] = ra[j].x, d[1] = ra[j].y, d[2] = ra[j].z, d[3] = ra[j].w;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
      const int f = t + j * T;
      if ((BN * Q) % T == 0 || f < BN * Q) {
        float *d = &Bs[buf][(f / Q) * LD + (f % Q) * 4];
        d[0] = rb[j].x, d[1] = rb[j].y, d[2] = rb[j].z, d[3] = rb[j].w;
      }
    }
  };

  f32x16 acc[NT];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  };
  // The products are issued transposed (W fragment as the MFMA's A operand, activation fragment as its B operand:
  // the two operand lane maps are the same, so the fragments need no change), which puts the output row m on the
  // lane (m = l&31) and four consecutive output columns n = 8*(reg>>2) + 4*(l>>5) + (reg&3) in consecutive
  // registers: a tile leaves as 4 dwordx4 stores per lane instead of 16 dword stores.
  auto flush = [&](int tile, bool whole, int slot) {
    const int ml = wm * 32 + (l & 31), m = tile * BM + ml;
    float *pt = g.part + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 + slot) * (BM * BN) + ml * BN;
    float *cr = g.C + (size_t)m * g.ldc + n0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int nl = (wn * NT + nt) * 32 + 8 * q + 4 * (l >> 5);
        f32x4 v = {acc[nt][4 * q], acc[nt][4 * q + 1], acc[nt][4 * q + 2], acc[nt][4 * q + 3]};
        if (whole) {
          if (g.bias) v += ldg4(g.bias + n0 + nl);
          if (m < g.M) *reinterpret_cast<f32x4 *>(cr + nl) = v;
        } else {
          *reinterpret_cast<f32x4 *>(pt + nl) = v;
        }
      }
    }
  };

  // Schedule of one unit (the compiler is held to it with sched_barrier): the unit's products run in GS groups of
  // two (k, k+2 -> one ds_read2_b32 per operand); the fragments of group i+1 are read from LDS before the MFMAs of
  // group i issue.  Half-way through, the next unit (in registers since the previous unit) is written to the other
  // LDS buffer and the loads of the unit after it are issued; the block's only barrier comes before the last
  // group, followed by the read of the next unit's first fragments, so both hide behind that group's MFMAs.
  float fa[2][2], fb[2][NT][2];
  auto fload = [&](int buf, int grp, int slot) {
    const float *as = &As[buf][(wm * 32 + (l & 31)) * LD + (l >> 5)];
    const float *bs = &Bs[buf][(wn * NT * 32 + (l & 31)) * LD + (l >> 5)];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      fa[slot][h] = as[4 * grp + 2 * h];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) fb[slot][nt][h] = bs[nt * 32 * LD + 4 * grp + 2 * h];
    }
  };

  // load cursor (two units ahead of the MFMAs) and compute cursor
  int tile_l = u0 / KT, kt_l = u0 - tile_l * KT;
  int tile_c = tile_l, kt_c = kt_l, seg_kt0 = kt_l;
  bool seg_first = true;
  auto load_next = [&]() {
    gload(kt_l);
    if (++kt_l == KT) {
      kt_l = 0;
      ++tile_l;
      if (tile_l < g.ntiles) setrow(tile_l);
    }
  };
  setrow(tile_l);
  load_next();
  lstore(0);
  __syncthreads();
  if (nu > 1) load_next();
  fload(0, 0, 0);
  zero_acc();
  for (int i = 0; i < nu; ++i) {
    const int buf = i & 1;
#pragma unroll
    for (int grp = 0; grp < GS; ++grp) {
      if (grp == GS / 2 && i + 1 < nu) {
        lstore(buf ^ 1);
        if (i + 2 < nu) load_next();
      }
      if (grp + 1 < GS) {
        fload(buf, grp + 1, (grp + 1) & 1);
      } else if (i + 1 < nu) {
        __syncthreads();
        fload(buf ^ 1, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[grp & 1][nt][h], fa[grp & 1][h], acc[nt], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (kt_c == KT - 1 || i == nu - 1) {
      flush(tile_c, seg_kt0 == 0 && kt_c == KT - 1, seg_first ? 0 : 1);
      zero_acc();
      seg_first = false;
      seg_kt0 = 0;
    }
    if (++kt_c == KT) kt_c = 0, ++tile_c;
  }
}

// Finishes the row tiles whose K range was cut by a run boundary: C = bias + the partial tiles in K order.  One
// block per run boundary; the boundary that is the first one inside its tile does the tile.
template <int BM>
__global__ __launch_bounds__(256) void k_gemm_fixup(Gemm g, int KT, int G) {
  const int b_lo = blockIdx.x, n0 = blockIdx.y * BN;
  const int cut = run_start(g, b_lo + 1);  // first unit of the next run
  if (cut % KT == 0) return;               // the boundary coincides with a tile boundary
  const int tile = cut / KT, ua = tile * KT;
  if (run_owner(g, ua) != b_lo) return;    // an earlier boundary inside the same tile owns it
  const int b_hi = run_owner(g, ua + KT - 1);
  const int m0 = tile * BM;
  constexpr int V = BM * BN / 4 / 256;     // float4 per thread
  f32x4 s[V];
#pragma unroll
  for (int j = 0; j < V; ++j) s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int b = b_lo; b <= b_hi; ++b) {
    const int slot = run_start(g, b) >= ua ? 0 : 1;  // a run's first segment is in slot 0, a later one in slot 1
    const float *pt = g.part + (((size_t)blockIdx.y * G + b) * 2 + slot) * (BM * BN);
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] += ldg4(pt + (threadIdx.x + 256 * j) * 4);
  }
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int e = (threadIdx.x + 256 * j) * 4, ml = e / BN, nl = e - ml * BN;
    if (m0 + ml < g.M) {
      f32x4 v = s[j];
      if (g.bias) v += ldg4(g.bias + n0 + nl);
      *reinterpret_cast<f32x4 *>(g.C + (size_t)(m0 + ml) * g.ldc + n0 + nl) = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// k_gemm_b3: the large-M products (conv1, conv2) on the bf16 matrix pipe at f32-level accuracy.
//
// Every f32 operand is written as hi + mid + lo, three bf16 numbers obtained by round-to-nearest of the running
// residual (x - hi and x - hi - mid are exact in f32, so hi + mid + lo == x: 3 x 8 significand bits and two signs cover
// f32's 24).  A product a*w then expands into nine bf16 products; the six of relative size >= 2^-16 are kept
//     hi*hi + (hi*mid + mid*hi) + (mid*mid + hi*lo + lo*hi)
// and the dropped ones (mid*lo, lo*mid, lo*lo) are <= 3 * 2^-24 |a*w|: the order of one f32 rounding of the
// product.  Each kept product is exact in the f32 accumulator (8 x 8 bits), so what differs from the f32 pipe is that
// dropped tail and the summation order.  v_mfma_f32_32x32x16_bf16 retires 16 times the products per cycle of
// v_mfma_f32_32x32x2_f32: six of them instead of eight f32 instructions per 32x32x16 block = 2.67 x fewer
// matrix-pipe cycles.  Non-finite inputs come out as NaN (inf - inf in the residual).
//
// W is split once on the host into the image the LDS wants (one 96-byte record [hi 16][mid 16][lo 16] per (K tile of
// 16, output column)); activations are split as they are stored to LDS (v_cvt_pk_bf16_f32 + shifts, ~5.5 VALU per
// element).  Block tile 256 rows x 160 columns x 16, one block per CU: eight compute waves of 32 rows x 160 columns
// (two per SIMD) and four loader waves, two LDS stages of 39 KB.
// Work split, pipeline and tile hand-over (stream-K runs, k_gemm_fixup) as in k_gemm.
// ---------------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// 8 compute waves (32 rows x 160 columns each, two per SIMD) + 4 loader waves (one per SIMD)
constexpr int B3_CW = 8, B3_LW = 4, B3_BM = 32 * B3_CW, B3_BK = 16, B3_T = 64 * (B3_CW + B3_LW), B3_LT = 64 * B3_LW, B3_RS = 96;
constexpr int B3_A_BYTES = B3_BM * B3_RS, B3_W_BYTES = BN * B3_RS, B3_STAGE = B3_A_BYTES + B3_W_BYTES;
constexpr int B3_LDS = 2 * B3_STAGE;                 // 79 872 bytes
constexpr int B3_W_PIECES = BN * 96 / 16;            // 16-byte pieces of one K tile of the W image: 960
constexpr int B3_SETS = 4;                           // register sets of a loader thread = units in flight from HBM

__device__ inline uint32_t pk_bf16(float a, float b) {
  const bf16x2 h = __builtin_convertvector(f32x2{a, b}, bf16x2);
  return __builtin_bit_cast(uint32_t, h);
}
// four f32 -> their hi / mid / lo bf16 parts, packed in k order
__device__ inline void split3(const f32x4 x, u32x2 &hi, u32x2 &mid, u32x2 &lo) {
  float r[4] = {x.x, x.y, x.z, x.w};
  uint32_t o[3][2];
#pragma unroll
  for (int lvl = 0; lvl < 3; ++lvl)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t pk = pk_bf16(r[2 * h], r[2 * h + 1]);
      o[lvl][h] = pk;
      if (lvl < 2) {
        // (asm: the compiler would pair these into v_pk_add_f32, which costs an MFMA-paced wave ~6x a plain one)
        asm("v_sub_f32 %0, %0, %1" : "+v"(r[2 * h]) : "v"(pk << 16));
        asm("v_sub_f32 %0, %0, %1" : "+v"(r[2 * h + 1]) : "v"(pk & 0xffff0000u));
      }
    }
  hi = u32x2{o[0][0], o[0][1]}, mid = u32x2{o[1][0], o[1][1]}, lo = u32x2{o[2][0], o[2][1]};
}

// W [N][K] f32 -> k_gemm_b3's image [N / 160][K / 16][160][hi 16 | mid 16 | lo 16] (sf_policy_gemm_split; the
// network's own weights are split on the host by split_weights, same arithmetic)
__global__ void k_split_weights(const float *W, uint16_t *img, int N, int K) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)N * K) return;
  const int n = (int)(e / K), k = (int)(e - (size_t)n * K);
  float r = W[e];
  uint16_t part[3];
#pragma unroll
  for (int lvl = 0; lvl < 3; ++lvl) {
    const uint32_t pk = pk_bf16(r, 0.f);
    part[lvl] = (uint16_t)pk;
    r -= __builtin_bit_cast(float, pk << 16);
  }
  const size_t rec = (((size_t)(n / BN) * (K / B3_BK) + k / B3_BK) * BN + n % BN) * 48 + k % B3_BK;
  img[rec] = part[0], img[rec + 16] = part[1], img[rec + 32] = part[2];
}

template <int MODE>
__global__ __launch_bounds__(B3_T, 1) void k_gemm_b3(Gemm g) {
  constexpr int BM = B3_BM, NT = 5;
  extern __shared__ __attribute__((aligned(16))) unsigned char b3_lds[];
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int n0 = blockIdx.y * BN;
  const int KT = g.K / B3_BK;
  const int u0 = run_start(g, blockIdx.x);
  const int nu = g.unit_base + ((int)blockIdx.x < g.unit_rem ? 1 : 0);
  if (nu == 0) return;
  // LDS image of a tile: row r = 96 bytes [hi 32][mid 32][lo 32], the two 16-byte k halves of each part swapped on rows
  // with bit 3 set.  Conflict-free for every access: the sixteen rows of a ds_read_b128 lane group land on sixteen
  // different 16-byte slots (6 r mod 16 alone would only reach the eight even ones), four rows of a ds_write_b64 group
  // tile the 128-byte bank window (96 r mod 128 = 0, 96, 64, 32), and the W pieces stay contiguous.
  if (w >= B3_CW) {
    // ------------------------------------------------------------------------------------------------------
    // Loader waves.  Unit u's operands go HBM / L2 -> registers (B3_SETS units in flight per thread) -> split -> LDS
    // stage u & 1, one unit ahead of the compute waves.  What a block moves per unit (16 KB of A + 15 KB of W) is what
    // bounds this kernel: a CU's vector-memory path delivered ~25 B/clk here (in-kernel stamps: 8 load instructions took
    // a loader wave ~1300 cycles to issue), about one unit's bytes per unit's MFMA time.  With the same loads, splits and
    // stores done as fillers between the compute waves' MFMAs, in-order issue put every stall of that path in front of
    // matrix instructions (57-66 % pipe use); here they stay in these four waves.  Every load is issued whatever the run
    // length (a unit past the run's end reads clamped, valid addresses and lands in the idle stage): with one static
    // instruction stream the compiler's vmcnt leaves the younger sets in flight.
    // ------------------------------------------------------------------------------------------------------
    const int lt = t - B3_CW * 64;
    constexpr int AJ = BM * 4 / B3_LT;                          // float4 of A per thread: 4 (rows lt/4 + 64 j)
    constexpr int NP = (B3_W_PIECES + B3_LT - 1) / B3_LT;       // W pieces per thread: 4 (the last one for lt < 192)
    const bool wlast = lt + (NP - 1) * B3_LT < B3_W_PIECES;
    const float *arow[AJ];
    auto setrow = [&](int tile) {
#pragma unroll
      for (int j = 0; j < AJ; ++j) {
        int m = tile * BM + (lt >> 2) + (BM / AJ) * j;
        if (m >= g.M) m = g.M - 1;
        if (MODE == MODE_DENSE) {
          arow[j] = g.A + (size_t)m * g.lda + (lt & 3) * 4;
        } else {
          const int so2 = g.So * g.So;
          const int b = m / so2, r = m - b * so2, oy = r / g.So, ox = r - oy * g.So;
          arow[j] = g.A + ((size_t)(b * g.S + 2 * oy) * g.S + 2 * ox) * g.Cin + (lt & 3) * 4;
        }
      }
    };
    const u32x4 *wimg = reinterpret_cast<const u32x4 *>(g.W3) + (size_t)blockIdx.y * KT * B3_W_PIECES;
    auto wdst = [](int piece) { const int n = piece / 6, c = piece % 6; return B3_A_BYTES + n * B3_RS + ((c ^ ((n >> 3) & 1)) * 16); };
    int wdstp[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) wdstp[q] = wdst(lt + q * B3_LT);
    const int adst = (lt >> 2) * B3_RS + ((((lt & 3) >> 1) ^ ((lt >> 5) & 1)) * 16) + (lt & 1) * 8;

    f32x4 ra[B3_SETS][AJ];
    u32x4 rb[B3_SETS][NP];
    int tile_l = u0 / KT, kt_l = u0 - tile_l * KT;
    auto load_next = [&](auto set) {
      constexpr int R = decltype(set)::value;
      int off = kt_l * B3_BK;
      if (MODE == MODE_NHWC) {
        const int tap = off / g.Cin, c0 = off - tap * g.Cin, ky = tap / 3, kx = tap - ky * 3;
        off = (ky * g.S + kx) * g.Cin + c0;
      }
#pragma unroll
      for (int j = 0; j < AJ; ++j) ra[R][j] = ldg4(arow[j] + off);
      const u32x4 *ws = wimg + (size_t)kt_l * B3_W_PIECES;
#pragma unroll
      for (int q = 0; q < NP; ++q) rb[R][q] = ws[q + 1 < NP || wlast ? lt + q * B3_LT : lt];
      if (++kt_l == KT) {
        kt_l = 0;
        ++tile_l;
        if (tile_l < g.ntiles) setrow(tile_l);
      }
    };
    auto lstore = [&](int stage, auto set) {
      constexpr int R = decltype(set)::value;
      unsigned char *base = b3_lds + stage * B3_STAGE;
#pragma unroll
      for (int j = 0; j < AJ; ++j) {
        u32x2 hi, mid, lo;
        split3(ra[R][j], hi, mid, lo);
        unsigned char *d = base + adst + j * ((BM / AJ) * B3_RS);
        *reinterpret_cast<u32x2 *>(d) = hi;
        *reinterpret_cast<u32x2 *>(d + 32) = mid;
        *reinterpret_cast<u32x2 *>(d + 64) = lo;
      }
#pragma unroll
      for (int q = 0; q < NP; ++q)
        if (q + 1 < NP || wlast) *reinterpret_cast<u32x4 *>(base + wdstp[q]) = rb[R][q];
    };
    // during unit i (between the barriers of units i - 1 and i): unit i + 1 -> stage (i + 1) & 1, then the loads of
    // unit i + 1 + B3_SETS into the freed set
    auto step = [&](int i, auto set) {
      lstore((i + 1) & 1, set);
      load_next(set);
      __syncthreads();
    };
    setrow(tile_l);
    load_next(std::integral_constant<int, 0>());
    lstore(0, std::integral_constant<int, 0>());
    load_next(std::integral_constant<int, 1>());
    load_next(std::integral_constant<int, 2>());
    load_next(std::integral_constant<int, 3>());
    load_next(std::integral_constant<int, 0>());
    __syncthreads();
    int i = 0;
    for (; i + 3 < nu; i += 4) {
      step(i, std::integral_constant<int, 1>());
      step(i + 1, std::integral_constant<int, 2>());
      step(i + 2, std::integral_constant<int, 3>());
      step(i + 3, std::integral_constant<int, 0>());
    }
    if (i < nu) step(i, std::integral_constant<int, 1>());
    if (i + 1 < nu) step(i + 1, std::integral_constant<int, 2>());
    if (i + 2 < nu) step(i + 2, std::integral_constant<int, 3>());
    return;
  }

  // ----------------------------------------------------------------------------------------------------------
  // Compute waves: fragments from LDS and MFMAs, nothing else.  One unit = one K tile of 16 = five groups (one per
  // 32-column tile) of six MFMAs.  The W fragments of group n + 1 are read behind the first MFMA of group n; behind
  // the first MFMA of group 4 the wave releases the stage it has now read completely, checks that the loaders have
  // filled the other one and reads the next unit's first fragments.  No barrier: with one per unit, the two waves
  // of a SIMD met at it with nothing queued and the matrix pipe drained once per unit (232 -> 205 TFLOP/s f32-equivalent
  // with the loaders switched off, against 306 for the same loop without the barrier).  sched_barrier pins the
  // order; ten groups make one period of the fragment slots, so the loop body is two units.
  // ----------------------------------------------------------------------------------------------------------
  f32x16 acc[NT];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  };
  // as in k_gemm: the W fragment is the MFMA's first operand, so a lane ends up with row m = l & 31 and four
  // consecutive columns per register quad
  auto flush = [&](int tile, bool whole, int slot) {
    const int ml = w * 32 + (l & 31), m = tile * BM + ml;
    float *pt = g.part + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 + slot) * (BM * BN) + ml * BN;
    float *cr = g.C + (size_t)m * g.ldc + n0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int nl = nt * 32 + 8 * q + 4 * (l >> 5);
        f32x4 v = {acc[nt][4 * q], acc[nt][4 * q + 1], acc[nt][4 * q + 2], acc[nt][4 * q + 3]};
        if (whole) {
          if (g.bias) v += ldg4(g.bias + n0 + nl);
          if (m < g.M) *reinterpret_cast<f32x4 *>(cr + nl) = v;
        } else {
          *reinterpret_cast<f32x4 *>(pt + nl) = v;
        }
      }
    }
  };
  // fragments: lane l holds k = 8 (l >> 5) .. +7 of row (l & 31), one ds_read_b128 per part
  bf16x8 fa[2][3], fw[2][3];
  const int frag = (l & 31) * B3_RS + (((l >> 5) ^ ((l >> 3) & 1)) * 16);
  auto read_a = [&](int stage, int slot) {
    const unsigned char *s = b3_lds + stage * B3_STAGE + w * 32 * B3_RS + frag;
#pragma unroll
    for (int part = 0; part < 3; ++part) fa[slot][part] = *reinterpret_cast<const bf16x8 *>(s + part * 32);
  };
  auto read_w = [&](int stage, int nt, int slot) {
    const unsigned char *s = b3_lds + stage * B3_STAGE + B3_A_BYTES + nt * 32 * B3_RS + frag;
#pragma unroll
    for (int part = 0; part < 3; ++part) fw[slot][part] = *reinterpret_cast<const bf16x8 *>(s + part * 32);
  };
  int tile_c = u0 / KT, kt_c = u0 - tile_c * KT, seg_kt0 = kt_c;
  bool seg_first = true;
  auto unit = [&](int i, auto parity) {
    constexpr int P = decltype(parity)::value;
    const int st = P;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int gslot = (P * NT + nt) & 1;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        // smallest terms first
        const int wp = k == 0 ? 2 : (k == 2 || k == 3) ? 1 : 0, ap = k == 1 ? 2 : (k == 2 || k == 4) ? 1 : 0;
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[gslot][wp], fa[P][ap], acc[nt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (k == 0) {
          if (nt + 1 < NT) read_w(st, nt + 1, gslot ^ 1);
          else read_w(st ^ 1, 0, gslot ^ 1);
        } else if (nt == 3 && k == 1) {
          __syncthreads();
          read_a(st ^ 1, P ^ 1);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (kt_c == KT - 1 || i == nu - 1) {
      flush(tile_c, seg_kt0 == 0 && kt_c == KT - 1, seg_first ? 0 : 1);
      zero_acc();
      seg_first = false;
      seg_kt0 = 0;
    }
    if (++kt_c == KT) kt_c = 0, ++tile_c;
  };
  __syncthreads();
  read_a(0, 0);
  read_w(0, 0, 0);
  zero_acc();
  int i = 0;
  for (; i + 1 < nu; i += 2) {
    unit(i, std::integral_constant<int, 0>());
    unit(i + 1, std::integral_constant<int, 1>());
  }
  if (i < nu) unit(i, std::integral_constant<int, 0>());
}

}  // namespace sfp
