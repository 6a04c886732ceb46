// sf_policy_conv.hpp — the convolution stack of the policy network on the observation's non-zeros (HIP only;
// sf_policy.hip includes it and launches them):
//   k_conv0_sparse<LIST>            conv0 applied to the non-zeros of one agent, its 15 x 15 x 160 output kept in LDS
//   k_fold, k_to_f64, k_fold_out    the four convolutions composed into one matrix F, once per object
//   k_feat_list, k_feat_dense       F applied to an agent's non-zeros: the 160 features behind the stack
#pragma once
#include "sf_policy_gemm.hpp"

namespace sfp {

// ---------------------------------------------------------------------------------------------------------
// conv0 on the observation as it really is: 0.8 % non-zero (a 31x31 window of mostly empty cells, 32 features each).
// One 16-wave workgroup per agent keeps the agent's whole conv0 output (15 x 15 x 160 f32 = 144 KB) in LDS, streams
// the 123 KB observation once, appends its non-zeros to an LDS list in scan order (block-wide prefix sum: the list
// order, hence the order of every f32 sum, is deterministic), and applies each (channel, y, x, value) to the <= 4
// output pixels whose 3x3/stride-2 window contains it: out[oy][ox][n] += value * W[n][c][ky][kx], n on the lanes.
// An output pixel belongs to the wavefront (oy & 3, ox & 3), so there are no atomics; a wavefront looks at 64 list
// entries at a time (one per lane: is one of its targets mine?), then walks its own ones in list order, weight rows
// fetched four targets ahead.  Work is proportional to the non-zeros (~250 per agent, against 65 000 products per
// output channel in the dense form); any density is handled (the list is flushed when full).
// ---------------------------------------------------------------------------------------------------------
constexpr int C0_OUT = 15, C0_ACC = C0_OUT * C0_OUT * HID;  // 36000 floats
constexpr int C0_T = 1024, C0_WAVES = C0_T / 64;
constexpr int C0_LCAP = 2048;
static_assert(C0_LCAP == SF_POLICY_LIST_MAX, "the entry points bound cap by the kernels' list limit");
constexpr size_t C0_LDS = (size_t)C0_ACC * 4 + (size_t)C0_LCAP * 8 + 4 * (2 * 16 * C0_WAVES + 4);

// LIST: the non-zeros arrive as a list (sf_observe_sparse_device: same keys, same order as the scan below builds), so the
// 123 KB scan of the dense observation is gone; `obs` is unused.
struct C0List {
  const uint32_t *keys;
  const float *vals;
  const uint32_t *counts;
  int cap;
  uint32_t *overflows;  // bumped once per agent whose list did not fit (it is then evaluated on an empty list)
};
template <bool LIST>
__global__ __launch_bounds__(C0_T) void k_conv0_sparse(const float *obs, const float *wt, float *act0, int agents, C0List li) {
  extern __shared__ __attribute__((aligned(16))) float c0_lds[];
  float *acc = c0_lds;
  float *lval = acc + C0_ACC;
  uint32_t *lkey = reinterpret_cast<uint32_t *>(lval + C0_LCAP);
  uint32_t *cnt = lkey + C0_LCAP;          // [16 pieces][16 waves] non-zero counts
  uint32_t *offs = cnt + 16 * C0_WAVES;    // their exclusive prefix sums, then the total
  const int t = threadIdx.x, w = t >> 6, l = t & 63;

  const int cy = w >> 2, cx = w & 3;  // this wavefront's output pixels: oy % 4 == cy, ox % 4 == cx
  // the candidate along one axis: input coordinate v lies in the windows of outputs (v - k) / 2 for k == v (mod 2);
  // at most one of them is congruent to `cls` modulo 4.  Returns the output coordinate or -1, and k.
  auto axis = [](int v, int cls, int &k) -> int {
    if (v & 1) {
      k = 1;
      const int o = (v - 1) >> 1;
      return ((o & 3) == cls && o < C0_OUT) ? o : -1;
    }
    const int o0 = v >> 1;  // k = 0
    if ((o0 & 3) == cls) {
      k = 0;
      return o0 < C0_OUT ? o0 : -1;
    }
    k = 2;
    const int o2 = o0 - 1;
    return (o2 >= 0 && (o2 & 3) == cls) ? o2 : -1;
  };
  auto process = [&](uint32_t n) {
    for (uint32_t e0 = 0; e0 < n; e0 += 64) {
      const uint32_t e = e0 + (uint32_t)l;
      uint32_t rowo = 0, wro = 0;
      float val = 0.f;
      bool mine = false;
      if (e < n) {
        const uint32_t key = lkey[e];
        int ky, kx;
        const int oy = axis((int)((key >> 9) & 31u), cy, ky), ox = axis((int)((key >> 14) & 31u), cx, kx);
        mine = oy >= 0 && ox >= 0;
        rowo = (uint32_t)((oy * C0_OUT + ox) * HID);
        wro = (uint32_t)(((int)(key & 511u) + ky * 3 + kx) * HID);
        val = lval[e];
      }
      uint64_t m = __builtin_amdgcn_ballot_w64(mine);
      while (m) {  // four of this wavefront's targets at a time: all weight loads first, then the LDS updates in order
        uint32_t ro[4], nt = 0;
        float vv[4], wv[4][3];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          ro[q] = 0, vv[q] = 0.f;
          wv[q][0] = wv[q][1] = wv[q][2] = 0.f;
          if (m) {
            const int src = __builtin_ctzll(m);
            m &= m - 1ull;
            ro[q] = (uint32_t)__builtin_amdgcn_readlane((int)rowo, src);
            const uint32_t wq = (uint32_t)__builtin_amdgcn_readlane((int)wro, src);
            vv[q] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, val), src));
            const float *wr = wt + wq;
            wv[q][0] = wr[l], wv[q][1] = wr[l + 64];
            if (l < HID - 128) wv[q][2] = wr[l + 128];
            nt = (uint32_t)q + 1u;
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if ((uint32_t)q < nt) {
            float *row = acc + ro[q];
            row[l] = fmaf(vv[q], wv[q][0], row[l]);
            row[l + 64] = fmaf(vv[q], wv[q][1], row[l + 64]);
            if (l < HID - 128) row[l + 128] = fmaf(vv[q], wv[q][2], row[l + 128]);
          }
      }
    }
  };

  if (LIST) {
    // entries of the next agent wait in registers (two per thread cover C0_LCAP) while this one's are applied
    constexpr int EPT = C0_LCAP / C0_T;
    uint32_t pk[EPT], pn = 0;
    float pvv[EPT];
    auto fetch = [&](int b) {
      pn = li.counts[b];
      if (pn > (uint32_t)C0_LCAP || pn > (uint32_t)li.cap) {  // (the 0xffffffff marker of a crowded window too)
        pn = 0u;
        if (t == 0 && li.overflows) atomicAdd(li.overflows, 1u);  // null: a dense fallback launch redoes this agent
      }
#pragma unroll
      for (int k = 0; k < EPT; ++k) {
        const uint32_t e = (uint32_t)(k * C0_T + t);
        pk[k] = 0u, pvv[k] = 0.f;
        if (e < pn) pk[k] = li.keys[(size_t)b * li.cap + e], pvv[k] = li.vals[(size_t)b * li.cap + e];
      }
    };
    if ((int)blockIdx.x < agents) fetch((int)blockIdx.x);
    for (int b = (int)blockIdx.x; b < agents; b += (int)gridDim.x) {
      for (int i = t; i < C0_ACC / 4; i += C0_T) reinterpret_cast<f32x4 *>(acc)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      const uint32_t n = pn;
#pragma unroll
      for (int k = 0; k < EPT; ++k) {
        const uint32_t e = (uint32_t)(k * C0_T + t);
        if (e < n) lkey[e] = pk[k], lval[e] = pvv[k];
      }
      __syncthreads();
      if (b + (int)gridDim.x < agents) fetch(b + (int)gridDim.x);
      process(n);
      __syncthreads();
      f32x4 *dst = reinterpret_cast<f32x4 *>(act0 + (size_t)b * C0_ACC);
      for (int i = t; i < C0_ACC / 4; i += C0_T) dst[i] = reinterpret_cast<const f32x4 *>(acc)[i];
      __syncthreads();  // the tile has been read out before the next agent zeroes it
    }
    return;
  }
  // The workgroup is persistent (one per CU: the output tile fills its LDS) and walks agents b, b + gridDim.x, ...:
  // the next agent's observation is requested as soon as this one's has been scanned, so its latency passes under
  // this agent's list processing and write-back, and the write-back's stores drain under the next agent's scan.
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  constexpr int NV = OBS_F / 2;  // 15376 8-byte pieces: a chunk adds at most 2 * 1024 = C0_LCAP entries
  constexpr int NIT = (NV + C0_T - 1) / C0_T;  // 16 pieces per thread, all requested before the first is looked at
  f32x2 pre[NIT];
  auto request = [&](int b) {
    const f32x2 *src = reinterpret_cast<const f32x2 *>(obs + (size_t)b * OBS_F);
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      const int i = k * C0_T + t;
      pre[k] = f32x2{0.f, 0.f};
      if (i < NV) pre[k] = __builtin_nontemporal_load(src + i);
    }
  };
  // li.counts given (the fallback launch behind a list-form forward): only the agents whose list did not fit — count
  // beyond cap or the kernel's list, or the crowded-window marker — are redone from the dense buffer; the others keep
  // what the list launch wrote.  nxt(b): the first such agent among b, b + gridDim.x, ... (uniform over the workgroup)
  auto nxt = [&](int b) {
    if (li.counts)
      while (b < agents && !(li.counts[b] > (uint32_t)C0_LCAP || li.counts[b] > (uint32_t)li.cap)) b += (int)gridDim.x;
    return b;
  };
  int bnext = nxt((int)blockIdx.x);
  if (bnext < agents) request(bnext);
  for (int b = bnext; b < agents; b = bnext) {
  bnext = nxt(b + (int)gridDim.x);
  for (int i = t; i < C0_ACC / 4; i += C0_T) reinterpret_cast<f32x4 *>(acc)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  uint32_t count = 0;  // list length, the same value in every thread
  auto append = [&](int k, uint32_t m, uint32_t pos) {
    if (m) {
      const int i = k * C0_T + t;
      const float vv[2] = {pre[k].x, pre[k].y};
#pragma unroll
      for (int j = 0; j < 2; ++j)
        if ((m >> j) & 1u) {
          const uint32_t idx = 2u * (uint32_t)i + (uint32_t)j;  // = ch * 961 + y * 31 + x
          const uint32_t ch = idx / (uint32_t)(OBS_W * OBS_W), r = idx - ch * (uint32_t)(OBS_W * OBS_W);
          const uint32_t y = r / (uint32_t)OBS_W, x = r - y * (uint32_t)OBS_W;
          lkey[pos] = (ch * 9u) | (y << 9) | (x << 14);
          lval[pos] = vv[j];
          ++pos;
        }
    }
  };
  // Where does every non-zero go?  Wave-level: two ballots per piece (x non-zero, y non-zero) give a lane's offset
  // (mbcnt) and the wave's count (popcount) without any shuffle; the 16 pieces x 16 waves counts go to LDS, wave 0
  // turns them into offsets in (piece, wave) order = scan order, and if everything fits the list (it does, unless the
  // input is not an observation) all entries are written in one go.  Three barriers instead of two per piece.
  uint32_t lanepre[NIT], mpack = 0;
#pragma unroll
  for (int k = 0; k < NIT; ++k) {
    const uint32_t m = (pre[k].x != 0.f ? 1u : 0u) | (pre[k].y != 0.f ? 2u : 0u);
    const uint64_t b0 = __builtin_amdgcn_ballot_w64((m & 1u) != 0u), b1 = __builtin_amdgcn_ballot_w64((m & 2u) != 0u);
    lanepre[k] = __builtin_amdgcn_mbcnt_hi((uint32_t)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b0, 0u)) +
                 __builtin_amdgcn_mbcnt_hi((uint32_t)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b1, 0u));
    if (l == k) cnt[k * C0_WAVES + w] = (uint32_t)(__builtin_popcountll(b0) + __builtin_popcountll(b1));
    mpack |= m << (2 * k);
  }
  __syncthreads();
  if (w == 0) {  // exclusive prefix of the 256 counts, four per lane
    uint32_t c4[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) c4[j] = cnt[4 * l + j], sum += c4[j];
    uint32_t incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
      if (l >= o) incl += up;
    }
    uint32_t run = incl - sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) offs[4 * l + j] = run, run += c4[j];
    if (l == 63) offs[NIT * C0_WAVES] = incl;
  }
  __syncthreads();
  // write and apply the list; an observation fits in one batch, anything denser goes in as many as it takes
  // (pieces [ks, ke) at a time, ke the furthest piece boundary that still fits: a single piece always does)
  int ks = 0;
  do {
    const uint32_t base = offs[ks * C0_WAVES];
    int ke = ks + 1;
#pragma unroll
    for (int kk = 2; kk <= NIT; ++kk)
      if (kk > ks + 1 && offs[kk * C0_WAVES] - base <= (uint32_t)C0_LCAP) ke = kk;
#pragma unroll
    for (int k = 0; k < NIT; ++k)
      if (k >= ks && k < ke) append(k, (mpack >> (2 * k)) & 3u, offs[k * C0_WAVES + w] - base + lanepre[k]);
    count = offs[ke * C0_WAVES] - base;
    __syncthreads();
    if (ke == NIT && bnext < agents) request(bnext);  // `pre` is free: fetch the next agent
    process(count);
    __syncthreads();
    ks = ke;
  } while (ks < NIT);
  f32x4 *dst = reinterpret_cast<f32x4 *>(act0 + (size_t)b * C0_ACC);
  for (int i = t; i < C0_ACC / 4; i += C0_T) dst[i] = reinterpret_cast<const f32x4 *>(acc)[i];
  __syncthreads();  // the tile has been read out before the next agent zeroes it
  }
}

// ---------------------------------------------------------------------------------------------------------
// The convolution stack folded into one matrix.
//
// GameCNN::forward (Modules.hpp:66-71) is conv3(conv2(conv1(conv0(x)))): four bias-free convolutions with nothing in
// between, i.e. one LINEAR map of the 32 x 31 x 31 observation onto the 160 features `feat`.  sf_policy_create composes
// the four weight tensors once (k_fold: the transposed convolutions applied to conv3's 160 output rows, in f64 on the
// device) into that map's matrix F [row = x << 10 | y << 5 | channel][160] f32 — 21 MB, which stays in the L2s / the
// infinity cache — and a forward pass is
//     feat = sum over the observation's non-zero floats of  value * F[row]          (~300 of 30 752 are non-zero)
// 0.1 MFLOP per agent instead of 48.6: the 15x15, 7x7 and 3x3 activations never exist, and neither do the three
// largest kernels of the layered path (k_conv0_sparse, two k_gemm_b3 launches), which stays in the library behind
// SF_POLICY_LAYERED=1 as the cross-check that evaluates the layers in the reference's order.
// Arithmetic: one partial sum per pair of channels — an fmaf chain in f32 over that pair's non-zeros in the observation's
// scan order — and the partial sums of the non-empty pairs added in f64 in channel order, one rounding to f32 at the
// end.  List form and dense form follow the same order, so their results are the same bits; against the reference's
// layer-by-layer f32 evaluation the difference is of the size of the reference's own rounding (F's entries are within
// half an ulp of the exact composition, a partial sum has ~20 terms where a convolution output has 288 to 1440).
// ---------------------------------------------------------------------------------------------------------
constexpr int FD_ROWS = 32 * 32 * 32;  // rows of F: x (5 bits), y (5 bits), channel (5 bits); x, y = 31 unused
constexpr int FD_G = OBS_C / 2;        // partial sums: one per pair of channels
constexpr int FD_SEG = 2 * OBS_W * OBS_W;  // floats of the dense observation behind one partial sum

// one transposed 3x3 / stride-2 convolution: Tout[o][y][x][cin] = sum over taps (ky, kx) with (y - ky, x - kx) even and
// inside, and over c:  Tin[o][(y - ky) / 2][(x - kx) / 2][c] * W[c][cin][ky][kx].  W is torch's [c][cin][3][3] (perm 0)
// or this file's [c][tap][cin] (perm 1).
__global__ __launch_bounds__(256) void k_fold(const double *Tin, const float *W, double *Tout, int So, int S, int C, int Cin, int perm) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)HID * S * S * Cin) return;
  const int cin = (int)(i % Cin);
  size_t r = i / Cin;
  const int x = (int)(r % S);
  r /= S;
  const int y = (int)(r % S), o = (int)(r / S);
  double acc = 0.0;
  for (int ky = 0; ky < 3; ++ky) {
    const int ty = y - ky;
    if (ty < 0 || (ty & 1) || (ty >> 1) >= So) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int tx = x - kx;
      if (tx < 0 || (tx & 1) || (tx >> 1) >= So) continue;
      const double *tin = Tin + (((size_t)o * So + (ty >> 1)) * So + (tx >> 1)) * C;
      const int tap = ky * 3 + kx;
      for (int c = 0; c < C; ++c)
        acc += tin[c] * (double)(perm ? W[((size_t)c * 9 + tap) * Cin + cin] : W[((size_t)c * Cin + cin) * 9 + tap]);
    }
  }
  Tout[i] = acc;
}
__global__ __launch_bounds__(256) void k_to_f64(const float *src, double *dst, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = (double)src[i];
}
// T0 [o][y][x][channel] f64 -> F [x << 10 | y << 5 | channel][o] f32
__global__ __launch_bounds__(256) void k_fold_out(const double *T0, float *F) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)OBS_W * OBS_W * OBS_C * HID) return;
  const int o = (int)(i % HID);
  size_t r = i / HID;
  const int ch = (int)(r % OBS_C);
  r /= OBS_C;
  const int x = (int)(r % OBS_W), y = (int)(r / OBS_W);
  F[((size_t)((x << 10) | (y << 5) | ch)) * HID + o] = (float)T0[(((size_t)o * OBS_W + y) * OBS_W + x) * OBS_C + ch];
}

// list form: one wavefront per agent walks the agent's list, 64 entries per fetch (one per lane, the next 64 requested
// before these are used); lane l < 40 owns features 4 l .. 4 l + 3 (one 16-byte piece of a row of F), an entry's row and
// value reach all lanes by v_readlane, eight rows are requested before the first is used.  Lanes past the list's end
// carry value 0 and row 0 (fmaf(0, w, c) == c: c starts at +0 and so is never -0), so a batch needs no end test.
__global__ __launch_bounds__(64) void k_feat_list(const float *__restrict__ F, float *__restrict__ feat, int agents, C0List li) {
  const int b = (int)blockIdx.x, l = (int)threadIdx.x;
  if (b >= agents) return;
  uint32_t n = li.counts[b];
  if (n > (uint32_t)C0_LCAP || n > (uint32_t)li.cap) {  // (the 0xffffffff marker of a crowded window too)
    n = 0u;
    if (l == 0 && li.overflows) atomicAdd(li.overflows, 1u);  // null: k_feat_dense redoes this agent
  }
  const uint32_t *__restrict__ keys = li.keys + (size_t)b * li.cap;
  const float *__restrict__ vals = li.vals + (size_t)b * li.cap;
  const float *Fl = F + 4 * (l < HID / 4 ? l : 0);
  double tot[4] = {0.0, 0.0, 0.0, 0.0};
  f32x2 c01 = {0.f, 0.f}, c23 = {0.f, 0.f};  // the open partial sum (v_pk_fma_f32: two features per instruction)
  uint32_t g = 0u;  // the pair of channels of the last entry seen
  uint32_t nkey = (uint32_t)l < n ? keys[l] : 0u;
  float nval = (uint32_t)l < n ? vals[l] : 0.f;
  auto close = [&]() {
    asm volatile("" ::: "memory");  // (a real branch, taken <= 16 times per agent: not selects on every entry)
    tot[0] += (double)c01.x, tot[1] += (double)c01.y, tot[2] += (double)c23.x, tot[3] += (double)c23.y;
    c01 = f32x2{0.f, 0.f}, c23 = f32x2{0.f, 0.f};
  };
  for (uint32_t e0 = 0u; e0 < n; e0 += 64u) {
    const uint32_t key = nkey;
    const float val = nval;
    {
      const uint32_t e = e0 + 64u + (uint32_t)l;
      nkey = e < n ? keys[e] : 0u, nval = e < n ? vals[e] : 0.f;
    }
    const uint32_t ch = ((key & 511u) * 57u) >> 9;  // the key's low field is 9 * channel
    const uint32_t rowo = ((((key >> 9) & 1023u) << 5) | ch) * (uint32_t)HID;
    const uint32_t cnt = n - e0 < 64u ? n - e0 : 64u;
    // which entries open a new pair of channels (the partial sum is closed in front of them)
    const uint32_t gl = ch >> 1;
    uint32_t gprev = (uint32_t)__shfl_up((int)gl, 1, 64);
    if (l == 0) gprev = g;
    const uint64_t opens = __builtin_amdgcn_ballot_w64((uint32_t)l < cnt && gl != gprev);
    g = (uint32_t)__builtin_amdgcn_readlane((int)gl, (int)(cnt - 1u));
    constexpr uint32_t U = 8u;
    for (uint32_t u0 = 0u; u0 < cnt; u0 += U) {
      f32x4 w4[U];
#pragma unroll
      for (uint32_t u = 0u; u < U; ++u) w4[u] = ldg4(Fl + (uint32_t)__builtin_amdgcn_readlane((int)rowo, (int)(u0 + u)));
      const uint32_t ob = (uint32_t)(opens >> u0) & 0xffu;
      if (ob == 0u) {  // the usual batch: all eight entries go on with the open partial sum
#pragma unroll
        for (uint32_t u = 0u; u < U; ++u) {
          const float v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, val), (int)(u0 + u)));
          const f32x2 vv = {v, v};
          c01 = __builtin_elementwise_fma(vv, f32x2{w4[u].x, w4[u].y}, c01);
          c23 = __builtin_elementwise_fma(vv, f32x2{w4[u].z, w4[u].w}, c23);
        }
      } else {
#pragma unroll
        for (uint32_t u = 0u; u < U; ++u) {
          if ((ob >> u) & 1u) close();
          const float v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, val), (int)(u0 + u)));
          const f32x2 vv = {v, v};
          c01 = __builtin_elementwise_fma(vv, f32x2{w4[u].x, w4[u].y}, c01);
          c23 = __builtin_elementwise_fma(vv, f32x2{w4[u].z, w4[u].w}, c23);
        }
      }
    }
  }
  if (l < HID / 4) {
    f32x4 o;
    o.x = (float)(tot[0] + (double)c01.x), o.y = (float)(tot[1] + (double)c01.y);
    o.z = (float)(tot[2] + (double)c23.x), o.w = (float)(tot[3] + (double)c23.y);
    *reinterpret_cast<f32x4 *>(feat + (size_t)b * HID + 4 * l) = o;
  }
}

// dense form: one 16-wave workgroup per agent, wavefront w scans channels 2 w and 2 w + 1 of the observation (its partial
// sum), the sixteen partial sums meet in LDS.  With li.counts given (the launch behind k_feat_list) only the agents whose
// list did not fit are done.
constexpr int FD_T = 64 * FD_G;
__global__ __launch_bounds__(FD_T) void k_feat_dense(const float *__restrict__ obs, const float *__restrict__ F, float *__restrict__ feat,
                                                     int agents, C0List li) {
  __shared__ float part[FD_G][HID];
  __shared__ uint32_t some[FD_G];
  const int t = (int)threadIdx.x, w = t >> 6, l = t & 63;
  auto nxt = [&](int b) {
    if (li.counts)
      while (b < agents && !(li.counts[b] > (uint32_t)C0_LCAP || li.counts[b] > (uint32_t)li.cap)) b += (int)gridDim.x;
    return b;
  };
  if (li.counts) {
    // the launch behind k_feat_list is idle when every list fitted: each thread looks at one of this workgroup's agents
    // (one load each, all in flight together — walking them with nxt() is a chain of dependent loads: 7 us of a 230 us loop)
    bool mine = false;
    for (int b = (int)blockIdx.x + t * (int)gridDim.x; b < agents; b += FD_T * (int)gridDim.x)
      mine = mine || li.counts[b] > (uint32_t)C0_LCAP || li.counts[b] > (uint32_t)li.cap;
    if (!__syncthreads_or(mine)) return;
  }
  constexpr int NIT = (FD_SEG + 63) / 64;  // 31 floats per lane
  const float *Fl = F + 4 * (l < HID / 4 ? l : 0);
  for (int b = nxt((int)blockIdx.x); b < agents; b = nxt(b + (int)gridDim.x)) {
    const float *src = obs + (size_t)b * OBS_F + (size_t)w * FD_SEG;
    float pre[NIT];
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      const int i = k * 64 + l;
      pre[k] = i < FD_SEG ? __builtin_nontemporal_load(src + i) : 0.f;
    }
    float cur[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t any = 0u;
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      uint64_t m = __builtin_amdgcn_ballot_w64(pre[k] != 0.f);
      if (!m) continue;
      any = 1u;
      const uint32_t idx = (uint32_t)(w * FD_SEG + k * 64 + l);  // = channel * 961 + y * 31 + x
      const uint32_t chn = idx / (uint32_t)(OBS_W * OBS_W), r = idx - chn * (uint32_t)(OBS_W * OBS_W);
      const uint32_t y = r / (uint32_t)OBS_W, x = r - y * (uint32_t)OBS_W;
      const uint32_t rowo = ((x << 10) | (y << 5) | chn) * (uint32_t)HID;
      while (m) {  // four non-zeros at a time: their rows of F first, then the sums in scan order
        f32x4 w4[4];
        float vv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          w4[q] = f32x4{0.f, 0.f, 0.f, 0.f}, vv[q] = 0.f;
          if (m) {
            const int s = __builtin_ctzll(m);
            m &= m - 1ull;
            vv[q] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pre[k]), s));
            w4[q] = ldg4(Fl + (uint32_t)__builtin_amdgcn_readlane((int)rowo, s));
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // (an unused slot: value 0 on a zero row, which leaves the sums as they are)
          cur[0] = fmaf(vv[q], w4[q].x, cur[0]);
          cur[1] = fmaf(vv[q], w4[q].y, cur[1]);
          cur[2] = fmaf(vv[q], w4[q].z, cur[2]);
          cur[3] = fmaf(vv[q], w4[q].w, cur[3]);
        }
      }
    }
    if (l < HID / 4) *reinterpret_cast<f32x4 *>(&part[w][4 * l]) = f32x4{cur[0], cur[1], cur[2], cur[3]};
    if (l == 0) some[w] = any;
    __syncthreads();
    if (t < HID) {
      double tot = 0.0;
      for (int g = 0; g < FD_G; ++g)
        if (some[g]) tot += (double)part[g][t];
      feat[(size_t)b * HID + t] = (float)tot;
    }
    __syncthreads();
  }
}

}  // namespace sfp
