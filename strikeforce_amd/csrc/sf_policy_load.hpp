// sf_policy_load.hpp — new parameters into a live object, from device memory, in stream order (sf_policy_load_weights), and
// the digests of the images an object derives from its parameters (sf_policy_weights_digest).  Included by sf_policy.hip
// behind `struct Policy`.
//
//   k_load_stage    the device form of sf_policy_stage.hpp: ONE launch walks a table of (source, destination, layout, dims)
//                   that travels in the kernel arguments (2.5 KB).  Every block belongs to one table row, every thread to
//                   one destination element (one 32-bit word of a bf16-split image): the index maps of
//                   sf_policy_stage_map.hpp give the source element or "zero", so stores are contiguous and the gathers hit
//                   sources of at most 0.9 MB that stay in the L2.  No LDS, no scratch.
//   k_digest        one 64-bit sum per image of a position-keyed mix of its words (test hook).
// The composed matrix F is rebuilt by sf_policy_conv.hpp's k_to_f64 / k_fold / k_fold_out as sf_policy_create runs them, on
// the object's stream and with an f64 workspace the object keeps.
#pragma once
#include "sf_policy_stage_map.hpp"

namespace sfp {

enum : int32_t { LK_COPY, LK_CONV0T, LK_PERM, LK_TILES, LK_SPLIT };
// n destination elements from block `first` on.  dims: LK_CONV0T a = N, b = CK; LK_PERM a = Cin; LK_TILES (which is also
// pad_zero when tile is 0) a = rows, b = cols, c = pcols; LK_SPLIT a = Cin (n counts 32-bit words: two bf16 of one part)
struct LoadItem {
  const float *src;
  void *dst;
  uint32_t first, n;
  int32_t kind;
  uint32_t a, b, c;
  uint32_t tile;  // LK_TILES: 1 = k_tail's stream order of the padded matrix, 0 = the padded matrix itself
};
constexpr int LOAD_MAX = 52;  // a policy has 50 images and copies, a reward model 36
struct LoadTable {
  LoadItem item[LOAD_MAX];
  int32_t items;
  uint32_t blocks;
};
static_assert(sizeof(LoadTable) <= 4096, "the table travels in the kernel arguments");

__global__ __launch_bounds__(256) void k_load_stage(const LoadTable t) {
  const uint32_t b = blockIdx.x;
  int i = 0;
  while (i + 1 < t.items && t.item[i + 1].first <= b) ++i;  // (uniform in the block: scalar loads of the arguments)
  const float *__restrict__ src = t.item[i].src;
  const uint32_t d = (b - t.item[i].first) * 256u + threadIdx.x;
  if (d >= t.item[i].n) return;
  const int32_t kind = t.item[i].kind;
  const uint32_t a = t.item[i].a, bb = t.item[i].b, c = t.item[i].c;
  if (kind == LK_SPLIT) {
    uint32_t part, part1, p0[3], p1[3];
    const uint32_t s0 = smap::split_of_permute(2u * d, a, &part), s1 = smap::split_of_permute(2u * d + 1u, a, &part1);
    smap::split3(src[s0], p0);
    smap::split3(src[s1], p1);
    const uint32_t lo = part == 0 ? p0[0] : part == 1 ? p0[1] : p0[2], hi = part == 0 ? p1[0] : part == 1 ? p1[1] : p1[2];
    static_cast<uint32_t *>(t.item[i].dst)[d] = lo | (hi << 16);
    return;
  }
  uint32_t s = d;
  if (kind == LK_CONV0T) s = smap::conv0_transpose(d, a, bb);
  else if (kind == LK_PERM) s = smap::conv_permute(d, a);
  else if (kind == LK_TILES) s = t.item[i].tile ? smap::tiles_of_pad(d, a, bb, c) : smap::pad(d, a, bb, c);
  static_cast<float *>(t.item[i].dst)[d] = s == smap::ZERO ? 0.f : src[s];
}

struct DigestItem {
  const uint32_t *p;
  uint32_t words, first;
};
constexpr int DIGEST_MAX = 40;
constexpr uint32_t DIGEST_PER_BLOCK = 256 * 16;
struct DigestTable {
  DigestItem item[DIGEST_MAX];
  int32_t items;
};
// out[image] = sum over its words w at position j of mix64(w + (j + 1) * golden ratio), mod 2^64: the sum does not depend
// on the order of the additions, a word that moves or a pad that is not zero changes it
__global__ __launch_bounds__(256) void k_digest(const DigestTable t, unsigned long long *out) {
  const uint32_t b = blockIdx.x;
  int i = 0;
  while (i + 1 < t.items && t.item[i + 1].first <= b) ++i;
  const uint32_t base = (b - t.item[i].first) * DIGEST_PER_BLOCK + threadIdx.x, words = t.item[i].words;
  const uint32_t *__restrict__ p = t.item[i].p;
  unsigned long long acc = 0;
  for (uint32_t k = 0; k < 16; ++k) {
    const uint32_t j = base + k * 256u;
    if (j >= words) break;
    unsigned long long z = (unsigned long long)p[j] + (unsigned long long)(j + 1u) * 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    acc += z ^ (z >> 31);
  }
  for (int off = 32; off; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63u) == 0 && acc) atomicAdd(out + i, acc);
}

// ---- host side -----------------------------------------------------------------------------------------------------------
constexpr size_t TAIL_HEAD_FLOATS = 3 * (size_t)HID * HID + 16 * (size_t)HID;  // one head's part of k_tail's block
// the f64 workspace of the fold: conv3's rows and the three transposed convolutions behind them, 97.3 MB
constexpr int FOLD_SIDE[4] = {31, 15, 7, 3};
constexpr size_t FOLD_ELEMS[4] = {(size_t)HID * 31 * 31 * OBS_C, (size_t)HID * 15 * 15 * HID, (size_t)HID * 7 * 7 * HID, (size_t)HID * 9 * HID};

struct Image {
  const void *p;
  size_t words;  // 32-bit words of the whole allocation
};
// every device image the object derives from its parameters, in the order strikeforce_policy.h documents
static std::vector<Image> images(const Policy &p) {
  std::vector<Image> v;
  const size_t conv = (size_t)HID * HID * 9;
  v.push_back({p.conv_w[0], (size_t)HID * OBS_C * 9});
  v.push_back({p.conv0_wt, (size_t)HID * OBS_C * 9});
  for (int i = 1; i < 4; ++i) v.push_back({p.conv_w[i], conv});
  for (int i = 1; i < 3; ++i) v.push_back({p.conv_w3[i], conv * 3 / 2});
  if (p.folded) v.push_back({p.fold, (size_t)FD_ROWS * HID});
  for (int g = 0; g < 2; ++g) {
    v.push_back({p.gru_w_ih[g], (size_t)G3 * HID});
    v.push_back({p.gru_w_hh[g], (size_t)G3 * HID});
    v.push_back({p.gru_b_ih[g], (size_t)G3});
    v.push_back({p.gru_b_hh[g], (size_t)G3});
  }
  v.push_back({p.comb_w, (size_t)HID * COMB_PAD});
  v.push_back({p.comb_b, (size_t)HID});
  const int heads = p.reward ? 1 : 2;
  for (int g = 0; g < heads; ++g) {
    const size_t rows = (p.reward || g) ? 1 : ACT;
    for (int i = 0; i < 3; ++i) v.push_back({p.res_w[g][i], (size_t)HID * HID});
    for (int i = 0; i < 3; ++i) v.push_back({p.res_b[g][i], (size_t)HID});
    v.push_back({p.head_w[g], rows * HID});
    v.push_back({p.head_b[g], rows});
    v.push_back({p.head_w16[g], (size_t)16 * HID});
    v.push_back({p.head_b16[g], (size_t)16});
  }
  v.push_back({p.tail_w, 4 * (size_t)G3 * HID + (size_t)HID * COMB_PAD + heads * TAIL_HEAD_FLOATS});
  return v;
}

// a source of `floats` floats: device memory of the object's device, 4-byte aligned, wholly inside its allocation
static int check_source(const Policy *p, const float *s, size_t floats, const char *name) {
  const std::string n(name);
  if (!s) return fail(SF_ERR_ARG, "sf_policy_load_weights: " + n + " is null");
  if (reinterpret_cast<uintptr_t>(s) & 3u) return fail(SF_ERR_ARG, "sf_policy_load_weights: " + n + " is not 4-byte aligned");
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, s) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != p->device) {
    (void)hipGetLastError();  // (a host pointer is an error of the query: it is answered here, not left behind)
    return fail(SF_ERR_ARG, "sf_policy_load_weights: " + n + " is not device memory of the object's device");
  }
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<float *>(s)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(SF_ERR_ARG, "sf_policy_load_weights: the allocation of " + n + " is unknown to the runtime");
  }
  const uintptr_t lo = reinterpret_cast<uintptr_t>(base), addr = reinterpret_cast<uintptr_t>(s);
  if (addr < lo || addr - lo > size || floats * sizeof(float) > size - (addr - lo))
    return fail(SF_ERR_ARG, "sf_policy_load_weights: " + n + " reaches past the end of its allocation");
  return SF_OK;
}

static int load_weights(Policy *p, const sf_policy_weights *w) {
  if (!p) return fail(SF_ERR_ARG, "null policy");
  if (!w) return fail(SF_ERR_ARG, "null sf_policy_weights");
  if (w->abi_version != SF_POLICY_ABI_VERSION) return fail(SF_ERR_ARG, "sf_policy_weights.abi_version mismatch");
  SFP_HIP(hipSetDevice(p->device));
  const int heads = p->reward ? 1 : 2;
  // head slot g -> the fields it is loaded from, as in create()
  const float *res_w[2][3], *res_b[2][3], *head_w[2], *head_b[2];
  for (int g = 0; g < heads; ++g) {
    const bool val = p->reward || g;
    for (int i = 0; i < 3; ++i) res_w[g][i] = val ? w->value_res_w[i] : w->policy_res_w[i], res_b[g][i] = val ? w->value_res_b[i] : w->policy_res_b[i];
    head_w[g] = val ? w->value_w : w->policy_w, head_b[g] = val ? w->value_b : w->policy_b;
  }
  // ---- everything is checked before anything is launched ----
  SFP_RC(check_source(p, w->conv_w[0], (size_t)HID * OBS_C * 9, "conv_w[0]"));
  for (int i = 1; i < 4; ++i) SFP_RC(check_source(p, w->conv_w[i], (size_t)HID * HID * 9, "conv_w[1..3]"));
  for (int g = 0; g < 2; ++g) {
    SFP_RC(check_source(p, w->gru_w_ih[g], (size_t)G3 * HID, "gru_w_ih"));
    SFP_RC(check_source(p, w->gru_w_hh[g], (size_t)G3 * HID, "gru_w_hh"));
    SFP_RC(check_source(p, w->gru_b_ih[g], G3, "gru_b_ih"));
    SFP_RC(check_source(p, w->gru_b_hh[g], G3, "gru_b_hh"));
  }
  SFP_RC(check_source(p, w->comb_w, (size_t)HID * COMB, "comb_w"));
  SFP_RC(check_source(p, w->comb_b, HID, "comb_b"));
  for (int g = 0; g < heads; ++g) {
    const bool val = p->reward || g;
    for (int i = 0; i < 3; ++i) {
      SFP_RC(check_source(p, res_w[g][i], (size_t)HID * HID, val ? "value_res_w" : "policy_res_w"));
      SFP_RC(check_source(p, res_b[g][i], HID, val ? "value_res_b" : "policy_res_b"));
    }
    SFP_RC(check_source(p, head_w[g], (size_t)(val ? 1 : ACT) * HID, val ? "value_w" : "policy_w"));
    SFP_RC(check_source(p, head_b[g], val ? 1 : ACT, val ? "value_b" : "policy_b"));
  }
  // ---- the table: every image create() uploads, in create()'s order ----
  LoadTable t{};
  bool fits = true;
  auto add = [&](int32_t kind, const float *src, void *dst, size_t n, uint32_t a = 0, uint32_t b = 0, uint32_t c = 0, uint32_t tile = 0) {
    if (t.items == LOAD_MAX) {
      fits = false;
      return;
    }
    LoadItem &it = t.item[t.items++];
    it.src = src, it.dst = dst, it.first = t.blocks, it.n = (uint32_t)n, it.kind = kind, it.a = a, it.b = b, it.c = c, it.tile = tile;
    t.blocks += (uint32_t)((n + 255) / 256);
  };
  auto tile = [&](const float *src, size_t off, uint32_t rows, uint32_t cols, uint32_t prows, uint32_t pcols) {
    add(LK_TILES, src, p->tail_w + off, (size_t)prows * pcols, rows, cols, pcols, 1);
  };
  const size_t conv = (size_t)HID * HID * 9;
  add(LK_COPY, w->conv_w[0], p->conv_w[0], (size_t)HID * OBS_C * 9);
  add(LK_CONV0T, w->conv_w[0], p->conv0_wt, (size_t)HID * OBS_C * 9, HID, OBS_C * 9);
  for (int i = 1; i < 4; ++i) {
    add(LK_PERM, w->conv_w[i], p->conv_w[i], conv, HID);
    if (i < 3) add(LK_SPLIT, w->conv_w[i], p->conv_w3[i], conv * 3 / 2, HID);
  }
  for (int g = 0; g < 2; ++g) {
    add(LK_COPY, w->gru_w_ih[g], p->gru_w_ih[g], (size_t)G3 * HID);
    add(LK_COPY, w->gru_w_hh[g], p->gru_w_hh[g], (size_t)G3 * HID);
    add(LK_COPY, w->gru_b_ih[g], p->gru_b_ih[g], G3);
    add(LK_COPY, w->gru_b_hh[g], p->gru_b_hh[g], G3);
    tile(w->gru_w_ih[g], p->gru_w_ih_t[g], G3, HID, G3, HID);
    tile(w->gru_w_hh[g], p->gru_w_hh_t[g], G3, HID, G3, HID);
  }
  add(LK_TILES, w->comb_w, p->comb_w, (size_t)HID * COMB_PAD, HID, COMB, COMB_PAD);
  tile(w->comb_w, p->comb_w_t, HID, COMB, HID, COMB_PAD);
  add(LK_COPY, w->comb_b, p->comb_b, HID);
  for (int g = 0; g < heads; ++g) {
    const uint32_t rows = (p->reward || g) ? 1 : ACT;
    for (int i = 0; i < 3; ++i) {
      add(LK_COPY, res_w[g][i], p->res_w[g][i], (size_t)HID * HID);
      tile(res_w[g][i], p->res_w_t[g][i], HID, HID, HID, HID);
      add(LK_COPY, res_b[g][i], p->res_b[g][i], HID);
    }
    add(LK_COPY, head_w[g], p->head_w[g], (size_t)rows * HID);
    add(LK_COPY, head_b[g], p->head_b[g], rows);
    add(LK_TILES, head_w[g], p->head_w16[g], (size_t)16 * HID, rows, HID, HID);
    tile(head_w[g], p->head_w16_t[g], rows, HID, 16, HID);
    add(LK_TILES, head_b[g], p->head_b16[g], 16, rows, 1, 1);
  }
  if (!fits) return fail(SF_ERR_STATE, "sf_policy_load_weights: more images than the table holds");
  // ---- the first call of a folded object allocates the fold's workspace: 97.3 MB, kept until sf_policy_destroy ----
  if (p->folded && !p->fold_ws[0]) {
    double *T[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ok = true;
    for (int i = 0; i < 4 && ok; ++i) ok = hipMalloc(reinterpret_cast<void **>(&T[i]), FOLD_ELEMS[i] * sizeof(double)) == hipSuccess;
    if (!ok) {
      for (double *d : T)
        if (d) (void)hipFree(d);
      (void)hipGetLastError();
      return fail(SF_ERR_MEMORY, "hipMalloc failed (the fold's workspace, 97 MB)");
    }
    for (int i = 0; i < 4; ++i) p->fold_ws[i] = T[i], p->owned.push_back(T[i]);
  }
  // ---- launches, all on the object's stream ----
  hipStream_t st = p->stream;
  hipLaunchKernelGGL(k_load_stage, dim3(t.blocks), dim3(256), 0, st, t);
  if (p->folded) {  // F from the images just written, as create() composes it (its pad rows stay the zeros create() set)
    double *const *T = p->fold_ws;
    hipLaunchKernelGGL(k_to_f64, dim3((unsigned)((FOLD_ELEMS[3] + 255) / 256)), dim3(256), 0, st, p->conv_w[3], T[3], FOLD_ELEMS[3]);
    for (int i = 2; i >= 0; --i)
      hipLaunchKernelGGL(k_fold, dim3((unsigned)((FOLD_ELEMS[i] + 255) / 256)), dim3(256), 0, st, T[i + 1], p->conv_w[i], T[i], FOLD_SIDE[i + 1],
                         FOLD_SIDE[i], HID, i ? HID : OBS_C, i ? 1 : 0);
    hipLaunchKernelGGL(k_fold_out, dim3((unsigned)(((size_t)OBS_F * HID + 255) / 256)), dim3(256), 0, st, T[0], p->fold);
  }
  SFP_HIP(hipGetLastError());
  return SF_OK;
}

static int weights_digest(Policy *p, uint64_t *out_host, int32_t *count) {
  if (!p || !out_host || !count) return fail(SF_ERR_ARG, "null argument");
  const std::vector<Image> im = images(*p);
  const int n = (int)im.size();
  if (n > DIGEST_MAX) return fail(SF_ERR_STATE, "sf_policy_weights_digest: more images than the table holds");
  if (*count < n) return fail(SF_ERR_ARG, "sf_policy_weights_digest: *count is below the number of images (" + std::to_string(n) + ")");
  SFP_HIP(hipSetDevice(p->device));
  if (!p->d_digest) {
    float *f = nullptr;
    SFP_RC(p->dalloc(&f, 2 * DIGEST_MAX));
    p->d_digest = reinterpret_cast<unsigned long long *>(f);
  }
  DigestTable t{};
  uint32_t blocks = 0;
  for (int i = 0; i < n; ++i) {
    t.item[i].p = static_cast<const uint32_t *>(im[i].p), t.item[i].words = (uint32_t)im[i].words, t.item[i].first = blocks;
    blocks += (uint32_t)((im[i].words + DIGEST_PER_BLOCK - 1) / DIGEST_PER_BLOCK);
  }
  t.items = n;
  SFP_HIP(hipMemsetAsync(p->d_digest, 0, (size_t)n * sizeof(unsigned long long), p->stream));
  hipLaunchKernelGGL(k_digest, dim3(blocks), dim3(256), 0, p->stream, t, p->d_digest);
  SFP_HIP(hipGetLastError());
  SFP_HIP(hipMemcpyAsync(out_host, p->d_digest, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, p->stream));
  SFP_HIP(hipStreamSynchronize(p->stream));
  *count = n;
  return SF_OK;
}

}  // namespace sfp
