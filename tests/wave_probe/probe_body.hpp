// probe_body.hpp — TEST INFRASTRUCTURE: one small function per operation of the wave backend interface that
// strikeforce_amd/csrc/sf_core.hpp is written against, templated on the backend W like the core itself.
//
// probe_gfx950.hip instantiates every probe with WaveGfx950 (one kernel each: one workgroup = one wavefront = one case),
// probe_emu.cpp with WaveEmu (a loop over the cases).  tests/wave_ref.py states what each operation means; the tests
// compare both instances with it bit for bit (tests/test_wave_probe.py, tests/test_gpu_wave_probe.py).
//
// A probe reads rows of 64 words (in0..in3: one word per lane) and wave-uniform scalars (s0..s3: one word per case) and
// writes rows (out0..out2), scalars (so[case][so_n]) and/or memory: `g` is the case's own region of HBM, `L` its own
// region of LDS.  The host fills both regions before the probe and reads both back after it, so that the words around
// the part an operation may write (sentinels) are checked like its results.  Every index comes from the case lists of
// tests/wave_cases.py; tests/wave_probe_lib.py checks them against the region sizes before anything runs.
//
// IO (given by the including file, never a backend operation under test): ld/st move a row between memory and a V,
// stp writes a predicate as a row of 0/1, stu writes a scalar; DEVICE is true where the probe runs on the GPU.
// The generator probes run Core<W, 1>'s own functions on an Arena whose generator fields are set by Core::load().
#pragma once

namespace sfp {

using sf::Params;

struct PArgs {
  const uint32_t *in0, *in1, *in2, *in3;  // [cases][64]
  const uint32_t *s0, *s1, *s2, *s3;      // [cases]
  uint32_t *out0, *out1, *out2;           // [cases][64]
  uint32_t *so;                           // [cases][so_n]
  uint8_t *g;                             // [cases][g_stride] bytes of HBM, in and out
  uint8_t *limg;                          // [cases][l_stride] bytes: the image of the case's LDS region, in and out
  uint32_t so_n, g_stride, l_stride, cases;
  // the generator probes: the product's tables and state arrays (sf_types.hpp Params), arena = case * per + k
  const uint16_t *logt;
  const uint32_t *exptab;
  uint32_t *rng, *rng2;  // [A][RNG_WORDS]
  int32_t *scal;         // [A][SC_WORDS]
  int32_t A, per;
};

constexpr uint32_t XT_BYTES = 2048;  // the power table at the start of LDS, the case's region behind it

template <class W, class IO>
struct Probes {
  using V = typename W::V;
  using P = typename W::P;
  using C = sf::Core<W, 1>;
  using Arena = typename C::Arena;

  static SF_DEV const uint32_t *row(const uint32_t *b, uint32_t c) { return b + (size_t)c * 64u; }
  static SF_DEV uint32_t *row(uint32_t *b, uint32_t c) { return b + (size_t)c * 64u; }
  static SF_DEV V in0(const PArgs &a, uint32_t c) { return IO::ld(row(a.in0, c)); }
  static SF_DEV V in1(const PArgs &a, uint32_t c) { return IO::ld(row(a.in1, c)); }
  static SF_DEV V in2(const PArgs &a, uint32_t c) { return IO::ld(row(a.in2, c)); }
  static SF_DEV V in3(const PArgs &a, uint32_t c) { return IO::ld(row(a.in3, c)); }
  static SF_DEV P pr2(const PArgs &a, uint32_t c) { return in2(a, c) != 0u; }  // a predicate comes as a row of 0 / 1
  static SF_DEV uint64_t mask(const PArgs &a, uint32_t c) { return ((uint64_t)a.s1[c] << 32) | a.s0[c]; }
  static SF_DEV uint32_t *so(const PArgs &a, uint32_t c) { return a.so + (size_t)c * a.so_n; }
  static SF_DEV uint8_t *g(const PArgs &a, uint32_t c) { return a.g + (size_t)c * a.g_stride; }
  static SF_DEV const uint32_t *xt(const uint8_t *lds) { return (const uint32_t *)lds; }
  static SF_DEV uint8_t *L(uint8_t *lds) { return lds + XT_BYTES; }
  static SF_DEV uint32_t *Lw(uint8_t *lds) { return (uint32_t *)(lds + XT_BYTES); }

  // ---- lane crossing ----------------------------------------------------------------------------------------------
  static SF_DEV void lane_all(const PArgs &a, uint32_t c, uint8_t *) {
    IO::st(row(a.out0, c), W::lane());
    IO::stp(row(a.out1, c), W::all());
  }
  static SF_DEV void shl1(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::shl1(in0(a, c))); }
  static SF_DEV void sum18_row1(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::sum18_row1(in0(a, c))); }
  static SF_DEV void readlane(const PArgs &a, uint32_t c, uint8_t *) { IO::stu(so(a, c), W::readlane(in0(a, c), a.s0[c])); }
  static SF_DEV void setlane(const PArgs &a, uint32_t c, uint8_t *) {
    V v = in0(a, c);
    W::setlane(v, a.s0[c], a.s1[c]);
    IO::st(row(a.out0, c), v);
  }
  // uni: the value of the first active lane.  Lanes below s0 sit out, so that lane is s0; they keep in1's word
  static SF_DEV void uni(const PArgs &a, uint32_t c, uint8_t *) {
    if constexpr (IO::DEVICE) {
      V r = in1(a, c);
      if (W::lane() >= a.s0[c]) r = W::uni(in0(a, c));
      IO::st(row(a.out0, c), r);
    }
  }
  static SF_DEV void ballot(const PArgs &a, uint32_t c, uint8_t *) {
    const uint64_t m = W::ballot(pr2(a, c));
    IO::stu(so(a, c), (uint32_t)m), IO::stu(so(a, c) + 1, (uint32_t)(m >> 32));
  }
  static SF_DEV void frombits(const PArgs &a, uint32_t c, uint8_t *) { IO::stp(row(a.out0, c), W::frombits(mask(a, c))); }
  static SF_DEV void rank_below(const PArgs &a, uint32_t c, uint8_t *) {
    if constexpr (IO::DEVICE) IO::st(row(a.out0, c), W::rank_below(mask(a, c)));
  }
  static SF_DEV void bits64(const PArgs &a, uint32_t c, uint8_t *) {  // masks are never 0 here: ctz / clz of 0 are undefined
    const uint64_t m = mask(a, c);
    IO::stu(so(a, c), (uint32_t)W::popc64(m)), IO::stu(so(a, c) + 1, (uint32_t)W::ctz64(m)), IO::stu(so(a, c) + 2, (uint32_t)W::clz64(m));
  }
  static SF_DEV void popc0(const PArgs &a, uint32_t c, uint8_t *) { IO::stu(so(a, c), (uint32_t)W::popc64(mask(a, c))); }

  // ---- per-lane arithmetic and predicates -------------------------------------------------------------------------
  static SF_DEV void select(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::select(pr2(a, c), in0(a, c), in1(a, c))); }
  static SF_DEV void sar31(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::sar31(in0(a, c))); }
  static SF_DEV void le0(const PArgs &a, uint32_t c, uint8_t *) { IO::stp(row(a.out0, c), W::le0(in0(a, c))); }
  static SF_DEV void gts(const PArgs &a, uint32_t c, uint8_t *) { IO::stp(row(a.out0, c), W::gts(in0(a, c), in1(a, c))); }
  static SF_DEV void ltu(const PArgs &a, uint32_t c, uint8_t *) {
    IO::stp(row(a.out0, c), W::ltu(in0(a, c), in1(a, c)));
    IO::stp(row(a.out1, c), W::ltu(in0(a, c), a.s0[c]));  // the form with a wave-uniform bound (sf_core.hpp: lane < 18)
  }
  static SF_DEV void minu(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::minu(in0(a, c), in1(a, c))); }
  static SF_DEV void shrv(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::shrv(in0(a, c), in1(a, c))); }
  static SF_DEV void shlv(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::shlv(in0(a, c), in1(a, c))); }
  static SF_DEV void mul24(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::mul24(in0(a, c), in1(a, c))); }
  static SF_DEV void mul24_su(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::mul24_su(a.s0[c], in1(a, c))); }
  static SF_DEV void mad24(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::mad24(in0(a, c), a.s0[c], in1(a, c))); }

  // ---- LDS --------------------------------------------------------------------------------------------------------
  static SF_DEV void lds_store_u8(const PArgs &a, uint32_t c, uint8_t *lds) { W::lds_store_u8(L(lds), in0(a, c), in1(a, c), pr2(a, c)); }
  static SF_DEV void lds_store_u32(const PArgs &a, uint32_t c, uint8_t *lds) { W::lds_store_u32(Lw(lds), in0(a, c), in1(a, c), pr2(a, c)); }
  static SF_DEV void ulds_store(const PArgs &a, uint32_t c, uint8_t *lds) {
    W::ulds_store_u8(L(lds), a.s0[c], a.s1[c]);
    W::ulds_store_u32(Lw(lds), a.s2[c], a.s3[c]);
  }
  static SF_DEV void ulds_load(const PArgs &a, uint32_t c, uint8_t *lds) {
    IO::stu(so(a, c), W::ulds_u8(L(lds), a.s0[c])), IO::stu(so(a, c) + 1, W::ulds_u32(Lw(lds), a.s2[c]));
  }
  static SF_DEV void lds_u8(const PArgs &a, uint32_t c, uint8_t *lds) {
    IO::st(row(a.out0, c), W::lds_u8(L(lds), in0(a, c), pr2(a, c)));
    IO::st(row(a.out1, c), W::lds_u8_any(L(lds), in0(a, c)));
  }
  static SF_DEV void lds_u32(const PArgs &a, uint32_t c, uint8_t *lds) { IO::st(row(a.out0, c), W::lds_u32(Lw(lds), in0(a, c), pr2(a, c))); }
  static SF_DEV void lds_or_u32(const PArgs &a, uint32_t c, uint8_t *lds) { W::lds_or_u32(Lw(lds), in0(a, c), in1(a, c), pr2(a, c)); }
  static SF_DEV void lds_or_rtn_u32(const PArgs &a, uint32_t c, uint8_t *lds) {
    IO::st(row(a.out0, c), W::lds_or_rtn_u32(Lw(lds), in0(a, c), in1(a, c), pr2(a, c)));
  }
  static SF_DEV void lds_zero(const PArgs &a, uint32_t c, uint8_t *lds) { W::lds_zero(Lw(lds), a.s0[c]); }

  // ---- copies: s0 bytes from the start of g to the start of L, or back --------------------------------------------
  static SF_DEV void copy_g2l(const PArgs &a, uint32_t c, uint8_t *lds) { W::copy_g2l(L(lds), g(a, c), a.s0[c]); }
  template <int U>
  static SF_DEV void g2l_split(const PArgs &a, uint32_t c, uint8_t *lds) {
    typename W::template G2L<U> q;
    W::template g2l_issue<U>(q, g(a, c), a.s0[c]);
    W::template g2l_store<U>(q, L(lds), a.s0[c]);
  }
  static SF_DEV void g2l_split1(const PArgs &a, uint32_t c, uint8_t *lds) { g2l_split<1>(a, c, lds); }
  static SF_DEV void g2l_split2(const PArgs &a, uint32_t c, uint8_t *lds) { g2l_split<2>(a, c, lds); }
  static SF_DEV void g2l_split4(const PArgs &a, uint32_t c, uint8_t *lds) { g2l_split<4>(a, c, lds); }
  static SF_DEV void copy_l2g(const PArgs &a, uint32_t c, uint8_t *lds) { W::copy_l2g(g(a, c), L(lds), a.s0[c]); }

  // ---- HBM --------------------------------------------------------------------------------------------------------
  static SF_DEV void gload(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::gload((const uint32_t *)g(a, c), in0(a, c), pr2(a, c))); }
  static SF_DEV void gload_u8(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::gload_u8(g(a, c), in0(a, c), pr2(a, c))); }
  static SF_DEV void gload_u16(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::gload_u16((const uint16_t *)g(a, c), in0(a, c), pr2(a, c))); }
  static SF_DEV void gstore(const PArgs &a, uint32_t c, uint8_t *) { W::gstore((uint32_t *)g(a, c), in0(a, c), in1(a, c), pr2(a, c)); }
  static SF_DEV void gstore_u8(const PArgs &a, uint32_t c, uint8_t *) {
    if constexpr (IO::DEVICE) W::gstore_u8(g(a, c), in0(a, c), in1(a, c), pr2(a, c));
  }
  static SF_DEV void gload_u16_at(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::gload_u16_at(a.logt, in0(a, c))); }
  // wave-uniform words: a load of what the host wrote, then a store and the load right behind it
  static SF_DEV void u_i32(const PArgs &a, uint32_t c, uint8_t *) {
    int32_t *p = (int32_t *)g(a, c);
    IO::stu(so(a, c), (uint32_t)W::uload_i32(p + a.s0[c]));
    W::ustore_i32(p + a.s1[c], (int32_t)a.s2[c]);
    IO::stu(so(a, c) + 1, (uint32_t)W::uload_i32(p + a.s1[c]));
  }
  static SF_DEV void u_i16(const PArgs &a, uint32_t c, uint8_t *) {
    int16_t *p = (int16_t *)g(a, c);
    IO::stu(so(a, c), (uint32_t)W::uload_i16(p + a.s0[c]));
    W::ustore_i16(p + a.s1[c], (int16_t)a.s2[c]);
    IO::stu(so(a, c) + 1, (uint32_t)W::uload_i16(p + a.s1[c]));
  }

  // ---- tables -----------------------------------------------------------------------------------------------------
  static SF_DEV void pow_bytes(const PArgs &a, uint32_t c, uint8_t *lds) { IO::st(row(a.out0, c), W::pow_bytes(xt(lds), in0(a, c))); }
  static SF_DEV void pow_pair(const PArgs &a, uint32_t c, uint8_t *lds) { IO::st(row(a.out0, c), W::pow_pair(xt(lds), in0(a, c))); }
  // the round trip store() -> load() makes: a value v in [1, 65536], its log from the table, 3^log
  static SF_DEV void log_pow(const PArgs &a, uint32_t c, uint8_t *lds) {
    const V lg = W::gload_u16(a.logt, in0(a, c) + (uint32_t)sf::LOGT_OFF, W::all());
    IO::st(row(a.out0, c), lg);
    IO::st(row(a.out1, c), C::pow3_v(xt(lds), lg, W::all()));
  }

  // ---- the generator's round, register for register ---------------------------------------------------------------
  // in0 = rl, in1 = la, in2 = seed, in3 = us, s0 = e (jomle): out0 = rl after the round, out1 = the byte offset of the
  // log lookup (before log_base), so[0] = the draw's value
  static SF_DEV void rng_round(const PArgs &a, uint32_t c, uint8_t *lds) {
    V rl = in0(a, c);
    uint32_t out = 0xdeadbeefu;
    const V off = W::rng_round(rl, a.s0[c], in1(a, c), in2(a, c), in3(a, c), V(C::SUM_BIAS_LANE), xt(lds), out);
    IO::st(row(a.out0, c), rl), IO::st(row(a.out1, c), off), IO::stu(so(a, c), out);
  }
  // the same registers through the split form draw() takes without FUSED_ROUND: rng_commit, then draw_issue's own
  // issue_offset (mul24, pow_bytes, rng_reduce) and extraction.  out2 = d, the signed powers
  static SF_DEV void rng_split(const PArgs &a, uint32_t c, uint8_t *lds) {
    const V rl = W::rng_commit(in0(a, c), a.s0[c], in1(a, c));
    V d;
    const V off = C::issue_offset(xt(lds), rl, in2(a, c), in3(a, c), d);
    const int32_t o = (int32_t)W::readlane(d, 18u);
    IO::st(row(a.out0, c), rl), IO::st(row(a.out1, c), off), IO::st(row(a.out2, c), d);
    IO::stu(so(a, c), (uint32_t)o);
  }
  // in0 = d, in1 = us, in2 = bias
  static SF_DEV void rng_reduce(const PArgs &a, uint32_t c, uint8_t *) { IO::st(row(a.out0, c), W::rng_reduce(in0(a, c), in1(a, c), in2(a, c))); }

  // ---- the generator through Core<W, 1> ---------------------------------------------------------------------------
  static SF_DEV Params params(const PArgs &a) {  // a world without entities: load() / store() move the generator and the scalars
    Params p{};
    p.A = a.A, p.logt = a.logt, p.exptab = a.exptab, p.rng = a.rng, p.rng2 = a.rng2, p.scal = a.scal;
    return p;
  }
  static SF_DEV void begin(Arena &S, const PArgs &a, const Params &p, uint32_t arena, uint8_t *lds) {
    S.xt = xt(lds), S.ht = nullptr, S.bm = nullptr, S.zl = nullptr, S.pl = nullptr;
    S.la2 = V(0u), S.la2_ok = 0u, S.wrate = 1u;
    C::load(S, L(lds), p, (int)arena, false);
    (void)a;
  }
  // (a) s0..s3 = tb, serial (lo, hi): srand_, then n = so_n draws; the state after every 512 of them goes to arena
  // case * per + k through store()
  static SF_DEV void gen_srand(const PArgs &a, uint32_t c, uint8_t *lds) {
    const Params p = params(a);
    Arena S;
    begin(S, a, p, c * (uint32_t)a.per, lds);
    C::srand_(S, L(lds), p, ((uint64_t)a.s1[c] << 32) | a.s0[c], ((uint64_t)a.s3[c] << 32) | a.s2[c]);
    for (uint32_t i = 0; i < a.so_n; ++i) {
      IO::stu(so(a, c) + i, C::draw(S, L(lds), p));
      if ((i + 1u) % 512u == 0u) C::store(S, L(lds), p, (int)(c * (uint32_t)a.per + (i + 1u) / 512u - 1u));
    }
  }
  // (b) the next episode's generator from its stored form (rng2, SC_WARM): s0 = 1 has the first lookup issued before
  // the first call (la2_ok), s1 calls of prewarm_one
  static SF_DEV void gen_prewarm(const PArgs &a, uint32_t c, uint8_t *lds) {
    const Params p = params(a);
    Arena S;
    begin(S, a, p, c, lds);
    if (a.s0[c]) C::prewarm_issue(S, p);
    for (uint32_t i = 0; i < a.s1[c]; ++i) C::prewarm_one(S, p);
    IO::stu(so(a, c), S.la2_ok);
    C::store(S, L(lds), p, (int)c);
  }
  // (d), (e) a stored state, so_n draws through draw() (the lookup of the first one issued as load() does)
  static SF_DEV void gen_draw(const PArgs &a, uint32_t c, uint8_t *lds) {
    const Params p = params(a);
    Arena S;
    begin(S, a, p, c, lds);
    C::draw_issue(S, p);
    for (uint32_t i = 0; i < a.so_n; ++i) IO::stu(so(a, c) + i, C::draw(S, L(lds), p));
    C::store(S, L(lds), p, (int)c);
  }
  // the same through the general form; it returns the value on every lane: out0 = the last draw's
  static SF_DEV void gen_draw_core(const PArgs &a, uint32_t c, uint8_t *lds) {
    const Params p = params(a);
    Arena S;
    begin(S, a, p, c, lds);
    V v(0u);
    for (uint32_t i = 0; i < a.so_n; ++i) {
      v = C::template draw_core<true>(S.rl, S.rus, S.rseed, S.jomle, S.xt, p);
      IO::stu(so(a, c) + i, W::readlane(v, 17u));
    }
    IO::st(row(a.out0, c), v);
    C::store(S, L(lds), p, (int)c);
  }
};

// every probe, by the name of its function above: probe_emu.cpp and probe_gfx950.hip make one export (and kernel) of each,
// tests/wave_probe_lib.py lists the same names (tests/test_wave_probe.py compares the two lists)
#define SFP_PROBES(X)                                                                                                  \
  X(lane_all) X(shl1) X(sum18_row1) X(readlane) X(setlane) X(uni) X(ballot) X(frombits) X(rank_below) X(bits64) X(popc0) \
  X(select) X(sar31) X(le0) X(gts) X(ltu) X(minu) X(shrv) X(shlv) X(mul24) X(mul24_su) X(mad24)                        \
  X(lds_store_u8) X(lds_store_u32) X(ulds_store) X(ulds_load) X(lds_u8) X(lds_u32) X(lds_or_u32) X(lds_or_rtn_u32)     \
  X(lds_zero) X(copy_g2l) X(g2l_split1) X(g2l_split2) X(g2l_split4) X(copy_l2g)                                        \
  X(gload) X(gload_u8) X(gload_u16) X(gstore) X(gstore_u8) X(gload_u16_at) X(u_i32) X(u_i16)                           \
  X(pow_bytes) X(pow_pair) X(log_pow) X(rng_round) X(rng_split) X(rng_reduce)                                          \
  X(gen_srand) X(gen_prewarm) X(gen_draw) X(gen_draw_core)

}  // namespace sfp
