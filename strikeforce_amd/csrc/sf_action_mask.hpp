// sf_action_mask.hpp — the device side of sf_action_mask_device (strikeforce.h): per (arena, commanded human) one word whose
// bit k says whether obey(SF_COMMANDS[k]) (sf_core.hpp obey, gameplay.hpp:695-821), run on the arena's state as it is stored
// now, would change at least one word of that state.  Bit 0 ('+') is set for every present agent; an agent that is not
// present (HF_ALIVE | HF_CTRL, as sf_signals.hpp has it) gets the word 0.  Nothing of the environment is written.
//
// One wavefront per arena, like the step kernels, so that the [field][arena][slot] rows load coalesced.  The body is a
// template over the wave backend (WaveGfx950 in k_action_mask, sf_api.hip; tests/emu/wave_emu.hpp in the tests' CPU
// program): the same text runs on both.
//
// Lane t stands for one TARGET CELL: the neighbour in direction d = t & 3 (0..3 = obey's 's', 'd', 'w', 'a'; way - 1 of the
// cell a human faces) of commanded human g = t >> 2 — 16 agents x 4 directions are the 64 lanes.  The lane loads slot g's
// row itself (four lanes share an address), computes its cell and loads that cell's flag byte from the plane in HBM.  The same
// lanes also hold the entity tables, lane = slot: the human rows, one 64-slot word of zombies, up to four of bullets, one of
// exits.  node::showit() of a target needs "is an occupying human / a live zombie / a designated bullet on it": a
// wave-uniform loop over the targets that exist reads the target's packed position from its lane and answers each question
// with one compare and one ballot per table word, collecting three 64-bit masks with bit t = target t.  From there on
// everything is lane-parallel again: the class of the lane's own cell, four ballots that bring the four directions of an
// agent together (a nibble of each mask), and obey's guards evaluated by every lane for its agent; the lane of direction 0
// stores.
//
// Loads: every row, the scalar block and the table words that depend on nothing are issued before the first is looked
// at; the flag byte and the ten words of the human's table block (Tables::der[h_block]) depend on the human's row and go
// out together as the second round.  Pools of more than 64 zombies or exits (sf_core.hpp ZL) are walked by their words in
// use (SC_ZWN, SC_PWN), the words behind the first loaded inside that walk; a word not yet in use counts as free, as
// p_ind() has it.  No LDS, no scratch.
#pragma once
#include <stddef.h>

#include "../../include/strikeforce.h"
#include "sf_types.hpp"

namespace sf {

// ActionMask, what k_action_mask takes by value in the kernel arguments, is in sf_types.hpp (the host side fills it).

// SF_COMMANDS' indices of the command groups
enum { AM_NOP = 0, AM_TURN_L = 1, AM_TURN_R = 2, AM_USE = 4, AM_PUNCH = 5, AM_FIRE = 6, AM_MOVE_A = 7, AM_MOVE_W = 8,
       AM_MOVE_S = 9, AM_MOVE_D = 10, AM_SELC = 11, AM_SELT = 15, AM_SELW = 19, AM_BLOCK = 27, AM_PORTAL = 28, AM_SUICIDE = 29 };

template <class W>
struct ActionMaskCore {
  using V = typename W::V;
  using P = typename W::P;

  static SF_DEV uint64_t capmask(int n) { return n >= 64 ? ~0ull : n <= 0 ? 0ull : ((1ull << n) - 1ull); }
  // the four bits of agent g (the lane's own) out of a ballot over the target lanes
  static SF_DEV V nibble(uint64_t bal, const V &g) {
    const V half = W::select(W::ltu(g, 8u), V((uint32_t)bal), V((uint32_t)(bal >> 32)));
    return W::shrv(half, (g & 7u) << 2) & 15u;
  }
  static SF_DEV V bit(P p, int k) { return W::select(p, V(1u << k), V(0u)); }
  // get16 of sf_core.hpp for a per-lane k (as a word: -1 is all ones): the low half of lo for k < 2 (signed), else of hi
  static SF_DEV V get16(const V &lo, const V &hi, const V &k) {
    const V w = W::select(W::gts(V(2u), k), lo, hi);
    return W::shrv(w, (k & 1u) << 4) & 0xffffu;
  }

  static SF_DEV void body(const ActionMask &k, int a) {
    const V ln = W::lane();
    const V g = ln >> 2, d = ln & 3u;
    const P ag = W::ltu(g, (uint32_t)k.n_agents);
    const size_t AH = (size_t)k.A * (size_t)k.H, AZ = (size_t)k.A * (size_t)k.Z, AB = (size_t)k.A * (size_t)k.B;
    const bool zl = large_pools(k.Z, k.P);

    // ---- round one: every load that depends on nothing ----
    const uint32_t *h = k.hum + (size_t)a * (size_t)k.H;
    const V pos = W::gload(h + HW_POS * AH, g, ag), fl = W::gload(h + HW_FLAGS * AH, g, ag);
    const V hp = W::gload(h + HW_HP * AH, g, ag), st = W::gload(h + HW_STAMINA * AH, g, ag);
    const V c01 = W::gload(h + HW_CONS01 * AH, g, ag), c23 = W::gload(h + HW_CONS23 * AH, g, ag);
    const V t01 = W::gload(h + HW_THR01 * AH, g, ag), t23 = W::gload(h + HW_THR23 * AH, g, ag);
    const V bpk = W::gload(h + HW_BPK * AH, g, ag);
    const P hin = W::ltu(ln, (uint32_t)k.H);
    const V ehpos = W::gload(h + HW_POS * AH, ln, hin), ehfl = W::gload(h + HW_FLAGS * AH, ln, hin);
    const uint32_t *z = k.zom + (size_t)a * (size_t)k.Z + ZW_POS * AZ;
    const V zp0 = W::gload(z, ln, W::ltu(ln, (uint32_t)k.Z));
    const uint32_t *b = k.bul + (size_t)a * (size_t)k.B + BW_A * AB;
    V ba[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ba[j] = 64 * j < k.B ? W::gload(b, ln + (uint32_t)(64 * j), W::ltu(ln + (uint32_t)(64 * j), (uint32_t)k.B)) : V(0u);
    const uint32_t *pr = k.por + (size_t)a * (size_t)k.P;
    const V pp0 = W::gload(pr, ln, W::ltu(ln, (uint32_t)k.P));
    const V sc = W::gload((const uint32_t *)k.scal + (size_t)a * SC_WORDS, ln, W::ltu(ln, (uint32_t)SC_WORDS));

    // ---- the lane's target cell; round two: its flag byte and the words of the human's table block ----
    const P present = ag & ((fl & (HF_ALIVE | HF_CTRL)) == (HF_ALIVE | HF_CTRL));
    const P placed = present & (pos != POS_NONE);
    const V f = (pos >> 20) & 3u, r = (pos >> 10) & 1023u, c = pos & 1023u;
    const V rr = W::select(d == 0u, r + 1u, W::select(d == 2u, r - 1u, r));  // wdx / wdy, Character.hpp:47
    const V cc = W::select(d == 1u, c + 1u, W::select(d == 3u, c - 1u, c));
    const P in = placed & W::ltu(f, (uint32_t)k.F) & W::ltu(rr, (uint32_t)k.N) & W::ltu(cc, (uint32_t)k.M);  // (-1 wraps past N)
    const V fb = W::gload_u8(k.flags + (size_t)a * (size_t)k.cells_pad, (f * (uint32_t)k.N + rr) * (uint32_t)k.M + cc, in);
    const V q = W::select(in, (f << 20) | (rr << 10) | cc, V(~0u));  // all ones: a word no entity compares equal to
    const V vs = (fl >> HF_VEC_SH) & 63u;                             // (vec + 1) | (sel + 1) << 2
    const V vec1 = vs & 3u, sel = (vs >> 2) - 1u;
    const V block = W::select((fl & HF_PROF) != 0u, V((uint32_t)k.npc_block), (fl >> HF_AGP_SH) & 15u);
    const V der = block * (uint32_t)(sizeof(Derived) / 4u) + (uint32_t)(offsetof(Tables, der) / 4u);
    const uint32_t *tw = reinterpret_cast<const uint32_t *>(k.tab);
    V wl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) wl[j] = W::gload(tw, der + (uint32_t)(offsetof(Derived, weapon_lvl) / 4u + j), present);
    const P thr_sel = present & (vec1 == 2u) & W::ltu(sel, 4u), wpn_sel = present & (vec1 == 3u) & W::ltu(sel, 8u);
    const V t0 = W::gload(tw, der + (uint32_t)(offsetof(Derived, thr) / 4u) + (sel << 2), thr_sel);      // thr[sel][0]: stamina
    const V w0 = W::gload(tw, der + (uint32_t)(offsetof(Derived, weapon) / 4u) + (sel << 2), wpn_sel);  // weapon[sel][0]

    // ---- the pools: words in use, a free bullet slot (b_ind), a free exit slot (p_ind) ----
    uint32_t zwn = 1u, pwn = 1u;
    if (zl) {
      zwn = W::readlane(sc, SC_ZWN), pwn = W::readlane(sc, SC_PWN);
      if (zwn > (uint32_t)zw_for(k.Z)) zwn = (uint32_t)zw_for(k.Z);
      if (pwn > (uint32_t)zw_for(k.P)) pwn = (uint32_t)zw_for(k.P);
    }
    bool free_b = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) free_b = free_b || (~W::ballot((ba[j] & BA_ALIVE) != 0u) & capmask(k.B - 64 * j)) != 0ull;
    bool free_p = zl && pwn < (uint32_t)zw_for(k.P);  // (a word not in use yet: p_write opens it)
    for (uint32_t j = 0; j < pwn && !free_p; ++j) {
      const V sl = ln + 64u * j;
      const V pw = j == 0u ? pp0 : W::gload(pr, sl, W::ltu(sl, (uint32_t)k.P));
      free_p = (~W::ballot((pw & PF_ACTIVE) != 0u) & capmask(k.P - (int)(64u * j))) != 0ull;
    }

    // ---- what stands on each target: bit t of three masks ----
    const uint64_t targets = W::ballot(in);
    uint64_t on_h = 0ull, on_z = 0ull, on_b = 0ull;
    const P hocc = (ehfl & HF_OCC) != 0u;
    for (uint64_t m = targets; m; m &= m - 1ull) {
      const int t = W::ctz64(m);
      const uint32_t qt = W::readlane(q, (uint32_t)t);
      const uint64_t one = 1ull << t;
      if (W::ballot(hocc & (ehpos == qt))) on_h |= one;
      if (zwn && W::ballot((zp0 & (ZF_ALIVE | POS_MASK)) == (ZF_ALIVE | qt))) on_z |= one;
      bool hit = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) hit = hit || W::ballot((ba[j] & (BA_REF | POS_MASK)) == (BA_REF | qt)) != 0ull;
      if (hit) on_b |= one;
    }
    for (uint32_t j = 1; j < zwn; ++j) {  // large pools only: the zombie words behind the first
      const V sl = ln + 64u * j;
      const V zp = W::gload(z, sl, W::ltu(sl, (uint32_t)k.Z));
      for (uint64_t m = targets & ~on_z; m; m &= m - 1ull) {
        const int t = W::ctz64(m);
        if (W::ballot((zp & (ZF_ALIVE | POS_MASK)) == (ZF_ALIVE | W::readlane(q, (uint32_t)t)))) on_z |= 1ull << t;
      }
    }

    // ---- node::showit() of the lane's own cell (gameplay.hpp:321-346) as the three things obey asks of it ----
    const P wall = (fb & SF_CELL_WALL) != 0u, pin = (fb & (SF_CELL_PIN_UP | SF_CELL_PIN_DN)) != 0u;
    const P body_ = W::frombits(on_h) | W::frombits(on_z);  // 'H' / 'Z' come before everything but the wall
    const P rest = W::frombits(on_b) | ((fb & SF_CELL_CHEST) != 0u) | ((fb & SF_CELL_POUT) == 0u);  // bullet, chest, or not a bare 'O'
    const P step_ok = in & !wall & !body_ & (pin | rest);                                             // G:756-765
    const P empty = in & !wall & !body_ & !pin & !W::frombits(on_b) & ((fb & (SF_CELL_CHEST | SF_CELL_POUT)) == 0u);
    const P shot_ok = in & ((!(wall | ((!body_) & pin))) | ((fb & SF_CELL_TEMP) != 0u));              // G:812
    // the agent's four directions side by side, and the one it faces
    const V steps = nibble(W::ballot(step_ok), g);
    const V face = ((fl & HF_WAY_MASK) - 1u) & 3u;
    const P f_in = (W::shrv(nibble(W::ballot(in), g), face) & 1u) != 0u;
    const P f_empty = (W::shrv(nibble(W::ballot(empty), g), face) & 1u) != 0u;
    const P f_shot = (W::shrv(nibble(W::ballot(shot_ok), g), face) & 1u) != 0u;

    // ---- obey's guards ----
    V word = V((1u << AM_NOP) | (1u << AM_TURN_L) | (1u << AM_TURN_R));
    word = word | (((steps >> 3) & 1u) << AM_MOVE_A) | (((steps >> 2) & 1u) << AM_MOVE_W) | ((steps & 1u) << AM_MOVE_S) |
           (((steps >> 1) & 1u) << AM_MOVE_D);
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // a selection takes hold where the item is owned and is not the selection already
      word = word | bit((get16(c01, c23, V((uint32_t)j)) != 0u) & (vs != (1u | ((uint32_t)(j + 1) << 2))), AM_SELC + j);
      word = word | bit((get16(t01, t23, V((uint32_t)j)) != 0u) & (vs != (2u | ((uint32_t)(j + 1) << 2))), AM_SELT + j);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) word = word | bit((wl[j] != 0u) & (vs != (3u | ((uint32_t)(j + 1) << 2))), AM_SELW + j);
    word = word | bit((vec1 == 1u) & (get16(c01, c23, sel) != 0u), AM_USE);  // Human::use: the count goes down
    word = word | bit(P(W::frombits(free_b ? ~0ull : 0ull)) & f_shot, AM_PUNCH);
    // throw_it: enough stamina — then either the count goes down or, at count 0, the selection goes; shot_it: enough
    // stamina — then the stamina moves unless the weapon is free, and the bullet enters or not
    const P thr_ok = (vec1 == 2u) & (W::sar31(st + t0) == 0u);
    const P wpn_ok = (vec1 == 3u) & (W::sar31(st + w0) == 0u) & ((w0 != 0u) | f_shot);
    word = word | bit(P(W::frombits(free_b ? ~0ull : 0ull)) & f_in & (thr_ok | wpn_ok), AM_FIRE);
    word = word | bit(f_empty & ((bpk & 255u) != 0u), AM_BLOCK);
    const P pending = ((bpk >> 16) & 255u) != 0u, has_portal = ((bpk >> 8) & 255u) != 0u;
    word = word | bit(f_empty & (pending | (has_portal & P(W::frombits(free_p ? ~0ull : 0ull)))), AM_PORTAL);
    word = word | bit(hp != 0u, AM_SUICIDE);
    word = W::select(present, W::select(placed, word, V(1u << AM_NOP)), V(0u));

    // ---- outputs: the lane of direction 0 stores its agent's word ----
    const P out = ag & (d == 0u);
    const size_t row = (size_t)a * (size_t)k.n_agents;
    if (k.commands) W::gstore(k.commands + row, g, word, out);
    if (k.actions) {
      V act = V(0u);
#pragma unroll
      for (int j = 0; j < 32; ++j) act = act | (((word >> (int)k.action_bit[j]) & 1u) << j);
      W::gstore(k.actions + row, g, act, out);
    }
  }
};

}  // namespace sf
