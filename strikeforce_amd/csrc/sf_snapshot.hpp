// sf_snapshot.hpp — the device side of sf_snapshot_save / sf_snapshot_load: one copy body between the environment's state
// buffers and a snapshot object's, written against the wave backend (W) like sf_core.hpp, so that k_snapshot (sf_api.hip)
// and the tests' wave emulator (tests/emu) run the same lines.
//
// One launch, grid (arenas, parts), one wavefront per workgroup.  Wavefront (a, part) reads slot_of_arena[a] — and, for a
// load, the slot's valid word — once, through the wave-uniform load: the verdict is the same on every lane, and the
// wavefront of an arena that takes no part (-1), names a slot outside [0, slots) or loads an empty slot ends there,
// before any address is formed from the index.  A wavefront that stays copies bytes [part * part_bytes, (part + 1) *
// part_bytes) of every piece's row (sf_types.hpp Snap): the entity rows are shorter than one part and fall to part 0, the
// cell planes of a large map spread over all parts.  16 bytes per lane where the row length allows it on both sides (rows
// of a multiple of 16 bytes start at multiples of 16 in both layouts), dwords otherwise, 16-bit words for the exit-number
// plane of a map with an odd cell count; every batch issues its four loads before its first store.  No LDS, no scratch.
//
// Copies never happen in place: source and destination are different allocations.  Whole rows travel — zom and por rows
// to their full capacity, the aux planes without looking at the flag bytes — so a destination ends up byte for byte as the
// source was, which also keeps the large pools' rule that the HBM tables are clear beyond the words in use.
#pragma once
#include "sf_types.hpp"

namespace sf {

template <class W, bool SAVE>
struct SnapCore {
  using V = typename W::V;
  using P = typename W::P;
  static constexpr int U = 4;  // loads in flight per lane before the batch's first store

  static SF_DEV void copy16(const uint8_t *src, uint8_t *dst, uint32_t lo, uint32_t hi) {
    const V l16 = W::lane() * 16u;
    for (uint32_t base = lo; base < hi; base += (uint32_t)U * 1024u) {
      typename W::V4 r[U];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const V off = l16 + (base + (uint32_t)i * 1024u);
        r[i] = W::gload16(src, off, W::ltu(off, hi));
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const V off = l16 + (base + (uint32_t)i * 1024u);
        W::gstore16(dst, off, r[i], W::ltu(off, hi));
      }
    }
  }
  static SF_DEV void copy4(const uint8_t *src, uint8_t *dst, uint32_t lo, uint32_t hi) {
    const V ln = W::lane();
    const uint32_t *s = reinterpret_cast<const uint32_t *>(src);
    uint32_t *d = reinterpret_cast<uint32_t *>(dst);
    for (uint32_t base = lo / 4u; base < hi / 4u; base += (uint32_t)U * 64u) {
      V r[U];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const V idx = ln + (base + (uint32_t)i * 64u);
        r[i] = W::gload(s, idx, W::ltu(idx, hi / 4u));
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const V idx = ln + (base + (uint32_t)i * 64u);
        W::gstore(d, idx, r[i], W::ltu(idx, hi / 4u));
      }
    }
  }
  static SF_DEV void copy2(const uint8_t *src, uint8_t *dst, uint32_t lo, uint32_t hi) {
    const V ln = W::lane();
    const uint16_t *s = reinterpret_cast<const uint16_t *>(src);
    uint16_t *d = reinterpret_cast<uint16_t *>(dst);
    for (uint32_t base = lo / 2u; base < hi / 2u; base += (uint32_t)U * 64u) {
      V r[U];
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const V idx = ln + (base + (uint32_t)i * 64u);
        r[i] = W::gload_u16(s, idx, W::ltu(idx, hi / 2u));
      }
#pragma unroll
      for (int i = 0; i < U; ++i) {
        const V idx = ln + (base + (uint32_t)i * 64u);
        W::gstore_u16(d, idx, r[i], W::ltu(idx, hi / 2u));
      }
    }
  }

  static SF_DEV void body(const Snap &s, int a, int part) {
    const int32_t slot = W::uload_i32(s.slot_of_arena + a);
    if (slot == -1) return;
    if ((uint32_t)slot >= (uint32_t)s.slots) {  // (every negative index but -1 lands here too)
      if (part == 0) W::ucount(s.counters + SNAP_RANGE);
      return;
    }
    if (!SAVE && W::uload_i32(s.valid + slot) == 0) {
      if (part == 0) W::ucount(s.counters + SNAP_EMPTY);
      return;
    }
    for (int i = 0; i < SNAP_PIECES; ++i) {
      const uint32_t row = s.piece[i].row_bytes, pb = s.piece[i].part_bytes, width = s.piece[i].width;
      const uint64_t lo64 = (uint64_t)(uint32_t)part * pb;
      if (pb == 0u || lo64 >= row) continue;
      const uint32_t lo = (uint32_t)lo64, hi = row - lo < pb ? row : lo + pb;
      const uint8_t *e = s.piece[i].env + (size_t)a * row;
      const uint8_t *n = s.piece[i].snap + (size_t)slot * row;
      const uint8_t *src = SAVE ? e : n;
      uint8_t *dst = const_cast<uint8_t *>(SAVE ? n : e);
      if (width == 16u)
        copy16(src, dst, lo, hi);
      else if (width == 4u)
        copy4(src, dst, lo, hi);
      else
        copy2(src, dst, lo, hi);
    }
    if (part == 0) {
      // the scalar block whole, but a load leaves the destination's episode count alone: it keeps counting
      const V ln = W::lane();
      P in = W::ltu(ln, (uint32_t)SC_WORDS);
      if (!SAVE) in = in & (ln != (uint32_t)SC_EPISODES);
      const uint32_t *src = reinterpret_cast<const uint32_t *>(SAVE ? s.scal_env + (size_t)a * SC_WORDS : s.scal_snap + (size_t)slot * SC_WORDS);
      uint32_t *dst = reinterpret_cast<uint32_t *>(SAVE ? s.scal_snap + (size_t)slot * SC_WORDS : s.scal_env + (size_t)a * SC_WORDS);
      W::gstore(dst, ln, W::gload(src, ln, in), in);
      if (SAVE) W::ustore_i32(s.valid + slot, 1);
    }
  }
};

}  // namespace sf
