// sf_snapshot_blob.hpp — the host blob of one snapshot slot (sf_snapshot_export / sf_snapshot_import): its header's
// build, parse and validate code, and the configuration fingerprint's hash.  No HIP and nothing of the library's state in
// here: the parser handles bytes read from files, and tests/snapshot_blob runs it alone under the sanitizers.
//
// A blob is 24 header bytes, little-endian whatever the host, then the slot's bytes (the pieces of sf_types.hpp Snap in
// their order, then the scalar block):
//    0  u32  magic    "SFSN"
//    4  u32  version  layout of header and payload; a blob of another version is refused, never converted
//    8  u64  payload  bytes behind the header: what sf_snapshot_slot_bytes reports, less the header
//   16  u64  fingerprint of every configuration field that shapes or interprets the state (sf_host.hpp snapshot_fingerprint)
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace sf {

constexpr uint32_t SNAP_BLOB_MAGIC = 0x4e534653u;  // "SFSN"
constexpr uint32_t SNAP_BLOB_VERSION = 1u;
constexpr int64_t SNAP_BLOB_HEADER = 24;

enum SnapBlobVerdict { SNAP_BLOB_OK = 0, SNAP_BLOB_SHORT, SNAP_BLOB_MAGIC_BAD, SNAP_BLOB_VERSION_BAD, SNAP_BLOB_LENGTH_BAD,
                       SNAP_BLOB_CONFIG_BAD };
inline const char *snap_blob_message(int v) {
  static const char *const m[] = {"ok", "the blob is shorter than its header and payload", "not a snapshot blob (magic)",
                                  "a blob of another layout version", "the blob's payload length is not this configuration's",
                                  "the blob was exported under another configuration (fingerprint)"};
  return v >= 0 && v <= SNAP_BLOB_CONFIG_BAD ? m[v] : "?";
}

inline void snap_put_le(uint8_t *out, uint64_t v, int bytes) {
  for (int i = 0; i < bytes; ++i) out[i] = (uint8_t)(v >> (8 * i));
}
inline uint64_t snap_get_le(const uint8_t *in, int bytes) {
  uint64_t v = 0;
  for (int i = 0; i < bytes; ++i) v |= (uint64_t)in[i] << (8 * i);
  return v;
}

// the 24 header bytes of a blob with `payload` bytes behind them
inline void snap_blob_header(uint8_t *out, uint64_t payload, uint64_t fingerprint) {
  snap_put_le(out, SNAP_BLOB_MAGIC, 4), snap_put_le(out + 4, SNAP_BLOB_VERSION, 4);
  snap_put_le(out + 8, payload, 8), snap_put_le(out + 16, fingerprint, 8);
}

// Whether `bytes` bytes at `blob` are a blob of `payload` payload bytes exported under `fingerprint`.  Reads the header
// only, and only once `bytes` covers it; SNAP_BLOB_OK means blob + SNAP_BLOB_HEADER .. + payload is readable.
inline int snap_blob_check(const void *blob, int64_t bytes, uint64_t payload, uint64_t fingerprint) {
  if (!blob || bytes < SNAP_BLOB_HEADER) return SNAP_BLOB_SHORT;
  const uint8_t *b = static_cast<const uint8_t *>(blob);
  if (snap_get_le(b, 4) != SNAP_BLOB_MAGIC) return SNAP_BLOB_MAGIC_BAD;
  if (snap_get_le(b + 4, 4) != SNAP_BLOB_VERSION) return SNAP_BLOB_VERSION_BAD;
  if (snap_get_le(b + 8, 8) != payload) return SNAP_BLOB_LENGTH_BAD;
  if ((uint64_t)(bytes - SNAP_BLOB_HEADER) < payload) return SNAP_BLOB_SHORT;
  if (snap_get_le(b + 16, 8) != fingerprint) return SNAP_BLOB_CONFIG_BAD;
  return SNAP_BLOB_OK;
}

// the fingerprint's hash: FNV-1a over the bytes fed, finished by a splitmix64 round
struct SnapHash {
  uint64_t h = 0xcbf29ce484222325ull;
  void bytes(const void *p, size_t n) {
    const uint8_t *b = static_cast<const uint8_t *>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
  }
  void word(int64_t v) {  // by value, eight little-endian bytes: the host's integer layout does not show
    uint8_t le[8];
    snap_put_le(le, (uint64_t)v, 8);
    bytes(le, 8);
  }
  uint64_t finish() const {
    uint64_t x = h;
    x ^= x >> 30, x *= 0xbf58476d1ce4e5b9ull, x ^= x >> 27, x *= 0x94d049bb133111ebull, x ^= x >> 31;
    return x;
  }
};

}  // namespace sf
