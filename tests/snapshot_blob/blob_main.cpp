// TEST PROGRAM: the snapshot blob's header code (strikeforce_amd/csrc/sf_snapshot_blob.hpp, HIP-free) alone, built with
// -fsanitize=address,undefined by tests/test_snapshot_blob.py.  Every candidate blob lives in a heap block of exactly its
// length, so a read past what the caller handed in is an AddressSanitizer report.  Fed: valid blobs of several payload
// lengths, every truncation of one, every single-bit flip of the header, a null pointer and negative lengths; each must be
// accepted or refused with the verdict the layout implies.  Prints "ok <checks>" and exits 0, or says what went wrong.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../strikeforce_amd/csrc/sf_snapshot_blob.hpp"

static long checks = 0;
static int failures = 0;

static void expect(int got, int want, const char *what, long detail) {
  ++checks;
  if (got != want) {
    printf("FAILED %s (%ld): verdict %d (%s), expected %d\n", what, detail, got, sf::snap_blob_message(got), want);
    ++failures;
  }
}

// the verdict on the first `bytes` bytes of `blob`, from a heap copy of exactly that length
static int verdict(const std::vector<uint8_t> &blob, int64_t bytes, uint64_t payload, uint64_t fp) {
  uint8_t *exact = static_cast<uint8_t *>(malloc(bytes > 0 ? (size_t)bytes : 1));
  if (bytes > 0) memcpy(exact, blob.data(), (size_t)bytes);
  const int v = sf::snap_blob_check(exact, bytes, payload, fp);
  free(exact);
  return v;
}

int main() {
  const uint64_t fp = 0x0123456789abcdefull;
  const uint64_t payloads[] = {0, 1, 96, 1000, 70000};
  for (uint64_t payload : payloads) {
    std::vector<uint8_t> blob((size_t)sf::SNAP_BLOB_HEADER + (size_t)payload, 0xA5);
    sf::snap_blob_header(blob.data(), payload, fp);
    expect(verdict(blob, (int64_t)blob.size(), payload, fp), sf::SNAP_BLOB_OK, "a valid blob", (long)payload);
    expect(verdict(blob, (int64_t)blob.size(), payload + 1, fp), sf::SNAP_BLOB_LENGTH_BAD, "another configuration's length", (long)payload);
    expect(verdict(blob, (int64_t)blob.size(), payload, fp ^ 1), sf::SNAP_BLOB_CONFIG_BAD, "another fingerprint", (long)payload);
    // every truncation: never read past the bytes given, always refused
    const int64_t step = payload > 2000 ? 997 : 1;
    for (int64_t n = 0; n < (int64_t)blob.size(); n += (n < 64 ? 1 : step))
      expect(verdict(blob, n, payload, fp), sf::SNAP_BLOB_SHORT, "a truncated blob", (long)n);
    // trailing bytes are not looked at
    std::vector<uint8_t> longer(blob);
    longer.resize(blob.size() + 7, 0x5A);
    expect(verdict(longer, (int64_t)longer.size(), payload, fp), sf::SNAP_BLOB_OK, "a blob with a tail", (long)payload);
    // every single-bit flip of the header
    for (int bit = 0; bit < 8 * (int)sf::SNAP_BLOB_HEADER; ++bit) {
      std::vector<uint8_t> bad(blob);
      bad[(size_t)bit / 8] ^= (uint8_t)(1u << (bit % 8));
      const int want = bit < 32 ? sf::SNAP_BLOB_MAGIC_BAD : bit < 64 ? sf::SNAP_BLOB_VERSION_BAD : bit < 128 ? sf::SNAP_BLOB_LENGTH_BAD : sf::SNAP_BLOB_CONFIG_BAD;
      expect(verdict(bad, (int64_t)bad.size(), payload, fp), want, "a flipped header bit", bit);
    }
    // a header that claims more than there is, checked by a reader that expects that much
    expect(verdict(blob, (int64_t)blob.size(), payload, fp), sf::SNAP_BLOB_OK, "again", 0);
    std::vector<uint8_t> liar(blob);
    sf::snap_blob_header(liar.data(), payload + 4096, fp);
    expect(verdict(liar, (int64_t)liar.size(), payload + 4096, fp), sf::SNAP_BLOB_SHORT, "a header longer than its blob", (long)payload);
    sf::snap_blob_header(liar.data(), ~0ull, fp);
    expect(verdict(liar, (int64_t)liar.size(), ~0ull, fp), sf::SNAP_BLOB_SHORT, "a header of 2^64 - 1 bytes", (long)payload);
  }
  expect(sf::snap_blob_check(nullptr, 100, 0, fp), sf::SNAP_BLOB_SHORT, "a null blob", 0);
  std::vector<uint8_t> tiny((size_t)sf::SNAP_BLOB_HEADER);
  sf::snap_blob_header(tiny.data(), 0, fp);
  expect(sf::snap_blob_check(tiny.data(), -1, 0, fp), sf::SNAP_BLOB_SHORT, "a negative length", -1);
  expect(sf::snap_blob_check(tiny.data(), INT64_MIN, 0, fp), sf::SNAP_BLOB_SHORT, "the most negative length", 0);
  // the header is little-endian byte for byte
  const uint8_t want[8] = {'S', 'F', 'S', 'N', 1, 0, 0, 0};
  expect(memcmp(tiny.data(), want, 8), 0, "magic and version bytes", 0);
  // the hash does not depend on how the bytes are fed
  sf::SnapHash a, b;
  a.bytes("abcdefgh", 8);
  b.bytes("abc", 3), b.bytes("defgh", 5);
  expect(a.finish() == b.finish(), 1, "hash of split input", 0);
  sf::SnapHash c;
  c.bytes("abcdefgi", 8);
  expect(a.finish() != c.finish(), 1, "hash of other input", 0);
  if (failures) return 1;
  printf("ok %ld\n", checks);
  return 0;
}
