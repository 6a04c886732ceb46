// stage_main.cpp — runs the weight staging of strikeforce_amd/csrc/sf_policy_stage.hpp on the CPU, for
// tests/test_policy_stage.py (which builds this with -fsanitize=address,undefined and compares what it writes bit for bit).
//
//   stage_main tiles IN OUT N K [N K ...]      the matrices of IN, back to back, appended to one stage_tiles block;
//                                              prints the offset of each
//   stage_main split IN OUT N K                split_weights (OUT: bf16 as uint16)
//   stage_main conv0 IN OUT N CK               conv0_transpose
//   stage_main perm  IN OUT N CIN              conv_permute
//   stage_main pad   IN OUT ROWS COLS PROWS PCOLS   pad_zero
// IN and OUT are raw little-endian float32 (OUT of split: uint16).  The input is handed over in a heap block of exactly its
// size, so a read outside the matrix is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "../../strikeforce_amd/csrc/sf_policy_stage.hpp"

static int die(const char *what) {
  std::fprintf(stderr, "stage_main: %s\n", what);
  return 2;
}

template <class T>
static bool write_all(const char *path, const std::vector<T> &v) {
  FILE *f = std::fopen(path, "wb");
  if (!f) return false;
  const bool ok = std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
  return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
  if (argc < 6) return die("usage: stage_main OP IN OUT DIMS...");
  const std::string op = argv[1];
  std::vector<int> d;
  for (int i = 4; i < argc; ++i) d.push_back(std::atoi(argv[i]));
  for (int v : d)
    if (v < 1) return die("dimensions must be positive");
  size_t floats = 0;
  if (op == "pad") {
    if (d.size() != 4 || d[2] < d[0] || d[3] < d[1]) return die("pad takes ROWS COLS PROWS PCOLS");
    floats = (size_t)d[0] * d[1];
  } else if (op == "tiles") {
    if (d.size() % 2) return die("tiles takes pairs N K");
    for (size_t i = 0; i < d.size(); i += 2) floats += (size_t)d[i] * d[i + 1];
  } else {
    if (d.size() != 2) return die("two dimensions");
    floats = (size_t)d[0] * d[1] * (op == "perm" ? 9 : 1);
  }
  std::unique_ptr<float[]> in(new float[floats]);
  {
    FILE *f = std::fopen(argv[2], "rb");
    if (!f) return die("cannot open IN");
    const size_t got = std::fread(in.get(), sizeof(float), floats, f);
    const bool more = std::fgetc(f) != EOF;
    std::fclose(f);
    if (got != floats || more) return die("IN does not have the size the dimensions give");
  }
  bool ok = false;
  if (op == "tiles") {
    std::vector<float> stage;
    const float *src = in.get();
    for (size_t i = 0; i < d.size(); i += 2) {
      std::printf("%zu\n", sfp::stage_tiles(stage, src, d[i], d[i + 1]));
      src += (size_t)d[i] * d[i + 1];
    }
    ok = write_all(argv[3], stage);
  } else if (op == "split") {
    ok = write_all(argv[3], sfp::split_weights(in.get(), d[0], d[1]));
  } else if (op == "conv0") {
    ok = write_all(argv[3], sfp::conv0_transpose(in.get(), d[0], d[1]));
  } else if (op == "perm") {
    ok = write_all(argv[3], sfp::conv_permute(in.get(), d[0], d[1]));
  } else if (op == "pad") {
    ok = write_all(argv[3], sfp::pad_zero(in.get(), d[0], d[1], d[2], d[3]));
  } else {
    return die("unknown OP");
  }
  return ok ? 0 : die("cannot write OUT");
}
