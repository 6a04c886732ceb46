// TEST INFRASTRUCTURE ONLY: a stand-alone program for the sanitizers (tests/test_signals_emu.py builds it with
// -fsanitize=address,undefined and runs it; nothing sanitized is loaded into Python).  It compiles the kernel's per-agent
// body (strikeforce_amd/csrc/sf_signals.hpp signals_agent — the text k_signals compiles) and runs it over emulator states
// the test has written to files: the raw hum / scal / results buffers of the emulator after consecutive operations, in
// order, one signals call per state on a baseline that lives across them.  Every combination of the optional outputs is
// called, each on a baseline of its own, into heap buffers of exactly the documented size, the inputs in heap buffers of
// exactly their size too: a word read or written past a row is a sanitizer report.  The outputs of the all-outputs
// combination are printed, one line of hex words per state and output, for the test to compare with the emulator's own.
//
// usage: signals_main STATE_FILE...      a state file: int32 A, H, n_agents, then hum [13][A][H], scal [A][24],
//                                        results [A][n_agents][8], rebase [A][n_agents] as int32 words
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../strikeforce_amd/csrc/sf_signals.hpp"

int main(int argc, char **argv) {
  std::vector<int32_t *> base(8, nullptr);
  unsigned long long counters[8][sf::SIG_COUNTERS] = {};
  size_t agents = 0;
  for (int f = 1; f < argc; ++f) {
    FILE *in = fopen(argv[f], "rb");
    int32_t dims[3];
    if (!in || fread(dims, 4, 3, in) != 3) return printf("cannot read %s\n", argv[f]), 2;
    const size_t A = (size_t)dims[0], H = (size_t)dims[1], n = (size_t)dims[2];
    uint32_t *hum = new uint32_t[sf::HW_WORDS * A * H];
    int32_t *scal = new int32_t[A * sf::SC_WORDS], *results = new int32_t[A * n * 8], *rb32 = new int32_t[A * n];
    uint8_t *rebase = new uint8_t[A * n];
    if (fread(hum, 4, sf::HW_WORDS * A * H, in) != sf::HW_WORDS * A * H || fread(scal, 4, A * sf::SC_WORDS, in) != A * sf::SC_WORDS ||
        fread(results, 4, A * n * 8, in) != A * n * 8 || fread(rb32, 4, A * n, in) != A * n)
      return printf("short state file %s\n", argv[f]), 2;
    fclose(in);
    bool any = false;
    for (size_t i = 0; i < A * n; ++i) rebase[i] = (uint8_t)rb32[i], any = any || rb32[i];
    if (!agents) {
      agents = A * n;
      for (int m = 0; m < 8; ++m) base[m] = new int32_t[agents * sf::SIG_BASE_WORDS](), memset(counters[m], 0, sizeof counters[m]);
    } else if (agents != A * n) {
      return printf("state files of different shapes\n"), 2;
    }
    for (int m = 0; m < 8; ++m) {  // bit 0 vitals, bit 1 delta, bit 2 reward
      sf::Signals k;
      memset(&k, 0, sizeof k);
      k.hum = hum, k.scal = scal, k.results = results, k.base = base[m], k.counters = counters[m];
      k.vitals = (m & 1) ? new int32_t[agents * SF_VITALS_WORDS] : nullptr;
      k.delta = (m & 2) ? new int32_t[agents * SF_DELTA_WORDS] : nullptr;
      k.reward = (m & 4) ? new float[agents] : nullptr;
      k.rebase = any ? rebase : nullptr;
      k.A = (int32_t)A, k.H = (int32_t)H, k.n_agents = (int32_t)n;
      k.w.per_step = -0.01f, k.w.died = -3.3f;
      const float w[6] = {1.5f, 0.25f, 0.001f, 0.003f, -0.002f, 0.01f}, oc[8] = {0.f, -1.1f, 2.2f, -0.7f, 0.9f, -0.5f, 0.05f, 0.f};
      memcpy(k.w.w, w, sizeof w), memcpy(k.w.outcome, oc, sizeof oc);
      for (size_t i = 0; i < agents; ++i) sf::signals_agent(k, (int)i);
      if (m == 7) {
        printf("v");
        for (size_t i = 0; i < agents * SF_VITALS_WORDS; ++i) printf(" %x", (unsigned)k.vitals[i]);
        printf("\nd");
        for (size_t i = 0; i < agents * SF_DELTA_WORDS; ++i) printf(" %x", (unsigned)k.delta[i]);
        printf("\nr");
        for (size_t i = 0; i < agents; ++i) {
          uint32_t bits;
          memcpy(&bits, &k.reward[i], 4);
          printf(" %x", bits);
        }
        printf("\ns %llu %llu\n", counters[m][sf::SIG_UNRESOLVED], counters[m][sf::SIG_DETECTED]);
      }
      delete[] k.vitals, delete[] k.delta, delete[] k.reward;
    }
    delete[] hum, delete[] scal, delete[] results, delete[] rb32, delete[] rebase;
  }
  for (int m = 0; m < 8; ++m) delete[] base[m];
  printf("signals_main ok\n");
  return 0;
}
