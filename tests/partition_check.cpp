// Stand-alone check of wave_word_range (csrc/rthx_partition.h), built with
// -fsanitize=address,undefined by tests/test_partition.py: for every word
// count a histogram can have near both ends of its range and every workgroup
// size, the waves' ranges [wb, we) tile [0, n_words) exactly once, in wave
// order, in whole 64-word steps, and agree with the 64-bit arithmetic the
// kernel used before.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rthx_partition.h"

static int check(uint32_t n_words, uint32_t n_waves) {
  std::vector<uint8_t> seen(n_words, 0);
  const int64_t per64 = (((int64_t)n_words + n_waves * 64 - 1) / ((int64_t)n_waves * 64)) * 64;
  uint32_t next = 0;
  for (uint32_t v = 0; v < n_waves; ++v) {
    const rthx::WordRange r = rthx::wave_word_range(n_words, n_waves, v);
    if (r.wb != next || r.we < r.wb || r.we > n_words) {
      std::printf("n_words %u waves %u wave %u: [%u, %u) after %u\n", n_words, n_waves, v, r.wb, r.we, next);
      return 1;
    }
    if (r.steps != (r.we - r.wb + 63u) / 64u || (r.we - r.wb) > (uint32_t)per64) {
      std::printf("n_words %u waves %u wave %u: %u steps for [%u, %u)\n", n_words, n_waves, v, r.steps, r.wb, r.we);
      return 1;
    }
    // the 64-bit form: [v per, min(v per + per, n_words)), empty when it starts past the end
    const int64_t wb64 = (int64_t)v * per64;
    const int64_t we64 = wb64 + per64 < (int64_t)n_words ? wb64 + per64 : (int64_t)n_words;
    if (wb64 < we64 ? (r.wb != wb64 || r.we != we64) : r.wb != r.we) {
      std::printf("n_words %u waves %u wave %u: [%u, %u), 64-bit form [%lld, %lld)\n", n_words, n_waves, v, r.wb,
                  r.we, (long long)wb64, (long long)we64);
      return 1;
    }
    for (uint32_t w = r.wb; w < r.we; ++w) ++seen[w];
    next = r.we;
  }
  if (next != n_words) {
    std::printf("n_words %u waves %u: ranges end at %u\n", n_words, n_waves, next);
    return 1;
  }
  for (uint32_t w = 0; w < n_words; ++w)
    if (seen[w] != 1) {
      std::printf("n_words %u waves %u: word %u covered %u times\n", n_words, n_waves, w, (unsigned)seen[w]);
      return 1;
    }
  return 0;
}

int main() {
  long cases = 0;
  for (uint32_t n_waves : {4u, 8u, 16u}) {
    for (uint32_t n = 0; n <= 6000u; ++n, ++cases)
      if (check(n, n_waves)) return 1;
    for (uint32_t n = 40897u; n <= 40960u; ++n, ++cases)
      if (check(n, n_waves)) return 1;
  }
  std::printf("partition ok: %ld cases\n", cases);
  return 0;
}
