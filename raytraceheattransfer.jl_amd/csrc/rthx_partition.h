// rthx_partition.h -- how compact_row (rthx_kernels.hip) shares a row's
// histogram words among the waves of a workgroup.  Host and device code, so
// the arithmetic is tested on the CPU (tests/test_partition.py).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTHX_HD __host__ __device__
#else
#define RTHX_HD
#endif

namespace rthx {

// The words [wb, we) of wave `wave` and their count in 64-word steps.
struct WordRange {
  uint32_t wb, we, steps;
};

// Wave v of n_waves (a power of two: workgroups are 256, 512 or 1024 lanes)
// owns the v-th run of `per` words, `per` the least multiple of 64 with
// n_waves * per >= n_words; the runs are clipped to n_words, so the ranges
// tile [0, n_words) and trailing waves own nothing.  32-bit throughout: a
// histogram lives in LDS and never exceeds 40960 words (160 KiB).
RTHX_HD inline WordRange wave_word_range(uint32_t n_words, uint32_t n_waves, uint32_t wave) {
  const uint32_t shift = (uint32_t)__builtin_ctz(n_waves) + 6u;
  const uint32_t per = ((n_words + (1u << shift) - 1u) >> shift) << 6;
  const uint32_t b = wave * per;
  const uint32_t wb = b < n_words ? b : n_words;
  const uint32_t we = n_words - wb < per ? n_words : wb + per;
  return WordRange{wb, we, (we - wb + 63u) >> 6};
}

}  // namespace rthx
