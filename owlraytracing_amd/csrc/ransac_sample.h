// ransac_sample.h -- the sample of one trial of tknnRansac (include/owlknn_global.h): a counter-based hash, no state.  Plain C++ shared
// by host and device: ransac.hip includes it, and tests/ransac_sample_host.py compiles it with the host compiler.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RANSAC_HD __host__ __device__
#else
#define RANSAC_HD
#endif

RANSAC_HD inline uint32_t ransac_hash(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

RANSAC_HD inline uint32_t ransac_key(uint32_t seed, uint32_t trial) { return ransac_hash(seed + 0x9e3779b9u * trial); }

// draw a (0 .. 7) of slot s: an index in [0, c)
RANSAC_HD inline uint32_t ransac_draw(uint32_t key, int s, int a, uint32_t c) {
  const uint32_t u = ransac_hash(key ^ (0x85ebca6bu * (uint32_t)(8 * s + a + 1)));
  return (uint32_t)(((uint64_t)u * c) >> 32);
}

// The n (<= 4) distinct indices of trial `trial` into idx; false: a slot found none among its eight draws (DUPLICATE).
RANSAC_HD inline bool ransac_sample(uint32_t seed, uint32_t trial, int n, uint32_t c, uint32_t *idx) {
  const uint32_t key = ransac_key(seed, trial);
  for (int s = 0; s < n; s++) {
    bool found = false;
    for (int a = 0; a < 8 && !found; a++) {
      const uint32_t i = ransac_draw(key, s, a, c);
      bool fresh = true;
      for (int e = 0; e < s; e++) fresh = fresh && idx[e] != i;
      if (fresh) idx[s] = i, found = true;
    }
    if (!found) return false;
  }
  return true;
}
