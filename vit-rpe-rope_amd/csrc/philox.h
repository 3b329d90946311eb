// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the dropout
// stream built on it ("Dropout streams").  Counter-based: the four output words are a pure function of
// (key, counter) -- no state in memory, the same source on the host and on the device.
//
// Stream of a dropout site with the pair rng = (seed, offset) (two 64-bit words in device memory):
//   key     = (lo32(seed), hi32(seed))
//   counter = (lo32(e >> 2), hi32(e >> 2), lo32(offset), hi32(offset)),  word e & 3   for the logical element e
//   keep(e) = word >= thr ,  thr = floor(p * 2^32)      (p a float, the product in double: exact)
//   kept values are multiplied by 1 / (1 - p) (one float division)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VITPE_HD __host__ __device__ __forceinline__
#else
#define VITPE_HD inline
#endif

namespace vitpe {

struct Philox4 { uint32_t w[4]; };

VITPE_HD uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

VITPE_HD Philox4 philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = philox_mulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = philox_mulhi(M1, c2), lo1 = M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += W0;
    k1 += W1;
  }
  Philox4 o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

// the (seed, offset) pair of a site, read once per thread, and the two constants derived from p on the host
struct DropKey {
  uint32_t k0, k1, o0, o1;
};
VITPE_HD DropKey drop_key(const unsigned long long* rng) {
  const unsigned long long seed = rng[0], off = rng[1];
  DropKey k;
  k.k0 = (uint32_t)seed; k.k1 = (uint32_t)(seed >> 32); k.o0 = (uint32_t)off; k.o1 = (uint32_t)(off >> 32);
  return k;
}
// the four words of elements 4 q .. 4 q + 3
VITPE_HD Philox4 drop_words(const DropKey& k, uint64_t q) {
  return philox4x32_10(k.k0, k.k1, (uint32_t)q, (uint32_t)(q >> 32), k.o0, k.o1);
}
inline uint32_t drop_threshold(float p) { return (uint32_t)((double)p * 4294967296.0); }
inline float drop_scale(float p) { return 1.0f / (1.0f - p); }
inline bool drop_p_ok(float p) { return p >= 0.0f && p < 1.0f; }   // (false for NaN)

}  // namespace vitpe
