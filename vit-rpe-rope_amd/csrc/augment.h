// Augmentation stream ("Augmentation stream"): RandomCrop(S, padding = pad) + RandomHorizontalFlip() of the
// resident uint8 dataset, decided per batch slot b by ONE Philox4x32-10 call on the site's (seed, offset) pair:
//   key = (lo32 seed, hi32 seed) ; counter = (lo32 b, hi32 b, lo32 offset, hi32 offset)    (elements 4b .. 4b+2 of philox.h)
//   oy = mulhi32(w0, 2 pad + 1) ; ox = mulhi32(w1, 2 pad + 1) ; flip = hflip && (w2 >> 31)
// Output pixel (c, y, x) of slot b reads the source pixel (y + oy - pad, (flip ? S-1-x : x) + ox - pad) of record index[b],
// or the byte 0 outside the image (zero padding of the uint8 image, in front of ToTensor + Normalize).
//
// Erasing stream ("Erasing stream"): RandomErasing(p, scale, ratio) after Normalize, on the OUTPUT pixel
// coordinates (after crop and flip), on the same pair.  Every draw is a Philox call with counter (c0, c1, lo32 offset,
// hi32 offset); (c0, c1) = (b, 0) is the crop/flip call above, whose fourth word w3 is the switch:
//   u(w) = ((w >> 9) + 0.5f) 2^-23                       (exact in fp32, strictly inside (0, 1))
//   on   = (uint64)w3 < thr ,  thr = floor((double)(float)prob 2^32)  (0: off, 2^32: always)
//   attempt a = 0..9, (c0, c1) = (b, a + 1):  area = (float)(S S) (smin + u(w0) (smax - smin)) ; r = expf(lmin + u(w1) (lmax - lmin))
//     h = (int)rintf(sqrtf(area r)) ; w = (int)rintf(sqrtf(area / r)) ; accepted iff h < S && w < S, then
//     i = mulhi32(w2, S - h + 1) ; j = mulhi32(w3, S - w + 1) ; no accepted attempt: nothing is erased
//   (fp32, every product and sum rounded on its own: no fused multiply-add, so the host build makes the same draws)
// Fill of the pixels i <= y < i + h, j <= x < j + w:  const 0.0f | rand: one normal per channel from (c0, c1) = (b, 11) |
//   pixel: one normal per pixel and channel from (c0, c1) = (lo32 e, 0x80000000 | hi32 e), e = (b S + y) S + x.
//   normal of channel c <= 3, k = c >> 1:  sqrtf(-2 logf(u(w[2k]))) * ((c & 1) ? sinf : cosf)(6.2831853f u(w[2k+1]))
#pragma once
#include <math.h>
#include "philox.h"

namespace vitpe {

struct AugDraw {
  int oy, ox, flip;
};

VITPE_HD AugDraw aug_draw(const unsigned long long* rng, unsigned long long b, int pad, int hflip) {
  const Philox4 w = drop_words(drop_key(rng), (uint64_t)b);
  const uint32_t span = 2u * (uint32_t)pad + 1u;
  AugDraw d;
  d.oy = (int)philox_mulhi(w.w[0], span);
  d.ox = (int)philox_mulhi(w.w[1], span);
  d.flip = (hflip != 0 && (w.w[2] >> 31) != 0) ? 1 : 0;
  return d;
}

// ---- erasing stream ---------------------------------------------------------------------------------------------------------
enum { ERASE_CONST = 0, ERASE_RAND = 1, ERASE_PIXEL = 2 };
constexpr int ERASE_ATTEMPTS = 10;

struct EraseDraw {
  int on, i, j, h, w;
};

VITPE_HD float erase_u(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f; }   // 2^-23

VITPE_HD EraseDraw erase_draw(const unsigned long long* rng, unsigned long long b, int S, unsigned long long thr, float smin,
                              float smax, float lmin, float lmax) {
#pragma clang fp contract(off)
  const DropKey k = drop_key(rng);
  EraseDraw d = {0, 0, 0, 0, 0};
  if ((unsigned long long)drop_words(k, (uint64_t)b).w[3] >= thr) return d;
  const float pixels = (float)(S * S), ds = smax - smin, dl = lmax - lmin;
  for (int a = 0; a < ERASE_ATTEMPTS; ++a) {
    const Philox4 w = philox4x32_10(k.k0, k.k1, (uint32_t)b, (uint32_t)(a + 1), k.o0, k.o1);
    const float area = pixels * (smin + erase_u(w.w[0]) * ds);
    const float r = expf(lmin + erase_u(w.w[1]) * dl);
    const int h = (int)rintf(sqrtf(area * r)), wd = (int)rintf(sqrtf(area / r));
    if (h < S && wd < S) {
      d.on = 1; d.h = h; d.w = wd;
      d.i = (int)philox_mulhi(w.w[2], (uint32_t)(S - h + 1));
      d.j = (int)philox_mulhi(w.w[3], (uint32_t)(S - wd + 1));
      return d;
    }
  }
  return d;
}

// the normal of channel c (0..3) out of one call's four words (selects, no indexed register array)
VITPE_HD float erase_normal(const Philox4& w, int c) {
  const uint32_t wr = (c >> 1) ? w.w[2] : w.w[0], wa = (c >> 1) ? w.w[3] : w.w[1];
  const float rad = sqrtf(-2.0f * logf(erase_u(wr)));
  const float ang = 6.2831853f * erase_u(wa);
  return rad * ((c & 1) ? sinf(ang) : cosf(ang));
}

// what a thread keeps per image beside the rectangle: the key, and in `rand` mode the four channel values
struct EraseFill {
  int mode;
  DropKey key;
  float z[4];
};

VITPE_HD EraseFill erase_fill(const unsigned long long* rng, unsigned long long b, int mode) {
  EraseFill f;
  f.mode = mode;
  f.key = drop_key(rng);
  f.z[0] = f.z[1] = f.z[2] = f.z[3] = 0.0f;
  if (mode == ERASE_RAND) {
    const Philox4 w = philox4x32_10(f.key.k0, f.key.k1, (uint32_t)b, 11u, f.key.o0, f.key.o1);
#pragma unroll
    for (int c = 0; c < 4; ++c) f.z[c] = erase_normal(w, c);
  }
  return f;
}

// the value of output pixel (c, y, x) of slot b inside the rectangle
VITPE_HD float erase_value(const EraseFill& f, unsigned long long b, int S, int y, int x, int c) {
  if (f.mode == ERASE_PIXEL) {
    const uint64_t e = ((uint64_t)b * (uint64_t)S + (uint64_t)y) * (uint64_t)S + (uint64_t)x;
    return erase_normal(philox4x32_10(f.key.k0, f.key.k1, (uint32_t)e, 0x80000000u | (uint32_t)(e >> 32), f.key.o0, f.key.o1), c);
  }
  return c == 0 ? f.z[0] : c == 1 ? f.z[1] : c == 2 ? f.z[2] : f.z[3];   // (const: the four are 0.0f)
}

VITPE_HD bool erase_inside(const EraseDraw& d, int y, int x) {
  return d.on != 0 && y >= d.i && y < d.i + d.h && x >= d.j && x < d.j + d.w;
}

// argument check of the C entries (NaNs fail every comparison)
inline bool erase_args_ok(unsigned long long thr, int mode, int C, float smin, float smax, float lmin, float lmax) {
  return thr <= 4294967296ull && mode >= ERASE_CONST && mode <= ERASE_PIXEL && (mode == ERASE_CONST || C <= 4) &&
         smin > 0.0f && smin <= smax && smax <= 1.0f && lmin <= lmax && lmin - lmin == 0.0f && lmax - lmax == 0.0f;
}

}  // namespace vitpe
