// Augmentation stream ("Augmentation stream"): RandomCrop(S, padding = pad) + RandomHorizontalFlip() of the
// resident uint8 dataset, decided per batch slot b by ONE Philox4x32-10 call on the site's (seed, offset) pair:
//   key = (lo32 seed, hi32 seed) ; counter = (lo32 b, hi32 b, lo32 offset, hi32 offset)    (elements 4b .. 4b+2 of philox.h)
//   oy = mulhi32(w0, 2 pad + 1) ; ox = mulhi32(w1, 2 pad + 1) ; flip = hflip && (w2 >> 31)
// Output pixel (c, y, x) of slot b reads the source pixel (y + oy - pad, (flip ? S-1-x : x) + ox - pad) of record index[b],
// or the byte 0 outside the image (zero padding of the uint8 image, in front of ToTensor + Normalize).
#pragma once
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

}  // namespace vitpe
