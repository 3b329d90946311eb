// Exponential moving average of the flat fp32 parameters (TrainEngine.set_ema; DESIGN.md, "Weight EMA"): the update that
// follows adamw_kernel inside the captured step, and the in-place exchange of the parameters with their average that
// evaluation on the average uses.  Both are pure streams: 16-byte loads and stores per lane over a grid capped at
// 256 CUs x 8 workgroups, grid-stride for the rest, the n % 4 last elements one lane each; no atomics, no LDS.
#include "common.h"

namespace vitpe {

constexpr int EMA_THREADS = 256;
constexpr int EMA_GRID_CAP = 256 * 8;

// workgroups for n elements: one lane per 4 elements, capped; n in 1..3 still needs one (the tail)
static inline int ema_blocks(long long n) {
  if (n <= 0) return 0;
  const long long nvec = n >> 2;
  const long long want = (nvec + EMA_THREADS - 1) / EMA_THREADS;
  return (int)(want < 1 ? 1 : (want > EMA_GRID_CAP ? EMA_GRID_CAP : want));
}

// e[i] = fma(w, p[i] - e[i], e[i]), w = 1 - d_t.  d_t = hp[13], or with WARM min(hp[13], (1 + t) / (10 + t)) at
// t = hp[5] - hp[14] (the optimizer's step counter, already advanced for this step, less its value when the average
// was switched on).  Every lane derives the same d_t from the same three words, which nothing writes during the launch;
// lane 0 of workgroup 0 leaves it in hp[15].  p[i] == e[i] gives fma(w, 0, e[i]) == e[i]: a converged average stays put.
template <bool WARM>
__global__ __launch_bounds__(EMA_THREADS) void ema_update_kernel(const float* __restrict__ p, float* __restrict__ e,
                                                                 float* hp, long long n) {
  float dt = hp[13];
  if (WARM) {
    const float t = hp[5] - hp[14];
    dt = fminf(dt, __fdiv_rn(1.0f + t, 10.0f + t));
  }
  const float w = 1.0f - dt;
  if (blockIdx.x == 0 && threadIdx.x == 0) hp[15] = dt;
  const long long nvec = n >> 2, stride = (long long)gridDim.x * EMA_THREADS;
  const f32x4* __restrict__ p4 = reinterpret_cast<const f32x4*>(p);
  f32x4* __restrict__ e4 = reinterpret_cast<f32x4*>(e);
  // (one vector per trip: with two sweeps' loads issued together the launch took 0.42 x the same run's AdamW at ViT-B/16's
  //  size against 0.34 x, and the same 8.65 us at the CIFAR model's)
  for (long long i = (long long)blockIdx.x * EMA_THREADS + threadIdx.x; i < nvec; i += stride) {
    const f32x4 pv = p4[i];
    f32x4 ev = e4[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) ev[k] = fmaf(w, pv[k] - ev[k], ev[k]);
    e4[i] = ev;
  }
  const long long t = 4 * nvec + threadIdx.x;
  if (blockIdx.x == 0 && t < n) e[t] = fmaf(w, p[t] - e[t], e[t]);
}

// p[i] <-> e[i]; shadow (nullable) [i] = bf16 of the new p[i], the rounding of cast_kernel<bf16>
__global__ __launch_bounds__(EMA_THREADS) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ e,
                                                               bf16* __restrict__ shadow, long long n) {
  const long long nvec = n >> 2, stride = (long long)gridDim.x * EMA_THREADS;
  f32x4* __restrict__ p4 = reinterpret_cast<f32x4*>(p);
  f32x4* __restrict__ e4 = reinterpret_cast<f32x4*>(e);
  for (long long i = (long long)blockIdx.x * EMA_THREADS + threadIdx.x; i < nvec; i += stride) {
    const f32x4 pv = p4[i], ev = e4[i];
    p4[i] = ev;
    e4[i] = pv;
    if (shadow != nullptr) {   // four bf16: one 8-byte store
      bf16x4 s;
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] = from_f32<bf16>(ev[k]);
      *reinterpret_cast<bf16x4*>(shadow + 4 * i) = s;
    }
  }
  const long long t = 4 * nvec + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    const float pv = p[t], ev = e[t];
    p[t] = ev;
    e[t] = pv;
    if (shadow != nullptr) shadow[t] = from_f32<bf16>(ev);
  }
}

static inline bool aligned16(const void* q) { return ((unsigned long long)q & 15) == 0; }

}  // namespace vitpe

using namespace vitpe;

extern "C" int vitpe_ema_blocks(long long n) { return ema_blocks(n); }

extern "C" int vitpe_ema_update(const float* p, float* e, float* hp, long long n, int warmup, hipStream_t st) {
  VITPE_REQUIRE(hp && n >= 0 && (n == 0 || (p && e)) && aligned16(p) && aligned16(e) && ((unsigned long long)hp & 3) == 0);
  if (n == 0) return 0;
  const dim3 grid(ema_blocks(n)), block(EMA_THREADS);
  if (warmup) hipLaunchKernelGGL(ema_update_kernel<true>, grid, block, 0, st, p, e, hp, n);
  else hipLaunchKernelGGL(ema_update_kernel<false>, grid, block, 0, st, p, e, hp, n);
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_ema_swap(float* p, float* e, void* shadow_bf16, long long n, hipStream_t st) {
  VITPE_REQUIRE(n >= 0 && (n == 0 || (p && e)) && aligned16(p) && aligned16(e) && aligned16(shadow_bf16));
  if (n == 0) return 0;
  hipLaunchKernelGGL(ema_swap_kernel, dim3(ema_blocks(n)), dim3(EMA_THREADS), 0, st, p, e, (bf16*)shadow_bf16, n);
  VITPE_CHECK_LAUNCH();
}
