// Everything that works on the flat buffers between the backward and the next forward of the captured step (vitpe/optim.py;
// DESIGN.md, "Optimizer side of the step"): the per-step learning-rate schedule, gradient clipping by global norm, fused
// AdamW (one group, or parameter groups), the weight EMA and its exchange with the parameters.  hp and sched are the
// device blocks of include/vitpe.h (HP_* / SCHED_* in common.h).  No atomics, no LDS beyond the clip's four partial sums:
// every kernel here is reproducible bit for bit (tests/test_optim_bits_gpu.py).
#include "common.h"

namespace vitpe {

constexpr int OPT_THREADS = 256;
constexpr int AG_GRID_CAP = 256 * 8;    // adamw_groups_kernel: 256 CUs x 8 workgroups
constexpr int EMA_GRID_CAP = 256 * 8;
constexpr int AG_MAX_GROUPS = 256;      // the map is one byte per granule

// workgroups of 256 for `lanes` lanes of work, at least one (a launch with only tail lanes), at most `cap` (grid-stride for
// the rest)
static inline int capped_grid(long long lanes, int cap) {
  const long long want = (lanes + OPT_THREADS - 1) / OPT_THREADS;
  return (int)(want < 1 ? 1 : (want > cap ? cap : want));
}
static inline int adamw_groups_blocks(long long n) { return n > 0 ? capped_grid((n + 7) >> 3, AG_GRID_CAP) : 0; }
static inline int ema_blocks(long long n) { return n > 0 ? capped_grid(n >> 2, EMA_GRID_CAP) : 0; }
static inline bool aligned(const void* q, unsigned long long a) { return ((unsigned long long)q & (a - 1)) == 0; }

// ---------------------------------------------------------------------------------------
// Fused AdamW over the flat fp32 parameter / gradient / moment buffers (train.py:195: decoupled weight decay on
// everything) + bf16 weight shadow + grad reset.
// (The step counter keeps its own one-thread launch: an in-kernel "last workgroup advances it" variant needs one
//  same-address arrival atomic per workgroup, ~12 ns each and serialised -- 4096 workgroups made the update 55 us.)
__global__ void adamw_tick_kernel(float* hp) { adamw_tick(hp); }

// One element of AdamW, the one copy both kernels run (so adamw_groups_kernel at scales (1, 1) is adamw_kernel bit for bit):
// p, m, v are updated in place, gi_raw is the gradient before the scale.
struct AdamwConst { float b1, b2, eps, bc1, inv_sqrt_bc2, gs; };
VITPE_DEV void adamw_element(float& pi, float gi_raw, float& mi_io, float& vi_io, float lr, float wd, const AdamwConst& c) {
  const float b1 = c.b1, b2 = c.b2, eps = c.eps, inv_sqrt_bc2 = c.inv_sqrt_bc2;
  const float step_size = lr / c.bc1;
  const float gi = gi_raw * c.gs;
  pi = pi * (1.0f - lr * wd);
  const float mi = b1 * mi_io + (1.0f - b1) * gi;
  const float vi = b2 * vi_io + (1.0f - b2) * gi * gi;
  pi -= step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
  mi_io = mi;
  vi_io = vi;
}

// GS: the hp slot of the gradient scale -- HP_GRAD_SCALE, or HP_CLIP_SCALE (grad_scale * clip coefficient,
// grad_clip_finalize_kernel).  One element per lane and trip.
template <int GS>
__global__ void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                             bf16* __restrict__ shadow, const float* __restrict__ hp, long long n, int zero_grad) {
  const float lr = hp[HP_LR], b1 = hp[HP_BETA1], b2 = hp[HP_BETA2], eps = hp[HP_EPS], wd = hp[HP_WEIGHT_DECAY],
              bc1 = hp[HP_BC1], bc2 = hp[HP_BC2], gs = hp[GS];
  const AdamwConst c = {b1, b2, eps, bc1, 1.0f / sqrtf(bc2), gs};
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float pi = p[i], mi = m[i], vi = v[i];
    adamw_element(pi, g[i], mi, vi, lr, wd, c);
    p[i] = pi; m[i] = mi; v[i] = vi;
    if (shadow) shadow[i] = (bf16)pi;
    if (zero_grad) g[i] = 0.f;
  }
}

// adamw_kernel with a per-granule (lr, weight decay) scale pair and 16-byte accesses: one lane per 8-element granule, the
// n % 8 last elements one lane each.  gid: one byte per granule (clamped to n_groups - 1: a bad map never reads outside
// gtab); gtab: n_groups pairs (lr scale, weight-decay scale) applied to hp[HP_LR] and hp[HP_WEIGHT_DECAY].
template <int GS>
__global__ __launch_bounds__(OPT_THREADS) void adamw_groups_kernel(float* __restrict__ p, float* __restrict__ g,
                                                                  float* __restrict__ m, float* __restrict__ v,
                                                                  bf16* __restrict__ shadow, const float* __restrict__ hp,
                                                                  long long n, int zero_grad,
                                                                  const unsigned char* __restrict__ gid,
                                                                  const float* __restrict__ gtab, int n_groups) {
  const float lr0 = hp[HP_LR], wd0 = hp[HP_WEIGHT_DECAY], bc2 = hp[HP_BC2];
  AdamwConst c;
  c.b1 = hp[HP_BETA1]; c.b2 = hp[HP_BETA2]; c.eps = hp[HP_EPS]; c.bc1 = hp[HP_BC1]; c.gs = hp[GS];
  c.inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
  const long long nvec = n >> 3, stride = (long long)gridDim.x * OPT_THREADS;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < nvec; i += stride) {
    const int k = min((int)gid[i], n_groups - 1);
    const float lr = lr0 * gtab[2 * k];
    const float wd = wd0 * gtab[2 * k + 1];
    f32x4* p4 = reinterpret_cast<f32x4*>(p) + 2 * i;
    f32x4* g4 = reinterpret_cast<f32x4*>(g) + 2 * i;
    f32x4* m4 = reinterpret_cast<f32x4*>(m) + 2 * i;
    f32x4* v4 = reinterpret_cast<f32x4*>(v) + 2 * i;
    f32x4 pv[2] = {p4[0], p4[1]}, gv[2] = {g4[0], g4[1]}, mv[2] = {m4[0], m4[1]}, vv[2] = {v4[0], v4[1]};
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float pi = pv[h][t], gi = gv[h][t], mi = mv[h][t], vi = vv[h][t];
        adamw_element(pi, gi, mi, vi, lr, wd, c);
        pv[h][t] = pi; mv[h][t] = mi; vv[h][t] = vi;
      }
    p4[0] = pv[0]; p4[1] = pv[1];
    m4[0] = mv[0]; m4[1] = mv[1];
    v4[0] = vv[0]; v4[1] = vv[1];
    if (shadow != nullptr) {   // eight bf16: one store per four, as the 8-byte alignment of the shadow allows
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        bf16x4 s;
#pragma unroll
        for (int t = 0; t < 4; ++t) s[t] = (bf16)pv[h][t];
        *reinterpret_cast<bf16x4*>(shadow + 8 * i + 4 * h) = s;
      }
    }
    if (zero_grad) { g4[0] = zero; g4[1] = zero; }
  }
  const long long t = 8 * nvec + threadIdx.x;   // the last, partial granule: index nvec of the map
  if (blockIdx.x == 0 && t < n) {
    const int k = min((int)gid[nvec], n_groups - 1);
    const float lr = lr0 * gtab[2 * k];
    const float wd = wd0 * gtab[2 * k + 1];
    float pi = p[t], gi = g[t], mi = m[t], vi = v[t];
    adamw_element(pi, gi, mi, vi, lr, wd, c);
    p[t] = pi; m[t] = mi; v[t] = vi;
    if (shadow != nullptr) shadow[t] = (bf16)pi;
    if (zero_grad) g[t] = 0.f;
  }
}

// Linear warm-up, then cos^2 (= the cosine annealing of torch's CosineAnnealingLR without the 1 + cos cancellation near its
// end); sched: the SCHED_* block.  One lane, fp64; writes hp[HP_LR] and sched[SCHED_LAST_LR] only.
__global__ void lr_schedule_kernel(float* hp, float* sched, int ticked) {
  const double base = sched[SCHED_BASE_LR], lo = sched[SCHED_MIN_LR], W = sched[SCHED_WARMUP], T = sched[SCHED_TOTAL],
               s0 = sched[SCHED_START_FACTOR];
  double k = (double)hp[HP_STEP] - (double)sched[SCHED_ORIGIN] - (ticked ? 1.0 : 0.0);
  k = k < 0.0 ? 0.0 : k;
  double lr;
  if (k < W) {
    lr = base * (s0 + (1.0 - s0) * k / W);
  } else if (k >= T) {   // (cos(fl(pi / 2)) is 6e-17, not 0: the end of the schedule is min_lr exactly)
    lr = lo;
  } else {
    const double r = fmin(k - W, T - W) / (T - W);
    const double cs = cos(1.5707963267948966 * r);
    lr = lo + (base - lo) * cs * cs;
  }
  const float out = (float)lr;
  hp[HP_LR] = out;
  sched[SCHED_LAST_LR] = out;
}

// ---------------------------------------------------------------------------------------
// Gradient clipping by global norm (torch.nn.utils.clip_grad_norm_, norm_type 2) on the flat gradient, between the
// backward and adamw_kernel<HP_CLIP_SCALE>:  total_norm = hp[HP_GRAD_SCALE] * sqrt(sum g^2), coef = min(1, hp[HP_MAX_NORM] /
// (total_norm + 1e-6)), hp[HP_CLIP_SCALE] = hp[HP_GRAD_SCALE] * coef.  Two launches, no atomics: the sum has ONE order, fixed
// by n and the alignment of g alone.  The grid depends on n only (never on the CU count), so two boxes add in the same order.
// (ceil(n / 4096) workgroups: 16 elements per lane, capped at 1024)
static inline int grad_clip_blocks(long long n) { return n > 0 ? capped_grid((n + 15) >> 4, 1024) : 0; }

// partial[b] = sum of g[i]^2 over workgroup b's share.  The 16-byte aligned body is read as float4, vector
// i -> thread i % (256 * gridDim.x), every thread keeping one running sum per float4 component (fma, in index order);
// the <= 3 floats in front of the body and the <= 3 behind it go to threads 0.. and 64.. of workgroup 0.  Then
// (c0 + c1) + (c2 + c3), a 6-step xor butterfly over the wave, (w0 + w1) + (w2 + w3) through LDS.
// Longest chain of roundings: ceil(nvec / (256 * gridDim.x)) + 1 (head / tail) + 2 + 6 + 2.
__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float* __restrict__ g, long long n,
                                                          float* __restrict__ partial) {
  const long long head = min(n, (long long)((4 - (int)(((unsigned long long)g >> 2) & 3)) & 3));
  const float4* __restrict__ body = reinterpret_cast<const float4*>(g + head);
  const long long nvec = (n - head) >> 2;
  const long long stride = (long long)gridDim.x * 256;
  float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
#define VITPE_SQ_ACC(q) do { c0 = fmaf(q.x, q.x, c0); c1 = fmaf(q.y, q.y, c1); c2 = fmaf(q.z, q.z, c2); c3 = fmaf(q.w, q.w, c3); } while (0)
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < nvec; i += 4 * stride) {   // four independent 16-B loads in flight, added in index order
    const float4 q0 = body[i], q1 = body[i + stride], q2 = body[i + 2 * stride], q3 = body[i + 3 * stride];
    VITPE_SQ_ACC(q0); VITPE_SQ_ACC(q1); VITPE_SQ_ACC(q2); VITPE_SQ_ACC(q3);
  }
  for (; i < nvec; i += stride) {
    const float4 q = body[i];
    VITPE_SQ_ACC(q);
  }
#undef VITPE_SQ_ACC
  if (blockIdx.x == 0) {
    const long long tail0 = head + 4 * nvec;
    const int t = threadIdx.x;
    if (t < head) c0 = fmaf(g[t], g[t], c0);
    if (t >= 64 && tail0 + (t - 64) < n) c0 = fmaf(g[tail0 + (t - 64)], g[tail0 + (t - 64)], c0);
  }
  float s = (c0 + c1) + (c2 + c3);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  __shared__ float ws[4];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}
// One wave: lane l adds partial[l], partial[l + 64], ... in fp64, then a 6-step xor butterfly in fp64; lane 0 writes
// hp[HP_TOTAL_NORM] (fp64 product and root, rounded once), hp[HP_CLIP_COEF] (fp64 on the ROUNDED norm, rounded once) and
// hp[HP_CLIP_SCALE] = hp[HP_GRAD_SCALE] * coef as an fp32 product (coef == 1 leaves hp[HP_GRAD_SCALE]'s bits).  A NaN norm
// gives a NaN coef: the clamp is a comparison, not fminf.  nb == 0 (an empty gradient): norm 0, coef 1.
// (A launch of its own for the reason adamw_tick_kernel is one: "the last workgroup finishes" costs one same-address
//  arrival atomic per workgroup.)
__global__ __launch_bounds__(64) void grad_clip_finalize_kernel(const float* __restrict__ partial, int nb, float* hp) {
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 64) s += (double)partial[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) {
    const float gs = hp[HP_GRAD_SCALE];
    const float norm = (float)((double)gs * sqrt(s));
    double coef = (double)hp[HP_MAX_NORM] / ((double)norm + 1e-6);
    coef = coef > 1.0 ? 1.0 : coef;
    const float cf = nb == 0 ? 1.0f : (float)coef;
    hp[HP_TOTAL_NORM] = norm;
    hp[HP_CLIP_COEF] = cf;
    hp[HP_CLIP_SCALE] = gs * cf;
  }
}

// ---------------------------------------------------------------------------------------
// Exponential moving average of the flat fp32 parameters ("Weight EMA"): the update that follows AdamW inside the
// captured step, and the in-place exchange of the parameters with their average that evaluation on the average uses.  Both
// are pure streams: 16-byte loads and stores per lane, the n % 4 last elements one lane each.
// e[i] = fma(w, p[i] - e[i], e[i]), w = 1 - d_t.  d_t = hp[HP_EMA_DECAY], or with WARM min(that, (1 + t) / (10 + t)) at
// t = hp[HP_STEP] - hp[HP_EMA_ORIGIN] (the optimizer's step counter, already advanced for this step, less its value when the
// average was switched on).  Every lane derives the same d_t from the same three words, which nothing writes during the
// launch; lane 0 of workgroup 0 leaves it in hp[HP_EMA_DT].  p[i] == e[i] gives fma(w, 0, e[i]) == e[i]: a converged average
// stays put.
template <bool WARM>
__global__ __launch_bounds__(OPT_THREADS) void ema_update_kernel(const float* __restrict__ p, float* __restrict__ e,
                                                                 float* hp, long long n) {
  float dt = hp[HP_EMA_DECAY];
  if (WARM) {
    const float t = hp[HP_STEP] - hp[HP_EMA_ORIGIN];
    dt = fminf(dt, __fdiv_rn(1.0f + t, 10.0f + t));
  }
  const float w = 1.0f - dt;
  if (blockIdx.x == 0 && threadIdx.x == 0) hp[HP_EMA_DT] = dt;
  const long long nvec = n >> 2, stride = (long long)gridDim.x * OPT_THREADS;
  const f32x4* __restrict__ p4 = reinterpret_cast<const f32x4*>(p);
  f32x4* __restrict__ e4 = reinterpret_cast<f32x4*>(e);
  // (one vector per trip: with two sweeps' loads issued together the launch took 0.42 x the same run's AdamW at ViT-B/16's
  //  size against 0.34 x, and the same 8.65 us at the CIFAR model's)
  for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < nvec; i += stride) {
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
__global__ __launch_bounds__(OPT_THREADS) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ e,
                                                               bf16* __restrict__ shadow, long long n) {
  const long long nvec = n >> 2, stride = (long long)gridDim.x * OPT_THREADS;
  f32x4* __restrict__ p4 = reinterpret_cast<f32x4*>(p);
  f32x4* __restrict__ e4 = reinterpret_cast<f32x4*>(e);
  for (long long i = (long long)blockIdx.x * OPT_THREADS + threadIdx.x; i < nvec; i += stride) {
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

}  // namespace vitpe

using namespace vitpe;

extern "C" int vitpe_adamw_step(float* p, float* g, float* m, float* v, void* shadow_bf16, float* hp, long long n,
                                int zero_grad, hipStream_t st) {
  VITPE_REQUIRE(p && g && m && v && hp && n >= 0);
  if (!(zero_grad & 2)) hipLaunchKernelGGL(adamw_tick_kernel, dim3(1), dim3(1), 0, st, hp);   // bit 1: the caller ticked already
  if (n > 0) {
    const dim3 grid(capped_grid(n, 4096)), block(OPT_THREADS);
    if (zero_grad & 4)   // bit 2: the gradient scale is hp[HP_CLIP_SCALE] (vitpe_grad_clip wrote it)
      hipLaunchKernelGGL(adamw_kernel<HP_CLIP_SCALE>, grid, block, 0, st, p, g, m, v, (bf16*)shadow_bf16, hp, n, zero_grad & 1);
    else
      hipLaunchKernelGGL(adamw_kernel<HP_GRAD_SCALE>, grid, block, 0, st, p, g, m, v, (bf16*)shadow_bf16, hp, n, zero_grad & 1);
  }
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_adamw_groups_blocks(long long n) { return adamw_groups_blocks(n); }

extern "C" int vitpe_adamw_step_groups(float* p, float* g, float* m, float* v, void* shadow_bf16, float* hp, long long n,
                                       int zero_grad, const unsigned char* gid, long long n_gid, const float* gtab,
                                       int n_groups, hipStream_t st) {
  VITPE_REQUIRE(hp && n >= 0 && n_groups >= 1 && n_groups <= AG_MAX_GROUPS);
  VITPE_REQUIRE(n == 0 || (p && g && m && v && gid && gtab && n_gid >= (n + 7) / 8));
  VITPE_REQUIRE(aligned(p, 16) && aligned(g, 16) && aligned(m, 16) && aligned(v, 16) && aligned(shadow_bf16, 8)
                && aligned(hp, 4) && aligned(gtab, 4));
  if (!(zero_grad & 2)) hipLaunchKernelGGL(adamw_tick_kernel, dim3(1), dim3(1), 0, st, hp);   // bit 1: ticked already
  if (n > 0) {
    const dim3 grid(adamw_groups_blocks(n)), block(OPT_THREADS);
    if (zero_grad & 4)   // bit 2: the gradient scale is hp[HP_CLIP_SCALE]
      hipLaunchKernelGGL(adamw_groups_kernel<HP_CLIP_SCALE>, grid, block, 0, st, p, g, m, v, (bf16*)shadow_bf16, hp, n,
                         zero_grad & 1, gid, gtab, n_groups);
    else
      hipLaunchKernelGGL(adamw_groups_kernel<HP_GRAD_SCALE>, grid, block, 0, st, p, g, m, v, (bf16*)shadow_bf16, hp, n,
                         zero_grad & 1, gid, gtab, n_groups);
  }
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_lr_schedule(float* hp, const float* sched, int ticked, hipStream_t st) {
  VITPE_REQUIRE(hp && sched && aligned(hp, 4) && aligned(sched, 4));
  hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(1), 0, st, hp, const_cast<float*>(sched), ticked);
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_grad_clip_blocks(long long n) { return grad_clip_blocks(n); }

extern "C" int vitpe_grad_clip(const float* g, long long n, float* hp, float* partial, int n_partial, hipStream_t st) {
  VITPE_REQUIRE(hp && n >= 0 && (n == 0 || (g && partial)) && aligned(g, 4));
  const int nb = grad_clip_blocks(n);
  VITPE_REQUIRE(n_partial >= nb);
  if (nb > 0) hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(nb), dim3(256), 0, st, g, n, partial);
  hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(64), 0, st, (const float*)partial, nb, hp);
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_ema_blocks(long long n) { return ema_blocks(n); }

extern "C" int vitpe_ema_update(const float* p, float* e, float* hp, long long n, int warmup, hipStream_t st) {
  VITPE_REQUIRE(hp && n >= 0 && (n == 0 || (p && e)) && aligned(p, 16) && aligned(e, 16) && aligned(hp, 4));
  if (n == 0) return 0;
  const dim3 grid(ema_blocks(n)), block(OPT_THREADS);
  if (warmup) hipLaunchKernelGGL(ema_update_kernel<true>, grid, block, 0, st, p, e, hp, n);
  else hipLaunchKernelGGL(ema_update_kernel<false>, grid, block, 0, st, p, e, hp, n);
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_ema_swap(float* p, float* e, void* shadow_bf16, long long n, hipStream_t st) {
  VITPE_REQUIRE(n >= 0 && (n == 0 || (p && e)) && aligned(p, 16) && aligned(e, 16) && aligned(shadow_bf16, 16));
  if (n == 0) return 0;
  hipLaunchKernelGGL(ema_swap_kernel, dim3(ema_blocks(n)), dim3(OPT_THREADS), 0, st, p, e, (bf16*)shadow_bf16, n);
  VITPE_CHECK_LAUNCH();
}
