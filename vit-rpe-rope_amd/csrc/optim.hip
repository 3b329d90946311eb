// AdamW with parameter groups and the per-step learning-rate schedule of the captured step (TrainEngine.set_param_groups /
// set_lr_schedule; DESIGN.md, "Parameter groups and LR schedule").  adamw_groups_kernel is adamw_kernel (misc.hip) with a
// per-granule (lr, weight decay) scale pair and 16-byte accesses: one lane per 8-element granule of the flat buffers, a
// grid capped at 256 CUs x 8 workgroups, grid-stride for the rest, the n % 8 last elements one lane each; no atomics,
// no LDS.  lr_schedule_kernel is one lane of fp64 arithmetic in front of it.
#include "common.h"

namespace vitpe {

constexpr int AG_THREADS = 256;
constexpr int AG_GRID_CAP = 256 * 8;
constexpr int AG_MAX_GROUPS = 256;   // the map is one byte per granule

// workgroups for n elements: one lane per 8-element granule, capped; n in 1..7 still needs one (the tail)
static inline int adamw_groups_blocks(long long n) {
  if (n <= 0) return 0;
  const long long ngran = (n + 7) >> 3;
  const long long want = (ngran + AG_THREADS - 1) / AG_THREADS;
  return (int)(want < 1 ? 1 : (want > AG_GRID_CAP ? AG_GRID_CAP : want));
}

// adamw_tick_kernel's three lines (misc.hip keeps its own: its object stays as compiled)
__global__ void adamw_groups_tick_kernel(float* hp) {
  const float step = hp[5] + 1.0f;
  hp[5] = step;
  hp[6] = 1.0f - powf(hp[1], step);
  hp[7] = 1.0f - powf(hp[2], step);
}

// One element of adamw_kernel, its expressions as written there (the same contraction under -ffp-contract=on): with
// lr == hp[0] and wd == hp[4] the five outputs are adamw_kernel's bit for bit.
struct AgConst { float b1, b2, eps, bc1, inv_sqrt_bc2, gs; };
VITPE_DEV void ag_element(float& pi, float& gi_io, float& mi_io, float& vi_io, float lr, float wd, const AgConst& c) {
  const float b1 = c.b1, b2 = c.b2, eps = c.eps, inv_sqrt_bc2 = c.inv_sqrt_bc2;
  const float step_size = lr / c.bc1;
  const float gi = gi_io * c.gs;
  pi = pi * (1.0f - lr * wd);
  const float mi = b1 * mi_io + (1.0f - b1) * gi;
  const float vi = b2 * vi_io + (1.0f - b2) * gi * gi;
  pi -= step_size * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
  mi_io = mi;
  vi_io = vi;
}

// GS: the hp slot of the gradient scale, as adamw_kernel's.  gid: one byte per granule (clamped to n_groups - 1: a bad
// map never reads outside gtab); gtab: n_groups pairs (lr scale, weight-decay scale) applied to hp[0] and hp[4].
template <int GS>
__global__ __launch_bounds__(AG_THREADS) void adamw_groups_kernel(float* __restrict__ p, float* __restrict__ g,
                                                                  float* __restrict__ m, float* __restrict__ v,
                                                                  bf16* __restrict__ shadow, const float* __restrict__ hp,
                                                                  long long n, int zero_grad,
                                                                  const unsigned char* __restrict__ gid,
                                                                  const float* __restrict__ gtab, int n_groups) {
  const float lr0 = hp[0], wd0 = hp[4], bc2 = hp[7];
  AgConst c;
  c.b1 = hp[1]; c.b2 = hp[2]; c.eps = hp[3]; c.bc1 = hp[6]; c.gs = hp[GS];
  c.inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
  const long long nvec = n >> 3, stride = (long long)gridDim.x * AG_THREADS;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (long long i = (long long)blockIdx.x * AG_THREADS + threadIdx.x; i < nvec; i += stride) {
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
        ag_element(pi, gi, mi, vi, lr, wd, c);
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
    ag_element(pi, gi, mi, vi, lr, wd, c);
    p[t] = pi; m[t] = mi; v[t] = vi;
    if (shadow != nullptr) shadow[t] = (bf16)pi;
    if (zero_grad) g[t] = 0.f;
  }
}

// Linear warm-up, then cos^2 (= the cosine annealing of torch's CosineAnnealingLR without the 1 + cos cancellation near its
// end); sched = {base, min, W, T, s0, origin, last lr, -}.  One lane, fp64; writes hp[0] and sched[6] only.
__global__ void lr_schedule_kernel(float* hp, float* sched, int ticked) {
  const double base = sched[0], lo = sched[1], W = sched[2], T = sched[3], s0 = sched[4];
  double k = (double)hp[5] - (double)sched[5] - (ticked ? 1.0 : 0.0);
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
  hp[0] = out;
  sched[6] = out;
}

static inline bool ag_aligned(const void* q, unsigned long long a) { return ((unsigned long long)q & (a - 1)) == 0; }

}  // namespace vitpe

using namespace vitpe;

extern "C" int vitpe_adamw_groups_blocks(long long n) { return adamw_groups_blocks(n); }

extern "C" int vitpe_adamw_step_groups(float* p, float* g, float* m, float* v, void* shadow_bf16, float* hp, long long n,
                                       int zero_grad, const unsigned char* gid, long long n_gid, const float* gtab,
                                       int n_groups, hipStream_t st) {
  VITPE_REQUIRE(hp && n >= 0 && n_groups >= 1 && n_groups <= AG_MAX_GROUPS);
  VITPE_REQUIRE(n == 0 || (p && g && m && v && gid && gtab && n_gid >= (n + 7) / 8));
  VITPE_REQUIRE(ag_aligned(p, 16) && ag_aligned(g, 16) && ag_aligned(m, 16) && ag_aligned(v, 16) && ag_aligned(shadow_bf16, 8)
                && ag_aligned(hp, 4) && ag_aligned(gtab, 4));
  if (!(zero_grad & 2)) hipLaunchKernelGGL(adamw_groups_tick_kernel, dim3(1), dim3(1), 0, st, hp);   // bit 1: ticked already
  if (n > 0) {
    const dim3 grid(adamw_groups_blocks(n)), block(AG_THREADS);
    if (zero_grad & 4)   // bit 2: the gradient scale is hp[9] (vitpe_grad_clip wrote it)
      hipLaunchKernelGGL(adamw_groups_kernel<9>, grid, block, 0, st, p, g, m, v, (bf16*)shadow_bf16, hp, n, zero_grad & 1,
                         gid, gtab, n_groups);
    else
      hipLaunchKernelGGL(adamw_groups_kernel<8>, grid, block, 0, st, p, g, m, v, (bf16*)shadow_bf16, hp, n, zero_grad & 1,
                         gid, gtab, n_groups);
  }
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_lr_schedule(float* hp, const float* sched, int ticked, hipStream_t st) {
  VITPE_REQUIRE(hp && sched && ag_aligned(hp, 4) && ag_aligned(sched, 4));
  hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(1), 0, st, hp, const_cast<float*>(sched), ticked);
  VITPE_CHECK_LAUNCH();
}
