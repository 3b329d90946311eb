// Statistics of the attention probabilities of the general core, reduced on the chip: per (image, head) the mean attention
// distance, the mean row entropy, the attention mass on the class token and the class row's entropy, and optionally the
// vector-times-map product colsum[j] = sum_i w_i p_ij that attention rollout needs (reference models/vit.py:71-84: `attn`
// after .softmax(-1) and before attn_drop, never materialised here).  4 (4 + N) bytes per (image, head) instead of the
// 4 N^2 of attn_core_probs.hip.  For analysis: no backward, no dropout variant.
//
// The kernel is attn_core_probs_kernel up to the row sum l -- one workgroup per (image, head), K~ in LDS, the query
// fragments from global with rotation and folded scale, logits_T, exp2-domain softmax, xg_sum; V is neither staged nor
// read -- and then reduces the tile instead of storing it.  In the swapped S^T tile a lane (c, g) holds query i = 16 it + c
// and, per key tile jt, the keys 16 jt + 4 g + r with e_j = 2^(s_j - m), p_ij = e_j / l:
//   distance    sum_{j >= 1} e_j d(i, j) / l for i >= 1, d = sqrt(dy^2 + dx^2) of the raster coordinates
//               (y, x) = ((t - 1) / G, (t - 1) % G): the coordinates are staged once as floats (small integers, exact),
//               the square root is one v_sqrt_f32 per entry;
//   entropy     ln l + ln 2 / l . sum_j e_j (m - s_j): two non-negative terms; an entry with e_j = 0 (a padding key at
//               s_j = -1e30, or an underflow) is selected to 0 and never multiplies;
//   class mass  e_0 / l for i >= 1 (lane group 0, key tile 0, register 0).
// Order of every sum (fixed: two launches give the same bits, with or without colsum):
//   lane: key tiles ascending, r ascending;  query: xg_sum over the four key groups;  query tile: row16_sum_lane15 over its
//   16 queries;  wave: its jobs it = wave, wave + NW, .. in registers (colsum: in the wave's own LDS slab, by the lane that
//   wrote it);  workgroup: wave 0 sums the per-wave slabs in wave order and stores.
// No atomics anywhere.  The slabs (NW x 16 MT floats) live in the LDS that core_fits budgets for the unstaged V.
//
// The Makefile compiles this file once per head dimension (-DVITPE_STATS_HD=24 ...); without the macro (tools/regs.sh) it
// instantiates every head dimension of VITPE_CORE_HDS.
#include "attn_core.h"

namespace vitpe {

template <typename T, int HD, int MT, int KM, int NW>
__global__ __launch_bounds__(64 * NW) void attn_core_stats_kernel(StatsArgs sa) {
  using C = AttnCfg<T, (HD + 31) / 32 * 32, (HD + 31) / 32 * 32, MT, 1, 0>;   // (HD = 24 / 48: padded tiles, PadMap)
  constexpr bool ROPE = (KM == KM_ROPE);
  const AttnArgs& a = sa.a;
  __shared__ __attribute__((aligned(16))) T kt[C::QSZ];  // K~ (row reads only)
  __shared__ __attribute__((aligned(16))) float s_tab[KM == KM_RELATIVE ? C::TABLD : 4];
  __shared__ __attribute__((aligned(16))) float s_coef[KM == KM_POLY ? C::PESZ : 4];
  __shared__ __attribute__((aligned(16))) float s_xy[2 * C::NP];     // [x | y][token] raster coordinates, 0 for t = 0, t >= N
  __shared__ __attribute__((aligned(16))) float s_col[NW * C::NP];   // per-wave colsum slabs
  __shared__ float s_part[NW * 4];                                   // per-wave distance | entropy | class mass sums
  __shared__ float s_cls;                                            // entropy of query 0

  const int N = a.N, H = a.H, Dr = H * HD, P = N - 1;
  const int b = blockIdx.x / H, hg = blockIdx.x % H;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const T* qg = reinterpret_cast<const T*>(a.qkv) + (size_t)b * N * 3 * Dr + hg * HD;
  const size_t hoff = (ROPE && a.mode == PE_ROPE_MIXED) ? (size_t)hg * P * (HD / 2) : 0;
  const float* cosb = ROPE ? a.cos + hoff : nullptr;
  const float* sinb = ROPE ? a.sin + hoff : nullptr;
  const bool wsum = sa.weights != nullptr;   // (kernel argument: uniform)

  stage_rows<T, C, ROPE, HD>(a, qg + Dr, 3 * Dr, cosb, sinb, 1.0f, kt, C::NP, threadIdx.x, 64 * NW);
  stage_pe<C, KM>(a, hg, s_tab, s_coef, threadIdx.x, 64 * NW);
  for (int t = threadIdx.x; t < C::NP; t += 64 * NW) {
    const bool patch = t >= 1 && t < N;
    const int pi = patch ? t - 1 : 0;
    s_xy[t] = patch ? (float)(pi % a.grid) : 0.f;
    s_xy[C::NP + t] = patch ? (float)(pi / a.grid) : 0.f;
  }
  __syncthreads();

  float acc_d = 0.f, acc_e = 0.f, acc_c = 0.f;   // this wave's sums over its jobs (valid in lane 15 of every row)
  for (int it = wave; it < MT; it += NW) {
    const int i = 16 * it + c, il = min(i, N - 1), tok = max(il, 1);
    Frag<T> bq[C::HC];
#pragma unroll
    for (int cs = 0; cs < C::HC; ++cs)
      bq[cs] = ld_head_frag<T, HD, ROPE>(qg + (size_t)il * 3 * Dr, 32 * cs + 8 * g, cosb + (size_t)(tok - 1) * (HD / 2),
                                         sinb + (size_t)(tok - 1) * (HD / 2), il >= 1, a.scale * LOG2E);
    // (the query fragments are finished before the K fragment reads start: attn_core_fwd_kernel, same place)
#pragma unroll
    for (int cs = 0; cs < C::HC; ++cs) pin_frag(bq[cs]);
    __builtin_amdgcn_sched_barrier(0);
    f32x4 s[MT];
    const float m = logits_T<T, C, KM>(a, kt, bq, s_tab, s_coef, 0, it, lane, s);
    const float xi = s_xy[il], yi = s_xy[C::NP + il];
    float l = 0.f, dsum = 0.f, esum = 0.f;
#pragma unroll
    for (int jt = 0; jt < MT; ++jt) {
      const f32x4 xj = *reinterpret_cast<const f32x4*>(&s_xy[16 * jt + 4 * g]);
      const f32x4 yj = *reinterpret_cast<const f32x4*>(&s_xy[C::NP + 16 * jt + 4 * g]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float sv = s[jt][r];
        const float p = __builtin_amdgcn_exp2f(sv - m);
        s[jt][r] = p;
        l += p;
        esum += p > 0.f ? p * (m - sv) : 0.f;   // 0 ln 0 = 0: padding keys and underflowed entries add exactly 0
        const float dx = xj[r] - xi, dy = yj[r] - yi;
        float d = __builtin_amdgcn_sqrtf(dx * dx + dy * dy);
        if (jt == 0 && r == 0) d = g == 0 ? 0.f : d;   // key 0 is the class token: no distance (padding keys: p = 0)
        dsum += p * d;
      }
    }
    l = xg_sum(l);
    const float inv = __builtin_amdgcn_rcpf(l);
    const bool qok = i < N, qpatch = qok && i >= 1;
    // per-lane shares of this query's distance, entropy and class mass: rows >= N add 0, the class row no distance or mass
    float qd = qpatch ? dsum * inv : 0.f;
    float qe = qok ? esum * inv * LN2 + (g == 0 ? __builtin_amdgcn_logf(l) * LN2 : 0.f) : 0.f;   // v_log_f32 = log2
    float qc = (qpatch && g == 0) ? s[0][0] * inv : 0.f;
    qd = xg_sum(qd);
    qe = xg_sum(qe);
    qc = xg_sum(qc);
    if (it == 0 && lane == 0) s_cls = qe;   // query 0's entropy, whole after the cross-group sum
    acc_d += row16_sum_lane15(qd);
    acc_e += row16_sum_lane15(qe);
    acc_c += row16_sum_lane15(qc);
    if (wsum) {
      // colsum: w_i p_ij summed over the tile's 16 queries; lane 15 of row g folds the four keys 16 jt + 4 g + r into
      // this wave's slab (first job: store, later jobs: the same lane adds to what it stored)
      const float wi = qok ? sa.weights[(size_t)b * N + il] * inv : 0.f;
      float* slab = s_col + wave * C::NP + 4 * g;
#pragma unroll
      for (int jt = 0; jt < MT; ++jt) {
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = row16_sum_lane15(wi * s[jt][r]);
        if (c == 15) {
          f32x4* dst = reinterpret_cast<f32x4*>(slab + 16 * jt);
          if (it != wave) {
            const f32x4 o = *dst;
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += o[r];
          }
          *dst = v;
        }
      }
    }
  }
  if (lane == 15) {
    s_part[4 * wave + 0] = acc_d;
    s_part[4 * wave + 1] = acc_e;
    s_part[4 * wave + 2] = acc_c;
  }
  __syncthreads();

  if (wave == 0) {   // one wave sums the slabs in wave order (every wave ran at least one job: NW <= MT)
    if (wsum) {
      float* cg = sa.colsum + (size_t)(b * H + hg) * N;
      for (int j = lane; j < N; j += 64) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += s_col[w * C::NP + j];
        cg[j] = t;
      }
    }
    if (lane == 0) {
      float td = 0.f, te = 0.f, tc = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        td += s_part[4 * w + 0];
        te += s_part[4 * w + 1];
        tc += s_part[4 * w + 2];
      }
      float* sg = sa.stats + (size_t)(b * H + hg) * 4;
      sg[STAT_DISTANCE] = td * (sa.unit / (float)P);
      sg[STAT_ENTROPY] = te / (float)N;
      sg[STAT_CLS_MASS] = tc / (float)P;
      sg[STAT_CLS_ENTROPY] = s_cls;
    }
  }
}

template <typename T, int HD, int MT>
int launch_core_stats(const StatsArgs& sa, hipStream_t s) {
  if constexpr (!core_fits<T, HD, MT>()) {
    return (int)hipErrorNotSupported;
  } else {
    // the wave counts of attn_core_probs.hip: one wave per query tile up to 10 tiles, seven waves at 13 tiles, six at 17
    // (256 registers a lane; tools/regs.sh attn_core_stats.hip: no scratch anywhere)
    constexpr int NW = MT <= 10 ? MT : MT <= 13 ? (MT + 1) / 2 : 6;
    const dim3 grid((unsigned)(sa.a.B * sa.a.H));
#define VITPE_STATS_LAUNCH(KM) hipLaunchKernelGGL((attn_core_stats_kernel<T, HD, MT, KM, NW>), grid, dim3(64 * NW), 0, s, sa)
    switch (sa.a.mode) {
      case PE_RELATIVE: VITPE_STATS_LAUNCH(KM_RELATIVE); break;
      case PE_POLY: VITPE_STATS_LAUNCH(KM_POLY); break;
      case PE_ROPE_AXIAL:
      case PE_ROPE_MIXED: VITPE_STATS_LAUNCH(KM_ROPE); break;
      default: VITPE_STATS_LAUNCH(KM_PLAIN); break;
    }
#undef VITPE_STATS_LAUNCH
    VITPE_CHECK_LAUNCH();
  }
}

#define VITPE_STATS_INST(T, HD, MT) template int launch_core_stats<T, HD, MT>(const StatsArgs&, hipStream_t);
#define VITPE_STATS_INST_HD(HD) VITPE_CORE_MTS(VITPE_STATS_INST, bf16, HD) VITPE_CORE_MTS(VITPE_STATS_INST, float, HD)
#ifdef VITPE_STATS_HD
VITPE_STATS_INST_HD(VITPE_STATS_HD)
#else
#define VITPE_STATS_INST_X(HD, OWN_TU) VITPE_STATS_INST_HD(HD)
VITPE_CORE_HDS(VITPE_STATS_INST_X)
#endif

}  // namespace vitpe
