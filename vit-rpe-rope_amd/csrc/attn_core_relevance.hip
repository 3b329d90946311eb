// Gradient-weighted attention relevance of the general core, reduced on the chip (Chefer, Gur & Wolf, "Generic
// Attention-model Explainability", ICCV 2021: R <- R + A~ R with A~ = mean_h max(0, G . A)).  Per (image, head), with
//   A = the reference's `attn` after .softmax(-1) and before attn_drop (models/vit.py:71-84),
//   G = dy/dA = dO_h V_h^T  (V fixed: what a backward hook on `attn` sees, NOT the gradient w.r.t. the logits),
// the kernel returns colsum[j] = sum_i w_i f(G_ij A_ij), f = max(0, .) with clamp, the identity without: the
// vector-times-map product one propagation step v <- v + v A~ needs.  Neither A nor G is ever stored.
//
// The kernel is attn_core_stats_kernel up to the row sum l -- one workgroup per (image, head), K~ in LDS, the query
// fragments from global with rotation and folded scale, logits_T, exp2-domain softmax, xg_sum.  V is staged once into a
// second LDS tile (plain layout, no rotation, scale 1; row reads only, so the tile has no zero tail) and the query's dO
// fragments are loaded like bq (plain layout, scale 1).  After the row sum the tile of G^T = V dO^T is formed on the matrix
// core one key tile at a time, in the S^T layout: a lane (c, g) holds query i = 16 it + c and, for key tile jt, the keys
// j = 16 jt + 4 g + r -- A operand: V rows 16 jt + c (ld_frag, as logits_T reads K~), B operand: the query's dO
// fragment, fp32 accumulation -- so G_ij meets e_j = 2^(s_j - m) in the same register and one f32x4 of G is live at a time.
// Padding: a key j >= N (last tile only) and a query i >= N are SELECTED to 0 (never multiplied: the V tile's rows past N
// and the dO row a padding query re-reads may hold anything); the padded columns of hd 24 / 48 are zero in both operands
// (PadMap, plain layout).
// Order of every sum (fixed: two launches give the same bits):
//   query tile: row16_sum_lane15 over its 16 queries;  wave: its jobs it = wave, wave + NW, .. in the wave's own LDS slab,
//   by the lane that wrote it;  workgroup: wave 0 sums the per-wave slabs in wave order and stores.  No atomics anywhere.
// LDS: K~ + V + bias table / coefficients + NW x 16 MT slab floats -- more than core_fits budgets, so the kernel has its
// own rule (relevance_lds_bytes / relevance_waves): the wave count of the statistics kernel, lowered until the real
// __shared__ total fits 160 KB; where one wave does not fit the geometry is refused ("Attention relevance").
//
// The Makefile compiles this file once per head dimension (-DVITPE_RELEVANCE_HD=24 ...); without the macro (tools/regs.sh)
// it instantiates every head dimension of VITPE_CORE_HDS.
#include "attn_core.h"

namespace vitpe {

// the kernel's __shared__ total in bytes: its declarations below, one for one
template <typename T, int HD, int MT, int KM, int NW>
constexpr size_t relevance_lds_bytes() {
  using C = AttnCfg<T, (HD + 31) / 32 * 32, (HD + 31) / 32 * 32, MT, 1, 0>;
  return 2 * (size_t)C::QSZ * sizeof(T) + sizeof(float) * ((KM == KM_RELATIVE ? C::TABLD : 4) + (KM == KM_POLY ? C::PESZ : 4) +
                                                            (size_t)NW * C::NP);
}
constexpr size_t RELEVANCE_LDS_MAX = 160 * 1024;
template <typename T, int HD, int MT, int NW>
constexpr bool relevance_fits_nw() {   // every PE class of the geometry runs at the same wave count
  return relevance_lds_bytes<T, HD, MT, KM_PLAIN, NW>() <= RELEVANCE_LDS_MAX &&
         relevance_lds_bytes<T, HD, MT, KM_RELATIVE, NW>() <= RELEVANCE_LDS_MAX &&
         relevance_lds_bytes<T, HD, MT, KM_POLY, NW>() <= RELEVANCE_LDS_MAX &&
         relevance_lds_bytes<T, HD, MT, KM_ROPE, NW>() <= RELEVANCE_LDS_MAX;
}
// the wave counts of attn_core_stats.hip (one wave per query tile up to 10 tiles, seven waves at 13 tiles, six at 17),
// lowered while the slabs do not fit; 0: not even one wave fits (K~ and V alone are too large)
template <typename T, int HD, int MT, int NW = (MT <= 10 ? MT : MT <= 13 ? (MT + 1) / 2 : 6)>
constexpr int relevance_waves() {
  if constexpr (MT > 17) return 0;
  else if constexpr (relevance_fits_nw<T, HD, MT, NW>()) return NW;
  else if constexpr (NW > 1) return relevance_waves<T, HD, MT, NW - 1>();
  else return 0;
}

template <typename T, int HD, int MT, int KM, int NW>
__global__ __launch_bounds__(64 * NW) void attn_core_relevance_kernel(RelevanceArgs ra) {
  using C = AttnCfg<T, (HD + 31) / 32 * 32, (HD + 31) / 32 * 32, MT, 1, 0>;   // (HD = 24 / 48: padded tiles, PadMap)
  constexpr bool ROPE = (KM == KM_ROPE);
  static_assert(relevance_lds_bytes<T, HD, MT, KM, NW>() <= RELEVANCE_LDS_MAX && NW >= 1 && NW <= MT, "LDS budget / wave count");
  const AttnArgs& a = ra.a;
  __shared__ __attribute__((aligned(16))) T kt[C::QSZ];  // K~ (row reads only)
  __shared__ __attribute__((aligned(16))) T vt[C::QSZ];  // V  (row reads only: rows >= N are never selected)
  __shared__ __attribute__((aligned(16))) float s_tab[KM == KM_RELATIVE ? C::TABLD : 4];
  __shared__ __attribute__((aligned(16))) float s_coef[KM == KM_POLY ? C::PESZ : 4];
  __shared__ __attribute__((aligned(16))) float s_col[NW * C::NP];   // per-wave colsum slabs

  const int N = a.N, H = a.H, Dr = H * HD, P = N - 1;
  const int b = blockIdx.x / H, hg = blockIdx.x % H;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const T* qg = reinterpret_cast<const T*>(a.qkv) + (size_t)b * N * 3 * Dr + hg * HD;
  const T* dog = reinterpret_cast<const T*>(a.dout) + (size_t)b * N * Dr + hg * HD;
  const size_t hoff = (ROPE && a.mode == PE_ROPE_MIXED) ? (size_t)hg * P * (HD / 2) : 0;
  const float* cosb = ROPE ? a.cos + hoff : nullptr;
  const float* sinb = ROPE ? a.sin + hoff : nullptr;
  const bool clamp = ra.clamp != 0;   // (kernel argument: uniform)

  stage_rows<T, C, ROPE, HD>(a, qg + Dr, 3 * Dr, cosb, sinb, 1.0f, kt, C::NP, threadIdx.x, 64 * NW);
  stage_rows<T, C, false, HD>(a, qg + 2 * Dr, 3 * Dr, nullptr, nullptr, 1.0f, vt, C::NP, threadIdx.x, 64 * NW);
  stage_pe<C, KM>(a, hg, s_tab, s_coef, threadIdx.x, 64 * NW);
  __syncthreads();

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
    // the query's dO row, plain layout: in flight under the logits
    Frag<T> bdo[C::HC];
#pragma unroll
    for (int cs = 0; cs < C::HC; ++cs)
      bdo[cs] = ld_head_frag<T, HD, false>(dog + (size_t)il * Dr, 32 * cs + 8 * g, nullptr, nullptr, false, 1.0f);
    f32x4 s[MT];
    const float m = logits_T<T, C, KM>(a, kt, bq, s_tab, s_coef, 0, it, lane, s);
    float l = 0.f;
#pragma unroll
    for (int jt = 0; jt < MT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(s[jt][r] - m);
        s[jt][r] = p;
        l += p;
      }
    l = xg_sum(l);
    const float inv = __builtin_amdgcn_rcpf(l);
    const bool qok = i < N;
    const float wi = qok ? ra.weights[(size_t)b * N + il] : 0.f;
    // G^T tile by tile: w_i f(G_ij p_ij) summed over the tile's 16 queries; lane 15 of row g folds the four keys
    // 16 jt + 4 g + r into this wave's slab (first job: store, later jobs: the same lane adds to what it stored)
    const T* vrow = vt + c * C::LDH + 8 * g;
    float* slab = s_col + wave * C::NP + 4 * g;
#pragma unroll
    for (int jt = 0; jt < MT; ++jt) {
      f32x4 gt = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int cs = 0; cs < C::HC; ++cs) mma(ld_frag(vrow + 16 * jt * C::LDH + 32 * cs), bdo[cs], gt);
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = qok && (jt < MT - 1 || 16 * jt + 4 * g + r < N);   // padding keys only exist in the last tile
        const float x = gt[r] * (s[jt][r] * inv);
        const float f = clamp ? fmaxf(x, 0.f) : x;
        v[r] = row16_sum_lane15(ok ? wi * f : 0.f);
      }
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
  __syncthreads();

  if (wave == 0) {   // one wave sums the slabs in wave order (every wave ran at least one job: NW <= MT)
    float* cg = ra.colsum + (size_t)(b * H + hg) * N;
    for (int j = lane; j < N; j += 64) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) t += s_col[w * C::NP + j];
      cg[j] = t;
    }
  }
}

template <typename T, int HD, int MT>
int launch_core_relevance(const RelevanceArgs& ra, hipStream_t s) {
  constexpr int NW = relevance_waves<T, HD, MT>();
  if constexpr (NW == 0) {
    return (int)hipErrorNotSupported;
  } else {
    const dim3 grid((unsigned)(ra.a.B * ra.a.H));
#define VITPE_RELEVANCE_LAUNCH(KM) \
  hipLaunchKernelGGL((attn_core_relevance_kernel<T, HD, MT, KM, NW>), grid, dim3(64 * NW), 0, s, ra)
    switch (ra.a.mode) {
      case PE_RELATIVE: VITPE_RELEVANCE_LAUNCH(KM_RELATIVE); break;
      case PE_POLY: VITPE_RELEVANCE_LAUNCH(KM_POLY); break;
      case PE_ROPE_AXIAL:
      case PE_ROPE_MIXED: VITPE_RELEVANCE_LAUNCH(KM_ROPE); break;
      default: VITPE_RELEVANCE_LAUNCH(KM_PLAIN); break;
    }
#undef VITPE_RELEVANCE_LAUNCH
    VITPE_CHECK_LAUNCH();
  }
}

#define VITPE_RELEVANCE_INST(T, HD, MT) template int launch_core_relevance<T, HD, MT>(const RelevanceArgs&, hipStream_t);
#define VITPE_RELEVANCE_INST_HD(HD) VITPE_CORE_MTS(VITPE_RELEVANCE_INST, bf16, HD) VITPE_CORE_MTS(VITPE_RELEVANCE_INST, float, HD)
#ifdef VITPE_RELEVANCE_HD
VITPE_RELEVANCE_INST_HD(VITPE_RELEVANCE_HD)
#else
#define VITPE_RELEVANCE_INST_X(HD, OWN_TU) VITPE_RELEVANCE_INST_HD(HD)
VITPE_CORE_HDS(VITPE_RELEVANCE_INST_X)
#endif

}  // namespace vitpe
