// The attention probabilities of the general core: softmax(QK^T * hd^-0.5 [+ bias]) itself, written out in fp32
// (reference models/vit.py:71-84: `attn` after .softmax(-1) and before attn_drop -- what a forward hook on softmax sees).
// For analysis (attention maps, class-token saliency, attention distance): no backward, no dropout variant.
//
// The kernel is attn_core_fwd_kernel (attn_core.h) up to the row sum -- one workgroup per (image, head), K~ in LDS, the
// query fragments from global with rotation and folded scale, logits_T, exp2-domain softmax, xg_sum -- and then, instead
// of acc_to_frag -> P.V, stores p / l.  V is neither staged nor read.
//
// Store layout: in the swapped S^T tile a lane (c, g) holds query i = 16 it + c and, per key tile jt, the four consecutive
// keys 16 jt + 4 g + r.  One store instruction per key tile: the four lane groups of a query write the 64 contiguous bytes
// of 16 keys, the 16 queries of the tile 16 rows 4 N bytes apart; the MT instructions of a job walk along the rows.  A row
// of probs starts at byte 4 N (..), 16-byte aligned only when N is a multiple of 4: there the quad is one 16-byte store
// (a quad is then wholly inside or wholly outside N), otherwise four dword stores, each guarded by its own key.  Nothing
// is written at i >= N or j >= N.
//
// The Makefile compiles this file once per head dimension (-DVITPE_PROBS_HD=24 ...); without the macro (tools/regs.sh) it
// instantiates every head dimension of VITPE_CORE_HDS.
#include "attn_core.h"

namespace vitpe {

template <typename T, int HD, int MT, int KM, int NW>
__global__ __launch_bounds__(64 * NW) void attn_core_probs_kernel(AttnArgs a) {
  using C = AttnCfg<T, (HD + 31) / 32 * 32, (HD + 31) / 32 * 32, MT, 1, 0>;   // (HD = 24 / 48: padded tiles, PadMap)
  constexpr bool ROPE = (KM == KM_ROPE);
  __shared__ __attribute__((aligned(16))) T kt[C::QSZ];  // K~ (row reads only)
  __shared__ __attribute__((aligned(16))) float s_tab[KM == KM_RELATIVE ? C::TABLD : 4];
  __shared__ __attribute__((aligned(16))) float s_coef[KM == KM_POLY ? C::PESZ : 4];

  const int N = a.N, H = a.H, Dr = H * HD, P = N - 1;
  const int b = blockIdx.x / H, hg = blockIdx.x % H;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const T* qg = reinterpret_cast<const T*>(a.qkv) + (size_t)b * N * 3 * Dr + hg * HD;
  const size_t hoff = (ROPE && a.mode == PE_ROPE_MIXED) ? (size_t)hg * P * (HD / 2) : 0;
  const float* cosb = ROPE ? a.cos + hoff : nullptr;
  const float* sinb = ROPE ? a.sin + hoff : nullptr;

  stage_rows<T, C, ROPE, HD>(a, qg + Dr, 3 * Dr, cosb, sinb, 1.0f, kt, C::NP, threadIdx.x, 64 * NW);
  stage_pe<C, KM>(a, hg, s_tab, s_coef, threadIdx.x, 64 * NW);
  __syncthreads();

  // cls_only: the query-tile job it = 0 alone (wave 0), of which row 0 is stored -- the same instructions on the same
  // operands as row 0 of the full result
  const bool cls = a.cls_only != 0;
  const int njobs = cls ? 1 : MT;
  float* pg = reinterpret_cast<float*>(a.out) + (size_t)(b * H + hg) * N * (cls ? 1 : (size_t)N);
  const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0;   // every row 16-byte aligned
  for (int it = wave; it < njobs; it += NW) {
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
    if (cls ? (c == 0) : (i < N)) {
      float* row = cls ? pg : pg + (size_t)i * N;
#pragma unroll
      for (int jt = 0; jt < MT; ++jt) {
        const int j0 = 16 * jt + 4 * g;
        if (vec) {
          if (jt < MT - 1 || j0 < N)   // padding keys only exist in the last tile
            *reinterpret_cast<f32x4*>(row + j0) = (f32x4){s[jt][0] * inv, s[jt][1] * inv, s[jt][2] * inv, s[jt][3] * inv};
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (jt < MT - 1 || j0 + r < N) row[j0 + r] = s[jt][r] * inv;
        }
      }
    }
  }
}

template <typename T, int HD, int MT>
int launch_core_probs(const AttnArgs& a, hipStream_t s) {
  if constexpr (!core_fits<T, HD, MT>()) {
    return (int)hipErrorNotSupported;
  } else {
    // one wave per query tile up to 10 tiles; 13 tiles: seven waves (two rounds), 17 tiles: six waves (three rounds) -- 256
    // registers a lane instead of 128 / 168, at which a few instantiations (relative bias at 17 tiles, fp32 rope at 13)
    // spilled 1-14 VGPRs (tools/regs.sh attn_core_probs.hip: no scratch anywhere now)
    constexpr int NW = MT <= 10 ? MT : MT <= 13 ? (MT + 1) / 2 : 6;
    const dim3 grid((unsigned)(a.B * a.H));
#define VITPE_PROBS_LAUNCH(KM) hipLaunchKernelGGL((attn_core_probs_kernel<T, HD, MT, KM, NW>), grid, dim3(64 * NW), 0, s, a)
    switch (a.mode) {
      case PE_RELATIVE: VITPE_PROBS_LAUNCH(KM_RELATIVE); break;
      case PE_POLY: VITPE_PROBS_LAUNCH(KM_POLY); break;
      case PE_ROPE_AXIAL:
      case PE_ROPE_MIXED: VITPE_PROBS_LAUNCH(KM_ROPE); break;
      default: VITPE_PROBS_LAUNCH(KM_PLAIN); break;
    }
#undef VITPE_PROBS_LAUNCH
    VITPE_CHECK_LAUNCH();
  }
}

#define VITPE_PROBS_INST(T, HD, MT) template int launch_core_probs<T, HD, MT>(const AttnArgs&, hipStream_t);
#define VITPE_PROBS_INST_HD(HD) VITPE_CORE_MTS(VITPE_PROBS_INST, bf16, HD) VITPE_CORE_MTS(VITPE_PROBS_INST, float, HD)
#ifdef VITPE_PROBS_HD
VITPE_PROBS_INST_HD(VITPE_PROBS_HD)
#else
#define VITPE_PROBS_INST_X(HD, OWN_TU) VITPE_PROBS_INST_HD(HD)
VITPE_CORE_HDS(VITPE_PROBS_INST_X)
#endif

}  // namespace vitpe
