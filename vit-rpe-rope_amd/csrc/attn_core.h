// Kernel templates of the general attention core (attn_core.hip: head dimensions 32 / 64, the C ABI and the fused
// hd-64 forward; attn_core_hd.hip: the padded head dimensions 24 / 48 and 96 / 128, one translation unit each;
// attn_core_probs.hip: the softmax probabilities themselves, every head dimension, one translation unit each;
// attn_core_stats.hip: their statistics reduced on the chip, likewise; attn_core_relevance.hip: the gradient-weighted
// relevance product, likewise).
#pragma once
#include "attn_common.h"
#include "philox.h"
#include <type_traits>

namespace vitpe {

// 16 bytes of row `rowp` (feature 0 of the head) at feature f0, rotated (rotate-half pairs
// (f, f+HD/2), rope_utils.py:85-101) with this token's cos/sin row and scaled
template <typename T, int HD, bool ROPE>
VITPE_DEV Chunk16 ld_rot_chunk(const T* rowp, int f0, const float* cs, const float* sn, bool rot, float sc) {
  constexpr int CHN = CH<T>::n;
  const Chunk16 x = *reinterpret_cast<const Chunk16*>(rowp + f0);
  if (!(ROPE && rot) && sc == 1.0f) return x;
  float f[CHN];
  chunk_to_f32<T>(x, f);
  if (ROPE && rot) {
    const bool lo = f0 < HD / 2;
    const Chunk16 y = *reinterpret_cast<const Chunk16*>(rowp + (lo ? f0 + HD / 2 : f0 - HD / 2));
    float p[CHN];
    chunk_to_f32<T>(y, p);
    const int ci = lo ? f0 : f0 - HD / 2;
    const float sg = lo ? -1.f : 1.f;
#pragma unroll
    for (int t = 0; t < CHN; ++t) f[t] = f[t] * cs[ci + t] + sg * p[t] * sn[ci + t];
  }
#pragma unroll
  for (int t = 0; t < CHN; ++t) f[t] *= sc;
  return f32_to_chunk<T>(f);
}

// K32-chunk operand fragment (8 elements at feature f0) of a global row
template <int HD, bool ROPE>
VITPE_DEV Frag<bf16> ld_rot_frag(const bf16* rowp, int f0, const float* cs, const float* sn, bool rot, float sc) {
  Frag<bf16> f;
  f.v = __builtin_bit_cast(bf16x8, ld_rot_chunk<bf16, HD, ROPE>(rowp, f0, cs, sn, rot, sc));
  return f;
}
template <int HD, bool ROPE>
VITPE_DEV Frag<float> ld_rot_frag(const float* rowp, int f0, const float* cs, const float* sn, bool rot, float sc) {
  Frag<float> f;
  const Chunk16 a = ld_rot_chunk<float, HD, ROPE>(rowp, f0, cs, sn, rot, sc);
  const Chunk16 b = ld_rot_chunk<float, HD, ROPE>(rowp, f0 + 4, cs, sn, rot, sc);
#pragma unroll
  for (int t = 0; t < 4; ++t) { f.v[t] = __uint_as_float(a[t]); f.v[4 + t] = __uint_as_float(b[t]); }
  return f;
}

// ---- padded head dimensions (HD = 24, 48) ------------------------------------------------------------------------------
// The LDS tiles, fragments and AttnCfg run at HDP = roundup(HD, 32): hd 24 on the hd-32 layout, hd 48 on the hd-64 one
// (row strides stay == 2 mod 4 slots).  A tile position p < HDP holds
//   plain layout  (V, dO; q and k without rotation): feature p for p < HD, zero above;
//   rotary layout (q~, k~ under RoPE): the two rotate-half halves HDP/2 apart -- p < HD/2 holds feature p, HDP/2 <= p <
//                 HDP/2 + HD/2 holds feature p - HDP/2 + HD/2, the rest zero -- so the partner of a position is +-HDP/2
//                 as at hd 32 / 64 (same register of the tile NT/2 over in the [feature][token] accumulators).
// The contractions over the head dimension do not see the order (q~ and k~ share it) and zero positions add nothing;
// global memory is only ever touched at the HD real features (the rest of a row is the next head's).
template <int HD, bool ROT>
struct PadMap {
  static constexpr int HDP = (HD + 31) / 32 * 32, H2 = HD / 2, HP = HDP / 2;
  // first feature of the run of n positions at p, and how many of them are real: 0, n, or n / 2 (8-runs at hd 24, rotary)
  static constexpr int feat(int p) { return (ROT && p >= HP) ? p - HP + H2 : p; }
  static constexpr int nreal(int p, int n) {
    const int q = (ROT && p >= HP) ? p - HP : p, lim = ROT ? H2 : HD;
    return q >= lim ? 0 : (lim - q < n ? lim - q : n);
  }
};
typedef __attribute__((ext_vector_type(2))) uint32_t Chunk8;

// the first nr elements of a 16-B chunk (nr = CH<T>::n: one 16-B load, else one 8-B load and a zero upper half)
template <typename T>
VITPE_DEV Chunk16 ld_chunk_part(const T* p, int nr) {
  if (nr == CH<T>::n) return *reinterpret_cast<const Chunk16*>(p);
  const Chunk8 h = *reinterpret_cast<const Chunk8*>(p);
  return (Chunk16){h[0], h[1], 0u, 0u};
}

// ld_rot_chunk at tile position p0 of a padded head (PadMap, rotary layout under ROPE): zero past the real features; at
// hd 24 (HD/2 = 12) an 8-run of bf16 may hold 4 real features, read with 8-B loads, its partner likewise
template <typename T, int HD, bool ROPE>
VITPE_DEV Chunk16 ld_rot_chunk_pad(const T* rowp, int p0, const float* cs, const float* sn, bool rot, float sc) {
  using M = PadMap<HD, ROPE>;
  constexpr int CHN = CH<T>::n;
  const int nr = M::nreal(p0, CHN);
  if (nr == 0) return (Chunk16){0u, 0u, 0u, 0u};
  const int f0 = M::feat(p0);
  const Chunk16 x = ld_chunk_part<T>(rowp + f0, nr);
  if (!(ROPE && rot) && sc == 1.0f) return x;
  float f[CHN];
  chunk_to_f32<T>(x, f);
  if (ROPE && rot) {
    const bool lo = f0 < HD / 2;
    const Chunk16 y = ld_chunk_part<T>(rowp + (lo ? f0 + HD / 2 : f0 - HD / 2), nr);
    float p[CHN];
    chunk_to_f32<T>(y, p);
    const int ci = lo ? f0 : f0 - HD / 2;
    const float sg = lo ? -1.f : 1.f;
#pragma unroll
    for (int t = 0; t < CHN; ++t)
      if (t < nr) f[t] = f[t] * cs[ci + t] + sg * p[t] * sn[ci + t];
  }
#pragma unroll
  for (int t = 0; t < CHN; ++t) f[t] *= sc;
  return f32_to_chunk<T>(f);
}

// K32-chunk operand fragment (8 elements at tile position p0) of a global row, any compiled head dimension
template <typename T, int HD, bool ROPE>
VITPE_DEV Frag<T> ld_head_frag(const T* rowp, int p0, const float* cs, const float* sn, bool rot, float sc) {
  if constexpr (HD % 32 == 0) {
    return ld_rot_frag<HD, ROPE>(rowp, p0, cs, sn, rot, sc);
  } else {
    Frag<T> f;
    if constexpr (sizeof(T) == 2) {
      f.v = __builtin_bit_cast(bf16x8, ld_rot_chunk_pad<T, HD, ROPE>(rowp, p0, cs, sn, rot, sc));
    } else {
      const Chunk16 a = ld_rot_chunk_pad<T, HD, ROPE>(rowp, p0, cs, sn, rot, sc);
      const Chunk16 b = ld_rot_chunk_pad<T, HD, ROPE>(rowp, p0 + 4, cs, sn, rot, sc);
#pragma unroll
      for (int t = 0; t < 4; ++t) { f.v[t] = __uint_as_float(a[t]); f.v[4 + t] = __uint_as_float(b[t]); }
    }
    return f;
  }
}

// does the 16-feature accumulator tile dt hold a real feature?  (hd 48, plain layout: tile 3 is all padding)
template <int HD, bool ROT>
constexpr bool tile_live(int dt) { return PadMap<HD, ROT>::nreal(16 * dt, 16) > 0; }

// 16-B store of two adjacent [feature][token] accumulator tiles (features 16 nt0 .. 16 nt0 + 31 of the lane's token row):
// one v_permlane16_swap per dword gives every lane 8 CONTIGUOUS features (as tail2.hip's t2_store_pair)
template <bool NT = false>
VITPE_DEV void f64_store_pair(bf16* rowp, int nt0, int g, const f32x4& o0, const f32x4& o1) {
  uint32_t lo[2], hi[2];
#pragma unroll
  for (int w2 = 0; w2 < 2; ++w2) {
    bf16x2 pa, pb;
    pa[0] = (bf16)o0[2 * w2]; pa[1] = (bf16)o0[2 * w2 + 1];
    pb[0] = (bf16)o1[2 * w2]; pb[1] = (bf16)o1[2 * w2 + 1];
    const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(uint32_t, pa), __builtin_bit_cast(uint32_t, pb), false, false);
    lo[w2] = r[0]; hi[w2] = r[1];
  }
  const Chunk16 v = {lo[0], lo[1], hi[0], hi[1]};
  Chunk16* dst = reinterpret_cast<Chunk16*>(rowp + 16 * (nt0 + (g & 1)) + 8 * (g >> 1));
  if (NT) __builtin_nontemporal_store(v, dst);   // (read again only by a much later kernel)
  else *dst = v;
}

// f64_store_pair of a head of any compiled dimension: a padded head stores its real features only (8 or 4 of a lane's 8)
// -- its padded positions would land in the next head's columns, another workgroup's
template <int HD, bool ROT>
VITPE_DEV void head_store_pair(bf16* rowp, int nt0, int g, const f32x4& o0, const f32x4& o1) {
  if constexpr (HD % 32 == 0) {
    f64_store_pair(rowp, nt0, g, o0, o1);
  } else {
    using M = PadMap<HD, ROT>;
    uint32_t lo[2], hi[2];
#pragma unroll
    for (int w2 = 0; w2 < 2; ++w2) {
      bf16x2 pa, pb;
      pa[0] = (bf16)o0[2 * w2]; pa[1] = (bf16)o0[2 * w2 + 1];
      pb[0] = (bf16)o1[2 * w2]; pb[1] = (bf16)o1[2 * w2 + 1];
      const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(uint32_t, pa), __builtin_bit_cast(uint32_t, pb), false, false);
      lo[w2] = r[0]; hi[w2] = r[1];
    }
    const int p = 16 * (nt0 + (g & 1)) + 8 * (g >> 1), nr = M::nreal(p, 8);
    bf16* dst = rowp + M::feat(p);
    if (nr == 8) *reinterpret_cast<Chunk16*>(dst) = (Chunk16){lo[0], lo[1], hi[0], hi[1]};
    else if (nr == 4) *reinterpret_cast<Chunk8*>(dst) = (Chunk8){lo[0], lo[1]};
  }
}
// st4 of the four features at tile position p (a multiple of 4) of a head of any compiled dimension
template <int HD, bool ROT, typename T>
VITPE_DEV void head_st4(T* rowp, int p, float x0, float x1, float x2, float x3) {
  if constexpr (HD % 32 == 0) {
    st4(rowp + p, x0, x1, x2, x3);
  } else {
    using M = PadMap<HD, ROT>;
    if (M::nreal(p, 4) > 0) st4(rowp + M::feat(p), x0, x1, x2, x3);
  }
}

// rows of one head's matrix -> LDS tile [nrows][LDH]; rows >= N read as zero (token contractions
// run over the padded tile)
// (HDR: the real head dimension; below the tile's C::HDD the positions follow PadMap)
template <typename T, typename C, bool ROPE, int HDR = C::HDD>
VITPE_DEV void stage_rows(const AttnArgs& a, const T* src, int rstride, const float* cosb, const float* sinb, float sc,
                          T* tile, int nrows, int tid, int nthreads) {
  constexpr int CHN = CH<T>::n, HD = C::HDD, CPR = HD / CHN;
  const int N = a.N;
  for (int q = tid; q < nrows * CPR; q += nthreads) {
    const int row = q / CPR, cc = q % CPR;
    Chunk16 v = {0u, 0u, 0u, 0u};
    if (row < N) {
      const int tok = max(row, 1);  // class token (row 0) is never rotated
      if constexpr (HDR == HD)
        v = ld_rot_chunk<T, HD, ROPE>(src + (size_t)row * rstride, cc * CHN, cosb + (size_t)(tok - 1) * (HD / 2),
                                      sinb + (size_t)(tok - 1) * (HD / 2), row >= 1, sc);
      else
        v = ld_rot_chunk_pad<T, HDR, ROPE>(src + (size_t)row * rstride, cc * CHN, cosb + (size_t)(tok - 1) * (HDR / 2),
                                           sinb + (size_t)(tok - 1) * (HDR / 2), row >= 1, sc);
    }
    *reinterpret_cast<Chunk16*>(tile + row * C::LDH + cc * CHN) = v;
  }
}

// bias table / coefficients of head hg, multiplied by log2 e (exp2-domain softmax)
template <typename C, int KM>
VITPE_DEV void stage_pe(const AttnArgs& a, int hg, float* s_tab, float* s_coef, int tid, int nthreads) {
  const int N = a.N;
  if (KM == KM_RELATIVE)
    for (int i = tid; i < C::TABLD; i += nthreads)
      s_tab[i] = (i < 2 * N - 1) ? a.table[(size_t)hg * (2 * N - 1) + i] * LOG2E : 0.f;
  if (KM == KM_POLY) stage_poly<C>(a, hg, s_coef, N, tid, nthreads);
}

// ---- attention-probability dropout (reference vit.py:84-88: softmax -> attn_drop -> @ v) -----------------------------------
// Site element of (image b, head h, query i, key j): e = ((b H + h) N + i) NP4 + j, NP4 = N rounded up to a multiple of 4
// ("Dropout streams"): the four keys 4 jq .. 4 jq + 3 of one query row are the four words of ONE Philox call,
// counter row_q + jq with row_q = ((b H + h) N + i) (NP4 / 4).
struct DropCtx {
  DropKey key;
  uint64_t bh_rows;   // (b H + h) N
  uint32_t nq, thr;
  float rs;
};
VITPE_DEV DropCtx drop_ctx(const AttnArgs& a, int b, int hg) {
  DropCtx d;
  d.key = drop_key(a.rng);
  d.bh_rows = (uint64_t)(b * a.H + hg) * (uint64_t)a.N;
  d.nq = (uint32_t)(a.N + 3) >> 2;
  d.thr = a.drop_thr;
  d.rs = a.drop_rs;
  return d;
}
// swapped S^T tile (lane: query i, keys 16 jt + 4 g + r): the lane's accumulator quad is one Philox call
VITPE_DEV Philox4 drop_quad(const DropCtx& d, int i, int jq) { return drop_words(d.key, (d.bh_rows + (uint64_t)i) * d.nq + (uint64_t)jq); }
// plain S tile (lane: key j = 16 jt + c, queries i0 + r, i0 = 16 it + 4 g): the four lanes of a DPP quad hold the keys
// 4 jq .. 4 jq + 3; lane t of the quad draws query i0 + t's call and packs its four keep bits, a quad broadcast hands every
// lane the nibble of each query, of which it reads its own key's bit.  -> keep bits of (i0 + r, j) in bit r.  Uniform
// control flow required (cross-lane reads).
VITPE_DEV uint32_t drop_keep_T(const DropCtx& d, int i0, int j, int lane) {
  const int t = lane & 3;
  const Philox4 w = drop_quad(d, i0 + t, j >> 2);
  const int nib = (w.w[0] >= d.thr ? 1 : 0) | (w.w[1] >= d.thr ? 2 : 0) | (w.w[2] >= d.thr ? 4 : 0) | (w.w[3] >= d.thr ? 8 : 0);
  const int n0 = __builtin_amdgcn_update_dpp(0, nib, 0x00, 0xF, 0xF, true);   // quad_perm:[0,0,0,0]
  const int n1 = __builtin_amdgcn_update_dpp(0, nib, 0x55, 0xF, 0xF, true);   // quad_perm:[1,1,1,1]
  const int n2 = __builtin_amdgcn_update_dpp(0, nib, 0xAA, 0xF, 0xF, true);   // quad_perm:[2,2,2,2]
  const int n3 = __builtin_amdgcn_update_dpp(0, nib, 0xFF, 0xF, 0xF, true);   // quad_perm:[3,3,3,3]
  return (uint32_t)(((n0 >> t) & 1) | (((n1 >> t) & 1) << 1) | (((n2 >> t) & 1) << 2) | (((n3 >> t) & 1) << 3));
}

// =========================================================================================
// Forward: NW = MT waves, one query tile each
// =========================================================================================
// DROP: attention-probability dropout on P in registers, between the softmax and the accumulator-as-operand P.V -- a
// compile-time variant: the DROP = false instantiations are the kernels without it
template <typename T, int HD, int MT, int KM, int NW, bool DROP = false>
__global__ __launch_bounds__(64 * NW) void attn_core_fwd_kernel(AttnArgs a) {
  using C = AttnCfg<T, (HD + 31) / 32 * 32, (HD + 31) / 32 * 32, MT, 1, 0>;   // (HD = 24 / 48: padded tiles, PadMap)
  constexpr bool ROPE = (KM == KM_ROPE);
  __shared__ __attribute__((aligned(16))) T kt[C::QSZ];  // K~ (row reads only)
  __shared__ __attribute__((aligned(16))) T vt[C::HSZ];  // V (column reads run into the zero tail)
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

  DropCtx dc{};   // (the site's pair and row base: read once per workgroup, wave-uniform)
  if constexpr (DROP) dc = drop_ctx(a, b, hg);

  stage_rows<T, C, ROPE, HD>(a, qg + Dr, 3 * Dr, cosb, sinb, 1.0f, kt, C::NP, threadIdx.x, 64 * NW);
  stage_rows<T, C, false, HD>(a, qg + 2 * Dr, 3 * Dr, nullptr, nullptr, 1.0f, vt, C::VR, threadIdx.x, 64 * NW);
  stage_pe<C, KM>(a, hg, s_tab, s_coef, threadIdx.x, 64 * NW);
  __syncthreads();

  T* outp = reinterpret_cast<T*>(a.out) + (size_t)b * N * Dr + hg * HD;
  for (int it = wave; it < MT; it += NW) {
    const int i = 16 * it + c, il = min(i, N - 1), tok = max(il, 1);
    Frag<T> bq[C::HC];
#pragma unroll
    for (int cs = 0; cs < C::HC; ++cs)
      bq[cs] = ld_head_frag<T, HD, ROPE>(qg + (size_t)il * 3 * Dr, 32 * cs + 8 * g, cosb + (size_t)(tok - 1) * (HD / 2),
                                         sinb + (size_t)(tok - 1) * (HD / 2), il >= 1, a.scale * LOG2E);
    // the rotated query fragments are FINISHED here (pinned), and the K fragment reads below stay below: unpinned, the
    // compiler hoists all 26 LDS reads above the query's global loads, carries the rotation's fp32 temporaries and spills 25
    // registers at the 128-VGPR cap of a 13-wave workgroup -- 60 MB of scratch writes per launch at the ViT-B/16 geometry
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
    if constexpr (DROP) {   // the row sum above is the softmax's (all keys); dropped entries leave P.V, 1/(1-p) rides on 1/l
#pragma unroll
      for (int jt = 0; jt < MT; ++jt) {
        const Philox4 w = drop_quad(dc, il, 4 * jt + g);
#pragma unroll
        for (int r = 0; r < 4; ++r) s[jt][r] = w.w[r] >= dc.thr ? s[jt][r] : 0.f;
      }
    }
    f32x4 o[C::NT];
#pragma unroll
    for (int dt = 0; dt < C::NT; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int sc = 0; sc < C::SC; ++sc) {
      const Frag<T> bp = acc_to_frag<T>(s[2 * sc], (2 * sc + 1 < MT) ? s[(2 * sc + 1 < MT) ? 2 * sc + 1 : 0] : z4);
#pragma unroll
      for (int dt = 0; dt < C::NT; ++dt)
        if (tile_live<HD, false>(dt)) mma(ld_frag_tr(vt, C::LDH, 32 * sc + 4 * g, 32 * sc + 16 + 4 * g, 16 * dt), bp, o[dt]);
    }
    const float inv = DROP ? __builtin_amdgcn_rcpf(l) * a.drop_rs : __builtin_amdgcn_rcpf(l);
    if (i < N) {
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int dt = 0; dt < C::NT; dt += 2) {
          f32x4 p0 = o[dt], p1 = o[dt + 1];
#pragma unroll
          for (int r = 0; r < 4; ++r) { p0[r] *= inv; p1[r] *= inv; }
          head_store_pair<HD, false>(reinterpret_cast<bf16*>(outp) + (size_t)i * Dr, dt, g, p0, p1);
        }
      } else {
#pragma unroll
        for (int dt = 0; dt < C::NT; ++dt)
          head_st4<HD, false>(outp + (size_t)i * Dr, 16 * dt + 4 * g, o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv,
                              o[dt][3] * inv);
      }
    }
  }
}

// =========================================================================================
// Backward
// =========================================================================================
constexpr int CORE_HMAX = 16;  // heads, for the RoPE-mixed frequency-gradient scratch

// Gradient w.r.t. the caller's rotary tables of one 16-token tile (KM_ROPE_TABLES; reference rope_utils.py:18-37 under
// autograd, cos and sin independent inputs).  acc: the [feature][token] accumulators of dq~ (or dk~) BEFORE the rotation
// back, in the rotary layout (rotate-half partners NT/2 tiles apart, PadMap); gs turns them into the gradient w.r.t. the
// rotated features, g = gs * acc.  For the pair (x1, x2) = (x[f], x[f + HD/2]) of the raw projection row xrow:
//   dcos[p][f] = g1 x1 + g2 x2 ,  dsin[p][f] = g2 x1 - g1 x2 ,  p = tok - 1
// written with plain vector stores into this (q/k, image[, head])'s partial slab -- every (p, f) of the slab exactly once
// per workgroup -- and summed in a fixed order afterwards (vitpe_attention_core_bwd_tables).  Slab layout: part
// [2 (q/k)][B] x [cos | sin] x [H][P][HD/2] for 3-D tables (rope-mixed), part [2][B][H] x [cos | sin] x [P][HD/2] for 2-D.
template <typename T, int HD, int NT>
VITPE_DEV void table_grad_tile(const AttnArgs& a, const f32x4* acc, const T* xrow, int tok, int qk, int b, int hg, int g,
                               float gs) {
  const int N = a.N, P = N - 1;
  if (tok < 1 || tok >= N) return;   // (class token: not rotated; padding tokens)
  const bool mixed = a.mode == PE_ROPE_MIXED;
  const size_t L = (size_t)(mixed ? a.H : 1) * P * (HD / 2);
  const size_t part = mixed ? (size_t)qk * a.B + b : ((size_t)qk * a.B + b) * a.H + hg;
  float* dc = a.tab_slab + part * 2 * L + (mixed ? (size_t)hg * P * (HD / 2) : 0) + (size_t)(tok - 1) * (HD / 2);
  float* ds = dc + L;
#pragma unroll
  for (int nt = 0; nt < NT / 2; ++nt) {
    const int f0 = 16 * nt + 4 * g;
    if (HD % 32 != 0 && f0 >= HD / 2) continue;   // padded head: positions past HD/2 hold no feature
    const f32x4 x1 = ld4(xrow + f0), x2 = ld4(xrow + f0 + HD / 2);
    f32x4 c, s;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float g1 = acc[nt][r] * gs, g2 = acc[nt + NT / 2][r] * gs;
      c[r] = g1 * x1[r] + g2 * x2[r];
      s[r] = g2 * x1[r] - g1 * x2[r];
    }
    *reinterpret_cast<f32x4*>(dc + f0) = c;
    *reinterpret_cast<f32x4*>(ds + f0) = s;
  }
}

// DROP: both recomputations of P regenerate the forward's keep mask m (drop_quad / drop_keep_T): dP = (dO V^T) . m / (1-p)
// in the query-tile jobs, dV from P . m / (1-p) and the same dP in the key-tile jobs; sum_j P_ij dP_ij is still dO_i . O_i
template <typename T, int HD, int MT, int KM, int NW, bool DROP = false>
__global__ __launch_bounds__(64 * NW) void attn_core_bwd_kernel(AttnArgs a) {
  using C = AttnCfg<T, (HD + 31) / 32 * 32, (HD + 31) / 32 * 32, MT, 1, 0>;   // (HD = 24 / 48: padded tiles, PadMap)
  // KM_ROPE_TABLES: RoPE with the caller's tables, whose gradients go to a.tab_slab (table_grad_tile) instead of the
  // RoPE-mixed frequency fold (s_dfreq)
  constexpr bool TABG = (KM == KM_ROPE_TABLES);
  constexpr bool ROPE = (KM == KM_ROPE) || TABG;
  // padded head: q~ / k~ / dQ / dK in the rotary layout under RoPE (partners NT/2 tiles apart), cos / sin rows HD/2 wide --
  // the lower-half positions past HD/2 read the row's last four entries (clamped) and produce nothing that is stored
  constexpr bool PAD = HD % 32 != 0;
  constexpr int NTH = 64 * NW;
  __shared__ __attribute__((aligned(16))) T t0[C::HSZ];  // step 1: K~ ; step 2: q~
  __shared__ __attribute__((aligned(16))) T t1[C::HSZ];  // step 1: V  ; step 2: dO
  __shared__ __attribute__((aligned(16))) float s_tab[KM == KM_RELATIVE ? C::TABLD : 4];
  __shared__ __attribute__((aligned(16))) float s_coef[KM == KM_POLY ? C::PESZ : 4];
  __shared__ __attribute__((aligned(16))) float s_stat[2 * C::NP];  // [lse2 | delta][token]
  __shared__ float s_dtab[KM == KM_RELATIVE ? C::TABLD : 4];
  __shared__ float s_dcoef[C::MAXDEG + 1];
  __shared__ float s_dfreq[KM == KM_ROPE ? 2 * CORE_HMAX * (HD / 2) : 4];

  const int N = a.N, H = a.H, Dr = H * HD, P = N - 1;
  const int b = blockIdx.x / H, hg = blockIdx.x % H;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const T* qg = reinterpret_cast<const T*>(a.qkv) + (size_t)b * N * 3 * Dr + hg * HD;
  const T* dog = reinterpret_cast<const T*>(a.dout) + (size_t)b * N * Dr + hg * HD;
  T* dq = reinterpret_cast<T*>(a.out) + (size_t)b * N * 3 * Dr + hg * HD;
  const bool mixed = KM == KM_ROPE && a.mode == PE_ROPE_MIXED;   // (the frequency fold)
  const size_t hoff = (ROPE && a.mode == PE_ROPE_MIXED) ? (size_t)hg * P * (HD / 2) : 0;
  const float* cosb = ROPE ? a.cos + hoff : nullptr;
  const float* sinb = ROPE ? a.sin + hoff : nullptr;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  const float qsc = a.scale * LOG2E;

  DropCtx dc{};   // (the site's pair and row base: read once per workgroup, wave-uniform)
  if constexpr (DROP) dc = drop_ctx(a, b, hg);

  stage_rows<T, C, ROPE, HD>(a, qg + Dr, 3 * Dr, cosb, sinb, 1.0f, t0, C::VR, threadIdx.x, NTH);
  stage_rows<T, C, false, HD>(a, qg + 2 * Dr, 3 * Dr, nullptr, nullptr, 1.0f, t1, C::NP, threadIdx.x, NTH);
  stage_pe<C, KM>(a, hg, s_tab, s_coef, threadIdx.x, NTH);
  if (KM == KM_RELATIVE)
    for (int q = threadIdx.x; q < C::TABLD; q += NTH) s_dtab[q] = 0.f;
  for (int q = threadIdx.x; q <= C::MAXDEG; q += NTH) s_dcoef[q] = 0.f;
  if (KM == KM_ROPE)
    for (int q = threadIdx.x; q < 2 * CORE_HMAX * (HD / 2); q += NTH) s_dfreq[q] = 0.f;
  __syncthreads();

  // ---- step 1: query-tile jobs on the swapped tiles: stats, dS^T, dQ -----------------------
  for (int it = wave; it < MT; it += NW) {
    const T* kh = t0;
    const T* vh = t1;
    const int i = 16 * it + c, il = min(i, N - 1), tok = max(il, 1);
    const float* csr = cosb + (size_t)(tok - 1) * (HD / 2);
    const float* snr = sinb + (size_t)(tok - 1) * (HD / 2);
    Frag<T> bq[C::HC], bdo[C::HC];
#pragma unroll
    for (int cs = 0; cs < C::HC; ++cs) {
      bq[cs] = ld_head_frag<T, HD, ROPE>(qg + (size_t)il * 3 * Dr, 32 * cs + 8 * g, csr, snr, il >= 1, qsc);
      bdo[cs] = ld_head_frag<T, HD, false>(dog + (size_t)il * Dr, 32 * cs + 8 * g, nullptr, nullptr, false, 1.0f);
    }
    f32x4 s[MT], dp[MT];
    const float m = logits_T<T, C, KM>(a, kh, bq, s_tab, s_coef, 0, it, lane, s);
    if (MT > 8) __builtin_amdgcn_sched_barrier(0);
    const T* vrow = vh + c * C::LDH + 8 * g;
#pragma unroll
    for (int jt = 0; jt < MT; ++jt) {
      dp[jt] = z4;
#pragma unroll
      for (int cs = 0; cs < C::HC; ++cs) mma(ld_frag(vrow + 16 * jt * C::LDH + 32 * cs), bdo[cs], dp[jt]);
      if (MT > 8 && (jt & 1)) __builtin_amdgcn_sched_barrier(0);  // bound the load hoisting (register pressure)
    }
    if constexpr (DROP) {
#pragma unroll
      for (int jt = 0; jt < MT; ++jt) {
        const Philox4 w = drop_quad(dc, il, 4 * jt + g);
#pragma unroll
        for (int r = 0; r < 4; ++r) dp[jt][r] = w.w[r] >= dc.thr ? dp[jt][r] * dc.rs : 0.f;
      }
    }
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
    float dl = 0.f;
#pragma unroll
    for (int jt = 0; jt < MT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[jt][r] *= inv;
        dl += s[jt][r] * dp[jt][r];
      }
    dl = xg_sum(dl);
    if (g == 0) {
      s_stat[0 * C::NP + i] = m + __builtin_amdgcn_logf(l);  // v_log_f32 = log2
      s_stat[1 * C::NP + i] = dl;
    }
    float cacc[C::MAXDEG + 1];
#pragma unroll
    for (int k = 0; k <= C::MAXDEG; ++k) cacc[k] = 0.f;
    const bool qvalid = i < N;
#pragma unroll
    for (int jt = 0; jt < MT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * jt + 4 * g + r;
        const bool valid = qvalid && ((jt < MT - 1) || (j < N));
        const float ds = valid ? s[jt][r] * (dp[jt][r] - dl) : 0.f;
        dp[jt][r] = ds;
        if (KM == KM_POLY) {
          if (valid && i >= 1 && j >= 1) {
            const float x = (float)pe_l1<C>(s_coef, i, j);
            float pw = 1.f;
#pragma unroll
            for (int k = 0; k <= C::MAXDEG; ++k) {
              if (k <= a.degree) cacc[k] += ds * pw;
              pw *= x;
            }
          }
        }
      }
    if (KM == KM_RELATIVE) {   // diagonals of every 16x16 tile reduced in registers, then conflict-free LDS atomics
#pragma unroll
      for (int jt = 0; jt < MT; ++jt) {
        float d0, d1;
        tile_diag_sums(dp[jt], lane, d0, d1);
        const int idx0 = 16 * (it - jt) + c + N - 1;
        if (g == 0) {
          if (idx0 >= 0 && idx0 <= 2 * N - 2) atomicAdd(&s_dtab[idx0], d0);
          if (c >= 1 && idx0 - 16 >= 0 && idx0 - 16 <= 2 * N - 2) atomicAdd(&s_dtab[idx0 - 16], d1);
        }
      }
    }
    if (KM == KM_POLY) {
#pragma unroll
      for (int k = 0; k <= C::MAXDEG; ++k) {
        if (k <= a.degree) {  // wave-uniform
          const float t = wave_sum(cacc[k]);
          if (lane == 0) atomicAdd(&s_dcoef[k], t);
        }
      }
    }
    // dQrot^T[d][i] / scale = sum_j K~^T[d][j] dS^T[j][i]
    f32x4 dqa[C::NT];
#pragma unroll
    for (int dt = 0; dt < C::NT; ++dt) dqa[dt] = z4;
#pragma unroll
    for (int sc = 0; sc < C::SC; ++sc) {
      const Frag<T> bs = acc_to_frag<T>(dp[2 * sc], (2 * sc + 1 < MT) ? dp[(2 * sc + 1 < MT) ? 2 * sc + 1 : 0] : z4);
#pragma unroll
      for (int dt = 0; dt < C::NT; ++dt)
        if (tile_live<HD, ROPE>(dt)) mma(ld_frag_tr(kh, C::LDH, 32 * sc + 4 * g, 32 * sc + 16 + 4 * g, 16 * dt), bs, dqa[dt]);
      if (MT > 8) __builtin_amdgcn_sched_barrier(0);
    }
    if (mixed) {   // uniform branch: row reductions inside (mixed_freq_grad_tile, attn_common.h)
      // dL/dphase = (dq~2 q~1 - dq~1 q~2), q~ = scale*log2e*rot(q) (see attn.hip): ln2 undoes the log2e
      const bool tok_ok = i >= 1 && i < N;
#pragma unroll
      for (int nt = 0; nt < C::NT / 2; ++nt) {
        const int gg = PAD ? min(g, (HD / 2 - 4 - 16 * nt) / 4) : g;
        const f32x4 cs = *reinterpret_cast<const f32x4*>(csr + 16 * nt + 4 * gg);
        const f32x4 sn = *reinterpret_cast<const f32x4*>(snr + 16 * nt + 4 * gg);
        const f32x4 x1 = ld4(qg + (size_t)il * 3 * Dr + 16 * nt + 4 * gg);
        const f32x4 x2 = ld4(qg + (size_t)il * 3 * Dr + (PAD ? 16 * nt + 4 * gg + HD / 2 : 16 * (nt + C::NT / 2) + 4 * g));
        f32x4 dph;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float q1 = (x1[r] * cs[r] - x2[r] * sn[r]) * qsc, q2 = (x1[r] * sn[r] + x2[r] * cs[r]) * qsc;
          dph[r] = dqa[nt + C::NT / 2][r] * q1 - dqa[nt][r] * q2;
        }
        mixed_freq_grad_tile<PAD>(s_dfreq, dph, i, tok_ok, 16 * it, hg, H, P, a.grid, HD / 2, 16 * nt + 4 * g, LN2, lane);
      }
    }
    // dL/d rot(q) = scale * dq~ (q~ = scale*log2e*rot(q), dqa carries 1/log2e: the scale the dQ store applies)
    if (TABG) table_grad_tile<T, HD, C::NT>(a, dqa, qg + (size_t)il * 3 * Dr, i, 0, b, hg, g, a.scale);
    if (ROPE && i >= 1 && i < N) {
#pragma unroll
      for (int nt = 0; nt < C::NT / 2; ++nt) {
        const int gg = PAD ? min(g, (HD / 2 - 4 - 16 * nt) / 4) : g;
        const f32x4 cs = *reinterpret_cast<const f32x4*>(csr + 16 * nt + 4 * gg);
        const f32x4 sn = *reinterpret_cast<const f32x4*>(snr + 16 * nt + 4 * gg);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float d1 = dqa[nt][r], d2 = dqa[nt + C::NT / 2][r];
          dqa[nt][r] = d1 * cs[r] + d2 * sn[r];
          dqa[nt + C::NT / 2][r] = -d1 * sn[r] + d2 * cs[r];
        }
      }
    }
    if (i < N) {
      if constexpr (sizeof(T) == 2) {   // 16-B pieces (lanes of one token pair up: both sides of a swap pass the guard together)
#pragma unroll
        for (int dt = 0; dt < C::NT; dt += 2) {
          f32x4 p0 = dqa[dt], p1 = dqa[dt + 1];
#pragma unroll
          for (int r = 0; r < 4; ++r) { p0[r] *= a.scale; p1[r] *= a.scale; }
          head_store_pair<HD, ROPE>(reinterpret_cast<bf16*>(dq) + (size_t)i * 3 * Dr, dt, g, p0, p1);
        }
      } else {
#pragma unroll
        for (int dt = 0; dt < C::NT; ++dt)
          head_st4<HD, ROPE>(dq + (size_t)i * 3 * Dr, 16 * dt + 4 * g, dqa[dt][0] * a.scale, dqa[dt][1] * a.scale,
                             dqa[dt][2] * a.scale, dqa[dt][3] * a.scale);
      }
    }
  }
  __syncthreads();
  // refill: q~ and dO with zero tails (token contractions of step 2)
  stage_rows<T, C, ROPE, HD>(a, qg, 3 * Dr, cosb, sinb, qsc, t0, C::VR, threadIdx.x, NTH);
  stage_rows<T, C, false, HD>(a, dog, Dr, nullptr, nullptr, 1.0f, t1, C::VR, threadIdx.x, NTH);
  __syncthreads();

  // ---- step 2: key-tile jobs on the plain tiles: dV, dK -------------------------------------
  for (int jt = wave; jt < MT; jt += NW) {
    const T* qh = t0;
    const T* doh = t1;
    const int j = 16 * jt + c, jl = min(j, N - 1), tok = max(jl, 1);
    const float* csr = cosb + (size_t)(tok - 1) * (HD / 2);
    const float* snr = sinb + (size_t)(tok - 1) * (HD / 2);
    Frag<T> bk[C::HC], bv[C::HC];
#pragma unroll
    for (int cs = 0; cs < C::HC; ++cs) {
      bk[cs] = ld_head_frag<T, HD, ROPE>(qg + Dr + (size_t)jl * 3 * Dr, 32 * cs + 8 * g, csr, snr, jl >= 1, 1.0f);
      bv[cs] = ld_head_frag<T, HD, false>(qg + 2 * Dr + (size_t)jl * 3 * Dr, 32 * cs + 8 * g, nullptr, nullptr, false, 1.0f);
    }
    const bool kvalid = j < N;
    const T* qrow = qh + c * C::LDH + 8 * g;
    const T* dorow = doh + c * C::LDH + 8 * g;
    f32x4 dva[C::NT], dka[C::NT];
#pragma unroll
    for (int dt = 0; dt < C::NT; ++dt) { dva[dt] = z4; dka[dt] = z4; }
    // the row statistics are known here, so the query tiles stream through in pairs (one K32 chunk
    // of the token contraction): only two P / dS tiles are live at a time
#pragma unroll
    for (int sc = 0; sc < C::SC; ++sc) {
      f32x4 p[2], ds[2];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int it = 2 * sc + hf;
        p[hf] = z4;
        ds[hf] = z4;
        if (it < MT) {
#pragma unroll
          for (int cs = 0; cs < C::HC; ++cs) {
            mma(ld_frag(qrow + 16 * it * C::LDH + 32 * cs), bk[cs], p[hf]);
            mma(ld_frag(dorow + 16 * it * C::LDH + 32 * cs), bv[cs], ds[hf]);
          }
          const f32x4 lse = *reinterpret_cast<const f32x4*>(&s_stat[0 * C::NP + 16 * it + 4 * g]);
          const f32x4 dl = *reinterpret_cast<const f32x4*>(&s_stat[1 * C::NP + 16 * it + 4 * g]);
          uint32_t keep = 0xFu;
          if constexpr (DROP) keep = drop_keep_T(dc, 16 * it + 4 * g, j, lane);   // (rows / keys >= N: masked below)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = 16 * it + 4 * g + r;
            float sv = p[hf][r];
            if (KM == KM_RELATIVE || KM == KM_POLY) sv += pe_bias2<C, KM>(a, s_tab, s_coef, 0, i, j, N);
            const bool valid = kvalid && ((it < MT - 1) || (i < N));
            const float pv = valid ? __builtin_amdgcn_exp2f(sv - lse[r]) : 0.f;
            if constexpr (DROP) {
              const bool kp = (keep >> r) & 1u;
              p[hf][r] = kp ? pv * a.drop_rs : 0.f;
              ds[hf][r] = pv * ((kp ? ds[hf][r] * a.drop_rs : 0.f) - dl[r]);
            } else {
              p[hf][r] = pv;
              ds[hf][r] = pv * (ds[hf][r] - dl[r]);
            }
          }
        }
      }
      const Frag<T> bp = acc_to_frag<T>(p[0], p[1]);
      const Frag<T> bs = acc_to_frag<T>(ds[0], ds[1]);
#pragma unroll
      for (int dt = 0; dt < C::NT; ++dt) {
        if (tile_live<HD, false>(dt)) mma(ld_frag_tr(doh, C::LDH, 32 * sc + 4 * g, 32 * sc + 16 + 4 * g, 16 * dt), bp, dva[dt]);
        if (tile_live<HD, ROPE>(dt)) mma(ld_frag_tr(qh, C::LDH, 32 * sc + 4 * g, 32 * sc + 16 + 4 * g, 16 * dt), bs, dka[dt]);
      }
      if (MT > 8) __builtin_amdgcn_sched_barrier(0);
    }
    // dK_rot = dS^T q~ / log2e  (q~ carries the folded scale and log2e)
#pragma unroll
    for (int dt = 0; dt < C::NT; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) dka[dt][r] *= LN2;
    if (mixed) {
      const bool tok_ok = j >= 1 && j < N;
#pragma unroll
      for (int nt = 0; nt < C::NT / 2; ++nt) {
        const int gg = PAD ? min(g, (HD / 2 - 4 - 16 * nt) / 4) : g;
        const f32x4 cs = *reinterpret_cast<const f32x4*>(csr + 16 * nt + 4 * gg);
        const f32x4 sn = *reinterpret_cast<const f32x4*>(snr + 16 * nt + 4 * gg);
        const f32x4 x1 = ld4(qg + Dr + (size_t)jl * 3 * Dr + 16 * nt + 4 * gg);
        const f32x4 x2 = ld4(qg + Dr + (size_t)jl * 3 * Dr + (PAD ? 16 * nt + 4 * gg + HD / 2 : 16 * (nt + C::NT / 2) + 4 * g));
        f32x4 dph;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float k1 = x1[r] * cs[r] - x2[r] * sn[r], k2 = x1[r] * sn[r] + x2[r] * cs[r];
          dph[r] = dka[nt + C::NT / 2][r] * k1 - dka[nt][r] * k2;
        }
        mixed_freq_grad_tile<PAD>(s_dfreq, dph, j, tok_ok, 16 * jt, hg, H, P, a.grid, HD / 2, 16 * nt + 4 * g, 1.0f, lane);
      }
    }
    if (TABG) table_grad_tile<T, HD, C::NT>(a, dka, qg + Dr + (size_t)jl * 3 * Dr, j, 1, b, hg, g, 1.0f);   // (LN2 applied)
    if (ROPE && j >= 1 && j < N) {
#pragma unroll
      for (int nt = 0; nt < C::NT / 2; ++nt) {
        const int gg = PAD ? min(g, (HD / 2 - 4 - 16 * nt) / 4) : g;
        const f32x4 cs = *reinterpret_cast<const f32x4*>(csr + 16 * nt + 4 * gg);
        const f32x4 sn = *reinterpret_cast<const f32x4*>(snr + 16 * nt + 4 * gg);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float d1 = dka[nt][r], d2 = dka[nt + C::NT / 2][r];
          dka[nt][r] = d1 * cs[r] + d2 * sn[r];
          dka[nt + C::NT / 2][r] = -d1 * sn[r] + d2 * cs[r];
        }
      }
    }
    if (j < N) {
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int dt = 0; dt < C::NT; dt += 2) {
          head_store_pair<HD, ROPE>(reinterpret_cast<bf16*>(dq) + Dr + (size_t)j * 3 * Dr, dt, g, dka[dt], dka[dt + 1]);
          head_store_pair<HD, false>(reinterpret_cast<bf16*>(dq) + 2 * Dr + (size_t)j * 3 * Dr, dt, g, dva[dt], dva[dt + 1]);
        }
      } else {
#pragma unroll
        for (int dt = 0; dt < C::NT; ++dt) {
          head_st4<HD, ROPE>(dq + Dr + (size_t)j * 3 * Dr, 16 * dt + 4 * g, dka[dt][0], dka[dt][1], dka[dt][2], dka[dt][3]);
          head_st4<HD, false>(dq + 2 * Dr + (size_t)j * 3 * Dr, 16 * dt + 4 * g, dva[dt][0], dva[dt][1], dva[dt][2],
                              dva[dt][3]);
        }
      }
    }
  }
  __syncthreads();

  // ---- flush this (image, head)'s positional-parameter gradients ----------------------------
  if (KM == KM_RELATIVE) {
    for (int q = threadIdx.x; q < 2 * N - 1; q += NTH) atomicAdd(a.dtable + (size_t)hg * (2 * N - 1) + q, s_dtab[q]);
  } else if (KM == KM_POLY) {
    for (int k = threadIdx.x; k <= a.degree; k += NTH)
      atomicAdd(a.dcoeff + (a.coeff_per_head ? hg * (a.degree + 1) : 0) + k, s_dcoef[k]);
  } else if (mixed) {
    for (int q = threadIdx.x; q < 2 * H * (HD / 2); q += NTH)
      if (s_dfreq[q] != 0.f) atomicAdd(a.dfreqs + q, s_dfreq[q]);
  }
}

template <typename T, int HD, int MT, bool DROP>
static int launch_core_v(bool bwd, const AttnArgs& a, hipStream_t s) {
  // forward: one wave per query tile (two rounds above 13 tiles); backward: half as many waves (two rounds) so that
  // the p/dS accumulators of a key-tile job (2*MT f32x4) stay in registers
  // Head dimensions beyond 32 / 64 at 17 tiles: six waves (three rounds, 256 registers a lane) -- at nine waves (168
  // registers) they spilled 14-112 VGPRs (tools/regs.sh attn_core_hd.hip)
  // The dropout variants at 17 tiles run on six waves at every head dimension: at nine they spilled 10-230 VGPRs
  constexpr bool SIX = (DROP || (HD != 32 && HD != 64)) && MT > 13;
  constexpr int NWF = SIX ? 6 : (MT > 13) ? (MT + 1) / 2 : MT, NWB = SIX ? 6 : (MT > 8) ? (MT + 1) / 2 : MT;
  const dim3 grid((unsigned)(a.B * a.H));
#define VITPE_CORE_LAUNCH(KM)                                                                                      \
  do {                                                                                                               \
    if (bwd) hipLaunchKernelGGL((attn_core_bwd_kernel<T, HD, MT, KM, NWB, DROP>), grid, dim3(64 * NWB), 0, s, a);    \
    else hipLaunchKernelGGL((attn_core_fwd_kernel<T, HD, MT, KM, NWF, DROP>), grid, dim3(64 * NWF), 0, s, a);        \
  } while (0)
  switch (a.mode) {
    case PE_RELATIVE: VITPE_CORE_LAUNCH(KM_RELATIVE); break;
    case PE_POLY: VITPE_CORE_LAUNCH(KM_POLY); break;
    case PE_ROPE_AXIAL:
    case PE_ROPE_MIXED:
      if constexpr (!DROP) {   // (table gradients together with dropout: not built, refused by the entry points)
        if (bwd && a.tab_slab) {
          hipLaunchKernelGGL((attn_core_bwd_kernel<T, HD, MT, KM_ROPE_TABLES, NWB>), grid, dim3(64 * NWB), 0, s, a);
          break;
        }
      }
      VITPE_CORE_LAUNCH(KM_ROPE);
      break;
    default: VITPE_CORE_LAUNCH(KM_PLAIN); break;
  }
#undef VITPE_CORE_LAUNCH
  VITPE_CHECK_LAUNCH();
}
// a.rng set: the dropout instantiations; otherwise exactly the kernels without it
template <typename T, int HD, int MT>
static int launch_core(bool bwd, const AttnArgs& a, hipStream_t s) {
  if (a.rng != nullptr) return a.tab_slab ? (int)hipErrorNotSupported : launch_core_v<T, HD, MT, true>(bwd, a, s);
  return launch_core_v<T, HD, MT, false>(bwd, a, s);
}

// Instantiated geometries: head dimension 32 / 64 and these token-tile counts MT = ceil(N / 16) -- the square grids the
// reference CLI can produce from its --img_size / --patch_size flags ((img/patch)^2 + 1 tokens): N = 17 (32/8),
// 50 (28/4, 224/32), 65 (32/4, 64/8: also the fused path), 145..160 (48/4), 197 (224/16: config 5), 257 (64/4, 32/2).
// Both LDS tiles of the backward must fit 160 KB: fp32 at hd = 64 stops at 13 tiles.
template <typename T, int HD, int MT>
constexpr bool core_fits() {
  using C = AttnCfg<T, (HD + 31) / 32 * 32, (HD + 31) / 32 * 32, MT, 1, 0>;
  return 2 * (size_t)C::HSZ * sizeof(T) + 6 * 1024 <= 160 * 1024 && MT <= 17;
}
#define VITPE_CORE_MTS(X, T, HD) X(T, HD, 2) X(T, HD, 4) X(T, HD, 5) X(T, HD, 10) X(T, HD, 13) X(T, HD, 17)

// THE list of head dimensions: X(HD, OWN_TU).  OWN_TU = 1: instantiated in attn_core_hd.hip, one translation unit per head
// dimension -- csrc/Makefile's CORE_HDS names exactly these, keep the two in step; 0: instantiated in attn_core.hip.
#define VITPE_CORE_HDS(X) X(64, 0) X(32, 0) X(24, 1) X(48, 1) X(96, 1) X(128, 1)

// what a launch of the core computes: dispatch_core's `op` (attn_core.hip)
enum { CORE_FWD = 0, CORE_BWD = 1, CORE_PROBS = 2 };

// CORE_PROBS: attn_core_probs_kernel, defined and instantiated in attn_core_probs.hip (every head dimension of
// VITPE_CORE_HDS x VITPE_CORE_MTS x {bf16, float}; csrc/Makefile's PROBS_HDS) -- everywhere else only this declaration
template <typename T, int HD, int MT>
__attribute__((visibility("hidden"))) int launch_core_probs(const AttnArgs& a, hipStream_t s);

// The statistics kernel (attn_core_stats.hip: attn_core_stats_kernel, every head dimension of VITPE_CORE_HDS x
// VITPE_CORE_MTS x {bf16, float}; csrc/Makefile's STATS_HDS): its arguments wrap AttnArgs, which stays as it is for every
// other kernel.  stats fp32 [B,H,4] (slots below = include/vitpe.h VITPE_STAT_*); weights fp32 [B,N] and colsum fp32 [B,H,N]
// both null or both set; unit: what one grid step of the distance is worth.
struct StatsArgs {
  AttnArgs a;
  float* stats;
  const float* weights;
  float* colsum;
  float unit;
};
enum { STAT_DISTANCE = 0, STAT_ENTROPY = 1, STAT_CLS_MASS = 2, STAT_CLS_ENTROPY = 3 };
template <typename T, int HD, int MT>
__attribute__((visibility("hidden"))) int launch_core_stats(const StatsArgs& sa, hipStream_t s);

// The relevance kernel (attn_core_relevance.hip: attn_core_relevance_kernel, the same instantiation list; csrc/Makefile's
// RELEVANCE_HDS): its arguments wrap AttnArgs likewise (a.qkv and a.dout set).  weights fp32 [B,N], colsum fp32 [B,H,N] =
// sum_i weights_i f(G_ij A_ij) with G = dO V^T; clamp: f = max(0, .), else the identity.  The kernel has its own LDS fit
// rule (it stages V beside K~): hipErrorNotSupported where it fails.
struct RelevanceArgs {
  AttnArgs a;
  const float* weights;
  float* colsum;
  int clamp;
};
template <typename T, int HD, int MT>
__attribute__((visibility("hidden"))) int launch_core_relevance(const RelevanceArgs& ra, hipStream_t s);

template <typename T, int HD>
__attribute__((visibility("hidden"))) int dispatch_core_t(int op, int MT, const AttnArgs& a, hipStream_t s) {
#define VITPE_CORE_CASE(T_, HD_, MT_)                                                                  \
  if (MT == MT_) {                                                                                     \
    if constexpr (core_fits<T_, HD_, MT_>())                                                           \
      return op == CORE_PROBS ? launch_core_probs<T_, HD_, MT_>(a, s) : launch_core<T_, HD_, MT_>(op == CORE_BWD, a, s); \
    else return (int)hipErrorNotSupported;                                                             \
  }
  VITPE_CORE_MTS(VITPE_CORE_CASE, T, HD)
#undef VITPE_CORE_CASE
  return (int)hipErrorNotSupported;
}

template <typename T, int HD>
__attribute__((visibility("hidden"))) bool core_supported_t(int MT) {
#define VITPE_CORE_CASE(T_, HD_, MT_) if (MT == MT_) return core_fits<T_, HD_, MT_>();
  VITPE_CORE_MTS(VITPE_CORE_CASE, T, HD)
#undef VITPE_CORE_CASE
  return false;
}

// VITPE_CORE_HD_TU (attn_core_hd.hip): the translation unit instantiates the OWN_TU head dimensions (all of them, or
// the one VITPE_CORE_HD names); everywhere else they are extern.
#ifdef VITPE_CORE_HD_TU
#define VITPE_CORE_HD_LINKAGE
#else
#define VITPE_CORE_HD_LINKAGE extern
#endif
#define VITPE_CORE_DECLARE_HD(HD)                                                                       \
  VITPE_CORE_HD_LINKAGE template int dispatch_core_t<bf16, HD>(int, int, const AttnArgs&, hipStream_t);   \
  VITPE_CORE_HD_LINKAGE template int dispatch_core_t<float, HD>(int, int, const AttnArgs&, hipStream_t);  \
  VITPE_CORE_HD_LINKAGE template bool core_supported_t<bf16, HD>(int);                                    \
  VITPE_CORE_HD_LINKAGE template bool core_supported_t<float, HD>(int);
#define VITPE_CORE_DECLARE_HD_0(HD)
#define VITPE_CORE_DECLARE_HD_1(HD) VITPE_CORE_DECLARE_HD(HD)
#define VITPE_CORE_DECLARE_X(HD, OWN_TU) VITPE_CORE_DECLARE_HD_##OWN_TU(HD)
#ifdef VITPE_CORE_HD
VITPE_CORE_DECLARE_HD(VITPE_CORE_HD)
#else
VITPE_CORE_HDS(VITPE_CORE_DECLARE_X)
#endif

}  // namespace vitpe
