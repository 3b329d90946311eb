// Fused attention-with-positional-encoding, forward and backward (the north-star kernels).
//
// Forward replaces, per layer, reference models/vit.py:47-88:
//   qkv Linear (no bias) -> head split -> RoPE rotate-half on patch tokens (rope_utils.py:18-37,
//   class token skipped, vit.py:56-68) -> QK^T * hd^-0.5 (vit.py:71,75) -> + relative / polynomial
//   bias (vit.py:78-81; positional_encoding.py:82-95 / 127-171 evaluated on the fly from the
//   [H,2N-1] table / the coefficients: the [H,N,N] bias is never materialised) -> softmax ->
//   @V -> merged-head [B,N,d].
// Backward is the hand-derived autograd of the same (the reference has no explicit backward):
//   recompute q,k,v and the probabilities, dV, dP, dS, dQ, dK, inverse rotation, and the
//   positional-parameter gradients (relative table scatter-add, polynomial coefficients,
//   RoPE-mixed frequencies through cos/sin and the reference's view-scramble).
//
// Forward mapping ("register-resident"): one workgroup per image, ONE WAVE PER HEAD.  The layer-normed token matrix
// x[N,d] is staged once into LDS (coalesced 16-B reads, LayerNorm applied on the way in); after that single barrier the
// waves never meet again.  A wave projects v, k and q of its head straight out of LDS x-fragments and packed weight
// fragments (one contiguous 1-KB read each) and keeps EVERYTHING else in registers:
//   * v is projected un-swapped (A = x rows, B = Wv rows): the accumulator tile pair (2sc, 2sc+1) of feature tile dt
//     IS the A-operand fragment of V^T for the P.V product (keys in the acc_to_frag order), no transpose, no LDS;
//   * k and q are projected swapped (A = W rows, B = x rows): accumulator tiles (nt = 0, 1) of token tile tt ARE the
//     K A-operand / Q B-operand fragments of S^T = K Q^T with the head dimension in the same permuted order on both
//     sides; RoPE rotates in registers first (the rotate-half partner j + hd/2 is the same lane and register of the
//     neighbouring accumulator tile);
//   * S^T = K Q^T puts one query column on each lane: softmax max / sum are in-lane reductions plus two v_permlane
//     swaps, the probabilities feed the P.V MFMA directly from registers.
// No wave ever waits for another after the staging barrier, so the waves of a SIMD drift apart and one's softmax VALU
// phase runs under another's projection MFMAs (the former per-pass workgroup barriers forced all waves through the
// same phase together).
// LDS per workgroup: x only (32 KB bf16) -> several workgroups per CU; the bank-conflicting q/k/v tiles are gone.
//
// Backward mapping: one workgroup (6 wavefronts) per image; heads are processed HPP at a time: three waves per head
// project q / k / v with MFMA, rotate in registers and park q,k,v in LDS; the core then runs one (head, 16-token
// tile) job per wave on the *swapped* product S^T = K Q^T (V is read column-wise with ds_read_b64_tr_b16).
//
// Instruction economy (the core is issue-bound, not MFMA-bound, at N=65): the PE mode and the
// token count are template parameters, the softmax runs in the exp2 domain (log2(e) is folded into
// the q scale and into the staged bias table / coefficients), keys are masked only in the last
// key tile, and every address is a compile-time offset from a per-lane base.
#include "attn_common.h"
#include <stdlib.h>
#include <type_traits>

namespace vitpe {

// ---- stage the image's tokens, PE tables (x log2 e); zero the tails ------------------------
template <typename T, typename C, int KM, int NTH = 384>
VITPE_DEV void stage_tokens(const AttnArgs& a, int b, T* xs, T* hbuf, int hbuf_elems, float* s_tab, float* s_coef,
                            int tid, int nthreads, bool stage_tables) {
  constexpr int CHN = CH<T>::n;
  constexpr int DCH = C::LDX / CHN;  // chunks per LDS row incl. pad
  constexpr int D = C::DD;
  const int N = C::ntok(a);
  const T* xg = reinterpret_cast<const T*>(a.xn) + (size_t)b * N * D;
  const Chunk16 zero = {0u, 0u, 0u, 0u};
  // all global loads of this thread first, then the LDS stores: one exposed latency, not one per chunk
  constexpr int TOTAL = C::NP * DCH;
  constexpr int ITERS = (TOTAL + NTH - 1) / NTH;
  Chunk16 v[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int q = tid + it * nthreads, row = q / DCH, cc = q % DCH;
    v[it] = zero;
    if (q < TOTAL && row < N && cc * CHN < D) v[it] = *reinterpret_cast<const Chunk16*>(xg + (size_t)row * D + cc * CHN);
  }
  if (a.ln_gamma != nullptr) {  // fused LayerNorm on the way in (uniform branch)
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int q = tid + it * nthreads, row = q / DCH, cc = q % DCH;
      if (q < TOTAL && row < N && cc * CHN < D) {
        const float mean = a.ln_mean[(size_t)b * N + row], rstd = a.ln_rstd[(size_t)b * N + row];
        float f[CHN];
        chunk_to_f32<T>(v[it], f);
#pragma unroll
        for (int h4 = 0; h4 < CHN / 4; ++h4) {
          const f32x4 gq = *reinterpret_cast<const f32x4*>(a.ln_gamma + cc * CHN + 4 * h4);
          const f32x4 bq = *reinterpret_cast<const f32x4*>(a.ln_beta + cc * CHN + 4 * h4);
#pragma unroll
          for (int t = 0; t < 4; ++t) f[4 * h4 + t] = (f[4 * h4 + t] - mean) * rstd * gq[t] + bq[t];
        }
        v[it] = f32_to_chunk<T>(f);
        if (a.xn_out != nullptr)
          __builtin_nontemporal_store(v[it], reinterpret_cast<Chunk16*>(reinterpret_cast<T*>(a.xn_out) + ((size_t)b * N + row) * D + cc * CHN));  // read again only in backward
      }
    }
  }
  // zero what must read as zero and is never written again (whole buffer when zero_all, else the caller's tails)
  for (int q = tid; q < hbuf_elems / CHN; q += nthreads) *reinterpret_cast<Chunk16*>(hbuf + q * CHN) = zero;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int q = tid + it * nthreads, row = q / DCH, cc = q % DCH;
    if (q < TOTAL) *reinterpret_cast<Chunk16*>(xs + row * C::LDX + cc * CHN) = v[it];
  }
  if (KM == KM_RELATIVE && stage_tables) {
    for (int q = tid; q < C::H * C::TABLD; q += nthreads) {
      const int h = q / C::TABLD, i = q % C::TABLD;
      s_tab[q] = (i < 2 * N - 1) ? a.table[h * (2 * N - 1) + i] * LOG2E : 0.f;
    }
  }
  if (KM == KM_POLY && stage_tables) stage_poly<C>(a, 0, s_coef, N, tid, nthreads);
}

// Forward-kernel staging: thread (row group tid / CPRW, chunk column tid % CPRW) walks down the rows with a FIXED chunk
// column, so the LayerNorm affine parameters of its column are loaded once (the generic version above re-derives the
// column per iteration: five unrolled iterations' gamma / beta loads in flight cost 80 registers).  The pad chunk of
// an LDS row is never read (fragment reads stop at column D - 1) and is left alone.
template <typename T, typename C, int KM, int NTH, bool LNF>
VITPE_DEV void stage_tokens_fwd(const AttnArgs& a, int b, T* xs, float* s_tab, float* s_coef, int tid, bool live,
                                bool stage_tables) {
  constexpr int CHN = CH<T>::n, D = C::DD;
  constexpr int CPRW = D / CHN;                 // 16-B chunks per token row
  static_assert(NTH % CPRW == 0 && C::NP % (NTH / CPRW) == 0, "thread grid must tile the token matrix");
  constexpr int RPP = NTH / CPRW, ITERS = C::NP / RPP;
  const int N = C::ntok(a);
  const int cc = tid % CPRW, r0 = tid / CPRW;
  const T* xg = reinterpret_cast<const T*>(a.xn) + (size_t)b * N * D + cc * CHN;
  const Chunk16 zero = {0u, 0u, 0u, 0u};
  constexpr bool ln = LNF;   // (compile-time: a run-time test put a branch around every load of the burst)
  Chunk16 v[ITERS];
  float mu[ITERS], rs[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int row = r0 + it * RPP, rowc = min(row, N - 1);
    v[it] = *reinterpret_cast<const Chunk16*>(xg + (size_t)rowc * D);   // clamped address, zeroed below: no branch
    if (row >= N) v[it] = zero;
    mu[it] = ln ? a.ln_mean[(size_t)b * N + rowc] : 0.f;                // same burst
    rs[it] = ln ? a.ln_rstd[(size_t)b * N + rowc] : 0.f;
  }
  if (ln) {  // fused LayerNorm on the way in
    float gq[CHN], bq[CHN];
#pragma unroll
    for (int t = 0; t < CHN; ++t) { gq[t] = a.ln_gamma[cc * CHN + t]; bq[t] = a.ln_beta[cc * CHN + t]; }
    T* xo = (a.xn_out != nullptr && live) ? reinterpret_cast<T*>(a.xn_out) + (size_t)b * N * D + cc * CHN : nullptr;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int row = r0 + it * RPP;
      if (row < N) {
        float f[CHN];
        chunk_to_f32<T>(v[it], f);
#pragma unroll
        for (int t = 0; t < CHN; ++t) f[t] = (f[t] - mu[it]) * rs[it] * gq[t] + bq[t];
        v[it] = f32_to_chunk<T>(f);
        if (xo != nullptr) __builtin_nontemporal_store(v[it], reinterpret_cast<Chunk16*>(xo + (size_t)row * D));  // read again only in backward
      }
    }
  }
#pragma unroll
  for (int it = 0; it < ITERS; ++it) *reinterpret_cast<Chunk16*>(xs + (r0 + it * RPP) * C::LDX + cc * CHN) = v[it];
  if (KM == KM_RELATIVE && stage_tables) {
    for (int q = tid; q < C::H * C::TABLD; q += NTH) {
      const int h = q / C::TABLD, i = q % C::TABLD;
      s_tab[q] = (i < 2 * N - 1) ? a.table[h * (2 * N - 1) + i] * LOG2E : 0.f;
    }
  }
  if (KM == KM_POLY && stage_tables) stage_poly<C>(a, 0, s_coef, N, tid, NTH);
}

// ---- QKV projection of one (head, matrix) by one wave, RoPE + scale, result to LDS --------
// Swapped MFMA orientation: A-operand = weight rows (feature n on the lane), B-operand = token rows,
// so acc[nt][tt][r] = qkv[token 16tt+c][feature 16nt+4g+r] and the rotate-half partner of
// feature f < HD/2 is acc[nt + NT/2] in the same lane and register.
// q is stored as q~ = rot(q) * hd^-0.5 * log2(e): the logits come out in the exp2 domain.
template <typename T, typename C>
struct WFrags { Frag<T> f[C::NT][C::KS]; };

// Packed layout (vitpe_pack_qkv_weights): block (h, mat, nt, ks) = 64 lanes x 8 elements, so one
// fragment load of a wave is ONE contiguous 1 KB (bf16) read -- fragment-shaped loads from the
// row-major matrix touch 16 half cache lines each and are address-unit bound (measured).
template <typename T, typename C>
VITPE_DEV void load_w(const AttnArgs& a, WFrags<T, C>& w, int h, int mat, int lane) {
  const T* W = reinterpret_cast<const T*>(a.wqkv) + ((size_t)(h * 3 + mat) * C::NT * C::KS * 64 + lane) * 8;
#pragma unroll
  for (int nt = 0; nt < C::NT; ++nt)
#pragma unroll
    for (int ks = 0; ks < C::KS; ++ks) w.f[nt][ks] = ld_frag(W + (size_t)(nt * C::KS + ks) * 64 * 8);
}

template <typename T, typename C, int KM>
VITPE_DEV void project_head(const AttnArgs& a, const WFrags<T, C>& w, const T* xs, T* dst, int h, int mat, int lane) {
  constexpr int HD = C::HDD, MT = C::MTT;
  const int N = C::ntok(a);
  const int c = lane & 15, g = lane >> 4;
  const bool rope = (KM == KM_ROPE) && mat < 2;
  // cos/sin rows of this lane's tokens: issued before the MFMA loop so the loads fly under it
  f32x4 cs[MT][C::NT / 2], sn[MT][C::NT / 2];
  if (rope) {
    const size_t hoff = (a.mode == PE_ROPE_MIXED) ? (size_t)h * (N - 1) * (HD / 2) : 0;
#pragma unroll
    for (int tt = 0; tt < MT; ++tt) {
      const int tok = min(max(16 * tt + c, 1), N - 1);  // clamped: out-of-range tokens are not rotated below
#pragma unroll
      for (int nt = 0; nt < C::NT / 2; ++nt) {
        const size_t o = hoff + (size_t)(tok - 1) * (HD / 2) + 16 * nt + 4 * g;
        cs[tt][nt] = *reinterpret_cast<const f32x4*>(a.cos + o);
        sn[tt][nt] = *reinterpret_cast<const f32x4*>(a.sin + o);
      }
    }
  }
  f32x4 acc[C::NT][MT];
#pragma unroll
  for (int nt = 0; nt < C::NT; ++nt)
#pragma unroll
    for (int tt = 0; tt < MT; ++tt) acc[nt][tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const T* xrow = xs + c * C::LDX + 8 * g;
#pragma unroll
  for (int ks = 0; ks < C::KS; ++ks) {
#pragma unroll
    for (int tt = 0; tt < MT; ++tt) {
      const Frag<T> fb = ld_frag(xrow + 16 * tt * C::LDX + 32 * ks);
#pragma unroll
      for (int nt = 0; nt < C::NT; ++nt) mma(w.f[nt][ks], fb, acc[nt][tt]);
    }
  }
  if (rope) {
#pragma unroll
    for (int tt = 0; tt < MT; ++tt) {
      const int tok = 16 * tt + c;
      const bool rot = (tt == 0) ? (tok >= 1) : ((tt == MT - 1) ? (tok < N) : true);  // class token never rotated
      if (rot) {
#pragma unroll
        for (int nt = 0; nt < C::NT / 2; ++nt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float x1 = acc[nt][tt][r], x2 = acc[nt + C::NT / 2][tt][r];
            acc[nt][tt][r] = x1 * cs[tt][nt][r] - x2 * sn[tt][nt][r];
            acc[nt + C::NT / 2][tt][r] = x1 * sn[tt][nt][r] + x2 * cs[tt][nt][r];
          }
        }
      }
    }
  }
  const float sc = (mat == 0) ? a.scale * LOG2E : 1.0f;
  T* drow = dst + c * C::LDH + 4 * g;
#pragma unroll
  for (int nt = 0; nt < C::NT; ++nt)
#pragma unroll
    for (int tt = 0; tt < MT; ++tt)
      st4(drow + 16 * tt * C::LDH + 16 * nt, acc[nt][tt][0] * sc, acc[nt][tt][1] * sc, acc[nt][tt][2] * sc,
          acc[nt][tt][3] * sc);
}

// =========================================================================================
// Forward
// =========================================================================================
// IPW images per workgroup.  Two 6-wave workgroups are NOT co-resident on a CU at three waves per SIMD (measured:
// wave lifetime 21 K cycles, kernel 45 K = two rounds; the second workgroup's waves do not fit the SIMDs the first one
// left uneven), so the bf16 build puts two images = 12 waves = exactly three per SIMD into ONE workgroup.  The images
// share nothing but the staging barrier.
template <typename T, int HD, int D, int MT, int KM, int NTOK, int IPW, bool LNF, bool CENSUS = false>
__global__ __launch_bounds__(64 * (D / HD) * IPW, (sizeof(T) == 2 ? 3 : 1)) void attn_fwd_kernel(AttnArgs a) {
  using C = AttnCfg<T, HD, D, MT, 1, NTOK>;
  constexpr int NT = C::NT, KS = C::KS, HC = C::HC, SC = C::SC, NTH = 64 * C::H;
  static_assert(NT % 2 == 0, "two 16-feature tiles per K32 chunk of the head dimension");
  __shared__ __attribute__((aligned(16))) T xs_all[IPW * C::NP * C::LDX];
  __shared__ __attribute__((aligned(16))) float s_tab[KM == KM_RELATIVE ? C::H * C::TABLD : 4];
  __shared__ __attribute__((aligned(16))) float s_coef[KM == KM_POLY ? C::PESZ : 4];
  // cos / sin rows of the patch tokens (rope): [table][token][HD/2 + 8]; the 32-B row padding makes the row stride
  // 6 slots (== 2 mod 4): the per-lane f32x4 reads are bank-conflict free like the x fragments.  A global read here
  // would expose an L2 round trip per token tile (measured: 860 cycles per tile for 190 cycles of MFMA).
  constexpr int CSLD = HD / 2 + 8;
  constexpr int CSROWS = C::NP;                                      // patch tokens 1 .. N-1 at rows 0 .. N-2
  constexpr int CSTAB = (KM == KM_ROPE) ? C::H * CSROWS * CSLD : 4;  // worst case: per-head tables (rope-mixed)
  __shared__ __attribute__((aligned(16))) float s_cos[CSTAB];
  __shared__ __attribute__((aligned(16))) float s_sin[CSTAB];

  const int N = C::ntok(a);
  const int lane = threadIdx.x & 63;
  const int wave_all = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int img = wave_all / C::H, h = wave_all % C::H;              // one wave per (image, head)
  const int b_raw = blockIdx.x * IPW + img;
  const bool live = b_raw < a.B;                                     // odd batch: the last workgroup's second slot idles
  const int b = live ? b_raw : a.B - 1;
  T* const xs = xs_all + img * C::NP * C::LDX;
  const int c = lane & 15, g = lane >> 4;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  // CENSUS (debug instantiation only): lane 0 of every wave stamps the shader clock at the phase boundaries
  auto stamp = [&](int slot) {
    if (CENSUS) {
      __builtin_amdgcn_sched_barrier(0);
      if (lane == 0) a.census[((size_t)blockIdx.x * 16 + wave_all) * 8 + slot] = __builtin_amdgcn_s_memtime();
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  stamp(0);
  // packed weights: block (h, mat, nt, ks) = 64 lanes x 8 elements (vitpe_pack_qkv_weights)
  const T* const Wh = reinterpret_cast<const T*>(a.wqkv) + ((size_t)h * 3 * NT * KS * 64 + lane) * 8;
  auto wload = [&](Frag<T> (&w)[NT][KS], int mat, int nt0, int nt1) {
#pragma unroll
    for (int nt = nt0; nt < nt1; ++nt)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) w[nt][ks] = ld_frag(Wh + (size_t)((mat * NT + nt) * KS + ks) * 64 * 8);
  };

  // Register budget (168 at three waves per SIMD, no spills: a scratch access would serialise behind the weight loads
  // in flight): one matrix' weight fragments are 48 registers, a projection's accumulators 40, the parked V^T / K / Q
  // fragments 24 + 20 + 20 -- the next matrix is prefetched only as far as that leaves room.
  Frag<T> wa[NT][KS], wb[NT][KS];
  wload(wa, 2, 0, NT);                                    // Wv flies under the token staging
  stage_tokens_fwd<T, C, KM, NTH, LNF>(a, b, xs, s_tab, s_coef, threadIdx.x % NTH, live, IPW == 1 || img == 0);
  if (KM == KM_ROPE) {   // cos / sin tables -> LDS (axial: one table for all heads; mixed: one per head), indexed by
    // TOKEN: the class token's row and the padding rows hold the identity rotation (1, 0), so the rotation below needs
    // no per-element select (vit.py:56-68: the class token is never rotated)
    const int ntab = (a.mode == PE_ROPE_MIXED) ? C::H : 1, P = N - 1;
    constexpr int F4 = HD / 8;
    for (int q = threadIdx.x; q < ntab * CSROWS * F4; q += NTH * IPW) {
      const int f4 = q % F4, row = (q / F4) % CSROWS, t = q / (F4 * CSROWS);
      f32x4 cv = {1.f, 1.f, 1.f, 1.f}, sv = {0.f, 0.f, 0.f, 0.f};
      if (row >= 1 && row < N) {
        const size_t src = ((size_t)t * P + row - 1) * (HD / 2) + 4 * f4;
        cv = *reinterpret_cast<const f32x4*>(a.cos + src);
        sv = *reinterpret_cast<const f32x4*>(a.sin + src);
      }
      *reinterpret_cast<f32x4*>(&s_cos[(t * CSROWS + row) * CSLD + 4 * f4]) = cv;
      *reinterpret_cast<f32x4*>(&s_sin[(t * CSROWS + row) * CSLD + 4 * f4]) = sv;
    }
  }
  stamp(1);
  __syncthreads();
  stamp(2);
  if (!live) return;                                      // (after the last barrier)
  const T* const xrow = xs + c * C::LDX + 8 * g;          // fragment of token tile tt, K32 chunk ks: + 16 tt LDX + 32 ks

  // The projections run token tile by token tile (all K32 chunks of one tile back to back into NT accumulators that are
  // converted to operand fragments at once): a whole matrix' accumulators (40 registers) would leave the scheduler no
  // room to read the next x fragments ahead, and every MFMA pair would wait out an LDS round trip.
  // ---- v, un-swapped: acc[dt][r] = v[token 16tt + 4g + r][feature 16dt + c] -> V^T operand fragments
  Frag<T> vf[NT][SC];
#pragma unroll
  for (int sc = 0; sc < SC; ++sc) {
    if (sc == SC - 1) wload(wb, 1, 0, NT);                // Wk under the last tiles of the v projection
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc[2][NT];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int tt = 2 * sc + half;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[half][nt] = z4;
      if (tt < MT) {
        Frag<T> xf[KS];      // the whole tile's fragments first: ONE exposed LDS round trip per tile, not one per MFMA pair
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) xf[ks] = ld_frag(xrow + 16 * tt * C::LDX + 32 * ks);
        __builtin_amdgcn_sched_barrier(0);   // (the scheduler otherwise sinks each read to just before its MFMA pair)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) mma(xf[ks], wa[nt][ks], acc[half][nt]);
      }
    }
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) vf[dt][sc] = acc_to_frag<T>(acc[0][dt], acc[1][dt]);
  }
  stamp(3);
  wload(wa, 0, 0, NT / 2);                                // first half of Wq under the k projection

  // ---- k and q, swapped: acc[nt][r] = k[token 16tt + c][feature 16nt + 4g + r]; rotate (q: scale); -> fragments
  const int cs_off = (KM == KM_ROPE && a.mode == PE_ROPE_MIXED) ? h * CSROWS * CSLD : 0;
  auto project_rot = [&](const Frag<T> (&w)[NT][KS], Frag<T> (&dst)[MT][HC], float sc, auto scaled) {
#pragma unroll
    for (int tt = 0; tt < MT; ++tt) {
      const int tok = 16 * tt + c;
      f32x4 cs4[NT / 2], sn4[NT / 2];
      f32x4 acc[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] = z4;
      {
        Frag<T> xf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) xf[ks] = ld_frag(xrow + 16 * tt * C::LDX + 32 * ks);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) mma(w[nt][ks], xf[ks], acc[nt]);
        __builtin_amdgcn_sched_barrier(0);
        if (KM == KM_ROPE) {   // this tile's cos / sin rows: read while the matrix pipe drains (no registers held under the MFMAs)
#pragma unroll
          for (int nt = 0; nt < NT / 2; ++nt) {
            cs4[nt] = *reinterpret_cast<const f32x4*>(&s_cos[cs_off + tok * CSLD + 16 * nt + 4 * g]);
            sn4[nt] = *reinterpret_cast<const f32x4*>(&s_sin[cs_off + tok * CSLD + 16 * nt + 4 * g]);
          }
        }
      }
      if (KM == KM_ROPE) {   // (f32x4 arithmetic: the compiler emits packed v_pk_mul / v_pk_fma pairs)
#pragma unroll
        for (int nt = 0; nt < NT / 2; ++nt) {
          const f32x4 x1 = acc[nt], x2 = acc[nt + NT / 2];
          acc[nt] = x1 * cs4[nt] - x2 * sn4[nt];
          acc[nt + NT / 2] = x1 * sn4[nt] + x2 * cs4[nt];
        }
      }
#pragma unroll
      for (int cs = 0; cs < HC; ++cs) {
        if constexpr (decltype(scaled)::value) dst[tt][cs] = acc_to_frag<T>(acc[2 * cs] * sc, acc[2 * cs + 1] * sc);
        else dst[tt][cs] = acc_to_frag<T>(acc[2 * cs], acc[2 * cs + 1]);
      }
    }
  };
  Frag<T> kf[MT][HC], qf[MT][HC];
  __builtin_amdgcn_sched_barrier(0);
  project_rot(wb, kf, 1.0f, std::false_type{});
  stamp(4);
  wload(wa, 0, NT / 2, NT);                                         // second half of Wq once Wk is dead
  __builtin_amdgcn_sched_barrier(0);
  project_rot(wa, qf, a.scale * LOG2E, std::true_type{});           // logits come out in the exp2 domain
  stamp(5);

  // ---- per 16-query tile: S^T = K Q^T (+bias), softmax in the exp2 domain, O^T = V^T P^T, store
  T* const outp = reinterpret_cast<T*>(a.out) + (size_t)b * N * D + h * HD;
#pragma unroll
  for (int it = 0; it < MT; ++it) {
    // (unrolled so that qf[it] is a static register index; the fence keeps the scheduler from interleaving the tiles'
    //  accumulators -- five tiles' worth of live S^T registers is what spills)
    __builtin_amdgcn_sched_barrier(0);
    const int i = 16 * it + c;
    // s[jt][r] = log2e * (scale q_i.k_j + bias(i,j)),  key j = 16jt + 4g + r, query i = 16it + c
    f32x4 s[MT];
    float m = -1e30f;
#pragma unroll
    for (int jt = 0; jt < MT; ++jt) {
      s[jt] = z4;
#pragma unroll
      for (int cs = 0; cs < HC; ++cs) mma(kf[jt][cs], qf[it][cs], s[jt]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * jt + 4 * g + r;
        float v = s[jt][r];
        if (KM == KM_RELATIVE || KM == KM_POLY) v += pe_bias2<C, KM>(a, s_tab, s_coef, h, i, j, N);
        if (jt == MT - 1) v = (j < N) ? v : -1e30f;        // padding keys only exist in the last tile
        s[jt][r] = v;
        m = fmaxf(m, v);
      }
    }
    m = xg_max(m);
    f32x2 l2 = {0.f, 0.f};
    const f32x4 m4 = {m, m, m, m};
#pragma unroll
    for (int jt = 0; jt < MT; ++jt) {
      const f32x4 d = s[jt] - m4;                          // packed subtract, packed row sum below: the issue port is
      f32x4 p;                                             // what this kernel runs out of, not the pipes
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] = __builtin_amdgcn_exp2f(d[r]);
      s[jt] = p;
      l2 += (f32x2){p[0], p[1]};
      l2 += (f32x2){p[2], p[3]};
    }
    float l = xg_sum(l2[0] + l2[1]);
    f32x4 o[NT];
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) o[dt] = z4;
#pragma unroll
    for (int sc = 0; sc < SC; ++sc) {
      const Frag<T> bp = acc_to_frag<T>(s[2 * sc], (2 * sc + 1 < MT) ? s[(2 * sc + 1 < MT) ? 2 * sc + 1 : 0] : z4);
#pragma unroll
      for (int dt = 0; dt < NT; ++dt) mma(vf[dt][sc], bp, o[dt]);
    }
    const float inv = __builtin_amdgcn_rcpf(l);
    if (sizeof(T) == 2) {
      // Lane (c, g) holds features 16dt + 4g .. +3 of query c for dt = 0, 1: two 8-B pieces 32 B apart.  One
      // v_permlane16_swap per dword hands the odd lane group's dt-0 piece to the even group and the even group's dt-1
      // piece to the odd one: every lane then owns 8 CONTIGUOUS features (16 B) -- half the store instructions, and a
      // row is written as one 64-B segment per 32 features instead of four 8-B pieces (the C-layout stores were
      // issue-bound: 16 row segments per instruction).
#pragma unroll
      for (int dp = 0; dp < NT; dp += 2) {
        uint32_t lo[2], hi[2];
#pragma unroll
        for (int w2 = 0; w2 < 2; ++w2) {
          bf16x2 pa, pb;
          const f32x4 oa = o[dp] * inv, ob = o[dp + 1] * inv;
          pa[0] = (bf16)oa[2 * w2]; pa[1] = (bf16)oa[2 * w2 + 1];
          pb[0] = (bf16)ob[2 * w2]; pb[1] = (bf16)ob[2 * w2 + 1];
          const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(uint32_t, pa), __builtin_bit_cast(uint32_t, pb),
                                                         false, false);
          lo[w2] = r[0]; hi[w2] = r[1];
        }
        // even g: [own dt, neighbour's dt] = features 16dp + 8(g/2) .. +7 ; odd g: the same of tile dp + 1
        const int f0 = 16 * (dp + (g & 1)) + 8 * (g >> 1);
        if (it < MT - 1 || i < N)
          *reinterpret_cast<Chunk16*>(outp + (size_t)i * D + f0) = (Chunk16){lo[0], lo[1], hi[0], hi[1]};
      }
    } else if (it < MT - 1 || i < N) {
#pragma unroll
      for (int dt = 0; dt < NT; ++dt)
        st4(outp + (size_t)i * D + 16 * dt + 4 * g, o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
    }
  }
  stamp(6);
}

// =========================================================================================
// Backward, register-resident (bf16 throughput build): the forward's mapping -- one wave per (image, head), two images
// per workgroup, no barrier after the staging one -- applied to the hand-derived backward:
//   staging : LayerNorm'd tokens x and the output gradient dO of the image -> LDS (both [token][D] rows)
//   project : v~, k~ (swapped: keys on the lane), K^T (un-swapped k~: features on the lane), q~ (swapped), later Q^T
//   step 1  : per 16-query tile on the SWAPPED tiles (lane = query): S^T, P^T, dP^T = V dO^T, delta, dS^T, the
//             positional-parameter gradients, dQ^T = K^T dS^T, inverse rotation, store; lse / delta -> wave-private LDS
//   step 2  : per 16-key tile on the PLAIN tiles (lane = key): S = Q K^T and dP = dO V^T re-derived from the same
//             fragments, P from the saved lse, dS; dV^T = dO^T P and dK^T = Q^T dS with the accumulators as operands
//             (dO^T by transposed LDS reads), inverse rotation, store.
// k and q are each projected twice (once per orientation) instead of being parked in LDS and read back transposed:
// 120 extra MFMAs per wave buy a kernel whose q/k/v never touch LDS and whose twelve waves per CU run unsynchronised.
// =========================================================================================
template <typename T, typename C, int NTH>
VITPE_DEV void stage_rows_plain(const T* src, T* dst, int ld, int N, int tid) {
  constexpr int CHN = CH<T>::n, D = C::DD, CPRW = D / CHN, RPP = NTH / CPRW, ITERS = C::NP / RPP;
  const int cc = tid % CPRW, r0 = tid / CPRW;
  const Chunk16 zero = {0u, 0u, 0u, 0u};
  Chunk16 v[ITERS];
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int row = r0 + it * RPP;
    v[it] = *reinterpret_cast<const Chunk16*>(src + (size_t)min(row, N - 1) * D + cc * CHN);
    if (row >= N) v[it] = zero;
  }
#pragma unroll
  for (int it = 0; it < ITERS; ++it) *reinterpret_cast<Chunk16*>(dst + (r0 + it * RPP) * ld + cc * CHN) = v[it];
}

// PDEG (polynomial mode): highest degree this instantiation accumulates (3: the reference's default, or MAXDEG)
template <int HD, int D, int MT, int KM, int NTOK, int IPW, bool LNF, bool MIXED, int PDEG = 7>
__global__ __launch_bounds__(64 * (D / HD) * IPW, 3) void attn_bwd_reg_kernel(AttnArgs a) {
  using T = bf16;
  using C = AttnCfg<T, HD, D, MT, 1, NTOK>;
  constexpr int NT = C::NT, KS = C::KS, HC = C::HC, SC = C::SC, NTH = 64 * C::H;
  static_assert(NT == 2 && HC == 1, "head dimension 32");
  constexpr int CSLD = HD / 2 + 8;
  constexpr int FRAG = 64 * 8;                       // elements of one parked fragment (lane-linear 16 B per lane)
  // x tiles; once the projections are done (second barrier) the region is re-used as the waves' dO-fragment scratch
  constexpr int XS_ELEMS = IPW * C::NP * C::LDX, DOS_ELEMS = IPW * C::H * MT * FRAG;
  __shared__ __attribute__((aligned(16))) T xs_all[XS_ELEMS > DOS_ELEMS ? XS_ELEMS : DOS_ELEMS];
  __shared__ __attribute__((aligned(16))) T qs_all[IPW * C::H * MT * FRAG];   // q~ fragments of every wave
  __shared__ __attribute__((aligned(16))) float s_tab[KM == KM_RELATIVE ? C::H * C::TABLD : 4];
  __shared__ __attribute__((aligned(16))) float s_coef[KM == KM_POLY ? C::PESZ : 4];
  __shared__ __attribute__((aligned(16))) float s_cos[KM == KM_ROPE ? C::NP * CSLD : 4];
  __shared__ __attribute__((aligned(16))) float s_sin[KM == KM_ROPE ? C::NP * CSLD : 4];
  __shared__ __attribute__((aligned(16))) float s_stat[IPW * C::H * 2 * C::NP];   // per wave: [lse2 | delta][token]
  __shared__ float s_dtab[KM == KM_RELATIVE ? C::H * C::TABLD : 4];   // per workgroup (both images)
  __shared__ float s_dcoef[C::H * (C::MAXDEG + 1)];
  __shared__ float s_dfreq[2 * C::H * (HD / 2)];

  const int N = C::ntok(a), P = N - 1;
  const int lane = threadIdx.x & 63;
  const int wave_all = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int img = wave_all / C::H, h = wave_all % C::H;
  const int b_raw = blockIdx.x * IPW + img;
  const bool live = b_raw < a.B;
  const int b = live ? b_raw : a.B - 1;
  const int tid_img = threadIdx.x % NTH;
  T* const xs = xs_all + img * C::NP * C::LDX;
  T* const qsw = qs_all + wave_all * MT * FRAG + lane * 8;     // this wave's parked q~ fragments (+ tile * FRAG)
  T* const dsw = xs_all + wave_all * MT * FRAG + lane * 8;     // this wave's parked dO fragments (after barrier 2)
  float* const lse_w = s_stat + (img * C::H + h) * 2 * C::NP;
  float* const del_w = lse_w + C::NP;
  float* const dtab_i = s_dtab;
  float* const dcoef_i = s_dcoef;
  float* const dfreq_i = s_dfreq;
  const int c = lane & 15, g = lane >> 4;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  constexpr bool mixed = (KM == KM_ROPE) && MIXED;   // (compile-time: the frequency-gradient code costs the axial build 100 spills)

  const T* const Wh = reinterpret_cast<const T*>(a.wqkv) + ((size_t)h * 3 * NT * KS * 64 + lane) * 8;
  auto wload = [&](Frag<T> (&w)[NT][KS], int mat) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) w[nt][ks] = ld_frag(Wh + (size_t)((mat * NT + nt) * KS + ks) * 64 * 8);
  };
  Frag<T> w[NT][KS];
  wload(w, 2);                                            // Wv under the staging
  stage_tokens_fwd<T, C, KM, NTH, LNF>(a, b, xs, s_tab, s_coef, tid_img, false, IPW == 1 || img == 0);
  if (KM == KM_ROPE && !mixed) {   // axial table by TOKEN, identity rows for the class token and the padding
    constexpr int F4 = HD / 8;
    for (int q = threadIdx.x; q < C::NP * F4; q += NTH * IPW) {
      const int f4 = q % F4, row = q / F4;
      f32x4 cv = {1.f, 1.f, 1.f, 1.f}, sv = {0.f, 0.f, 0.f, 0.f};
      if (row >= 1 && row < N) {
        cv = *reinterpret_cast<const f32x4*>(a.cos + (size_t)(row - 1) * (HD / 2) + 4 * f4);
        sv = *reinterpret_cast<const f32x4*>(a.sin + (size_t)(row - 1) * (HD / 2) + 4 * f4);
      }
      *reinterpret_cast<f32x4*>(&s_cos[row * CSLD + 4 * f4]) = cv;
      *reinterpret_cast<f32x4*>(&s_sin[row * CSLD + 4 * f4]) = sv;
    }
  }
  if (KM == KM_RELATIVE)
    for (int q = threadIdx.x; q < C::H * C::TABLD; q += NTH * IPW) s_dtab[q] = 0.f;
  for (int q = threadIdx.x; q < C::H * (C::MAXDEG + 1); q += NTH * IPW) s_dcoef[q] = 0.f;
  for (int q = threadIdx.x; q < 2 * C::H * (HD / 2); q += NTH * IPW) s_dfreq[q] = 0.f;
  __syncthreads();

  const T* const xrow = xs + c * C::LDX + 8 * g;
  const unsigned hoff = mixed ? (unsigned)(h * P * (HD / 2)) : 0u;   // (32-bit offsets from a uniform base: the 64-bit per-lane
                                                                      //  addresses were what the mixed build spilled)
  // cos / sin of token `tok`, features f .. f+3 (identity outside the patch tokens)
  auto cs_vec = [&](int tok, int f, f32x4& cv, f32x4& sv) {
    if (!mixed) {
      cv = *reinterpret_cast<const f32x4*>(&s_cos[tok * CSLD + f]);
      sv = *reinterpret_cast<const f32x4*>(&s_sin[tok * CSLD + f]);
    } else {
      const bool ok = tok >= 1 && tok < N;
      const unsigned o = hoff + (unsigned)((min(max(tok, 1), N - 1) - 1) * (HD / 2) + f);
      const f32x4 cg = *reinterpret_cast<const f32x4*>(a.cos + o), sg = *reinterpret_cast<const f32x4*>(a.sin + o);
      cv = ok ? cg : (f32x4){1.f, 1.f, 1.f, 1.f};
      sv = ok ? sg : z4;
    }
  };
  // swapped projection of token tile tt: acc[nt][r] = (x W^T)[token 16tt + c][feature 16nt + 4g + r]; rotate; scale
  auto proj_sw = [&](int tt, bool rope, float sc, Frag<T>& dst) {
    Frag<T> xf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) xf[ks] = ld_frag(xrow + 16 * tt * C::LDX + 32 * ks);
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc[NT] = {z4, z4};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) mma(w[nt][ks], xf[ks], acc[nt]);
    __builtin_amdgcn_sched_barrier(0);
    if (KM == KM_ROPE && rope) {
      f32x4 cv, sv;
      cs_vec(16 * tt + c, 4 * g, cv, sv);
      const f32x4 x1 = acc[0], x2 = acc[1];
      acc[0] = x1 * cv - x2 * sv;
      acc[1] = x1 * sv + x2 * cv;
    }
    dst = acc_to_frag<T>(acc[0] * sc, acc[1] * sc);
    // pin the packed fragment here: left alone the compiler sinks the conversion to the fragment's first use (after the
    // barrier) and carries -- and spills -- the fp32 accumulators, twice the registers
    asm volatile("" : "+v"(dst.v));
  };
  // Transposition on the matrix core.  A swapped fragment f[tt] holds X[token 16tt + c][feature phi(g, t)] (phi = the
  // acc_to_frag order: t < 4 -> 4g + t, t >= 4 -> 16 + 4g + t - 4); multiplied by the 0/1 selection matrix E_nt
  // (E_nt[k = (g, t)][col c'] = 1 iff phi(g, t) == 16nt + c') it comes out as acc[r] = X[token 16tt + 4g + r][feature
  // 16nt + c]: the token index in the registers, where acc_to_frag turns tile pairs into the operand of a product that
  // contracts over TOKENS (K^T for dQ, Q^T for dK, dO^T for dV).  Exact (one 1.0 per column), 2 MFMAs per tile --
  // instead of a second projection (12) or a round trip through a transposed LDS image.
  Frag<T> e0, e1;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    e0.v[t] = (bf16)((t < 4 && 4 * g + t == c) ? 1.0f : 0.0f);
    e1.v[t] = (bf16)((t >= 4 && 4 * g + t - 4 == c) ? 1.0f : 0.0f);
  }
  auto transpose_pair = [&](const Frag<T>& fa, const Frag<T>* fb, Frag<T>& d0, Frag<T>& d1) {
    f32x4 a0 = z4, a1 = z4, b0 = z4, b1 = z4;
    mma(fa, e0, a0);
    mma(fa, e1, a1);
    if (fb != nullptr) { mma(*fb, e0, b0); mma(*fb, e1, b1); }
    d0 = acc_to_frag<T>(a0, b0);
    d1 = acc_to_frag<T>(a1, b1);
  };

  const float qsc = a.scale * LOG2E;
  Frag<T> vkf[MT], kf[MT];
#pragma unroll
  for (int tt = 0; tt < MT; ++tt) proj_sw(tt, false, 1.0f, vkf[tt]);
  wload(w, 1);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int tt = 0; tt < MT; ++tt) proj_sw(tt, true, 1.0f, kf[tt]);
  wload(w, 0);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int tt = 0; tt < MT; ++tt) {   // q~ fragments are parked (lane-linear: conflict-free 16-B accesses)
    Frag<T> qf;
    proj_sw(tt, true, qsc, qf);
    *reinterpret_cast<bf16x8*>(qsw + tt * FRAG) = qf.v;
  }
  __syncthreads();                     // every wave is done with the x tiles: the region becomes the dO scratch
  if (!live) return;
  {  // this head's dO rows as operand fragments: lane (c, g) <- dO[token 16tt + c][features 4g..4g+3 | 16+4g..]
    const T* dog = reinterpret_cast<const T*>(a.dout) + (size_t)b * N * D + h * HD;
    Frag<T> df[MT];
#pragma unroll
    for (int tt = 0; tt < MT; ++tt) {
      const int tok = 16 * tt + c;
      bf16x4 lo = {(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f}, hi = lo;
      if (tok < N) {
        lo = *reinterpret_cast<const bf16x4*>(dog + (size_t)tok * D + 4 * g);
        hi = *reinterpret_cast<const bf16x4*>(dog + (size_t)tok * D + 16 + 4 * g);
      }
      df[tt].v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    }
#pragma unroll
    for (int tt = 0; tt < MT; ++tt) *reinterpret_cast<bf16x8*>(dsw + tt * FRAG) = df[tt].v;
  }
  auto qf_load = [&](int tt) { Frag<T> f; f.v = *reinterpret_cast<const bf16x8*>(qsw + tt * FRAG); return f; };
  auto dof_load = [&](int tt) { Frag<T> f; f.v = *reinterpret_cast<const bf16x8*>(dsw + tt * FRAG); return f; };
  Frag<T> ktf[NT][SC];
#pragma unroll
  for (int scx = 0; scx < SC; ++scx)
    transpose_pair(kf[2 * scx], (2 * scx + 1 < MT) ? &kf[(2 * scx + 1 < MT) ? 2 * scx + 1 : 0] : nullptr, ktf[0][scx], ktf[1][scx]);

  T* const dqg = reinterpret_cast<T*>(a.out) + (size_t)b * N * 3 * D + h * HD;
  // 16-B stores of a swapped-orientation result pair (features 16dt + 4g + r of token c): see the forward kernel
  auto store_pair = [&](T* rowp, const f32x4& o0, const f32x4& o1, bool ok) {
    uint32_t lo[2], hi[2];
#pragma unroll
    for (int w2 = 0; w2 < 2; ++w2) {
      bf16x2 pa, pb;
      pa[0] = (bf16)o0[2 * w2]; pa[1] = (bf16)o0[2 * w2 + 1];
      pb[0] = (bf16)o1[2 * w2]; pb[1] = (bf16)o1[2 * w2 + 1];
      const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(uint32_t, pa), __builtin_bit_cast(uint32_t, pb), false, false);
      lo[w2] = r[0]; hi[w2] = r[1];
    }
    const int f0 = 16 * (g & 1) + 8 * (g >> 1);
    if (ok) *reinterpret_cast<Chunk16*>(rowp + f0) = (Chunk16){lo[0], lo[1], hi[0], hi[1]};
  };

  // Polynomial-RPE coefficient gradient, d coeff[k] = sum_ij dS[i][j] dist(i, j)^k over patch pairs (positional_encoding.py
  // :127-171 backwards): ONE set of PDEG + 1 per-lane accumulators for the whole wave, reduced once at the end.  (The
  // first version ran a MAXDEG-long power loop with a run-time degree test per element and a wave reduction per tile:
  // ~26 VALU per logit, 57 spilled registers -- the mode's backward took 75 us against 34.)
  float cacc[PDEG + 1];
#pragma unroll
  for (int k = 0; k <= PDEG; ++k) cacc[k] = 0.f;
  // ---- step 1: query tiles on the swapped tiles --------------------------------------------------------------
#pragma unroll
  for (int it = 0; it < MT; ++it) {
    __builtin_amdgcn_sched_barrier(0);
    const int i = 16 * it + c;
    const Frag<T> dof = dof_load(it), qfi = qf_load(it);
    f32x4 s[MT], dp[MT];
    float m = -1e30f;
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    // polynomial bias by L1 grid distance: the packed coordinates of this lane's query (once per tile) and of its four
    // keys (one 16-B LDS read per key tile) instead of two coordinate reads per logit; class-token row / column = 0
    const unsigned xyi = (KM == KM_POLY) ? reinterpret_cast<const unsigned*>(s_coef + C::H * C::PBLD)[i] : 0u;
    const float* const ptab = s_coef + (a.coeff_per_head ? h : 0) * C::PBLD;
    const bool qcls = (it == 0) && (c == 0);
#pragma unroll
    for (int jt = 0; jt < MT; ++jt) {
      s[jt] = z4;
      mma(kf[jt], qfi, s[jt]);
      dp[jt] = z4;
      mma(vkf[jt], dof, dp[jt]);
      const u32x4 xyj = (KM == KM_POLY) ? *reinterpret_cast<const u32x4*>(s_coef + C::H * C::PBLD + 16 * jt + 4 * g) : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * jt + 4 * g + r;
        float v = s[jt][r];
        if (KM == KM_RELATIVE) v += pe_bias2<C, KM>(a, s_tab, s_coef, h, i, j, N);
        if (KM == KM_POLY) {
          const float bv = ptab[__builtin_amdgcn_sad_u8(xyi, xyj[r], 0u)];
          const bool cls = qcls || (jt == 0 && r == 0 && g == 0);
          v += cls ? 0.f : bv;
        }
        if (jt == MT - 1) v = (j < N) ? v : -1e30f;
        s[jt][r] = v;
        m = fmaxf(m, v);
      }
    }
    m = xg_max(m);
    float l = 0.f;
#pragma unroll
    for (int jt = 0; jt < MT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) { const float p = __builtin_amdgcn_exp2f(s[jt][r] - m); s[jt][r] = p; l += p; }
    l = xg_sum(l);
    const float inv = __builtin_amdgcn_rcpf(l);
    float dl = 0.f;
#pragma unroll
    for (int jt = 0; jt < MT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) { s[jt][r] *= inv; dl += s[jt][r] * dp[jt][r]; }
    dl = xg_sum(dl);
    if (g == 0) { lse_w[i] = m + __builtin_amdgcn_logf(l); del_w[i] = dl; }   // v_log_f32 = log2
    const bool qvalid = (it < MT - 1) || (i < N);
    float tacc[PDEG + 1];                  // this tile's contribution (one query per lane: the class-token mask is per tile)
#pragma unroll
    for (int k = 0; k <= PDEG; ++k) tacc[k] = 0.f;
#pragma unroll
    for (int jt = 0; jt < MT; ++jt) {
      // (fenced per key tile: left alone the scheduler computes the distances and their powers of all twenty logits
      //  ahead of the dS values -- sixty live registers, 184 spilled)
      if (KM == KM_POLY) __builtin_amdgcn_sched_barrier(0);
      // packed (x | y << 8) grid coordinates of this lane's four keys: one 16-B LDS read
      const u32x4 xyj = (KM == KM_POLY) ? *reinterpret_cast<const u32x4*>(s_coef + C::H * C::PBLD + 16 * jt + 4 * g) : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * jt + 4 * g + r;
        const bool valid = qvalid && ((jt < MT - 1) || (j < N));
        const float ds = valid ? s[jt][r] * (dp[jt][r] - dl) : 0.f;
        dp[jt][r] = ds;
        if (KM == KM_POLY) {
          // the class-token COLUMN is key 0 = element (jt 0, g 0, r 0) only; the class-token ROW is masked per tile below
          const float dsk = (jt == 0 && r == 0) ? (g == 0 ? 0.f : ds) : ds;
          const float x = (float)__builtin_amdgcn_sad_u8(xyi, xyj[r], 0u);
          float pw = x;
          tacc[0] += dsk;
#pragma unroll
          for (int k = 1; k <= PDEG; ++k) { tacc[k] = fmaf(dsk, pw, tacc[k]); if (k < PDEG) pw *= x; }
        }
      }
    }
    if (KM == KM_POLY) {
      const float qm = (it == 0 && c == 0) ? 0.f : 1.f;      // query 0 is the class token: its row of the bias is zero
#pragma unroll
      for (int k = 0; k <= PDEG; ++k) {
        cacc[k] = fmaf(qm, tacc[k], cacc[k]);
        asm volatile("" : "+v"(cacc[k]));   // final HERE: left alone the compiler sinks the whole accumulation of all five tiles
      }                                     // behind the loop (its only use) and parks the hundred dS values in scratch meanwhile
    }
    if (KM == KM_RELATIVE) {
#pragma unroll
      for (int jt = 0; jt < MT; ++jt) {
        float d0, d1;
        tile_diag_sums(dp[jt], lane, d0, d1);
        const int idx0 = 16 * (it - jt) + c + N - 1;
        if (g == 0) {
          if (idx0 >= 0 && idx0 <= 2 * N - 2) atomicAdd(&dtab_i[h * C::TABLD + idx0], d0);
          if (c >= 1 && idx0 - 16 >= 0 && idx0 - 16 <= 2 * N - 2) atomicAdd(&dtab_i[h * C::TABLD + idx0 - 16], d1);
        }
      }
    }
    // dQrot^T[d][i] / scale = sum_j K^T[d][j] dS^T[j][i]
    f32x4 dqa[NT] = {z4, z4};
#pragma unroll
    for (int scx = 0; scx < SC; ++scx) {
      const Frag<T> bs = acc_to_frag<T>(dp[2 * scx], (2 * scx + 1 < MT) ? dp[(2 * scx + 1 < MT) ? 2 * scx + 1 : 0] : z4);
#pragma unroll
      for (int dt = 0; dt < NT; ++dt) mma(ktf[dt][scx], bs, dqa[dt]);
    }
    if (mixed) {   // dL/dphase = (dq~2 q~1 - dq~1 q~2): q~ = the fragment this tile's logits were made from
      const bool tok_ok = i >= 1 && i < N;
      f32x4 dph;
#pragma unroll
      for (int r = 0; r < 4; ++r) dph[r] = dqa[1][r] * (float)qfi.v[r] - dqa[0][r] * (float)qfi.v[4 + r];
      mixed_freq_grad_tile(dfreq_i, dph, i, tok_ok, 16 * it, h, C::H, P, a.grid, HD / 2, 4 * g, LN2, lane);
    }
    if (KM == KM_ROPE) {   // inverse rotation (identity rows outside the patch tokens)
      f32x4 cv, sv;
      cs_vec(min(i, C::NP - 1), 4 * g, cv, sv);
      const f32x4 d1 = dqa[0], d2 = dqa[1];
      dqa[0] = d1 * cv + d2 * sv;
      dqa[1] = d2 * cv - d1 * sv;
    }
    store_pair(dqg + (size_t)i * 3 * D, dqa[0] * a.scale, dqa[1] * a.scale, qvalid);
  }

  if (KM == KM_POLY) {
#pragma unroll
    for (int k = 0; k <= PDEG; ++k)
      if (k <= a.degree) {
        const float t = wave_sum(cacc[k]);
        if (lane == 0) atomicAdd(&dcoef_i[(a.coeff_per_head ? h : 0) * (C::MAXDEG + 1) + k], t);
      }
  }
  // ---- Q^T and dO^T operands for dK / dV (K^T is dead now) -------------------------------------------------------
  Frag<T> qtf[NT][SC], dotf[NT][SC];
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int scx = 0; scx < SC; ++scx) {
    const bool two = 2 * scx + 1 < MT;
    const Frag<T> qa = qf_load(2 * scx), qb = qf_load(two ? 2 * scx + 1 : 0);
    transpose_pair(qa, two ? &qb : nullptr, qtf[0][scx], qtf[1][scx]);
    const Frag<T> da = dof_load(2 * scx), db = dof_load(two ? 2 * scx + 1 : 0);
    transpose_pair(da, two ? &db : nullptr, dotf[0][scx], dotf[1][scx]);
  }
  __builtin_amdgcn_s_waitcnt(0xC07F);   // this wave's lse / delta stores (LDS operations of a wave complete in order)

  // ---- step 2: key tiles on the plain tiles -------------------------------------------------------------------
#pragma unroll
  for (int jt = 0; jt < MT; ++jt) {
    __builtin_amdgcn_sched_barrier(0);
    const int j = 16 * jt + c;
    const bool kvalid = (jt < MT - 1) || (j < N);
    const unsigned xyk = (KM == KM_POLY) ? reinterpret_cast<const unsigned*>(s_coef + C::H * C::PBLD)[j] : 0u;
    const float* const ptab2 = s_coef + (a.coeff_per_head ? h : 0) * C::PBLD;
    const bool kcls = (jt == 0) && (c == 0);
    f32x4 p[MT], ds[MT];
#pragma unroll
    for (int it = 0; it < MT; ++it) {
      const Frag<T> dof = dof_load(it), qfi = qf_load(it);
      p[it] = z4;
      mma(qfi, kf[jt], p[it]);             // S[query 16it + 4g + r][key j]
      ds[it] = z4;
      mma(dof, vkf[jt], ds[it]);           // dP[query][key]
      const f32x4 lse = *reinterpret_cast<const f32x4*>(&lse_w[16 * it + 4 * g]);
      const f32x4 dlv = *reinterpret_cast<const f32x4*>(&del_w[16 * it + 4 * g]);
      typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
      const u32x4 xyq = (KM == KM_POLY) ? *reinterpret_cast<const u32x4*>(s_coef + C::H * C::PBLD + 16 * it + 4 * g) : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * it + 4 * g + r;
        float sv = p[it][r];
        if (KM == KM_RELATIVE) sv += pe_bias2<C, KM>(a, s_tab, s_coef, h, i, j, N);
        if (KM == KM_POLY) {
          const float bv = ptab2[__builtin_amdgcn_sad_u8(xyk, xyq[r], 0u)];
          const bool cls = kcls || (it == 0 && r == 0 && g == 0);
          sv += cls ? 0.f : bv;
        }
        const bool valid = kvalid && ((it < MT - 1) || (i < N));
        const float pv = valid ? __builtin_amdgcn_exp2f(sv - lse[r]) : 0.f;
        p[it][r] = pv;
        ds[it][r] = pv * (ds[it][r] - dlv[r]);
      }
    }
    f32x4 dva[NT] = {z4, z4}, dka[NT] = {z4, z4};
#pragma unroll
    for (int scx = 0; scx < SC; ++scx) {
      const bool two = (2 * scx + 1 < MT);
      const Frag<T> bp = acc_to_frag<T>(p[2 * scx], two ? p[two ? 2 * scx + 1 : 0] : z4);
      const Frag<T> bs = acc_to_frag<T>(ds[2 * scx], two ? ds[two ? 2 * scx + 1 : 0] : z4);
#pragma unroll
      for (int dt = 0; dt < NT; ++dt) {
        mma(dotf[dt][scx], bp, dva[dt]);
        mma(qtf[dt][scx], bs, dka[dt]);
      }
    }
    dka[0] *= LN2; dka[1] *= LN2;          // q~ carries scale * log2e
    if (mixed) {
      const bool tok_ok = j >= 1 && j < N;
      f32x4 dph;
#pragma unroll
      for (int r = 0; r < 4; ++r) dph[r] = dka[1][r] * (float)kf[jt].v[r] - dka[0][r] * (float)kf[jt].v[4 + r];
      mixed_freq_grad_tile(dfreq_i, dph, j, tok_ok, 16 * jt, h, C::H, P, a.grid, HD / 2, 4 * g, 1.0f, lane);
    }
    if (KM == KM_ROPE) {
      f32x4 cv, sv;
      cs_vec(min(j, C::NP - 1), 4 * g, cv, sv);
      const f32x4 d1 = dka[0], d2 = dka[1];
      dka[0] = d1 * cv + d2 * sv;
      dka[1] = d2 * cv - d1 * sv;
    }
    store_pair(dqg + (size_t)j * 3 * D + D, dka[0], dka[1], kvalid);
    store_pair(dqg + (size_t)j * 3 * D + 2 * D, dva[0], dva[1], kvalid);
  }

  // ---- positional-parameter gradients: accumulated per WORKGROUP in LDS (both images, all heads), flushed once -- the
  // global adds all land on the same few hundred addresses, where an atomic costs ~12 ns serialised: one flush per
  // workgroup instead of one per image halves them
  __syncthreads();   // (waves of an idle image slot have exited: the barrier counts the running waves only)
  // threads still running: the live images are the leading ones, so they are threadIdx.x < nrun
  const int nrun = NTH * min(IPW, a.B - (int)blockIdx.x * IPW);
  if (KM == KM_RELATIVE) {
    for (int q = threadIdx.x; q < C::H * (2 * N - 1); q += nrun) {
      const int hh = q / (2 * N - 1), i = q % (2 * N - 1);
      atomicAdd(a.dtable + q, s_dtab[hh * C::TABLD + i]);
    }
  } else if (KM == KM_POLY) {
    const int nh = a.coeff_per_head ? C::H : 1;
    for (int q = threadIdx.x; q < nh * (a.degree + 1); q += nrun) {
      const int hh = q / (a.degree + 1), k = q % (a.degree + 1);
      atomicAdd(a.dcoeff + q, s_dcoef[hh * (C::MAXDEG + 1) + k]);
    }
  } else if (mixed) {
    for (int q = threadIdx.x; q < 2 * C::H * (HD / 2); q += nrun) atomicAdd(a.dfreqs + q, s_dfreq[q]);
  }
}

// =========================================================================================
// Backward
// =========================================================================================
template <typename T, int HD, int D, int MT, int HPP, int KM, int NTOK>
__global__ __launch_bounds__(384) void attn_bwd_kernel(AttnArgs a) {
  using C = AttnCfg<T, HD, D, MT, HPP, NTOK>;
  __shared__ __attribute__((aligned(16))) T xs[C::NP * C::LDX];
  __shared__ __attribute__((aligned(16))) T hb[4 * HPP * C::HSZ];  // q,k,v,dO: [mat][hh][VR][LDH]
  __shared__ __attribute__((aligned(16))) float s_tab[KM == KM_RELATIVE ? C::H * C::TABLD : 4];
  __shared__ __attribute__((aligned(16))) float s_coef[KM == KM_POLY ? C::PESZ : 4];
  __shared__ __attribute__((aligned(16))) float s_stat[HPP * 2 * C::NP];  // [hh][lse2 | delta][token]
  __shared__ float s_dtab[KM == KM_RELATIVE ? C::H * C::TABLD : 4];  // relative-table gradient of this image
  __shared__ float s_dcoef[C::H * (C::MAXDEG + 1)];
  __shared__ float s_dfreq[2 * C::H * (HD / 2)];
  // d_qkv of the pass's heads, [mat][token][HPP*HD] so that a token row holds HPP*HD contiguous
  // elements per matrix: flushed with coalesced 16-B stores (the C-layout stores run at < 1/2 rate)
  constexpr int SLD = HPP * HD + Pad<T>::elems;
  __shared__ __attribute__((aligned(16))) T s_dq[3 * C::NP * SLD];

  const int N = C::ntok(a);
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int P = N - 1;
  WFrags<T, C> wf;
  {
    const int hh = wave / 3, mat = wave % 3;
    if (hh < HPP && hh < C::H) load_w<T, C>(a, wf, hh, mat, lane);
  }
  stage_tokens<T, C, KM>(a, b, xs, hb, 4 * HPP * C::HSZ, s_tab, s_coef, threadIdx.x, 384, true);
  if (KM == KM_RELATIVE)
    for (int q = threadIdx.x; q < C::H * C::TABLD; q += 384) s_dtab[q] = 0.f;
  for (int q = threadIdx.x; q < C::H * (C::MAXDEG + 1); q += 384) s_dcoef[q] = 0.f;
  for (int q = threadIdx.x; q < 2 * C::H * (HD / 2); q += 384) s_dfreq[q] = 0.f;
  __syncthreads();

  constexpr int CHN = CH<T>::n;
  const T* dog = reinterpret_cast<const T*>(a.dout) + (size_t)b * N * D;
  T* dq = reinterpret_cast<T*>(a.out) + (size_t)b * N * 3 * D;
  const bool mixed = (KM == KM_ROPE) && a.mode == PE_ROPE_MIXED;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};

  for (int h0 = 0; h0 < C::H; h0 += HPP) {
    {
      const int hh = wave / 3, mat = wave % 3, h = h0 + hh;
      if (hh < HPP && h < C::H) project_head<T, C, KM>(a, wf, xs, hb + (mat * HPP + hh) * C::HSZ, h, mat, lane);
      if (hh < HPP && h + HPP < C::H) load_w<T, C>(a, wf, h + HPP, mat, lane);
    }
    // stage dO of the pass's heads (rows >= N stay zero from the initial clear)
    for (int q = threadIdx.x; q < HPP * N * (HD / CHN); q += 384) {
      const int hh = q / (N * (HD / CHN)), rem = q % (N * (HD / CHN));
      const int row = rem / (HD / CHN), cc = rem % (HD / CHN);
      if (h0 + hh < C::H)
        *reinterpret_cast<Chunk16*>(hb + (3 * HPP + hh) * C::HSZ + row * C::LDH + cc * CHN) =
            *reinterpret_cast<const Chunk16*>(dog + (size_t)row * D + (h0 + hh) * HD + cc * CHN);
    }
    __syncthreads();

    // ---- step 1: (head, query tile) jobs on the swapped tiles: stats, dS^T, dQ ------------
    for (int job = wave; job < HPP * MT; job += 6) {
      const int hh = job / MT, it = job % MT, h = h0 + hh;
      if (h >= C::H) continue;
      const T* qh = hb + (0 * HPP + hh) * C::HSZ;
      const T* kh = hb + (1 * HPP + hh) * C::HSZ;
      const T* vh = hb + (2 * HPP + hh) * C::HSZ;
      const T* doh = hb + (3 * HPP + hh) * C::HSZ;
      Frag<T> bq[C::HC], bdo[C::HC];
#pragma unroll
      for (int cs = 0; cs < C::HC; ++cs) {
        bq[cs] = ld_frag(qh + (16 * it + c) * C::LDH + 32 * cs + 8 * g);
        bdo[cs] = ld_frag(doh + (16 * it + c) * C::LDH + 32 * cs + 8 * g);
      }
      f32x4 s[MT], dp[MT];
      const int i = 16 * it + c;
      const float m = logits_T<T, C, KM>(a, kh, bq, s_tab, s_coef, h, it, lane, s);
      const T* vrow = vh + c * C::LDH + 8 * g;
#pragma unroll
      for (int jt = 0; jt < MT; ++jt) {
        dp[jt] = z4;
#pragma unroll
        for (int cs = 0; cs < C::HC; ++cs) mma(ld_frag(vrow + 16 * jt * C::LDH + 32 * cs), bdo[cs], dp[jt]);
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
        s_stat[(hh * 2 + 0) * C::NP + i] = m + __builtin_amdgcn_logf(l);  // v_log_f32 = log2
        s_stat[(hh * 2 + 1) * C::NP + i] = dl;
      }
      // dS^T (in place of dp) and the bias-parameter gradients
      float cacc[C::MAXDEG + 1];
#pragma unroll
      for (int k = 0; k <= C::MAXDEG; ++k) cacc[k] = 0.f;
      const bool qvalid = (it < MT - 1) || (i < N);
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
      if (KM == KM_RELATIVE) {   // dtab[i - j + N - 1] += dS[i][j] (invalid entries are zero), one diagonal per lane
#pragma unroll
        for (int jt = 0; jt < MT; ++jt) {
          float d0, d1;
          tile_diag_sums(dp[jt], lane, d0, d1);
          const int idx0 = 16 * (it - jt) + c + N - 1;   // column - row == c ; d1: c - 16
          if (g == 0) {
            if (idx0 >= 0 && idx0 <= 2 * N - 2) atomicAdd(&s_dtab[h * C::TABLD + idx0], d0);
            if (c >= 1 && idx0 - 16 >= 0 && idx0 - 16 <= 2 * N - 2) atomicAdd(&s_dtab[h * C::TABLD + idx0 - 16], d1);
          }
        }
      }
      if (KM == KM_POLY) {
#pragma unroll
        for (int k = 0; k <= C::MAXDEG; ++k) {
          if (k <= a.degree) {  // wave-uniform
            const float t = wave_sum(cacc[k]);
            if (lane == 0) atomicAdd(&s_dcoef[(a.coeff_per_head ? h : 0) * (C::MAXDEG + 1) + k], t);
          }
        }
      }
      // dQrot^T[d][i] / scale = sum_j K^T[d][j] dS^T[j][i]
      f32x4 dqa[C::NT];
#pragma unroll
      for (int dt = 0; dt < C::NT; ++dt) dqa[dt] = z4;
#pragma unroll
      for (int sc = 0; sc < C::SC; ++sc) {
        const Frag<T> bs = acc_to_frag<T>(dp[2 * sc], (2 * sc + 1 < MT) ? dp[(2 * sc + 1 < MT) ? 2 * sc + 1 : 0] : z4);
#pragma unroll
        for (int dt = 0; dt < C::NT; ++dt)
          mma(ld_frag_tr(kh, C::LDH, 32 * sc + 4 * g, 32 * sc + 16 + 4 * g, 16 * dt), bs, dqa[dt]);
      }
      // inverse rotation (+ RoPE-mixed phase gradient), undo the folded scale, store the q part
      if (mixed) {   // (uniform branch: the row reductions inside need every lane)
        // dL/dphase = (dq~2 q~1 - dq~1 q~2) with q~ = scale*log2e*rot(q) held in LDS and
        // dqa = dL/d(rot q)/scale: the scale cancels, log2e does not -> ln2
        const bool tok_ok = i >= 1 && i < N;
        const int il = min(i, C::NP - 1);
#pragma unroll
        for (int nt = 0; nt < C::NT / 2; ++nt) {
          const f32x4 q1 = ld4(qh + il * C::LDH + 16 * nt + 4 * g);
          const f32x4 q2 = ld4(qh + il * C::LDH + 16 * (nt + C::NT / 2) + 4 * g);
          f32x4 dph;
#pragma unroll
          for (int r = 0; r < 4; ++r) dph[r] = dqa[nt + C::NT / 2][r] * q1[r] - dqa[nt][r] * q2[r];
          mixed_freq_grad_tile(s_dfreq, dph, i, tok_ok, 16 * it, h, C::H, P, a.grid, HD / 2, 16 * nt + 4 * g, LN2, lane);
        }
      }
      if (KM == KM_ROPE && i >= 1 && i < N) {
        const size_t hoff = mixed ? (size_t)h * P * (HD / 2) : 0;
#pragma unroll
        for (int nt = 0; nt < C::NT / 2; ++nt) {
          const size_t o = hoff + (size_t)(i - 1) * (HD / 2) + 16 * nt + 4 * g;
          const f32x4 cs = *reinterpret_cast<const f32x4*>(a.cos + o);
          const f32x4 sn = *reinterpret_cast<const f32x4*>(a.sin + o);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float d1 = dqa[nt][r], d2 = dqa[nt + C::NT / 2][r];
            dqa[nt][r] = d1 * cs[r] + d2 * sn[r];
            dqa[nt + C::NT / 2][r] = -d1 * sn[r] + d2 * cs[r];
          }
        }
      }
#pragma unroll
      for (int dt = 0; dt < C::NT; ++dt)
        st4(s_dq + (0 * C::NP + i) * SLD + hh * HD + 16 * dt + 4 * g, dqa[dt][0] * a.scale, dqa[dt][1] * a.scale,
            dqa[dt][2] * a.scale, dqa[dt][3] * a.scale);
    }
    __syncthreads();

    // ---- step 2: (head, key tile) jobs on the plain tiles: dV, dK ---------------------------
    for (int job = wave; job < HPP * MT; job += 6) {
      const int hh = job / MT, jt = job % MT, h = h0 + hh;
      if (h >= C::H) continue;
      const T* qh = hb + (0 * HPP + hh) * C::HSZ;
      const T* kh = hb + (1 * HPP + hh) * C::HSZ;
      const T* vh = hb + (2 * HPP + hh) * C::HSZ;
      const T* doh = hb + (3 * HPP + hh) * C::HSZ;
      Frag<T> bk[C::HC], bv[C::HC];
#pragma unroll
      for (int cs = 0; cs < C::HC; ++cs) {
        bk[cs] = ld_frag(kh + (16 * jt + c) * C::LDH + 32 * cs + 8 * g);
        bv[cs] = ld_frag(vh + (16 * jt + c) * C::LDH + 32 * cs + 8 * g);
      }
      const int j = 16 * jt + c;
      const bool kvalid = (jt < MT - 1) || (j < N);
      f32x4 p[MT], ds[MT];
      const T* qrow = qh + c * C::LDH + 8 * g;
      const T* dorow = doh + c * C::LDH + 8 * g;
#pragma unroll
      for (int it = 0; it < MT; ++it) {
        p[it] = z4;
        ds[it] = z4;
#pragma unroll
        for (int cs = 0; cs < C::HC; ++cs) {
          mma(ld_frag(qrow + 16 * it * C::LDH + 32 * cs), bk[cs], p[it]);
          mma(ld_frag(dorow + 16 * it * C::LDH + 32 * cs), bv[cs], ds[it]);
        }
        const f32x4 lse = *reinterpret_cast<const f32x4*>(&s_stat[(hh * 2 + 0) * C::NP + 16 * it + 4 * g]);
        const f32x4 dl = *reinterpret_cast<const f32x4*>(&s_stat[(hh * 2 + 1) * C::NP + 16 * it + 4 * g]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * it + 4 * g + r;
          float sv = p[it][r];
          if (KM == KM_RELATIVE || KM == KM_POLY) sv += pe_bias2<C, KM>(a, s_tab, s_coef, h, i, j, N);
          const bool valid = kvalid && ((it < MT - 1) || (i < N));
          const float pv = valid ? __builtin_amdgcn_exp2f(sv - lse[r]) : 0.f;
          p[it][r] = pv;
          ds[it][r] = pv * (ds[it][r] - dl[r]);
        }
      }
      f32x4 dva[C::NT], dka[C::NT];
#pragma unroll
      for (int dt = 0; dt < C::NT; ++dt) { dva[dt] = z4; dka[dt] = z4; }
#pragma unroll
      for (int sc = 0; sc < C::SC; ++sc) {
        const bool two = (2 * sc + 1 < MT);
        const Frag<T> bp = acc_to_frag<T>(p[2 * sc], two ? p[two ? 2 * sc + 1 : 0] : z4);
        const Frag<T> bs = acc_to_frag<T>(ds[2 * sc], two ? ds[two ? 2 * sc + 1 : 0] : z4);
#pragma unroll
        for (int dt = 0; dt < C::NT; ++dt) {
          mma(ld_frag_tr(doh, C::LDH, 32 * sc + 4 * g, 32 * sc + 16 + 4 * g, 16 * dt), bp, dva[dt]);
          mma(ld_frag_tr(qh, C::LDH, 32 * sc + 4 * g, 32 * sc + 16 + 4 * g, 16 * dt), bs, dka[dt]);
        }
      }
      // dK_rot = dS^T q~ / log2e  (q~ carries the folded scale and log2e)
#pragma unroll
      for (int dt = 0; dt < C::NT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dka[dt][r] *= LN2;
      if (mixed) {   // (uniform branch; see step 1)
        const bool tok_ok = j >= 1 && j < N;
        const int jl = min(j, C::NP - 1);
#pragma unroll
        for (int nt = 0; nt < C::NT / 2; ++nt) {
          const f32x4 k1 = ld4(kh + jl * C::LDH + 16 * nt + 4 * g);
          const f32x4 k2 = ld4(kh + jl * C::LDH + 16 * (nt + C::NT / 2) + 4 * g);
          f32x4 dph;
#pragma unroll
          for (int r = 0; r < 4; ++r) dph[r] = dka[nt + C::NT / 2][r] * k1[r] - dka[nt][r] * k2[r];
          mixed_freq_grad_tile(s_dfreq, dph, j, tok_ok, 16 * jt, h, C::H, P, a.grid, HD / 2, 16 * nt + 4 * g, 1.0f, lane);
        }
      }
      if (KM == KM_ROPE && j >= 1 && j < N) {
        const size_t hoff = mixed ? (size_t)h * P * (HD / 2) : 0;
#pragma unroll
        for (int nt = 0; nt < C::NT / 2; ++nt) {
          const size_t o = hoff + (size_t)(j - 1) * (HD / 2) + 16 * nt + 4 * g;
          const f32x4 cs = *reinterpret_cast<const f32x4*>(a.cos + o);
          const f32x4 sn = *reinterpret_cast<const f32x4*>(a.sin + o);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float d1 = dka[nt][r], d2 = dka[nt + C::NT / 2][r];
            dka[nt][r] = d1 * cs[r] + d2 * sn[r];
            dka[nt + C::NT / 2][r] = -d1 * sn[r] + d2 * cs[r];
          }
        }
      }
#pragma unroll
      for (int dt = 0; dt < C::NT; ++dt) {
        st4(s_dq + (1 * C::NP + j) * SLD + hh * HD + 16 * dt + 4 * g, dka[dt][0], dka[dt][1], dka[dt][2], dka[dt][3]);
        st4(s_dq + (2 * C::NP + j) * SLD + hh * HD + 16 * dt + 4 * g, dva[dt][0], dva[dt][1], dva[dt][2], dva[dt][3]);
      }
    }
    __syncthreads();
    {  // coalesced flush: per token row and matrix, nh*HD contiguous elements
      constexpr int CPH = HD / CHN;
      const int nh = min(HPP, C::H - h0);
      for (int q = threadIdx.x; q < 3 * N * nh * CPH; q += 384) {
        const int mat = q / (N * nh * CPH), rem = q % (N * nh * CPH);
        const int row = rem / (nh * CPH), cc = rem % (nh * CPH);
        *reinterpret_cast<Chunk16*>(dq + (size_t)row * 3 * D + mat * D + h0 * HD + cc * CHN) =
            *reinterpret_cast<const Chunk16*>(s_dq + (mat * C::NP + row) * SLD + cc * CHN);
      }
    }
    // (the next pass writes s_dq only after its projection barrier: no extra barrier needed)
  }

  // ---- flush this image's positional-parameter gradients ----------------------------------
  if (KM == KM_RELATIVE) {
    for (int q = threadIdx.x; q < C::H * (2 * N - 1); q += 384) {
      const int h = q / (2 * N - 1), i = q % (2 * N - 1);
      atomicAdd(a.dtable + q, s_dtab[h * C::TABLD + i]);
    }
  } else if (KM == KM_POLY) {
    const int nh = a.coeff_per_head ? C::H : 1;
    for (int q = threadIdx.x; q < nh * (a.degree + 1); q += 384) {
      const int h = q / (a.degree + 1), k = q % (a.degree + 1);
      atomicAdd(a.dcoeff + q, s_dcoef[h * (C::MAXDEG + 1) + k]);
    }
  } else if (mixed) {
    for (int q = threadIdx.x; q < 2 * C::H * (HD / 2); q += 384) atomicAdd(a.dfreqs + q, s_dfreq[q]);
  }
}

// dst block (h, mat, nt, ks), lane l = 16g + c, element e  <-  W[mat*D + h*HD + 16nt + c][32ks + 8g + e]
template <typename T>
__global__ void pack_qkv_kernel(const float* __restrict__ w, T* __restrict__ dst, int D, int HD) {
  const int NT = HD / 16, KS = D / 32, H = D / HD;
  const long long total = (long long)3 * D * D;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int e = (int)(idx & 7), l = (int)((idx >> 3) & 63);
    long long blk = idx >> 9;
    const int ks = (int)(blk % KS); blk /= KS;
    const int nt = (int)(blk % NT); blk /= NT;
    const int mat = (int)(blk % 3);
    const int h = (int)(blk / 3);
    if (h >= H) continue;
    const int c = l & 15, g = l >> 4;
    dst[idx] = from_f32<T>(w[(size_t)(mat * D + h * HD + 16 * nt + c) * D + 32 * ks + 8 * g + e]);
  }
}

}  // namespace vitpe

using namespace vitpe;

extern "C" int vitpe_pack_qkv_weights(int dtype, const float* wqkv, void* packed, int D, int HD, hipStream_t stream) {
  VITPE_REQUIRE(wqkv && packed && D > 0 && HD > 0 && D % HD == 0 && HD % 16 == 0 && D % 32 == 0);
  VITPE_REQUIRE(dtype == 0 || dtype == 1);
  const long long total = (long long)3 * D * D;
  const unsigned blocks = (unsigned)min((total + 255) / 256, (long long)2048);
  if (dtype == 1) hipLaunchKernelGGL(pack_qkv_kernel<bf16>, dim3(blocks), dim3(256), 0, stream, wqkv, (bf16*)packed, D, HD);
  else hipLaunchKernelGGL(pack_qkv_kernel<float>, dim3(blocks), dim3(256), 0, stream, wqkv, (float*)packed, D, HD);
  VITPE_CHECK_LAUNCH();
}

template <typename T, int HD, int D, int MT, int HPP, int KM, int NTOK>
static int launch_attn3(bool bwd, const AttnArgs& a, hipStream_t s) {
  constexpr bool REG_BWD = sizeof(T) == 2 && D / HD <= 6;   // every bf16 geometry vitpe_fused_attention_supported admits
  if constexpr (REG_BWD) {
    if (bwd) {   // register-resident backward: one wave per (image, head), two images per workgroup
      const dim3 grid((a.B + 1) / 2), block(64 * (D / HD) * 2);
      const bool ln = a.ln_gamma != nullptr;
      if constexpr (KM == KM_ROPE) {
        if (a.mode == PE_ROPE_MIXED) {
          if (ln) hipLaunchKernelGGL((attn_bwd_reg_kernel<HD, D, MT, KM, NTOK, 2, true, true>), grid, block, 0, s, a);
          else hipLaunchKernelGGL((attn_bwd_reg_kernel<HD, D, MT, KM, NTOK, 2, false, true>), grid, block, 0, s, a);
          VITPE_CHECK_LAUNCH();
        }
      }
      if constexpr (KM == KM_POLY) {
        if (a.degree <= 3) {   // the reference's default degree: four accumulators instead of eight
          if (ln) hipLaunchKernelGGL((attn_bwd_reg_kernel<HD, D, MT, KM, NTOK, 2, true, false, 3>), grid, block, 0, s, a);
          else hipLaunchKernelGGL((attn_bwd_reg_kernel<HD, D, MT, KM, NTOK, 2, false, false, 3>), grid, block, 0, s, a);
          VITPE_CHECK_LAUNCH();
        }
      }
      if (ln) hipLaunchKernelGGL((attn_bwd_reg_kernel<HD, D, MT, KM, NTOK, 2, true, false>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((attn_bwd_reg_kernel<HD, D, MT, KM, NTOK, 2, false, false>), grid, block, 0, s, a);
      VITPE_CHECK_LAUNCH();
    }
  }
  if (bwd) {   // fp32 (the parity path): the LDS-tile backward; not instantiated for bf16
    if constexpr (!REG_BWD) hipLaunchKernelGGL((attn_bwd_kernel<T, HD, D, MT, HPP, KM, NTOK>), dim3(a.B), dim3(384), 0, s, a);
  } else {  // one wave per (image, head); bf16: two images per workgroup (see attn_fwd_kernel)
    constexpr int IPW = (sizeof(T) == 2 && D / HD <= 6) ? 2 : 1;
    const dim3 grid((a.B + IPW - 1) / IPW), block(64 * (D / HD) * IPW);
    if (a.ln_gamma != nullptr) hipLaunchKernelGGL((attn_fwd_kernel<T, HD, D, MT, KM, NTOK, IPW, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((attn_fwd_kernel<T, HD, D, MT, KM, NTOK, IPW, false>), grid, block, 0, s, a);
  }
  VITPE_CHECK_LAUNCH();
}

template <typename T, int HD, int D, int MT, int HPP, int NTOK>
static int launch_attn2(bool bwd, const AttnArgs& a, hipStream_t s) {
  switch (a.mode) {
    case PE_RELATIVE: return launch_attn3<T, HD, D, MT, HPP, KM_RELATIVE, NTOK>(bwd, a, s);
    case PE_POLY: return launch_attn3<T, HD, D, MT, HPP, KM_POLY, NTOK>(bwd, a, s);
    case PE_ROPE_AXIAL:
    case PE_ROPE_MIXED: return launch_attn3<T, HD, D, MT, HPP, KM_ROPE, NTOK>(bwd, a, s);
    default: return launch_attn3<T, HD, D, MT, HPP, KM_PLAIN, NTOK>(bwd, a, s);
  }
}

template <typename T, int HD, int D, int MT, int HPP>
static int launch_attn(bool bwd, const AttnArgs& a, hipStream_t s) {
  // N = 65 (32x32 images, patch 4) is the benchmark geometry: compile-time token count
  if (a.N == 65) return launch_attn2<T, HD, D, MT, HPP, 65>(bwd, a, s);
  return launch_attn2<T, HD, D, MT, HPP, 0>(bwd, a, s);
}

static int dispatch_attn(bool bwd, int dtype, int D, int HD, const AttnArgs& a, hipStream_t s) {
  const int MT = (a.N + 15) / 16;
  if (HD != 32 || MT != 5) return (int)hipErrorNotSupported;
  if (dtype == 1) {
    if (D == 192) return launch_attn<bf16, 32, 192, 5, 2>(bwd, a, s);
    if (D == 96) return launch_attn<bf16, 32, 96, 5, 2>(bwd, a, s);
  } else if (dtype == 0) {
    if (D == 192) return launch_attn<float, 32, 192, 5, 1>(bwd, a, s);
    if (D == 96) return launch_attn<float, 32, 96, 5, 1>(bwd, a, s);
  }
  return (int)hipErrorNotSupported;
}

extern "C" int vitpe_fused_attention_supported(int dtype, int N, int D, int HD) {
  const int MT = (N + 15) / 16;
  return (dtype == 0 || dtype == 1) && HD == 32 && MT == 5 && (D == 192 || D == 96);
}

// The four product entry points share one body each way: gamma == NULL is the plain variant (x already layer-normed).
static int fused_fwd(int dtype, const void* x, const float* gamma, const float* beta, const float* mean,
                     const float* rstd, void* xn_out, const void* wqkv, void* out, int B, int N, int D, int HD,
                     const PeArgs& pe, hipStream_t stream) {
  VITPE_REQUIRE(x && wqkv && out && B >= 0 && N >= 2);
  VITPE_REQUIRE(pe_ok(pe, N, 0, 0));
  if (B == 0) return 0;
  AttnArgs a = attn_args(pe, B, N, 0, HD);
  a.xn = x; a.wqkv = wqkv; a.out = out;
  a.ln_gamma = gamma; a.ln_beta = beta; a.ln_mean = mean; a.ln_rstd = rstd; a.xn_out = xn_out;
  return dispatch_attn(false, dtype, D, HD, a, stream);
}

static int fused_bwd(int dtype, const void* x, const float* gamma, const float* beta, const float* mean,
                     const float* rstd, const void* wqkv, const void* dout, void* dqkv, int B, int N, int D, int HD,
                     const PeArgs& pe, float* dtable, float* dcoeff, float* dfreqs, hipStream_t stream) {
  VITPE_REQUIRE(x && wqkv && dout && dqkv && B >= 0 && N >= 2);
  VITPE_REQUIRE(pe_ok(pe, N, 0, 0));
  VITPE_REQUIRE(pe_grads_ok(pe.mode, dtable, dcoeff, dfreqs));
  if (B == 0) return 0;
  AttnArgs a = attn_args(pe, B, N, 0, HD);
  a.xn = x; a.wqkv = wqkv; a.out = dqkv; a.dout = dout;
  a.dtable = dtable; a.dcoeff = dcoeff; a.dfreqs = dfreqs;
  a.ln_gamma = gamma; a.ln_beta = beta; a.ln_mean = mean; a.ln_rstd = rstd;
  return dispatch_attn(true, dtype, D, HD, a, stream);
}

extern "C" int vitpe_fused_attention_fwd(int dtype, const void* xn, const void* wqkv, void* out, int B, int N,
                                         int D, int HD, int mode, const float* cos, const float* sin,
                                         const float* table, const float* coeff, int grid, int degree,
                                         int coeff_per_head, hipStream_t stream) {
  return fused_fwd(dtype, xn, nullptr, nullptr, nullptr, nullptr, nullptr, wqkv, out, B, N, D, HD,
                   {mode, cos, sin, table, coeff, grid, degree, coeff_per_head}, stream);
}

// Same as vitpe_fused_attention_fwd with the preceding LayerNorm fused into the token staging:
// x holds the RAW tokens, mean/rstd their row statistics (e.g. from vitpe_linear's stats output);
// xn_out (nullable) receives LayerNorm(x) for the backward pass.
extern "C" int vitpe_fused_attention_fwd_ln(int dtype, const void* x, const float* gamma, const float* beta,
                                            const float* mean, const float* rstd, void* xn_out, const void* wqkv,
                                            void* out, int B, int N, int D, int HD, int mode, const float* cos,
                                            const float* sin, const float* table, const float* coeff, int grid,
                                            int degree, int coeff_per_head, hipStream_t stream) {
  VITPE_REQUIRE(gamma && beta && mean && rstd);
  return fused_fwd(dtype, x, gamma, beta, mean, rstd, xn_out, wqkv, out, B, N, D, HD,
                   {mode, cos, sin, table, coeff, grid, degree, coeff_per_head}, stream);
}

extern "C" int vitpe_fused_attention_bwd(int dtype, const void* xn, const void* wqkv, const void* dout,
                                         void* dqkv, int B, int N, int D, int HD, int mode, const float* cos,
                                         const float* sin, const float* table, const float* coeff, int grid,
                                         int degree, int coeff_per_head, float* dtable, float* dcoeff,
                                         float* dfreqs, hipStream_t stream) {
  return fused_bwd(dtype, xn, nullptr, nullptr, nullptr, nullptr, wqkv, dout, dqkv, B, N, D, HD,
                   {mode, cos, sin, table, coeff, grid, degree, coeff_per_head}, dtable, dcoeff, dfreqs, stream);
}

// vitpe_fused_attention_bwd with the LayerNorm recomputed while staging (x = RAW tokens + their row statistics): the
// normalised tokens are a pure function of tensors the forward keeps anyway, so it does not store them.
extern "C" int vitpe_fused_attention_bwd_ln(int dtype, const void* x, const float* gamma, const float* beta,
                                            const float* mean, const float* rstd, const void* wqkv, const void* dout,
                                            void* dqkv, int B, int N, int D, int HD, int mode, const float* cos,
                                            const float* sin, const float* table, const float* coeff, int grid,
                                            int degree, int coeff_per_head, float* dtable, float* dcoeff,
                                            float* dfreqs, hipStream_t stream) {
  VITPE_REQUIRE(gamma && beta && mean && rstd);
  return fused_bwd(dtype, x, gamma, beta, mean, rstd, wqkv, dout, dqkv, B, N, D, HD,
                   {mode, cos, sin, table, coeff, grid, degree, coeff_per_head}, dtable, dcoeff, dfreqs, stream);
}

// debug: bf16 d=192 rope-axial forward with phase stamps: census[(wg * 16 + wave) * 8 + slot], slots 0 start,
// 1 tokens staged, 2 barrier passed, 3 v projected, 4 k, 5 q, 6 end (tools/census_attn.py)
extern "C" int vitpe_debug_attn_census(const void* xn, const void* wqkv, void* out, const float* cos, const float* sin,
                                       int B, unsigned long long* census, hipStream_t stream) {
  VITPE_REQUIRE(xn && wqkv && out && cos && sin && census && B > 0);
  AttnArgs a = attn_args({PE_ROPE_AXIAL, cos, sin, nullptr, nullptr, 8, 0, 0}, B, 65, 0, 32);
  a.xn = xn; a.wqkv = wqkv; a.out = out; a.census = census;
  hipLaunchKernelGGL((attn_fwd_kernel<bf16, 32, 192, 5, KM_ROPE, 65, 2, false, true>), dim3((B + 1) / 2), dim3(768), 0, stream, a);
  VITPE_CHECK_LAUNCH();
}
