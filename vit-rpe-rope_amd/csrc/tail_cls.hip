// Block tail on the CLASS-TOKEN rows only: the top block of a class-token-pooled ViT (reference models/vit.py: the head reads
// x[:, 0] alone) needs its tail -- attention projection + residual + LayerNorm2 + MLP + residual (vit.py:91,116-118,122-124)
// -- and that tail's backward on one row per image.  Everything outside the class rows is neither read nor written: the
// kernels work in place on the full-layout [batch x tokens, .] buffers with a ROW STEP (logical row r lives at row
// r * row_step of every operand and every statistic), so no gathered copy exists that a consumer would have to know about.
//
// Same arithmetic and rounding points as tail2.hip (block_tail2_fwd_kernel with SAVE / block_tail2_bwd_kernel<false>), same
// fragment-packed weight copies, but the opposite mapping.  There one wave carries a 16-token tile through the whole chain
// and a launch is one such chain long however few tiles it has; batch = 512 class rows are 32 tiles, which would occupy
// 32 waves of the chip for the full ~55 us.  Here a WORKGROUP of 12 waves takes a 16-row tile and splits the COLUMNS:
//   proj / fc2 / the data gradients into the 192-wide stream: wave w computes output tile w (16 of 192 features),
//   fc1 / the gradient of the hidden layer: wave w computes hidden tiles w, w + 12, ... (HID / 16 tiles),
// all as transposed products (A = weight fragment, B = token fragment: the accumulator holds [feature 4g + r][token c], so a
// lane owns 4 consecutive features of its token = one 8-B store).  The 16 x 192 and 16 x HID intermediates cross the waves
// through LDS (two barriers forward, two backward); LayerNorm's row statistics are computed by every wave on the full tile
// (48 values per lane, the layout and summation order of tail2.hip).
//
// Weight fragments are read straight from global memory (0.66 MB per direction, read once by every workgroup), and a
// launch is 32 workgroups on an otherwise idle chip: what it costs is the chain of waits for those loads.  No weight
// fragment, bias, LayerNorm parameter or saved row depends on an activation, so none is loaded where it is used:
//   * everything known at entry goes out at entry, in the order of its use (the operands of the first product, the small
//     vectors, the wave's first hidden tile, the first batch of the second k loop behind it); gamma / beta are loaded once
//     per workgroup and staged in LDS under the first product;
//   * the hidden tiles (six fragments each) are loaded one tile ahead; the k loops over the hidden layer run in batches of
//     eight fragments, two register sets alternating, MFMA k waiting for fragment k alone (counted waits: the counter of
//     outstanding memory operations retires in issue order) -- k ascending into one accumulator, as a plain loop would;
//   * stores stay out of the way of those waits: the forward holds gelu'(u) back by one tile and writes h from LDS at the
//     end, the backward writes du from LDS at the end;
//   * the backward's LayerNorm phase keeps 2 + 4 registers per tile and forms xhat and gy twice instead of carrying 96
//     products over the row sums (it used to spill 35 registers; scratch accesses queue behind every load in flight), reads
//     gamma from LDS, takes the residual rows and Wp^T's fragments from loads issued before its barrier, and sends dgamma /
//     dbeta as ONE atomic instruction per wave (they execute at the memory side, all workgroups into the same 1.5 KB).
// Every output is bit-identical to the plain-loop kernels this file held before (dgamma / dbeta: fp32 atomics, order free).
// Both kernels: 0 spilled registers, 3 waves per SIMD (tools/regs.sh tail_cls.hip).  Measured: DESIGN.md 4, "Top block on
// the class-token rows"; stand-alone: tools/kbench_tail_cls.py.  What is left there: every wave repeats the LayerNorm
// arithmetic of the whole tile (about half the backward's instructions).
// Rows past the batch in the last tile are copies of the last row (clamped index for loads and stores), masked out of the
// dgamma / dbeta sums.
#include "common.h"

namespace vitpe {

constexpr int TC_D = 192, TC_NT = 12, TC_KS = 6, TC_THREADS = 64 * TC_NT, TC_MAXHID = 1536;
constexpr int TC_XLD = TC_D + 8;      // bf16 elements per LDS row of a 16 x 192 tile
constexpr int TC_FLD = TC_D + 4;      // floats per LDS row of the fp32 16 x 192 tile (backward)
constexpr int TC_HPAD = 8;            // the 16 x HID tile: HID + 8 elements per row

struct TailClsFwdArgs {
  const bf16* a;  const bf16* xin;
  const bf16* wp; const float* bp; const float* gamma; const float* beta;
  const bf16* w1; const float* b1; const bf16* w2; const float* b2;
  bf16* xmid; float* mean2; float* rstd2;
  bf16* xn_out;          // nullable
  _Float16* gp_out;      // nullable together with h_out
  bf16* h_out;
  bf16* out;
  int B, HID, row_step;
  float eps2;
};

VITPE_DEV void tc_st4(bf16* p, const f32x4& v) { st4(p, v[0], v[1], v[2], v[3]); }

// the B fragment (acc_to_frag k order: t < 4 -> 4g + t, else 16 + 4g + t - 4) of a 32-wide chunk of a bf16 row
VITPE_DEV Frag<bf16> tc_phi_frag(const bf16* chunk_plus_4g) {
  const bf16x4 lo = *reinterpret_cast<const bf16x4*>(chunk_plus_4g), hi = *reinterpret_cast<const bf16x4*>(chunk_plus_4g + 16);
  Frag<bf16> f;
  f.v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return f;
}

// h = gelu(x), g = gelu'(x): tail2.hip's t2_gelu, instruction for instruction (the saved values must agree)
VITPE_DEV void tc_gelu(float x, float& h, float& g) {
  constexpr float C = 0.39894228040143267794f;
  const float ax = fabsf(x);
  const float T = __builtin_amdgcn_rcpf(fmaf(ax, 0.3275911f * 0.70710678118654752440f, 1.0f));
  float q = fmaf(T, 1.061405429f / (2.f * C), -1.453152027f / (2.f * C));
  q = fmaf(T, q, 1.421413741f / (2.f * C));
  q = fmaf(T, q, -0.284496736f / (2.f * C));
  q = fmaf(T, q, 0.254829592f / (2.f * C));
  const float E = __builtin_amdgcn_exp2f(fmaf(x * x, -0.72134752044448170368f, -1.32574806473615827f));
  const float H = (q * T) * E;
  h = fmaf(-ax, H, fmaxf(x, 0.f));
  const float r = fmaf(ax, E, -H);
  g = x >= 0.f ? 1.0f + r : -r;
}

// ---- weight streams -------------------------------------------------------------------------------------------------------
// No weight fragment depends on an activation, so none is loaded where it is used: a product's fragments are issued one
// batch ahead, in the order they are consumed (the counter of outstanding loads retires in order: MFMA k waits for
// fragment k alone while the rest of its batch and the whole next batch stay in flight).
constexpr int TC_KB = 8;              // fragments per batch of the k loops over the hidden layer (32 registers)

// the six fragments of one 16-feature tile of a kchunk-192 weight
VITPE_DEV void tc_ld_tile(Frag<bf16> (&f)[TC_KS], const bf16* wf) {
#pragma unroll
  for (int ks = 0; ks < TC_KS; ++ks) f[ks] = ld_frag(wf + ks * 512);
}

// fragments k0 .. k0 + 7 of the wave's k-major stream (kchunk-32 weight: TC_NT fragments per k); past the end the last
// one again (loaded, never used: only the last batch of a stream whose length is no multiple of 8 has such entries)
VITPE_DEV void tc_ld_batch(Frag<bf16> (&f)[TC_KB], const bf16* wf, int k0, int nk) {
#pragma unroll
  for (int j = 0; j < TC_KB; ++j) f[j] = ld_frag(wf + (size_t)min(k0 + j, nk - 1) * (TC_NT * 512));
}

VITPE_DEV void tc_mma_batch(const Frag<bf16> (&f)[TC_KB], const bf16* src, int k0, f32x4& acc) {
#pragma unroll
  for (int j = 0; j < TC_KB; ++j) mma(f[j], tc_phi_frag(src + 32 * (k0 + j)), acc);
}

// the last batch: nk - k0 in {2, 4, 6, 8} chunks (HID is a multiple of 64)
VITPE_DEV void tc_mma_tail(const Frag<bf16> (&f)[TC_KB], const bf16* src, int k0, int nk, f32x4& acc) {
#pragma unroll
  for (int j = 0; j < TC_KB; j += 2)
    if (k0 + j < nk) {
      mma(f[j], tc_phi_frag(src + 32 * (k0 + j)), acc);
      mma(f[j + 1], tc_phi_frag(src + 32 * (k0 + j + 1)), acc);
    }
}

// acc += sum over k < nk of W[k] phi(src + 32 k): k ascending into ONE accumulator (the summation order of a plain k loop).
// fa holds batch 0, issued by the caller long before; the two batch buffers alternate.
VITPE_DEV void tc_kloop(Frag<bf16> (&fa)[TC_KB], const bf16* wf, const bf16* src, int nk, f32x4& acc) {
  Frag<bf16> fb[TC_KB];
  int k0 = 0;
  // (the sched_barriers keep each batch's loads in front of the MFMAs they fly under; the pair loop is one basic block, so
  // that no wait is placed for a path the loop never takes)
  for (; k0 + 2 * TC_KB < nk; k0 += 2 * TC_KB) {
    tc_ld_batch(fb, wf, k0 + TC_KB, nk);
    __builtin_amdgcn_sched_barrier(0);
    tc_mma_batch(fa, src, k0, acc);
    tc_ld_batch(fa, wf, k0 + 2 * TC_KB, nk);
    __builtin_amdgcn_sched_barrier(0);
    tc_mma_batch(fb, src, k0 + TC_KB, acc);
  }
  if (k0 + TC_KB < nk) {
    tc_ld_batch(fb, wf, k0 + TC_KB, nk);
    __builtin_amdgcn_sched_barrier(0);
    tc_mma_batch(fa, src, k0, acc);
    tc_mma_tail(fb, src, k0 + TC_KB, nk, acc);
  } else {
    tc_mma_tail(fa, src, k0, nk, acc);
  }
}

__global__ __launch_bounds__(TC_THREADS) void tail_cls_fwd_kernel(TailClsFwdArgs a) {
  constexpr int D = TC_D, NT = TC_NT, KS = TC_KS;
  __shared__ __attribute__((aligned(16))) bf16 sX[16 * TC_XLD];
  __shared__ __attribute__((aligned(16))) bf16 sH[16 * (TC_MAXHID + TC_HPAD)];
  __shared__ __attribute__((aligned(16))) float sGB[2 * TC_D];       // gamma, beta: loaded once per workgroup
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int HID = a.HID, HLD = HID + TC_HPAD, ntiles = HID / 16, nk = HID / 32;
  const size_t row = (size_t)min(16 * (int)blockIdx.x + c, a.B - 1) * a.row_step;   // rows past B: copies of row B - 1 (such lanes store
  // the SAME values to the SAME addresses as the lane that owns row B - 1: a benign race, as in tail2.hip)
  const int f0 = 16 * wave + 4 * g;             // this lane's 4 features of the wave's 192-wide output tile

  // ---- everything known at entry, in the order of its use: proj operands, the small vectors, the wave's first fc1 tile ------
  Frag<bf16> fp[KS], fa[KS];
  {
    const bf16* ar = a.a + row * D + 8 * g;
    const bf16* wf = a.wp + (size_t)wave * KS * 512 + lane * 8;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) { fp[ks] = ld_frag(wf + ks * 512); fa[ks] = ld_frag(ar + 32 * ks); }
  }
  const bf16x4 xr = *reinterpret_cast<const bf16x4*>(a.xin + row * D + f0);
  const f32x4 bpv = *reinterpret_cast<const f32x4*>(a.bp + f0);
  // threads 0 .. 47 carry gamma, 48 .. 95 beta (the others load beta's last piece and drop it)
  const f32x4 gbv = *reinterpret_cast<const f32x4*>(tid < D / 4 ? a.gamma + 4 * tid : a.beta + 4 * (min(tid, D / 2 - 1) - D / 4));
  const bf16* const w1f = a.w1 + lane * 8;
  const int lo = 4 * g;                          // the lane's offset inside a 16-feature hidden tile
  Frag<bf16> wa[KS];
  f32x4 ba;
  {
    const int nt0 = min(wave, ntiles - 1);       // (fewer hidden tiles than waves: loaded, not used)
    tc_ld_tile(wa, w1f + (size_t)nt0 * KS * 512);
    ba = *reinterpret_cast<const f32x4*>(a.b1 + 16 * nt0 + lo);
  }
  __builtin_amdgcn_sched_barrier(0);             // all of it in flight before the first MFMA

  // ---- x_mid = x_in + a Wp^T + bp: output tile `wave` -----------------------------------------------------------------------
  {
    f32x4 acc = bpv;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) mma(fp[ks], fa[ks], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = to_f32(from_f32<bf16>(acc[r] + (float)xr[r]));   // values as stored
    tc_st4(a.xmid + row * D + f0, acc);
    tc_st4(sX + c * TC_XLD + f0, acc);
    if (tid < D / 2) *reinterpret_cast<f32x4*>(sGB + 4 * tid) = gbv;
  }
  __syncthreads();

  // ---- LayerNorm2 on the whole tile, every wave (the layout and summation order of tail2.hip) ----------------------------
  Frag<bf16> bf[KS];
  {
    f32x4 xa[NT];
    float s1 = 0.f;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      xa[nt] = ld4(sX + c * TC_XLD + 16 * nt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) s1 += xa[nt][r];
    }
    const float invD = 1.0f / (float)D;
    const float mean = xgroup_sum(s1) * invD;
    float s2 = 0.f;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) { const float d = xa[nt][r] - mean; s2 += d * d; }
    const float rstd = 1.0f / sqrtf(xgroup_sum(s2) * invD + a.eps2);
    if (wave == 0 && g == 0) { a.mean2[row] = mean; a.rstd2[row] = rstd; }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int nt = 2 * ks; nt < 2 * ks + 2; ++nt) {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(sGB + 16 * nt + 4 * g);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(sGB + D + 16 * nt + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) xa[nt][r] = fmaf((xa[nt][r] - mean) * rstd, gv[r], bv[r]);
      }
      bf[ks] = acc_to_frag<bf16>(xa[2 * ks], xa[2 * ks + 1]);
      if (a.xn_out != nullptr && ks == wave) {      // waves 0 .. 5 write one 32-wide chunk of the normalised rows each
        bf16* xo = a.xn_out + row * D + 32 * ks + 4 * g;
        *reinterpret_cast<bf16x4*>(xo) = __builtin_shufflevector(bf[ks].v, bf[ks].v, 0, 1, 2, 3);
        *reinterpret_cast<bf16x4*>(xo + 16) = __builtin_shufflevector(bf[ks].v, bf[ks].v, 4, 5, 6, 7);
      }
      __builtin_amdgcn_sched_barrier(0);            // one chunk at a time: the fp32 values die as the fragment is formed
    }
  }

  // the first batch of fc2's stream goes out ahead of the whole fc1 loop (and of the barrier behind it)
  const bf16* const w2f = a.w2 + (size_t)wave * 512 + lane * 8;
  Frag<bf16> f2[TC_KB];
  tc_ld_batch(f2, w2f, 0, nk);
  const f32x4 b2v = *reinterpret_cast<const f32x4*>(a.b2 + f0);

  // ---- u = xn W1^T + b1; h = gelu(u), g' = gelu'(u): hidden tiles wave, wave + 12, ... -------------------------------------
  // One register set: tile t + 1's fragments and bias go out right behind tile t's MFMAs (which have read the registers
  // they land in) and fly under tile t's GELU.  Loads and stores share one in-order counter, and the stores here sit under
  // a branch (training only), so a store between a tile's loads and their use makes the compiler wait for the worse of
  // the two paths: tile t - 1's gelu'(u) -- the only store of the loop, held back by one tile -- is issued WITH the loads,
  // and h goes to memory from LDS at the end of the kernel.
  const bool save = a.gp_out != nullptr;
  const size_t hrow = row * HID + lo;
  if (wave < ntiles) {
    bf16* const shr = sH + c * HLD + lo;
    uint2 pk = {0u, 0u};
    for (int nt = wave; nt < ntiles; nt += NT) {
      f32x4 acc = ba;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) mma(wa[ks], bf[ks], acc);
      __builtin_amdgcn_sched_barrier(0);
      if (nt + NT < ntiles) {
        tc_ld_tile(wa, w1f + (size_t)(nt + NT) * KS * 512);
        ba = *reinterpret_cast<const f32x4*>(a.b1 + 16 * (nt + NT) + lo);
      }
      if (save && nt != wave) *reinterpret_cast<uint2*>(a.gp_out + hrow + 16 * (nt - NT)) = pk;
      __builtin_amdgcn_sched_barrier(0);
      f32x4 hh, gp;
#pragma unroll
      for (int r = 0; r < 4; ++r) { float hv, gv; tc_gelu(acc[r], hv, gv); hh[r] = hv; gp[r] = gv; }
      tc_st4(shr + 16 * nt, hh);
      // IEEE half, round toward zero: the conversion block_tail2_fwd_kernel uses (t2_store_pair_f16)
      pk = {__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(gp[0], gp[1])),
            __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(gp[2], gp[3]))};
    }
    if (save) *reinterpret_cast<uint2*>(a.gp_out + hrow + 16 * (wave + (ntiles - 1 - wave) / NT * NT)) = pk;
  }
  __syncthreads();
  // everything issued so far has landed (fc2's first batch long ago) or is a store of the loop above: drain here, so that
  // the k loop's waits count its own loads only
  __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0)

  // ---- out = x_mid + h W2^T + b2: output tile `wave`, k = the whole hidden layer from LDS -----------------------------------
  {
    f32x4 acc = b2v;
    tc_kloop(f2, w2f, sH + c * HLD + 4 * g, nk, acc);
    const f32x4 xm_own = ld4(sX + c * TC_XLD + f0);       // the lane's own x_mid values, as stored
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] += xm_own[r];
    tc_st4(a.out + row * D + f0, acc);
  }
  // h, as the lane wrote it to LDS
  if (save)
    for (int nt = wave; nt < ntiles; nt += NT)
      *reinterpret_cast<bf16x4*>(a.h_out + hrow + 16 * nt) = *reinterpret_cast<const bf16x4*>(sH + c * HLD + lo + 16 * nt);
}

struct TailClsBwdArgs {
  const bf16* dy; const _Float16* gp; const bf16* xmid; const float* mean2; const float* rstd2; const float* gamma;
  const bf16* w2t; const bf16* w1t; const bf16* wpt;
  bf16* du; bf16* dxmid; bf16* da;
  float* dgamma; float* dbeta;
  int B, HID, row_step;
};

// one hidden tile of the backward: dh = dy W2, du = dh * gelu'(u) to LDS (to memory from there at the end of the kernel:
// the loop's counted waits then count loads only)
VITPE_DEV void tc_dh_tile(const Frag<bf16> (&fw)[TC_KS], const Frag<bf16> (&bf)[TC_KS], uint2 gw, bf16* sdu) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < TC_KS; ++ks) mma(fw[ks], bf[ks], acc);
  f32x4 d;
  d[0] = acc[0] * (float)__builtin_bit_cast(_Float16, (unsigned short)(gw.x & 0xffffu));
  d[1] = acc[1] * (float)__builtin_bit_cast(_Float16, (unsigned short)(gw.x >> 16));
  d[2] = acc[2] * (float)__builtin_bit_cast(_Float16, (unsigned short)(gw.y & 0xffffu));
  d[3] = acc[3] * (float)__builtin_bit_cast(_Float16, (unsigned short)(gw.y >> 16));
  tc_st4(sdu, d);
}

__global__ __launch_bounds__(TC_THREADS) void tail_cls_bwd_kernel(TailClsBwdArgs a) {
  constexpr int D = TC_D, NT = TC_NT, KS = TC_KS;
  __shared__ __attribute__((aligned(16))) float sDx[16 * TC_FLD];
  __shared__ __attribute__((aligned(16))) bf16 sDu[16 * (TC_MAXHID + TC_HPAD)];
  __shared__ __attribute__((aligned(16))) float sG[TC_D];            // gamma: loaded once per workgroup
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int HID = a.HID, HLD = HID + TC_HPAD, ntiles = HID / 16, nk = HID / 32;
  const int lrow = 16 * (int)blockIdx.x + c;
  const size_t row = (size_t)min(lrow, a.B - 1) * a.row_step;   // (clamped lanes: identical stores to row B - 1, see the forward)
  const float valid = lrow < a.B ? 1.0f : 0.0f;
  const int f0 = 16 * wave + 4 * g;

  // ---- everything known at entry, in the order of its use: the dy rows, the
  // wave's first hidden tile with its gelu'(u), the row statistics, gamma, the lane's own x_mid piece (dgamma) ---------------
  const bf16* const dyr = a.dy + row * D + 4 * g;
  Frag<bf16> bf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) bf[ks] = tc_phi_frag(dyr + 32 * ks);
  const bf16* const w2f = a.w2t + lane * 8;
  const int lo = 4 * g;
  const size_t hrow = row * HID + lo;
  Frag<bf16> wa[KS], wb[KS];
  uint2 ga, gb;
  {
    const int nt0 = min(wave, ntiles - 1);       // (fewer hidden tiles than waves: loaded, not used)
    tc_ld_tile(wa, w2f + (size_t)nt0 * KS * 512);
    ga = *reinterpret_cast<const uint2*>(a.gp + hrow + 16 * nt0);
  }
  const float mean = a.mean2[row], rstd = a.rstd2[row];
  const f32x4 gmv = *reinterpret_cast<const f32x4*>(a.gamma + 4 * min(tid, D / 4 - 1));
  const bf16x4 xown = *reinterpret_cast<const bf16x4*>(a.xmid + row * D + f0);
  // the first batch of the dxn stream, ahead of the whole dh loop (and of the barrier behind it)
  const bf16* const w1f = a.w1t + (size_t)wave * 512 + lane * 8;
  Frag<bf16> f1[TC_KB];
  tc_ld_batch(f1, w1f, 0, nk);

  // ---- dh = dy W2; du = dh * gelu'(u): hidden tiles wave, wave + 12, ...; tile t + 1's fragments and gelu'(u) are loaded
  // under tile t (two register sets, alternating) ----------------------------------------------------------------------------
  if (wave < ntiles) {
    bf16* const sdr = sDu + c * HLD + lo;
    int nt = wave;
    for (; nt + 2 * NT < ntiles; nt += 2 * NT) {
      tc_ld_tile(wb, w2f + (size_t)(nt + NT) * KS * 512);
      gb = *reinterpret_cast<const uint2*>(a.gp + hrow + 16 * (nt + NT));
      __builtin_amdgcn_sched_barrier(0);
      tc_dh_tile(wa, bf, ga, sdr + 16 * nt);
      tc_ld_tile(wa, w2f + (size_t)(nt + 2 * NT) * KS * 512);
      ga = *reinterpret_cast<const uint2*>(a.gp + hrow + 16 * (nt + 2 * NT));
      __builtin_amdgcn_sched_barrier(0);
      tc_dh_tile(wb, bf, gb, sdr + 16 * (nt + NT));
    }
    if (nt + NT < ntiles) {
      tc_ld_tile(wb, w2f + (size_t)(nt + NT) * KS * 512);
      gb = *reinterpret_cast<const uint2*>(a.gp + hrow + 16 * (nt + NT));
      __builtin_amdgcn_sched_barrier(0);
      tc_dh_tile(wa, bf, ga, sdr + 16 * nt);
      tc_dh_tile(wb, bf, gb, sdr + 16 * (nt + NT));
    } else {
      tc_dh_tile(wa, bf, ga, sdr + 16 * nt);
    }
  }
  if (tid < D / 4) *reinterpret_cast<f32x4*>(sG + 4 * tid) = gmv;
  __syncthreads();

  // the x_mid rows of the LayerNorm phase go out under the dxn loop
  bf16x4 xmv[NT];
  {
    const bf16* xr = a.xmid + row * D + 4 * g;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) xmv[nt] = *reinterpret_cast<const bf16x4*>(xr + 16 * nt);
  }

  // ---- dxn = du W1: output tile `wave`, k = the whole hidden layer from LDS; the fp32 tile crosses the waves through LDS -------
  Frag<bf16> fwp[KS];
  bf16x4 rv[NT];
  {
    f32x4 dxo = {0.f, 0.f, 0.f, 0.f};
    tc_kloop(f1, w1f, sDu + c * HLD + 4 * g, nk, dxo);
    *reinterpret_cast<f32x4*>(sDx + c * TC_FLD + f0) = dxo;
    // the residual rows (dy again: L2) and Wp^T's fragments for the last product go out under the LayerNorm phase
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) rv[nt] = *reinterpret_cast<const bf16x4*>(dyr + 16 * nt);
    tc_ld_tile(fwp, a.wpt + (size_t)wave * KS * 512 + lane * 8);
    // dgamma / dbeta: wave w owns columns 16 w .. 16 w + 15, which are its own dxn tile.  Column sums over the tile's 16
    // tokens, then ONE atomic instruction per wave: lanes c = 0 .. 3 of every group carry its four dgamma columns, lanes
    // 4 .. 7 the dbeta columns (the adds execute at the memory side, every workgroup into the same 1.5 KB: their number is
    // what they cost -- eight instructions of four lanes each took four times as long)
    float sg[4], sb[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float xhat = ((float)xown[r] - mean) * rstd;
      const float dxn = dxo[r];
      sg[r] = group16_sum(dxn * xhat * valid);
      sb[r] = group16_sum(dxn * valid);
    }
    const int qc = c & 3;
    const float vg = qc == 0 ? sg[0] : qc == 1 ? sg[1] : qc == 2 ? sg[2] : sg[3];
    const float vb = qc == 0 ? sb[0] : qc == 1 ? sb[1] : qc == 2 ? sb[2] : sb[3];
    if (c < 8) atomicAdd((c < 4 ? a.dgamma : a.dbeta) + f0 + qc, c < 4 ? vg : vb);
  }
  __syncthreads();

  // ---- dx_mid = dy + LayerNorm2'(dxn) on the whole tile, every wave (t2_ln_backward's arithmetic); wave w stores tile w ------
  f32x4 acc[NT];
  {
    const float invD = 1.0f / (float)D;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = *reinterpret_cast<const f32x4*>(sDx + c * TC_FLD + 16 * nt + 4 * g);
    // four tiles at a time (the scheduler fences): each pass keeps its sums only, and the second pass forms xhat and gy
    // again from the 2 + 4 registers per tile that stay (carrying the 96 products of the first pass over the row sums is
    // what spilled here) -- the same instructions on the same operands, the same values
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const f32x4 gam = *reinterpret_cast<const f32x4*>(sG + 16 * nt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float xhat = ((float)xmv[nt][r] - mean) * rstd;
        const float gy = acc[nt][r] * gam[r];
        s1 += gy;
        s2 = fmaf(gy, xhat, s2);
      }
      if (nt % 4 == 3) __builtin_amdgcn_sched_barrier(0);
    }
    const float m1 = xgroup_sum(s1) * invD, m2 = xgroup_sum(s2) * invD;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { asm volatile("" : "+v"(acc[nt])); asm volatile("" : "+v"(xmv[nt])); }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const f32x4 gam = *reinterpret_cast<const f32x4*>(sG + 16 * nt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float xhat = ((float)xmv[nt][r] - mean) * rstd;
        const float gy = acc[nt][r] * gam[r];
        acc[nt][r] = to_f32(from_f32<bf16>(fmaf(rstd, gy - m1 - xhat * m2, (float)rv[nt][r])));   // as stored
      }
      if (nt == wave) tc_st4(a.dxmid + row * D + 16 * nt + 4 * g, acc[nt]);
      if (nt % 4 == 3) __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- da = dx_mid Wp: output tile `wave` ---------------------------------------------------------------------------------------
  {
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) mma(fwp[ks], acc_to_frag<bf16>(acc[2 * ks], acc[2 * ks + 1]), o);
    tc_st4(a.da + row * D + f0, o);
  }
  // du, as the lane wrote it to LDS
  for (int nt = wave; nt < ntiles; nt += NT)
    *reinterpret_cast<bf16x4*>(a.du + hrow + 16 * nt) = *reinterpret_cast<const bf16x4*>(sDu + c * HLD + lo + 16 * nt);
}

}  // namespace vitpe

using namespace vitpe;

extern "C" int vitpe_block_tail2_supported(int dtype, int D, int HID);

extern "C" int vitpe_tail_cls_fwd(int dtype, const void* attn_out, const void* x_in, const void* Wp_packed, const float* bp,
                                  const float* gamma, const float* beta, void* x_mid, float* mean2, float* rstd2, void* xn_out,
                                  const void* W1_packed, const float* b1, const void* W2_packed, const float* b2, void* gp_out,
                                  void* h_out, void* out, float eps2, int B, int row_step, int D, int HID, hipStream_t stream) {
  VITPE_REQUIRE(attn_out && x_in && Wp_packed && bp && gamma && beta && x_mid && mean2 && rstd2 && W1_packed && b1 &&
                W2_packed && b2 && out && B >= 0 && row_step >= 1);
  VITPE_REQUIRE((gp_out == nullptr) == (h_out == nullptr));
  if (!vitpe_block_tail2_supported(dtype, D, HID)) return (int)hipErrorNotSupported;
  if (B == 0) return 0;
  TailClsFwdArgs a{};
  a.a = (const bf16*)attn_out; a.xin = (const bf16*)x_in; a.wp = (const bf16*)Wp_packed; a.bp = bp; a.gamma = gamma; a.beta = beta;
  a.w1 = (const bf16*)W1_packed; a.b1 = b1; a.w2 = (const bf16*)W2_packed; a.b2 = b2; a.xmid = (bf16*)x_mid; a.mean2 = mean2;
  a.rstd2 = rstd2; a.xn_out = (bf16*)xn_out; a.gp_out = (_Float16*)gp_out; a.h_out = (bf16*)h_out; a.out = (bf16*)out;
  a.B = B; a.HID = HID; a.row_step = row_step; a.eps2 = eps2;
  hipLaunchKernelGGL(tail_cls_fwd_kernel, dim3((B + 15) / 16), dim3(TC_THREADS), 0, stream, a);
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_tail_cls_bwd(int dtype, const void* dy, const void* gp, const void* W2t_packed, const void* W1t_packed,
                                  const void* x_mid, const float* mean2, const float* rstd2, const float* gamma, void* du,
                                  void* dx_mid, float* dgamma, float* dbeta, const void* WpT_packed, void* da, int B, int row_step,
                                  int D, int HID, hipStream_t stream) {
  VITPE_REQUIRE(dy && gp && W2t_packed && W1t_packed && x_mid && mean2 && rstd2 && gamma && du && dx_mid && dgamma && dbeta &&
                WpT_packed && da && B >= 0 && row_step >= 1);
  if (!vitpe_block_tail2_supported(dtype, D, HID)) return (int)hipErrorNotSupported;
  if (B == 0) return 0;
  TailClsBwdArgs a{};
  a.dy = (const bf16*)dy; a.gp = (const _Float16*)gp; a.xmid = (const bf16*)x_mid; a.mean2 = mean2; a.rstd2 = rstd2; a.gamma = gamma;
  a.w2t = (const bf16*)W2t_packed; a.w1t = (const bf16*)W1t_packed; a.wpt = (const bf16*)WpT_packed; a.du = (bf16*)du;
  a.dxmid = (bf16*)dx_mid; a.da = (bf16*)da; a.dgamma = dgamma; a.dbeta = dbeta; a.B = B; a.HID = HID; a.row_step = row_step;
  hipLaunchKernelGGL(tail_cls_bwd_kernel, dim3((B + 15) / 16), dim3(TC_THREADS), 0, stream, a);
  VITPE_CHECK_LAUNCH();
}
