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
// (48 values per lane, the layout and summation order of tail2.hip).  Weight fragments are read straight from global
// memory (L2-resident: 0.66 MB per direction, read by every workgroup) -- the kernels are bound by the
// latency of those loads (traced: 28 us forward, 46 us backward at batch 512; DESIGN.md 4, "Top block on the class-token
// rows": the k loops over the hidden layer issue one fragment load per MFMA, 24 dependent round trips in a row).
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

__global__ __launch_bounds__(TC_THREADS) void tail_cls_fwd_kernel(TailClsFwdArgs a) {
  constexpr int D = TC_D, NT = TC_NT, KS = TC_KS;
  __shared__ __attribute__((aligned(16))) bf16 sX[16 * TC_XLD];
  __shared__ __attribute__((aligned(16))) bf16 sH[16 * (TC_MAXHID + TC_HPAD)];
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int HID = a.HID, HLD = HID + TC_HPAD;
  const size_t row = (size_t)min(16 * (int)blockIdx.x + c, a.B - 1) * a.row_step;   // rows past B: copies of row B - 1 (such lanes store
  // the SAME values to the SAME addresses as the lane that owns row B - 1: a benign race, as in tail2.hip)
  const int f0 = 16 * wave + 4 * g;             // this lane's 4 features of the wave's 192-wide output tile

  // ---- x_mid = x_in + a Wp^T + bp: output tile `wave` -----------------------------------------------------------------------
  f32x4 xm_own;
  {
    const bf16* ar = a.a + row * D + 8 * g;
    const bf16* wf = a.wp + (size_t)wave * KS * 512 + lane * 8;
    Frag<bf16> fa[KS], fw[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) { fw[ks] = ld_frag(wf + ks * 512); fa[ks] = ld_frag(ar + 32 * ks); }
    const bf16x4 xr = *reinterpret_cast<const bf16x4*>(a.xin + row * D + f0);
    f32x4 acc = *reinterpret_cast<const f32x4*>(a.bp + f0);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) mma(fw[ks], fa[ks], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = to_f32(from_f32<bf16>(acc[r] + (float)xr[r]));   // values as stored
    xm_own = acc;
    tc_st4(a.xmid + row * D + f0, acc);
    tc_st4(sX + c * TC_XLD + f0, acc);
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
    for (int nt = 0; nt < NT; ++nt) {
      const f32x4 gv = *reinterpret_cast<const f32x4*>(a.gamma + 16 * nt + 4 * g);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(a.beta + 16 * nt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) xa[nt][r] = fmaf((xa[nt][r] - mean) * rstd, gv[r], bv[r]);
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      bf[ks] = acc_to_frag<bf16>(xa[2 * ks], xa[2 * ks + 1]);
      if (a.xn_out != nullptr && ks == wave) {      // waves 0 .. 5 write one 32-wide chunk of the normalised rows each
        bf16* xr = a.xn_out + row * D + 32 * ks + 4 * g;
        *reinterpret_cast<bf16x4*>(xr) = __builtin_shufflevector(bf[ks].v, bf[ks].v, 0, 1, 2, 3);
        *reinterpret_cast<bf16x4*>(xr + 16) = __builtin_shufflevector(bf[ks].v, bf[ks].v, 4, 5, 6, 7);
      }
    }
  }

  // ---- u = xn W1^T + b1; h = gelu(u), g' = gelu'(u): hidden tiles wave, wave + 12, ... --------------------------------------
  const bool save = a.gp_out != nullptr;
  for (int nt = wave; nt < HID / 16; nt += NT) {
    const bf16* wf = a.w1 + (size_t)nt * KS * 512 + lane * 8;
    Frag<bf16> fw[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) fw[ks] = ld_frag(wf + ks * 512);
    f32x4 acc = *reinterpret_cast<const f32x4*>(a.b1 + 16 * nt + 4 * g);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) mma(fw[ks], bf[ks], acc);
    f32x4 hh, gp;
#pragma unroll
    for (int r = 0; r < 4; ++r) { float hv, gv; tc_gelu(acc[r], hv, gv); hh[r] = hv; gp[r] = gv; }
    tc_st4(sH + c * HLD + 16 * nt + 4 * g, hh);
    if (save) {
      tc_st4(a.h_out + row * HID + 16 * nt + 4 * g, hh);
      // IEEE half, round toward zero: the conversion block_tail2_fwd_kernel uses (t2_store_pair_f16)
      const uint2 pk = {__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(gp[0], gp[1])),
                        __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(gp[2], gp[3]))};
      *reinterpret_cast<uint2*>(a.gp_out + row * HID + 16 * nt + 4 * g) = pk;
    }
  }
  __syncthreads();

  // ---- out = x_mid + h W2^T + b2: output tile `wave`, k = the whole hidden layer from LDS -----------------------------------
  {
    f32x4 acc = *reinterpret_cast<const f32x4*>(a.b2 + f0);
    const bf16* wf = a.w2 + (size_t)wave * 512 + lane * 8;
    const bf16* hr = sH + c * HLD + 4 * g;
    for (int kc = 0; kc < HID / 32; ++kc) mma(ld_frag(wf + (size_t)kc * NT * 512), tc_phi_frag(hr + 32 * kc), acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] += xm_own[r];
    tc_st4(a.out + row * D + f0, acc);
  }
}

struct TailClsBwdArgs {
  const bf16* dy; const _Float16* gp; const bf16* xmid; const float* mean2; const float* rstd2; const float* gamma;
  const bf16* w2t; const bf16* w1t; const bf16* wpt;
  bf16* du; bf16* dxmid; bf16* da;
  float* dgamma; float* dbeta;
  int B, HID, row_step;
};

__global__ __launch_bounds__(TC_THREADS) void tail_cls_bwd_kernel(TailClsBwdArgs a) {
  constexpr int D = TC_D, NT = TC_NT, KS = TC_KS;
  __shared__ __attribute__((aligned(16))) float sDx[16 * TC_FLD];
  __shared__ __attribute__((aligned(16))) bf16 sDu[16 * (TC_MAXHID + TC_HPAD)];
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int HID = a.HID, HLD = HID + TC_HPAD;
  const int lrow = 16 * (int)blockIdx.x + c;
  const size_t row = (size_t)min(lrow, a.B - 1) * a.row_step;   // (clamped lanes: identical stores to row B - 1, see the forward)
  const float valid = lrow < a.B ? 1.0f : 0.0f;
  const int f0 = 16 * wave + 4 * g;

  // ---- dh = dy W2; du = dh * gelu'(u): hidden tiles wave, wave + 12, ... ----------------------------------------------------
  const bf16* const dyr = a.dy + row * D + 4 * g;
  Frag<bf16> bf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) bf[ks] = tc_phi_frag(dyr + 32 * ks);
  for (int nt = wave; nt < HID / 16; nt += NT) {
    const bf16* wf = a.w2t + (size_t)nt * KS * 512 + lane * 8;
    Frag<bf16> fw[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) fw[ks] = ld_frag(wf + ks * 512);
    const uint2 gw = *reinterpret_cast<const uint2*>(a.gp + row * HID + 16 * nt + 4 * g);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) mma(fw[ks], bf[ks], acc);
    f32x4 d;
    d[0] = acc[0] * (float)__builtin_bit_cast(_Float16, (unsigned short)(gw.x & 0xffffu));
    d[1] = acc[1] * (float)__builtin_bit_cast(_Float16, (unsigned short)(gw.x >> 16));
    d[2] = acc[2] * (float)__builtin_bit_cast(_Float16, (unsigned short)(gw.y & 0xffffu));
    d[3] = acc[3] * (float)__builtin_bit_cast(_Float16, (unsigned short)(gw.y >> 16));
    tc_st4(a.du + row * HID + 16 * nt + 4 * g, d);
    tc_st4(sDu + c * HLD + 16 * nt + 4 * g, d);
  }
  __syncthreads();

  // ---- dxn = du W1: output tile `wave`, k = the whole hidden layer from LDS; the fp32 tile crosses the waves through LDS -------
  {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const bf16* wf = a.w1t + (size_t)wave * 512 + lane * 8;
    const bf16* dr = sDu + c * HLD + 4 * g;
    for (int kc = 0; kc < HID / 32; ++kc) mma(ld_frag(wf + (size_t)kc * NT * 512), tc_phi_frag(dr + 32 * kc), acc);
    *reinterpret_cast<f32x4*>(sDx + c * TC_FLD + f0) = acc;
  }
  __syncthreads();

  // ---- dx_mid = dy + LayerNorm2'(dxn) on the whole tile, every wave (t2_ln_backward's arithmetic); wave w stores tile w and
  // owns its dgamma / dbeta columns
  f32x4 acc[NT];
  {
    const float mean = a.mean2[row], rstd = a.rstd2[row];
    const bf16* xr = a.xmid + row * D + 4 * g;
    const float invD = 1.0f / (float)D;
    bf16x4 xmv[NT];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      xmv[nt] = *reinterpret_cast<const bf16x4*>(xr + 16 * nt);
      acc[nt] = *reinterpret_cast<const f32x4*>(sDx + c * TC_FLD + 16 * nt + 4 * g);
      const f32x4 gam = *reinterpret_cast<const f32x4*>(a.gamma + 16 * nt + 4 * g);
      float tg[4], tb[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float xhat = ((float)xmv[nt][r] - mean) * rstd;
        const float dxn = acc[nt][r];
        tg[r] = dxn * xhat * valid;
        tb[r] = dxn * valid;
        const float gy = dxn * gam[r];
        s1 += gy;
        s2 = fmaf(gy, xhat, s2);
      }
      if (nt == wave) {     // column sums over the tile's 16 tokens: one atomic per column and workgroup
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float sg = group16_sum(tg[r]), sb = group16_sum(tb[r]);
          if (c == 0) { atomicAdd(a.dgamma + 16 * nt + 4 * g + r, sg); atomicAdd(a.dbeta + 16 * nt + 4 * g + r, sb); }
        }
      }
    }
    const float m1 = xgroup_sum(s1) * invD, m2 = xgroup_sum(s2) * invD;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const bf16x4 rv = *reinterpret_cast<const bf16x4*>(dyr + 16 * nt);      // the residual rows
      const f32x4 gam = *reinterpret_cast<const f32x4*>(a.gamma + 16 * nt + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float xhat = ((float)xmv[nt][r] - mean) * rstd;
        const float gy = acc[nt][r] * gam[r];
        acc[nt][r] = to_f32(from_f32<bf16>(fmaf(rstd, gy - m1 - xhat * m2, (float)rv[r])));   // as stored
      }
      if (nt == wave) tc_st4(a.dxmid + row * D + 16 * nt + 4 * g, acc[nt]);
    }
  }

  // ---- da = dx_mid Wp: output tile `wave` ---------------------------------------------------------------------------------------
  {
    const bf16* wf = a.wpt + (size_t)wave * KS * 512 + lane * 8;
    Frag<bf16> fwp[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) fwp[ks] = ld_frag(wf + ks * 512);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) mma(fwp[ks], acc_to_frag<bf16>(acc[2 * ks], acc[2 * ks + 1]), o);
    tc_st4(a.da + row * D + f0, o);
  }
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
