// Patch-embed unfold, positional-encoding table builders, stand-alone rotary apply, classifier
// head + cross-entropy, the weight shadows, and the primitive self-tests.
#include "common.h"
#include "augment.h"

namespace vitpe {

// ---------------------------------------------------------------------------------------
// Patch-embed unfold (reference models/vit.py:164,248-250: Conv2d(k=s=p) == unfold + GEMM).
// patches[(b*P + gy*g + gx)][c*p*p + ky*p + kx] = img[b][c][gy*p+ky][gx*p+kx]
// One thread per (b, patch, c, ky) moves p contiguous pixels (fp32 in, T out).
template <typename T>
__global__ void unfold_kernel(const float* __restrict__ img, T* __restrict__ patches, int B, int Cc, int S, int p) {
  const int g = S / p, P = g * g, Kp = Cc * p * p;
  const long long total = (long long)B * P * Cc * p;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int ky = (int)(idx % p);
    long long t = idx / p;
    const int ch = (int)(t % Cc); t /= Cc;
    const int n = (int)(t % P);
    const int b = (int)(t / P);
    const int gy = n / g, gx = n % g;
    const float* src = img + (((size_t)b * Cc + ch) * S + gy * p + ky) * S + gx * p;
    T* dst = patches + ((size_t)b * P + n) * Kp + ch * p * p + ky * p;
    for (int kx = 0; kx < p; ++kx) dst[kx] = from_f32<T>(src[kx]);
  }
}

// bf16, p % 8 == 0 (224 / 16): one thread per 8 pixels -- two 16-B loads, one 16-B store; consecutive threads write
// consecutive 16-B pieces of the patch matrix (the scalar loop above ran at 0.7 TB/s: 78 us per ViT-B/16 step)
__global__ void unfold8_kernel(const float* __restrict__ img, bf16* __restrict__ patches, int B, int Cc, int S, int p) {
  const int g = S / p, P = g * g, Kp = Cc * p * p, p8 = p / 8;
  const long long total = (long long)B * P * Cc * p * p8;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int hx = (int)(idx % p8);
    long long t = idx / p8;
    const int ky = (int)(t % p); t /= p;
    const int ch = (int)(t % Cc); t /= Cc;
    const int n = (int)(t % P);
    const int b = (int)(t / P);
    const int gy = n / g, gx = n % g;
    const float* src = img + (((size_t)b * Cc + ch) * S + gy * p + ky) * S + gx * p + 8 * hx;
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
    float f[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    *reinterpret_cast<Chunk16*>(patches + ((size_t)b * P + n) * Kp + ch * p * p + ky * p + 8 * hx) = f32_to_chunk<bf16>(f);
  }
}

// Same from a uint8 dataset resident in HBM (reference train.py:69-92: DataLoader gather ->
// ToTensor (x/255) -> Normalize((x-mean)/std) -> model): record index[b] of data [Ndata,C,S,S] (the
// CIFAR-10 binary / MNIST idx pixel order) is normalised in fp32 with the reference's operation
// order and written straight as the patch matrix; img_out (nullable) receives the fp32 image.
// AUG (vitpe_unfold_u8_aug): the source pixel goes through the augmentation stream of augment.h (random crop with zero
// padding + horizontal flip per batch slot b); the draw is repeated only when a thread moves on to another image.
template <typename T, bool AUG>
__global__ void unfold_u8_kernel(const unsigned char* __restrict__ data, const long long* __restrict__ index,
                                 const float* __restrict__ mean, const float* __restrict__ stdv, T* __restrict__ patches,
                                 float* __restrict__ img_out, int B, int Cc, int S, int p,
                                 const unsigned long long* __restrict__ rng, int pad, int hflip) {
  const int g = S / p, P = g * g, Kp = Cc * p * p;
  const long long total = (long long)B * P * Cc * p;
  AugDraw aug = {0, 0, 0};
  int aug_b = -1;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int ky = (int)(idx % p);
    long long t = idx / p;
    const int ch = (int)(t % Cc); t /= Cc;
    const int n = (int)(t % P);
    const int b = (int)(t / P);
    const int gy = n / g, gx = n % g;
    const long long rec = index != nullptr ? index[b] : (long long)b;
    const size_t pix = ((size_t)ch * S + gy * p + ky) * S + gx * p;
    const unsigned char* src = data + (size_t)rec * Cc * S * S + pix;
    T* dst = patches + ((size_t)b * P + n) * Kp + ch * p * p + ky * p;
    const float m = mean[ch], sd = stdv[ch];
    if (AUG) {
      if (b != aug_b) { aug = aug_draw(rng, (unsigned long long)b, pad, hflip); aug_b = b; }
      const int sy = gy * p + ky + aug.oy - pad;
      const bool rowok = sy >= 0 && sy < S;
      const unsigned char* row = data + (size_t)rec * Cc * S * S + ((size_t)ch * S + (rowok ? sy : 0)) * S;
      for (int kx = 0; kx < p; ++kx) {
        const int sx = (aug.flip ? S - 1 - (gx * p + kx) : gx * p + kx) + aug.ox - pad;
        unsigned char u = 0;   // the zero padding
        if (rowok && sx >= 0 && sx < S) u = row[sx];
        const float v = ((float)u / 255.0f - m) / sd;
        dst[kx] = from_f32<T>(v);
        if (img_out != nullptr) img_out[(size_t)b * Cc * S * S + pix + kx] = v;
      }
      continue;
    }
    for (int kx = 0; kx < p; ++kx) {
      const float v = ((float)src[kx] / 255.0f - m) / sd;   // ToTensor then Normalize, IEEE division
      dst[kx] = from_f32<T>(v);
      if (img_out != nullptr) img_out[(size_t)b * Cc * S * S + pix + kx] = v;
    }
  }
}

// the draws of the first B batch slots as integers (tests): out [B,3] = (oy, ox, flip)
__global__ void augment_params_kernel(const unsigned long long* __restrict__ rng, int* __restrict__ out, int B, int pad,
                                      int hflip) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const AugDraw d = aug_draw(rng, (unsigned long long)b, pad, hflip);
  out[3 * b] = d.oy; out[3 * b + 1] = d.ox; out[3 * b + 2] = d.flip;
}

// ---------------------------------------------------------------------------------------
// Integer tables (bit-exact contract)
__global__ void rel_index_kernel(long long* out, int L) {  // positional_encoding.py:67-75
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= L * L) return;
  const int i = idx / L, j = idx % L;
  long long v = (long long)i - j + (L - 1);
  v = v < 0 ? 0 : (v > 2LL * L - 2 ? 2LL * L - 2 : v);
  out[idx] = v;
}
__global__ void l1_matrix_kernel(long long* out, int G) {  // positional_encoding.py:136-142
  const int P = G * G;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= P * P) return;
  const int i = idx / P, j = idx % P;
  out[idx] = (long long)(abs(i % G - j % G) + abs(i / G - j / G));
}

// RoPE tables.  axial: phase[n][f] = (f < q ? n%G : n/G) * inv_freq[f mod q]   (positional_encoding.py:228-245)
__global__ void rope_axial_kernel(const float* __restrict__ inv_freq, float* cosv, float* sinv, int G, int half) {
  const int P = G * G, q = half / 2;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= P * half) return;
  const int n = idx / half, f = idx % half;
  const float t = (f < q) ? (float)(n % G) : (float)(n / G);
  const float ph = __fmul_rn(t, inv_freq[f < q ? f : f - q]);
  cosv[idx] = cosf(ph);
  sinv[idx] = sinf(ph);
}
// mixed: slot [h,n] = phase of head (n*H+h)/P at position (n*H+h)%P -- the reference's
// view-scramble (positional_encoding.py:337-342).  Output contiguous [H,P,half].
__global__ void rope_mixed_kernel(const float* __restrict__ freqs, float* cosv, float* sinv, int H, int G, int half) {
  const int P = G * G;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= H * P * half) return;
  const int f = idx % half, n = (idx / half) % P, h = idx / (half * P);
  const int flat = n * H + h, hs = flat / P, ps = flat % P;
  const float tx = (float)(ps % G), ty = (float)(ps / G);
  const float ph = __fadd_rn(__fmul_rn(tx, freqs[(0 * H + hs) * half + f]), __fmul_rn(ty, freqs[(1 * H + hs) * half + f]));
  cosv[idx] = cosf(ph);
  sinv[idx] = sinf(ph);
}

// bias[h,i,j] materialised for the get_bias() API surface (positional_encoding.py:82-95, 127-171)
__global__ void rel_bias_kernel(const float* __restrict__ table, float* out, int H, int L) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= H * L * L) return;
  const int j = idx % L, i = (idx / L) % L, h = idx / (L * L);
  int r = i - j + L - 1;
  r = max(0, min(r, 2 * L - 2));
  out[idx] = table[h * (2 * L - 1) + r];
}
__global__ void poly_bias_kernel(const float* __restrict__ coeff, float* out, int H, int G, int degree, int per_head) {
  const int P = G * G, L = P + 1;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= H * L * L) return;
  const int j = idx % L, i = (idx / L) % L, h = idx / (L * L);
  float v = 0.f;
  if (i >= 1 && j >= 1) {
    const int pi = i - 1, pj = j - 1;
    const float x = (float)(abs(pi % G - pj % G) + abs(pi / G - pj / G));
    const float* cf = coeff + (per_head ? h * (degree + 1) : 0);
    float pw = 1.f;  // sum_k c_k * x^k in ascending k like the reference's feats @ coeffs
    for (int k = 0; k <= degree; ++k) { v += pw * cf[k]; pw *= x; }
  }
  out[idx] = v;
}

// Transposes of the three table builders above, for the stand-alone modules' differentiable get_bias() /
// get_freqs_cis() (the reference returns autograd-tracked tensors, positional_encoding.py:82-95,127-171,313-351).
// Deterministic (fixed summation order), not on the hot path: inside the model the attention backward kernels
// produce these gradients directly.
__global__ void rel_bias_bwd_kernel(const float* __restrict__ dbias, float* __restrict__ dtable, int H, int L) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;   // (h, r): the r-th diagonal i - j = r - (L-1)
  if (idx >= H * (2 * L - 1)) return;
  const int h = idx / (2 * L - 1), r = idx % (2 * L - 1);
  float s = 0.f;
  for (int i = 0; i < L; ++i) {
    const int j = i - (r - (L - 1));
    if (j >= 0 && j < L) s += dbias[((size_t)h * L + i) * L + j];
  }
  dtable[idx] = s;
}
// one workgroup per (head group, power k): dcoeff[hh][k] = sum_{h in group} sum_{i,j>=1} dbias[h,i,j] * l1(i,j)^k
__global__ __launch_bounds__(256) void poly_bias_bwd_kernel(const float* __restrict__ dbias, float* __restrict__ dcoeff,
                                                            int H, int G, int degree, int per_head) {
  __shared__ float red[256];
  const int P = G * G, L = P + 1;
  const int hh = blockIdx.x / (degree + 1), k = blockIdx.x % (degree + 1);
  const int h0 = per_head ? hh : 0, h1 = per_head ? hh + 1 : H;
  float s = 0.f;
  for (int h = h0; h < h1; ++h)
    for (int q = threadIdx.x; q < P * P; q += 256) {
      const int pi = q / P, pj = q % P;
      const float x = (float)(abs(pi % G - pj % G) + abs(pi / G - pj / G));
      float pw = 1.f;
      for (int t = 0; t < k; ++t) pw *= x;
      s += dbias[((size_t)h * L + pi + 1) * L + pj + 1] * pw;
    }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) dcoeff[blockIdx.x] = red[0];
}
// dfreqs[a][hs][f] = sum over the slots [h,n] the view-scramble maps to head hs of t_a(ps) * (cos*dsin - sin*dcos)
__global__ void rope_mixed_bwd_kernel(const float* __restrict__ freqs, const float* __restrict__ dcos,
                                      const float* __restrict__ dsin, float* __restrict__ dfreqs, int H, int G, int half) {
  const int P = G * G;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * H * half) return;
  const int f = idx % half, hs = (idx / half) % H, a = idx / (half * H);
  const float fx = freqs[(0 * H + hs) * half + f], fy = freqs[(1 * H + hs) * half + f];
  float s = 0.f;
  for (int ps = 0; ps < P; ++ps) {
    const int flat = hs * P + ps, n = flat / H, h = flat % H;   // inverse of flat = n*H + h
    const float tx = (float)(ps % G), ty = (float)(ps / G);
    const float ph = __fadd_rn(__fmul_rn(tx, fx), __fmul_rn(ty, fy));
    const size_t o = ((size_t)h * P + n) * half + f;
    s += (a == 0 ? tx : ty) * (cosf(ph) * dsin[o] - sinf(ph) * dcos[o]);
  }
  dfreqs[idx] = s;
}

// stand-alone rotate-half (models/rope_utils.py:3-37): x [B,H,P,HD] fp32, cos/sin [P,HD/2] or [H,P,HD/2]
__global__ void rotary_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ cosv,
                              const float* __restrict__ sinv, long long total_pairs, int H, int P, int half, int per_head) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total_pairs) return;
  const int f = (int)(idx % half);
  long long t = idx / half;
  const int n = (int)(t % P); t /= P;
  const int h = (int)(t % H);
  const size_t row = (size_t)(idx / half) * 2 * half;
  const size_t o = ((per_head ? (size_t)h * P : 0) + n) * half + f;
  const float c = cosv[o], s = sinv[o];
  const float x1 = x[row + f], x2 = x[row + half + f];
  y[row + f] = __fsub_rn(__fmul_rn(x1, c), __fmul_rn(x2, s));
  y[row + half + f] = __fadd_rn(__fmul_rn(x1, s), __fmul_rn(x2, c));
}

// ---------------------------------------------------------------------------------------
// Classifier head (vit.py:284-285): LayerNorm of the class row only, then Linear(d, classes).
// One wave per image.  ws_* (optional, for backward): xhat [B,D], yn [B,D] fp32.
template <typename T>
__global__ __launch_bounds__(256) void head_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ Wh,
                                                       const float* __restrict__ bh, float* __restrict__ logits,
                                                       float* __restrict__ ws_xhat, float* __restrict__ ws_yn,
                                                       float* __restrict__ ws_rstd, int B, int Ntok, int D, int Cn,
                                                       float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float invD = 1.0f / (float)D;
  for (int b = blockIdx.x * 4 + wave; b < B; b += gridDim.x * 4) {
    const T* row = x + (size_t)b * Ntok * D;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += to_f32(row[d]);
    const float mean = wave_sum(s) * invD;
    float s2 = 0.f;
    for (int d = lane; d < D; d += 64) { const float t = to_f32(row[d]) - mean; s2 += t * t; }
    const float rstd = 1.0f / sqrtf(wave_sum(s2) * invD + eps);
    for (int cI = 0; cI < Cn; ++cI) {
      float acc = 0.f;
      for (int d = lane; d < D; d += 64) {
        const float xh = (to_f32(row[d]) - mean) * rstd;
        acc += (xh * gamma[d] + beta[d]) * Wh[(size_t)cI * D + d];
      }
      acc = wave_sum(acc);
      if (lane == 0) logits[(size_t)b * Cn + cI] = acc + bh[cI];
    }
    if (ws_xhat) {
      for (int d = lane; d < D; d += 64) {
        const float xh = (to_f32(row[d]) - mean) * rstd;
        ws_xhat[(size_t)b * D + d] = xh;
        ws_yn[(size_t)b * D + d] = xh * gamma[d] + beta[d];
      }
      if (lane == 0) ws_rstd[b] = rstd;
    }
  }
}

// mean cross-entropy + dlogits = (softmax - onehot) * gscale ; single workgroup, fixed order.
// out[0] = mean loss, out[1] = #correct (argmax == label)   (train.py:113,119-121)
// ctl (nullable, device): {grad_scale, loss_scale, n_valid} -- read on the device so that a captured graph follows a
// ragged last batch (reference train.py:89-90: no drop_last): rows b >= n_valid are padding, they get dlogits = 0
// (every downstream gradient is linear in dlogits, so padded images contribute exactly nothing) and are left out of
// the loss / accuracy.  out[0] = loss_scale * sum of the valid rows' losses.  acc (nullable): out is also added to it.
__global__ __launch_bounds__(256) void ce_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                 float* __restrict__ dlogits, float* __restrict__ out, int B, int Cn,
                                                 float gscale, const float* __restrict__ ctl, float* __restrict__ acc) {
  __shared__ float sl[256], sc[256];
  float lsum = 0.f, csum = 0.f;
  float lscale = 1.0f / (float)B;
  int nvalid = B;
  if (ctl != nullptr) { gscale = ctl[0]; lscale = ctl[1]; nvalid = min(B, (int)ctl[2]); }
  for (int b = threadIdx.x; b < B; b += 256) {
    if (b >= nvalid) {
      if (dlogits) for (int k = 0; k < Cn; ++k) dlogits[(size_t)b * Cn + k] = 0.f;
      continue;
    }
    const float* z = logits + (size_t)b * Cn;
    float m = z[0];
    int am = 0;
    for (int k = 1; k < Cn; ++k) if (z[k] > m) { m = z[k]; am = k; }
    float se = 0.f;
    for (int k = 0; k < Cn; ++k) se += expf(z[k] - m);
    const int y = (int)labels[b];
    lsum += (m + logf(se)) - z[y];
    csum += (am == y) ? 1.f : 0.f;
    if (dlogits) {
      const float inv = 1.0f / se;
      for (int k = 0; k < Cn; ++k) dlogits[(size_t)b * Cn + k] = (expf(z[k] - m) * inv - (k == y ? 1.f : 0.f)) * gscale;
    }
  }
  sl[threadIdx.x] = lsum;
  sc[threadIdx.x] = csum;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (threadIdx.x < o) { sl[threadIdx.x] += sl[threadIdx.x + o]; sc[threadIdx.x] += sc[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float l = sl[0] * lscale, c = sc[0];
    out[0] = l; out[1] = c;
    if (acc != nullptr) { acc[0] += l; acc[1] += c; }
  }
}

// The train step's head in ONE launch (+ the parameter-gradient kernel): final LayerNorm of the class row, logits,
// cross-entropy with the device-side scalars of ce_kernel (ragged batches), accuracy, dlogits and the data gradient
// through the LayerNorm -- one wave per image, every dependent chain as short as the arithmetic allows:
//   * lane l holds elements l, l + 64, ... of the class row (KD = ceil(D / 64) registers): coalesced 2-B / 4-B loads;
//   * the logits of up to 8 classes are reduced TOGETHER (eight independent butterfly sums in flight; a loop over the
//     classes runs its ten wave reductions back to back: ~6 K cycles of shuffle latency per image, measured in round 1);
//   * rows 1.. of dx are NOT written: the caller keeps them zero (they never change), only the class row is stored.
// Batch totals: every wave leaves (loss, correct) of its image in per_image [B,2]; head_bwd_params_kernel, which follows
// anyway, sums them in fixed order into out2 / metric_acc (deterministic, no atomics).
template <typename T, int KD, bool WLDS>
__global__ __launch_bounds__(256) void head_step_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ Wh,
                                                        const float* __restrict__ bh, const long long* __restrict__ labels,
                                                        float* __restrict__ logits, float* __restrict__ dlogits,
                                                        float* __restrict__ ws_xhat, float* __restrict__ ws_yn,
                                                        float* __restrict__ ws_dyn, T* __restrict__ dx,
                                                        float* __restrict__ per_image, const float* __restrict__ ctl,
                                                        int B, int Ntok, int D, int Cn, float eps) {
  // The head weight is read twice by every wave (logits, then the class row's gradient); from global those were 2 x Cn
  // dependent L2 round trips in a one-wave-per-image chain.  Staged into LDS once per workgroup, under the HBM latency
  // of the class rows (heads up to HS_LDS floats; larger ones keep reading global).
  constexpr int HS_LDS = 16 * 768;
  __shared__ float sWh[WLDS ? HS_LDS : 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b_raw = blockIdx.x * 4 + wave;
  const bool live = b_raw < B;
  const int b = live ? b_raw : B - 1;
  const float invD = 1.0f / (float)D;
  const float gscale = ctl[0], lscale = ctl[1];
  const int nvalid = min(B, (int)ctl[2]);
  const T* row = x + (size_t)b * Ntok * D;
  float xv[KD], gam[KD], bet[KD];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < KD; ++k) {
    const int d = lane + 64 * k;
    const bool ok = d < D;
    xv[k] = ok ? to_f32(row[d]) : 0.f;
    gam[k] = ok ? gamma[d] : 0.f;
    bet[k] = ok ? beta[d] : 0.f;
  }
  if (WLDS)
    for (int i = threadIdx.x; i < Cn * D; i += 256) sWh[i] = Wh[i];
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int k = 0; k < KD; ++k) s += xv[k];
  const float mean = wave_sum(s) * invD;
  float s2 = 0.f;
#pragma unroll
  for (int k = 0; k < KD; ++k) { const float t = (lane + 64 * k < D) ? xv[k] - mean : 0.f; s2 += t * t; }
  const float rstd = 1.0f / sqrtf(wave_sum(s2) * invD + eps);
  float xh[KD], yn[KD];
#pragma unroll
  for (int k = 0; k < KD; ++k) {
    const int d = lane + 64 * k;
    xh[k] = (d < D) ? (xv[k] - mean) * rstd : 0.f;
    yn[k] = xh[k] * gam[k] + bet[k];
    if (d < D) { ws_xhat[(size_t)b * D + d] = xh[k]; ws_yn[(size_t)b * D + d] = yn[k]; }
  }
  float z = -3.0e38f;   // lane c < Cn holds logit c
  for (int c0 = 0; c0 < Cn; c0 += 8) {
    float part[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      part[j] = 0.f;
      const int cI = min(c0 + j, Cn - 1);
#pragma unroll
      for (int k = 0; k < KD; ++k) {
        const int d = lane + 64 * k;
        part[j] += (d < D) ? yn[k] * (WLDS ? sWh[cI * D + d] : Wh[(size_t)cI * D + d]) : 0.f;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
#pragma unroll
      for (int j = 0; j < 8; ++j) part[j] += __shfl_xor(part[j], o, 64);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (lane == c0 + j && c0 + j < Cn) z = part[j] + bh[c0 + j];
  }
  if (lane < Cn) logits[(size_t)b * Cn + lane] = z;
  float m = z;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  int am = (lane < Cn && z == m) ? lane : 1 << 20;   // first index of the maximum (torch.max semantics)
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) am = min(am, __shfl_xor(am, o, 64));
  const float e = lane < Cn ? expf(z - m) : 0.f;
  const float se = wave_sum(e);
  const int y = (int)labels[b];
  const float zy = __shfl(z, y, 64);
  const bool valid = b < nvalid;
  const float dl = (lane < Cn && valid) ? (e * (1.0f / se) - (lane == y ? 1.f : 0.f)) * gscale : 0.f;
  if (lane < Cn) dlogits[(size_t)b * Cn + lane] = dl;
  // data gradient: dyn = dlogits @ Wh, then the LayerNorm backward of the class row
  float dyn[KD];
#pragma unroll
  for (int k = 0; k < KD; ++k) dyn[k] = 0.f;
  for (int c = 0; c < Cn; ++c) {
    const float dc = __shfl(dl, c, 64);
#pragma unroll
    for (int k = 0; k < KD; ++k) {
      const int d = lane + 64 * k;
      dyn[k] += (d < D) ? dc * (WLDS ? sWh[c * D + d] : Wh[(size_t)c * D + d]) : 0.f;
    }
  }
  float t1 = 0.f, t2 = 0.f;
#pragma unroll
  for (int k = 0; k < KD; ++k) {
    const int d = lane + 64 * k;
    if (d < D) ws_dyn[(size_t)b * D + d] = dyn[k];
    const float gv = dyn[k] * gam[k];
    t1 += gv;
    t2 += gv * xh[k];
  }
  t1 = wave_sum(t1) * invD;
  t2 = wave_sum(t2) * invD;
  T* drow = dx + (size_t)b * Ntok * D;
#pragma unroll
  for (int k = 0; k < KD; ++k) {
    const int d = lane + 64 * k;
    if (d < D) drow[d] = from_f32<T>(rstd * (dyn[k] * gam[k] - t1 - xh[k] * t2));
  }
  if (lane == 0) {   // per-image results; head_bwd_params_kernel sums them (no same-address atomics: ~12 ns each, serialised)
    per_image[2 * b] = valid ? ((m + logf(se)) - zy) * lscale : 0.f;
    per_image[2 * b + 1] = (valid && am == y) ? 1.f : 0.f;
  }
}

// head backward, stage 1 (one wave per image): dyn = dlogits @ Wh ; LN backward of the class row;
// dx row 0 written, rows 1.. zeroed.  ws_dyn [B,D] kept for stage 2.
template <typename T>
__global__ __launch_bounds__(256) void head_bwd_rows_kernel(const float* __restrict__ dlogits, const float* __restrict__ Wh,
                                                            const float* __restrict__ gamma, const float* __restrict__ ws_xhat,
                                                            const float* __restrict__ ws_rstd, float* __restrict__ ws_dyn,
                                                            T* __restrict__ dx, int B, int Ntok, int D, int Cn) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float invD = 1.0f / (float)D;
  for (int b = blockIdx.x * 4 + wave; b < B; b += gridDim.x * 4) {
    float s1 = 0.f, s2 = 0.f;
    for (int d = lane; d < D; d += 64) {
      float dyn = 0.f;
      for (int k = 0; k < Cn; ++k) dyn += dlogits[(size_t)b * Cn + k] * Wh[(size_t)k * D + d];
      ws_dyn[(size_t)b * D + d] = dyn;
      const float gv = dyn * gamma[d];
      s1 += gv;
      s2 += gv * ws_xhat[(size_t)b * D + d];
    }
    s1 = wave_sum(s1) * invD;
    s2 = wave_sum(s2) * invD;
    const float rstd = ws_rstd[b];
    T* drow = dx + (size_t)b * Ntok * D;
    for (int d = lane; d < D; d += 64) {
      const float gv = ws_dyn[(size_t)b * D + d] * gamma[d];
      drow[d] = from_f32<T>(rstd * (gv - s1 - ws_xhat[(size_t)b * D + d] * s2));
    }
    if (D % CH<T>::n == 0) {   // rows 1.. are zero: 16-B stores
      const Chunk16 z16 = {0u, 0u, 0u, 0u};
      for (size_t q = D / CH<T>::n + lane; q < (size_t)Ntok * D / CH<T>::n; q += 64)
        *reinterpret_cast<Chunk16*>(drow + q * CH<T>::n) = z16;
    } else {
      for (size_t q = D + lane; q < (size_t)Ntok * D; q += 64) drow[q] = from_f32<T>(0.f);
    }
  }
}
// stage 2: column sums over the batch, split over batch chunks (blockIdx.y) + fp32 atomics.
//   dWh[k][d] += sum_b dlogits[b][k]*yn[b][d] ; dbh[k] += sum_b dlogits[b][k]
//   dgamma[d] += sum_b dyn*xhat ; dbeta[d] += sum_b dyn
// per_image (nullable, with out2 / metric_acc): [B,2] (loss, correct) of vitpe_head_step's images, summed in fixed
// order by workgroup (0,0) into out2 and added to metric_acc.
__global__ void head_bwd_params_kernel(const float* __restrict__ dlogits, const float* __restrict__ ws_yn,
                                       const float* __restrict__ ws_dyn, const float* __restrict__ ws_xhat,
                                       float* dWh, float* dbh, float* dgamma, float* dbeta, int B, int D, int Cn,
                                       int bchunk, const float* __restrict__ per_image, float* out2, float* metric_acc,
                                       float* hp_tick) {
  if (hp_tick != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    adamw_tick(hp_tick);   // adamw_tick_kernel's work (optim.hip): one launch less per step
  }
  if (per_image != nullptr && blockIdx.x == 0 && blockIdx.y == 0) {
    __shared__ float sl[256], sc[256];
    float l = 0.f, cr = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) { l += per_image[2 * b]; cr += per_image[2 * b + 1]; }
    sl[threadIdx.x] = l;
    sc[threadIdx.x] = cr;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
      if (threadIdx.x < o) { sl[threadIdx.x] += sl[threadIdx.x + o]; sc[threadIdx.x] += sc[threadIdx.x + o]; }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      out2[0] = sl[0]; out2[1] = sc[0];
      if (metric_acc != nullptr) { metric_acc[0] += sl[0]; metric_acc[1] += sc[0]; }
    }
  }
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int b0 = blockIdx.y * bchunk, b1 = min(B, b0 + bchunk);
  const int nW = Cn * D;
  if (idx < nW) {
    const int k = idx / D, d = idx % D;
    float s = 0.f;
    for (int b = b0; b < b1; ++b) s += dlogits[(size_t)b * Cn + k] * ws_yn[(size_t)b * D + d];
    atomicAdd(dWh + idx, s);
  } else if (idx < nW + Cn) {
    const int k = idx - nW;
    float s = 0.f;
    for (int b = b0; b < b1; ++b) s += dlogits[(size_t)b * Cn + k];
    atomicAdd(dbh + k, s);
  } else if (idx < nW + Cn + D) {
    const int d = idx - nW - Cn;
    float sg = 0.f, sb = 0.f;
    for (int b = b0; b < b1; ++b) {
      const float dy = ws_dyn[(size_t)b * D + d];
      sg += dy * ws_xhat[(size_t)b * D + d];
      sb += dy;
    }
    atomicAdd(dgamma + d, sg);
    atomicAdd(dbeta + d, sb);
  }
}

// patch-embed parameter gradients that are plain column sums of the token gradient:
//   dcls[d] += sum_b dtok[b,0,d] ; dape[p][d] += sum_b dtok[b,1+p,d]   (vit.py:253-258)
// and repacking of the patch-token gradient rows into the GEMM layout [B*P, D]
template <typename T>
__global__ void embed_bwd_kernel(const T* __restrict__ dtok, float* dcls, float* dape, T* __restrict__ dpatch,
                                 int B, int Ntok, int D, int bchunk) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // over Ntok*D ; blockIdx.y over batch chunks
  if (idx >= Ntok * D) return;
  const int n = idx / D, d = idx % D;
  const int b0 = blockIdx.y * bchunk, b1 = min(B, b0 + bchunk);
  float s = 0.f;
  for (int b = b0; b < b1; ++b) {
    const T v = dtok[((size_t)b * Ntok + n) * D + d];
    s += to_f32(v);
    if (n >= 1) dpatch[((size_t)b * (Ntok - 1) + n - 1) * D + d] = v;
  }
  if (n == 0) atomicAdd(dcls + d, s);
  else if (dape) atomicAdd(dape + (size_t)(n - 1) * D + d, s);
}

template <typename T>
__global__ void cast_kernel(const float* __restrict__ src, T* __restrict__ dst, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    dst[i] = from_f32<T>(src[i]);
}
// dst[c][r] = (T) src[r][c]  -- transposed weight shadows for the data-gradient GEMMs
template <typename T>
__global__ void transpose_cast_kernel(const float* __restrict__ src, T* __restrict__ dst, int R, int Cc) {
  __shared__ float tile[32][33];
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + threadIdx.x;
    tile[i][threadIdx.x] = (r < R && c < Cc) ? src[(size_t)r * Cc + c] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int c = c0 + i, r = r0 + threadIdx.x;
    if (c < Cc && r < R) dst[(size_t)c * R + r] = from_f32<T>(tile[threadIdx.x][i]);
  }
}

// All weight shadows of the model in ONE launch (after the optimizer step): a descriptor per matrix,
// each workgroup handles one 32x32 tile.  kind 0: dst[c][r] = src[r][c] (transposed shadow for the
// data-gradient GEMMs); kind 1: fragment-major packing of attn.qkv.weight (see pack_qkv_kernel); kind 2 / 3: the
// fragment-major packing of tail2.hip (natural / acc_to_frag k order, HD field = k chunk); kind 4 / 5: the same of W^T;
// kind 6: the wide qkv pack of attn32.hip (HD field = head dim = 32).
// A descriptor may name a SECOND shadow of the same matrix (kind2 >= 0): the source tile is loaded once for both (a weight
// and its transpose packs, the qkv pack and its transposed pack).  tile_map[block] = descriptor index (host-built; without
// it every block scans the descriptor list -- 48 dependent-latency loads per block were most of this kernel's time).
struct ShadowDesc { long long src_off, dst_off, dst_off2; int R, C, tile0, kind, HD, kind2, HD2, pad; };

template <typename T>
__global__ __launch_bounds__(256) void refresh_shadows_kernel(const float* __restrict__ flat, T* __restrict__ dst_base,
                                                              const ShadowDesc* __restrict__ desc, int ndesc,
                                                              const unsigned short* __restrict__ tile_map) {
  __shared__ float tile[32][33];
  int d = 0;
  if (tile_map != nullptr) {
    d = tile_map[blockIdx.x];
  } else {
    for (int i = 1; i < ndesc; ++i)
      if ((int)blockIdx.x >= desc[i].tile0) d = i;   // wave-uniform scan of a handful of descriptors
  }
  const ShadowDesc ds = desc[d];
  const int t = blockIdx.x - ds.tile0;
  const int tc = (ds.C + 31) / 32;
  const int r0 = (t / tc) * 32, c0 = (t % tc) * 32;
  const float* src = flat + ds.src_off;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int r = r0 + i, c = c0 + tx;
    tile[i][tx] = (r < ds.R && c < ds.C) ? src[(size_t)r * ds.C + c] : 0.f;
  }
  __syncthreads();
  auto emit = [&](int kind, T* dst, int hd) {
    if (kind == 0) {
      for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (c < ds.C && r < ds.R) dst[(size_t)c * ds.R + r] = from_f32<T>(tile[tx][i]);
      }
    } else if (kind == 6) {
      // wide pack of attn.qkv.weight (csrc/attn32.hip, vitpe_pack_qkv_weights_wide): block ((h * 3 + mat) * (D / 16) + s),
      // lane (r = row % 32) + 32 * hh, element j <- W[mat D + 32 h + r][16 s + 8 hh + j]; q rows x hd^-0.5 log2(e)
      const int D = ds.C, S = D / 16;
      const float qs = 1.4426950408889634f * rsqrtf((float)hd);
      for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        if (r < ds.R && c < ds.C) {
          const int mat = r / D, rr = r % D, h = rr / 32, f = rr % 32;
          const int sidx = c / 16, hh = (c % 16) / 8, e = c % 8;
          const size_t blk = ((size_t)(h * 3 + mat) * S + sidx);
          dst[(blk * 64 + f + 32 * hh) * 8 + e] = from_f32<T>(tile[i][tx] * (mat == 0 ? qs : 1.0f));
        }
      }
    } else if (kind >= 2) {
      // vitpe_pack_weight_frags layout (tail2.hip): hd = k chunk; kinds 2 / 3 pack W itself in natural / acc_to_frag
      // k order, kinds 4 / 5 pack W^T (the backward kernels' operands) the same two ways.
      // A 32x32 tile is exactly two 1-KB fragments (output tiles p0/16, p0/16 + 1 of one k step): every thread writes 4
      // consecutive destination elements (both dimensions are multiples of 32 for these matrices).
      const bool tr = kind >= 4, phi = (kind & 1) != 0;
      const int PR = tr ? ds.C : ds.R;                       // rows of the packed matrix
      const int p0 = tr ? c0 : r0, k0 = tr ? r0 : c0;        // its row / column origin of this tile
      const int kch = hd, KSC = kch / 32, NTr = PR / 16;
      const int kc = k0 / kch, ks = (k0 % kch) / 32;
      const int dd = threadIdx.x * 4, frag = dd >> 9, within = dd & 511, l = within >> 3, e0 = within & 7;
      const int nt = p0 / 16 + frag, cc = l & 15, g = l >> 4;
      if (16 * nt < PR) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = e0 + j;
          const int k = phi ? (e < 4 ? 4 * g + e : 16 + 4 * g + e - 4) : 8 * g + e;
          v[j] = tr ? tile[k][16 * frag + cc] : tile[16 * frag + cc][k];
        }
        const size_t blk = ((size_t)kc * NTr + nt) * KSC + ks;
        st4(dst + blk * 512 + within, v[0], v[1], v[2], v[3]);
      }
    } else {
      // W[3D, D]: row = mat*D + h*HD + 16nt + cc ; col = 32ks + 8g + e  ->  block (h,mat,nt,ks), lane 16g+cc, e
      const int D = ds.C, HD = hd, NT = HD / 16, KS = D / 32;
      for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        if (r < ds.R && c < ds.C) {
          const int mat = r / D, rr = r % D, h = rr / HD, nt = (rr % HD) / 16, cc = rr % 16;
          const int ks = c / 32, g = (c % 32) / 8, e = c % 8;
          const size_t blk = (((size_t)(h * 3 + mat) * NT + nt) * KS + ks);
          dst[(blk * 64 + 16 * g + cc) * 8 + e] = from_f32<T>(tile[i][tx]);
        }
      }
    }
  };
  emit(ds.kind, dst_base + ds.dst_off, ds.HD);
  if (ds.kind2 >= 0) emit(ds.kind2, dst_base + ds.dst_off2, ds.HD2);
}

// ---------------------------------------------------------------------------------------
// Self-tests of the primitives every kernel relies on (run by tests/ on the GPU box):
//  C[16x16] = A[16x32] * B[32x16] through mma<T>, with A given row-major [16][32] and B either
//  as B^T row-major [16][32] (row fragments) or as B row-major [32][16] read through ld_frag_tr.
template <typename T>
__global__ void selftest_mma_kernel(const T* __restrict__ A, const T* __restrict__ Bt, const T* __restrict__ Brow,
                                    float* __restrict__ C_row, float* __restrict__ C_tr) {
  __shared__ __attribute__((aligned(16))) T sB[32 * 24];  // row-major [32][16], ld 24
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  for (int q = lane; q < 32 * 16; q += 64) sB[(q / 16) * 24 + (q % 16)] = Brow[q];
  __syncthreads();
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  mma(ld_frag(A + c * 32 + 8 * g), ld_frag(Bt + c * 32 + 8 * g), acc);
  for (int r = 0; r < 4; ++r) C_row[(4 * g + r) * 16 + c] = acc[r];
  f32x4 acc2 = {0.f, 0.f, 0.f, 0.f};
  mma(ld_frag(A + c * 32 + 8 * g), ld_frag_tr(sB, 24, 8 * g, 8 * g + 4, 0), acc2);
  for (int r = 0; r < 4; ++r) C_tr[(4 * g + r) * 16 + c] = acc2[r];
}

}  // namespace vitpe

using namespace vitpe;

#define GRID1D(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256)

extern "C" int vitpe_unfold(int dtype, const float* img, void* patches, int B, int C, int S, int p, hipStream_t st) {
  VITPE_REQUIRE(img && patches && B >= 0 && C > 0 && p > 0 && S % p == 0 && (dtype == 0 || dtype == 1));
  const long long total = (long long)B * (S / p) * (S / p) * C * p;
  if (total == 0) return 0;
  const unsigned blocks = (unsigned)min((total + 255) / 256, (long long)8192);
  if (dtype == 1 && p % 8 == 0) {   // (image rows are S fp32 = a multiple of 32 B, patch rows p^2 bf16: every piece is 16-B aligned)
    const long long total8 = total * (p / 8);
    hipLaunchKernelGGL(unfold8_kernel, dim3((unsigned)min((total8 + 255) / 256, (long long)16384)), dim3(256), 0, st, img,
                       (bf16*)patches, B, C, S, p);
    VITPE_CHECK_LAUNCH();
  }
  if (dtype == 1) hipLaunchKernelGGL(unfold_kernel<bf16>, dim3(blocks), dim3(256), 0, st, img, (bf16*)patches, B, C, S, p);
  else hipLaunchKernelGGL(unfold_kernel<float>, dim3(blocks), dim3(256), 0, st, img, (float*)patches, B, C, S, p);
  VITPE_CHECK_LAUNCH();
}

static int launch_unfold_u8(int dtype, const unsigned char* data, const long long* index, const float* mean,
                            const float* stdv, void* patches, float* img_out, int B, int C, int S, int p,
                            const unsigned long long* rng, int pad, int hflip, hipStream_t st) {
  VITPE_REQUIRE(data && mean && stdv && patches && B >= 0 && C > 0 && p > 0 && S % p == 0 && (dtype == 0 || dtype == 1));
  VITPE_REQUIRE(rng == nullptr || (pad >= 0 && pad <= S));
  const long long total = (long long)B * (S / p) * (S / p) * C * p;
  if (total == 0) return 0;
  const unsigned blocks = (unsigned)min((total + 255) / 256, (long long)8192);
  if (rng != nullptr) {
    if (dtype == 1)
      hipLaunchKernelGGL((unfold_u8_kernel<bf16, true>), dim3(blocks), dim3(256), 0, st, data, index, mean, stdv, (bf16*)patches, img_out, B, C, S, p, rng, pad, hflip);
    else
      hipLaunchKernelGGL((unfold_u8_kernel<float, true>), dim3(blocks), dim3(256), 0, st, data, index, mean, stdv, (float*)patches, img_out, B, C, S, p, rng, pad, hflip);
  } else {
    if (dtype == 1)
      hipLaunchKernelGGL((unfold_u8_kernel<bf16, false>), dim3(blocks), dim3(256), 0, st, data, index, mean, stdv, (bf16*)patches, img_out, B, C, S, p, rng, 0, 0);
    else
      hipLaunchKernelGGL((unfold_u8_kernel<float, false>), dim3(blocks), dim3(256), 0, st, data, index, mean, stdv, (float*)patches, img_out, B, C, S, p, rng, 0, 0);
  }
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_unfold_u8(int dtype, const unsigned char* data, const long long* index, const float* mean,
                               const float* stdv, void* patches, float* img_out, int B, int C, int S, int p,
                               hipStream_t st) {
  return launch_unfold_u8(dtype, data, index, mean, stdv, patches, img_out, B, C, S, p, nullptr, 0, 0, st);
}

// the same with the augmentation stream (rng NULL: exactly vitpe_unfold_u8)
extern "C" int vitpe_unfold_u8_aug(int dtype, const unsigned char* data, const long long* index, const float* mean,
                                   const float* stdv, void* patches, float* img_out, int B, int C, int S, int p,
                                   const unsigned long long* rng, int pad, int hflip, hipStream_t st) {
  return launch_unfold_u8(dtype, data, index, mean, stdv, patches, img_out, B, C, S, p, rng, pad, hflip, st);
}

extern "C" int vitpe_augment_params(const unsigned long long* rng, int* out, int B, int pad, int hflip, hipStream_t st) {
  VITPE_REQUIRE(rng && B >= 0 && (out || B == 0) && pad >= 0);
  if (B == 0) return 0;
  hipLaunchKernelGGL(augment_params_kernel, GRID1D(B), 0, st, rng, out, B, pad, hflip);
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_relative_position_index(long long* out, int L, hipStream_t st) {
  VITPE_REQUIRE(out && L > 0);
  hipLaunchKernelGGL(rel_index_kernel, GRID1D(L * L), 0, st, out, L);
  VITPE_CHECK_LAUNCH();
}
extern "C" int vitpe_l1_distance_matrix(long long* out, int G, hipStream_t st) {
  VITPE_REQUIRE(out && G > 0);
  hipLaunchKernelGGL(l1_matrix_kernel, GRID1D(G * G * G * G), 0, st, out, G);
  VITPE_CHECK_LAUNCH();
}
extern "C" int vitpe_rope_axial_tables(const float* inv_freq, float* cosv, float* sinv, int G, int half, hipStream_t st) {
  VITPE_REQUIRE(inv_freq && cosv && sinv && G > 0 && half > 0 && half % 2 == 0);
  hipLaunchKernelGGL(rope_axial_kernel, GRID1D(G * G * half), 0, st, inv_freq, cosv, sinv, G, half);
  VITPE_CHECK_LAUNCH();
}
extern "C" int vitpe_rope_mixed_tables(const float* freqs, float* cosv, float* sinv, int H, int G, int half, hipStream_t st) {
  VITPE_REQUIRE(freqs && cosv && sinv && H > 0 && G > 0 && half > 0);
  hipLaunchKernelGGL(rope_mixed_kernel, GRID1D(H * G * G * half), 0, st, freqs, cosv, sinv, H, G, half);
  VITPE_CHECK_LAUNCH();
}
extern "C" int vitpe_relative_bias(const float* table, float* out, int H, int L, hipStream_t st) {
  VITPE_REQUIRE(table && out && H > 0 && L > 0);
  hipLaunchKernelGGL(rel_bias_kernel, GRID1D(H * L * L), 0, st, table, out, H, L);
  VITPE_CHECK_LAUNCH();
}
extern "C" int vitpe_polynomial_bias(const float* coeff, float* out, int H, int G, int degree, int per_head, hipStream_t st) {
  VITPE_REQUIRE(coeff && out && H > 0 && G > 0 && degree >= 0);
  const int L = G * G + 1;
  hipLaunchKernelGGL(poly_bias_kernel, GRID1D(H * L * L), 0, st, coeff, out, H, G, degree, per_head);
  VITPE_CHECK_LAUNCH();
}
extern "C" int vitpe_relative_bias_bwd(const float* dbias, float* dtable, int H, int L, hipStream_t st) {
  VITPE_REQUIRE(dbias && dtable && H > 0 && L > 0);
  hipLaunchKernelGGL(rel_bias_bwd_kernel, GRID1D(H * (2 * L - 1)), 0, st, dbias, dtable, H, L);
  VITPE_CHECK_LAUNCH();
}
extern "C" int vitpe_polynomial_bias_bwd(const float* dbias, float* dcoeff, int H, int G, int degree, int per_head,
                                         hipStream_t st) {
  VITPE_REQUIRE(dbias && dcoeff && H > 0 && G > 0 && degree >= 0);
  hipLaunchKernelGGL(poly_bias_bwd_kernel, dim3((per_head ? H : 1) * (degree + 1)), dim3(256), 0, st, dbias, dcoeff, H, G,
                     degree, per_head);
  VITPE_CHECK_LAUNCH();
}
extern "C" int vitpe_rope_mixed_tables_bwd(const float* freqs, const float* dcos, const float* dsin, float* dfreqs, int H,
                                           int G, int half, hipStream_t st) {
  VITPE_REQUIRE(freqs && dcos && dsin && dfreqs && H > 0 && G > 0 && half > 0);
  hipLaunchKernelGGL(rope_mixed_bwd_kernel, GRID1D(2 * H * half), 0, st, freqs, dcos, dsin, dfreqs, H, G, half);
  VITPE_CHECK_LAUNCH();
}
extern "C" int vitpe_apply_rotary(const float* x, float* y, const float* cosv, const float* sinv, int B, int H, int P,
                                  int HD, int per_head, hipStream_t st) {
  VITPE_REQUIRE(x && y && cosv && sinv && B >= 0 && H > 0 && P > 0 && HD > 0 && HD % 2 == 0);
  const long long total = (long long)B * H * P * (HD / 2);
  if (total == 0) return 0;
  hipLaunchKernelGGL(rotary_kernel, GRID1D(total), 0, st, x, y, cosv, sinv, total, H, P, HD / 2, per_head);
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_head_fwd(int dtype, const void* x, const float* gamma, const float* beta, const float* Wh,
                              const float* bh, float* logits, float* ws_xhat, float* ws_yn, float* ws_rstd, int B,
                              int Ntok, int D, int Cn, float eps, hipStream_t st) {
  VITPE_REQUIRE(x && gamma && beta && Wh && bh && logits && B >= 0 && (dtype == 0 || dtype == 1));
  VITPE_REQUIRE((ws_xhat == nullptr) == (ws_yn == nullptr) && (ws_xhat == nullptr) == (ws_rstd == nullptr));
  if (B == 0) return 0;
  const int blocks = min((B + 3) / 4, 1024);
  if (dtype == 1)
    hipLaunchKernelGGL(head_fwd_kernel<bf16>, dim3(blocks), dim3(256), 0, st, (const bf16*)x, gamma, beta, Wh, bh,
                       logits, ws_xhat, ws_yn, ws_rstd, B, Ntok, D, Cn, eps);
  else
    hipLaunchKernelGGL(head_fwd_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)x, gamma, beta, Wh, bh,
                       logits, ws_xhat, ws_yn, ws_rstd, B, Ntok, D, Cn, eps);
  VITPE_CHECK_LAUNCH();
}
extern "C" int vitpe_cross_entropy(const float* logits, const long long* labels, float* dlogits, float* out2, int B,
                                   int Cn, float grad_scale, hipStream_t st) {
  VITPE_REQUIRE(logits && labels && out2 && B > 0 && Cn > 0);
  hipLaunchKernelGGL(ce_kernel, dim3(1), dim3(256), 0, st, logits, labels, dlogits, out2, B, Cn, grad_scale,
                     (const float*)nullptr, (float*)nullptr);
  VITPE_CHECK_LAUNCH();
}
extern "C" int vitpe_cross_entropy_ctl(const float* logits, const long long* labels, float* dlogits, float* out2,
                                       float* metric_acc, const float* ctl, int B, int Cn, hipStream_t st) {
  VITPE_REQUIRE(logits && labels && out2 && ctl && B > 0 && Cn > 0);
  hipLaunchKernelGGL(ce_kernel, dim3(1), dim3(256), 0, st, logits, labels, dlogits, out2, B, Cn, 0.f, ctl, metric_acc);
  VITPE_CHECK_LAUNCH();
}
extern "C" int vitpe_head_bwd(int dtype, const float* dlogits, const float* Wh, const float* gamma,
                              const float* ws_xhat, const float* ws_yn, const float* ws_rstd, float* ws_dyn, void* dx,
                              float* dWh, float* dbh, float* dgamma, float* dbeta, int B, int Ntok, int D, int Cn,
                              hipStream_t st) {
  VITPE_REQUIRE(dlogits && Wh && gamma && ws_xhat && ws_yn && ws_rstd && ws_dyn && dx && dWh && dbh && dgamma && dbeta);
  VITPE_REQUIRE(B >= 0 && (dtype == 0 || dtype == 1));
  if (B == 0) return 0;
  const int blocks = min((B + 3) / 4, 1024);
  if (dtype == 1)
    hipLaunchKernelGGL(head_bwd_rows_kernel<bf16>, dim3(blocks), dim3(256), 0, st, dlogits, Wh, gamma, ws_xhat,
                       ws_rstd, ws_dyn, (bf16*)dx, B, Ntok, D, Cn);
  else
    hipLaunchKernelGGL(head_bwd_rows_kernel<float>, dim3(blocks), dim3(256), 0, st, dlogits, Wh, gamma, ws_xhat,
                       ws_rstd, ws_dyn, (float*)dx, B, Ntok, D, Cn);
  int e = (int)hipGetLastError();
  if (e) return e;
  hipLaunchKernelGGL(head_bwd_params_kernel, dim3((Cn * D + Cn + D + 255) / 256, (B + 31) / 32), dim3(256), 0, st,
                     dlogits, ws_yn, ws_dyn, ws_xhat, dWh, dbh, dgamma, dbeta, B, D, Cn, 32, (const float*)nullptr, (float*)nullptr, (float*)nullptr,
                     (float*)nullptr);
  VITPE_CHECK_LAUNCH();
}
template <typename T>
static int head_step_launch(const T* x, const float* gamma, const float* beta, const float* Wh, const float* bh,
                            const long long* labels, float* logits, float* dlogits, float* ws_xhat, float* ws_yn,
                            float* ws_dyn, T* dx, float* per_image, const float* ctl, int B, int Ntok, int D, int Cn,
                            float eps, hipStream_t st) {
  const dim3 grid((B + 3) / 4), block(256);
#define VITPE_HEAD_STEP(KD)                                                                                              \
  do {                                                                                                                   \
    if (Cn * D <= 16 * 768)                                                                                              \
      hipLaunchKernelGGL((head_step_kernel<T, KD, true>), grid, block, 0, st, x, gamma, beta, Wh, bh, labels, logits,    \
                         dlogits, ws_xhat, ws_yn, ws_dyn, dx, per_image, ctl, B, Ntok, D, Cn, eps);                      \
    else                                                                                                                 \
      hipLaunchKernelGGL((head_step_kernel<T, KD, false>), grid, block, 0, st, x, gamma, beta, Wh, bh, labels, logits,   \
                         dlogits, ws_xhat, ws_yn, ws_dyn, dx, per_image, ctl, B, Ntok, D, Cn, eps);                      \
  } while (0)
  const int kd = (D + 63) / 64;
  if (kd <= 2) VITPE_HEAD_STEP(2);
  else if (kd == 3) VITPE_HEAD_STEP(3);
  else if (kd <= 6) VITPE_HEAD_STEP(6);
  else if (kd <= 12) VITPE_HEAD_STEP(12);
  else return (int)hipErrorNotSupported;
#undef VITPE_HEAD_STEP
  return (int)hipGetLastError();
}
extern "C" int vitpe_head_step(int dtype, const void* x, const float* gamma, const float* beta, const float* Wh,
                               const float* bh, const long long* labels, float* logits, float* dlogits, float* ws_xhat,
                               float* ws_yn, float* ws_dyn, void* dx, float* out2, float* metric_acc, float* per_image,
                               const float* ctl, float* dWh, float* dbh, float* dgamma, float* dbeta, int B, int Ntok,
                               int D, int Cn, float eps, float* hp_tick, hipStream_t st) {
  VITPE_REQUIRE(x && gamma && beta && Wh && bh && labels && logits && dlogits && ws_xhat && ws_yn && ws_dyn && dx && out2 &&
                per_image && ctl && dWh && dbh && dgamma && dbeta && B >= 0 && (dtype == 0 || dtype == 1));
  if (Cn < 1 || Cn > 64 || D > 768) return (int)hipErrorNotSupported;
  if (B == 0) return 0;
  int e = dtype == 1 ? head_step_launch<bf16>((const bf16*)x, gamma, beta, Wh, bh, labels, logits, dlogits, ws_xhat, ws_yn,
                                              ws_dyn, (bf16*)dx, per_image, ctl, B, Ntok, D, Cn, eps, st)
                     : head_step_launch<float>((const float*)x, gamma, beta, Wh, bh, labels, logits, dlogits, ws_xhat, ws_yn,
                                               ws_dyn, (float*)dx, per_image, ctl, B, Ntok, D, Cn, eps, st);
  if (e) return e;
  hipLaunchKernelGGL(head_bwd_params_kernel, dim3((Cn * D + Cn + D + 255) / 256, (B + 31) / 32), dim3(256), 0, st,
                     dlogits, ws_yn, ws_dyn, ws_xhat, dWh, dbh, dgamma, dbeta, B, D, Cn, 32, (const float*)per_image, out2,
                     metric_acc, hp_tick);
  VITPE_CHECK_LAUNCH();
}
extern "C" int vitpe_embed_bwd(int dtype, const void* dtok, float* dcls, float* dape, void* dpatch, int B, int Ntok,
                               int D, hipStream_t st) {
  VITPE_REQUIRE(dtok && dcls && dpatch && B >= 0 && (dtype == 0 || dtype == 1));
  if (dtype == 1)
    hipLaunchKernelGGL(embed_bwd_kernel<bf16>, dim3((Ntok * D + 255) / 256, (B + 15) / 16), dim3(256), 0, st,
                       (const bf16*)dtok, dcls, dape, (bf16*)dpatch, B, Ntok, D, 16);
  else
    hipLaunchKernelGGL(embed_bwd_kernel<float>, dim3((Ntok * D + 255) / 256, (B + 15) / 16), dim3(256), 0, st,
                       (const float*)dtok, dcls, dape, (float*)dpatch, B, Ntok, D, 16);
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_cast(int dtype, const float* src, void* dst, long long n, hipStream_t st) {
  VITPE_REQUIRE(src && dst && n >= 0 && (dtype == 0 || dtype == 1));
  if (n == 0) return 0;
  const unsigned blocks = (unsigned)min((n + 255) / 256, (long long)4096);
  if (dtype == 1) hipLaunchKernelGGL(cast_kernel<bf16>, dim3(blocks), dim3(256), 0, st, src, (bf16*)dst, n);
  else hipLaunchKernelGGL(cast_kernel<float>, dim3(blocks), dim3(256), 0, st, src, (float*)dst, n);
  VITPE_CHECK_LAUNCH();
}
extern "C" int vitpe_transpose_cast(int dtype, const float* src, void* dst, int R, int C, hipStream_t st) {
  VITPE_REQUIRE(src && dst && R > 0 && C > 0 && (dtype == 0 || dtype == 1));
  dim3 grid((C + 31) / 32, (R + 31) / 32), block(32, 8);
  if (dtype == 1) hipLaunchKernelGGL(transpose_cast_kernel<bf16>, grid, block, 0, st, src, (bf16*)dst, R, C);
  else hipLaunchKernelGGL(transpose_cast_kernel<float>, grid, block, 0, st, src, (float*)dst, R, C);
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_refresh_shadows(int dtype, const float* flat, void* dst_base, const void* desc, int ndesc,
                                     int total_tiles, const unsigned short* tile_map, hipStream_t st) {
  VITPE_REQUIRE(flat && dst_base && desc && ndesc > 0 && total_tiles > 0 && (dtype == 0 || dtype == 1));
  if (dtype == 1)
    hipLaunchKernelGGL(refresh_shadows_kernel<bf16>, dim3(total_tiles), dim3(256), 0, st, flat, (bf16*)dst_base,
                       (const ShadowDesc*)desc, ndesc, tile_map);
  else
    hipLaunchKernelGGL(refresh_shadows_kernel<float>, dim3(total_tiles), dim3(256), 0, st, flat, (float*)dst_base,
                       (const ShadowDesc*)desc, ndesc, tile_map);
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_selftest_mma(int dtype, const void* A, const void* Bt, const void* Brow, float* C_row, float* C_tr,
                                  hipStream_t st) {
  VITPE_REQUIRE(A && Bt && Brow && C_row && C_tr && (dtype == 0 || dtype == 1));
  if (dtype == 1)
    hipLaunchKernelGGL(selftest_mma_kernel<bf16>, dim3(1), dim3(64), 0, st, (const bf16*)A, (const bf16*)Bt,
                       (const bf16*)Brow, C_row, C_tr);
  else
    hipLaunchKernelGGL(selftest_mma_kernel<float>, dim3(1), dim3(64), 0, st, (const float*)A, (const float*)Bt,
                       (const float*)Brow, C_row, C_tr);
  VITPE_CHECK_LAUNCH();
}

// debug: what the memory system gives a kernel that ONLY reads -- `bytes` streamed with 16-B loads, `depth` independent
// loads in flight per lane, one workgroup of 256 threads per 256 * depth * 16 B; nothing written unless the xor of all
// words is a magic value (it never is).  tools/membw.py: the read ceiling the weight-gradient kernel is measured against.
template <int DEPTH>
__global__ __launch_bounds__(256) void read_bw_kernel(const uint4* __restrict__ src, long long nvec, unsigned* sink) {
  const long long stride = (long long)gridDim.x * 256;
  unsigned acc = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride * DEPTH) {
    uint4 v[DEPTH];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) v[d] = (i + d * stride < nvec) ? src[i + d * stride] : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) acc ^= v[d].x ^ v[d].y ^ v[d].z ^ v[d].w;
  }
  if (acc == 0x9E3779B9u) *sink = acc;
}
extern "C" int vitpe_debug_read_bw(const void* src, long long bytes, int depth, int workgroups, unsigned* sink, hipStream_t st) {
  VITPE_REQUIRE(src && sink && bytes >= 16 && workgroups > 0 && (depth == 1 || depth == 4 || depth == 8));
  const long long nvec = bytes / 16;
  if (depth == 1) hipLaunchKernelGGL(read_bw_kernel<1>, dim3(workgroups), dim3(256), 0, st, (const uint4*)src, nvec, sink);
  else if (depth == 4) hipLaunchKernelGGL(read_bw_kernel<4>, dim3(workgroups), dim3(256), 0, st, (const uint4*)src, nvec, sink);
  else hipLaunchKernelGGL(read_bw_kernel<8>, dim3(workgroups), dim3(256), 0, st, (const uint4*)src, nvec, sink);
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_abi_version(void) { return 5; }   // 5: - vitpe_head_loss, vitpe_reduce_partials (retired: no caller)
