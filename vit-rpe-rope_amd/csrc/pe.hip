// Positional-encoding tables (reference models/positional_encoding.py): the integer index tables, the RoPE cos / sin
// tables, the materialised relative / polynomial biases of the get_bias() API surface, and the transposes of the three
// float builders for the stand-alone modules' autograd.  None of it is on the train step's hot path except
// rope_mixed_kernel, which follows the learnable frequencies once per forward.
#include "common.h"

namespace vitpe {

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

}  // namespace vitpe

using namespace vitpe;

#define GRID1D(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256)

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
