// Dropout on the Philox stream of philox.h ("Dropout streams"): the elementwise site (torch.nn.Dropout as the
// reference places it -- attn.proj_drop, vit.py:14-98, and timm Mlp's drop1 / drop2), the per-sample site (timm DropPath,
// scale_by_keep=True: reference vit.py:115,122,124 with drop_path > 0) and the keep masks of every site for the tests.
// Nothing stores a mask: the backward regenerates the forward's decisions from the same (seed, offset) pair, which the
// kernels read from device memory -- a captured graph replays with whatever the pair holds then.
#include "common.h"
#include "philox.h"

namespace vitpe {

// one thread per four consecutive elements (one Philox call); VEC: 16-byte-aligned (fp32) / 8-byte-aligned (bf16) quads
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void dropout_kernel(const T* __restrict__ x, const T* __restrict__ resid, T* __restrict__ y,
                                                      long long n, const unsigned long long* __restrict__ rng, uint32_t thr,
                                                      float rs) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long e0 = 4 * q;
  if (e0 >= n) return;
  const Philox4 w = drop_words(drop_key(rng), (uint64_t)q);
  if (VEC && e0 + 4 <= n) {
    f32x4 v = ld4(x + e0);
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (resid) r = ld4(resid + e0);
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = r[t] + (w.w[t] >= thr ? v[t] * rs : 0.f);
    st4(y + e0, v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (e0 + t < n) {
        const float r = resid ? to_f32(resid[e0 + t]) : 0.f;
        y[e0 + t] = from_f32<T>(r + (w.w[t] >= thr ? to_f32(x[e0 + t]) * rs : 0.f));
      }
  }
}

// per-sample decision (element e = b): sample b of `per` elements, y = resid + x * m_b * rs; workgroup blockIdx.x handles
// slice blockIdx.x % slices of sample blockIdx.x / slices
template <typename T>
__global__ __launch_bounds__(256) void drop_path_kernel(const T* __restrict__ x, const T* __restrict__ resid, T* __restrict__ y,
                                                        long long per, int slices, const unsigned long long* __restrict__ rng,
                                                        uint32_t thr, float rs) {
  const int b = blockIdx.x / slices, sl = blockIdx.x % slices;
  const Philox4 w = drop_words(drop_key(rng), (uint64_t)(b >> 2));
  const float f = w.w[b & 3] >= thr ? rs : 0.f;
  const size_t base = (size_t)b * per;
  for (long long i = (long long)sl * 256 + threadIdx.x; i < per; i += (long long)slices * 256) {
    const float r = resid ? to_f32(resid[base + i]) : 0.f;
    y[base + i] = from_f32<T>(r + to_f32(x[base + i]) * f);
  }
}

// keep mask (1 = kept) of n consecutive elements
__global__ __launch_bounds__(256) void mask_linear_kernel(unsigned char* __restrict__ mask, long long n,
                                                          const unsigned long long* __restrict__ rng, uint32_t thr) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (4 * q >= n) return;
  const Philox4 w = drop_words(drop_key(rng), (uint64_t)q);
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (4 * q + t < n) mask[4 * q + t] = w.w[t] >= thr ? 1 : 0;
}

// keep mask [B,H,N,N] of the attention site: e = ((b H + h) N + i) NP + j, NP = N rounded up to a multiple of 4
__global__ __launch_bounds__(256) void mask_attn_kernel(unsigned char* __restrict__ mask, long long rows, int N,
                                                        const unsigned long long* __restrict__ rng, uint32_t thr) {
  const int NQ = (N + 3) / 4;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= rows * NQ) return;
  const long long row = t / NQ;
  const int jq = (int)(t % NQ);
  const Philox4 w = drop_words(drop_key(rng), (uint64_t)t);   // (row * NQ + jq)
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (4 * jq + k < N) mask[row * N + 4 * jq + k] = w.w[k] >= thr ? 1 : 0;
}

template <typename T>
static int launch_dropout(const void* x, const void* resid, void* y, long long n, const unsigned long long* rng, float p,
                          hipStream_t st) {
  const long long quads = (n + 3) / 4;
  const dim3 grid((unsigned)((quads + 255) / 256));
  const uintptr_t al = 4 * sizeof(T) - 1;
  const bool vec = !(((uintptr_t)x | (uintptr_t)y | (uintptr_t)resid) & al);
  const T* xp = static_cast<const T*>(x);
  const T* rp = static_cast<const T*>(resid);
  if (vec) hipLaunchKernelGGL((dropout_kernel<T, true>), grid, dim3(256), 0, st, xp, rp, static_cast<T*>(y), n, rng, drop_threshold(p), drop_scale(p));
  else hipLaunchKernelGGL((dropout_kernel<T, false>), grid, dim3(256), 0, st, xp, rp, static_cast<T*>(y), n, rng, drop_threshold(p), drop_scale(p));
  VITPE_CHECK_LAUNCH();
}

template <typename T>
static int launch_drop_path(const void* x, const void* resid, void* y, int B, long long per, const unsigned long long* rng,
                            float p, hipStream_t st) {
  long long gx = (per + 255) / 256;
  gx = gx > 64 ? 64 : gx;
  hipLaunchKernelGGL((drop_path_kernel<T>), dim3((unsigned)(gx * B)), dim3(256), 0, st, static_cast<const T*>(x),
                     static_cast<const T*>(resid), static_cast<T*>(y), per, (int)gx, rng, drop_threshold(p), drop_scale(p));
  VITPE_CHECK_LAUNCH();
}

}  // namespace vitpe

using namespace vitpe;

extern "C" int vitpe_philox4x32_10(const unsigned int* key2, const unsigned int* ctr4, unsigned int* out4) {
  VITPE_REQUIRE(key2 && ctr4 && out4);
  const Philox4 w = philox4x32_10(key2[0], key2[1], ctr4[0], ctr4[1], ctr4[2], ctr4[3]);
  for (int t = 0; t < 4; ++t) out4[t] = w.w[t];
  return 0;
}

extern "C" int vitpe_dropout_mask(int site, const unsigned long long* rng, unsigned char* mask, long long n, int B, int H,
                                  int N, float p, hipStream_t st) {
  VITPE_REQUIRE(rng && mask && drop_p_ok(p));
  if (site == 0 || site == 1) {   // elementwise / per-sample: n consecutive elements
    VITPE_REQUIRE(n >= 0);
    if (n == 0) return 0;
    hipLaunchKernelGGL(mask_linear_kernel, dim3((unsigned)(((n + 3) / 4 + 255) / 256)), dim3(256), 0, st, mask, n, rng,
                       drop_threshold(p));
    VITPE_CHECK_LAUNCH();
  }
  VITPE_REQUIRE(site == 2 && B >= 0 && H >= 1 && N >= 1);
  if (B == 0) return 0;
  const long long rows = (long long)B * H * N, work = rows * ((N + 3) / 4);
  hipLaunchKernelGGL(mask_attn_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, mask, rows, N, rng,
                     drop_threshold(p));
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_dropout_fwd(int dtype, const void* x, const void* resid, void* y, long long n,
                                 const unsigned long long* rng, float p, hipStream_t st) {
  VITPE_REQUIRE(x && y && rng && n >= 0 && drop_p_ok(p) && (dtype == 0 || dtype == 1));
  if (n == 0) return 0;
  return dtype == 1 ? launch_dropout<bf16>(x, resid, y, n, rng, p, st) : launch_dropout<float>(x, resid, y, n, rng, p, st);
}

extern "C" int vitpe_dropout_bwd(int dtype, const void* dy, void* dx, long long n, const unsigned long long* rng, float p,
                                 hipStream_t st) {
  return vitpe_dropout_fwd(dtype, dy, nullptr, dx, n, rng, p, st);   // dx = dy . m / (1 - p): the forward's own kernel
}

extern "C" int vitpe_drop_path_fwd(int dtype, const void* x, const void* resid, void* y, int B, long long per,
                                   const unsigned long long* rng, float p, hipStream_t st) {
  VITPE_REQUIRE(x && y && rng && B >= 0 && B <= (1 << 24) && per >= 0 && drop_p_ok(p) && (dtype == 0 || dtype == 1));
  if (B == 0 || per == 0) return 0;
  return dtype == 1 ? launch_drop_path<bf16>(x, resid, y, B, per, rng, p, st)
                    : launch_drop_path<float>(x, resid, y, B, per, rng, p, st);
}

extern "C" int vitpe_drop_path_bwd(int dtype, const void* dy, void* dx, int B, long long per, const unsigned long long* rng,
                                   float p, hipStream_t st) {
  return vitpe_drop_path_fwd(dtype, dy, nullptr, dx, B, per, rng, p, st);
}
