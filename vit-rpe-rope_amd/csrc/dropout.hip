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

// One residual branch's elementwise dropout + per-sample drop-path + residual in one pass ("Engine route"):
//   y = [resid +] f_b * round_T(x . m_e * rs_e) ,  f_b = m_b * rs_p
// bit for bit dropout_kernel (no residual) followed by drop_path_kernel: the intermediate is rounded to T, the products and
// sums have the shape those two compile to (multiply, select, add there; one fma here).  E / P: the elementwise / per-sample
// site is present.  Workgroup blockIdx.x handles slice blockIdx.x % slices of sample blockIdx.x / slices, one thread per
// quad (per % 4 == 0: a quad never straddles two samples), so the per-sample word is uniform over the workgroup.
template <typename T, bool VEC, bool E, bool P>
__global__ __launch_bounds__(256) void branch_drop_kernel(const T* __restrict__ x, const T* __restrict__ resid, T* __restrict__ y,
                                                          long long per, int slices, const unsigned long long* __restrict__ rng_e,
                                                          uint32_t thr_e, float rs_e, const unsigned long long* __restrict__ rng_p,
                                                          uint32_t thr_p, float rs_p) {
  const int b = blockIdx.x / slices, sl = blockIdx.x % slices;
  const long long lq = (long long)sl * 256 + threadIdx.x;   // quad of the sample
  if (4 * lq >= per) return;
  float f = 0.f;
  if (P) {
    const Philox4 wb = drop_words(drop_key(rng_p), (uint64_t)(b >> 2));
    const int k = b & 3;
    const uint32_t word = k == 0 ? wb.w[0] : k == 1 ? wb.w[1] : k == 2 ? wb.w[2] : wb.w[3];
    f = word >= thr_p ? rs_p : 0.f;
  }
  const long long e0 = (long long)b * per + 4 * lq;
  Philox4 w = {};
  if (E) w = drop_words(drop_key(rng_e), (uint64_t)(e0 >> 2));
  float v[4], r[4] = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    const f32x4 xv = ld4(x + e0);
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = xv[t];
    if (resid) {
      const f32x4 rv = ld4(resid + e0);
#pragma unroll
      for (int t = 0; t < 4; ++t) r[t] = rv[t];
    }
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      v[t] = to_f32(x[e0 + t]);
      if (resid) r[t] = to_f32(resid[e0 + t]);
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    float a = v[t];
    if (E) {
      a = w.w[t] >= thr_e ? __fmul_rn(a, rs_e) : 0.f;
      if (P) a = to_f32(from_f32<T>(__fadd_rn(0.f, a)));   // what dropout_kernel stores without a residual
    }
    v[t] = P ? fmaf(a, f, r[t]) : __fadd_rn(r[t], a);
  }
  if (VEC) {
    st4(y + e0, v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) y[e0 + t] = from_f32<T>(v[t]);
  }
}

// offset[i] += inc (mod 2^64) for the n (seed, offset) pairs of a site table; the seeds stay
__global__ __launch_bounds__(256) void rng_advance_kernel(unsigned long long* __restrict__ table, int n, unsigned long long inc) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) table[2 * (size_t)i + 1] += inc;
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

template <typename T, bool E, bool P>
static int launch_branch_drop(const void* x, const void* resid, void* y, int B, long long per, const unsigned long long* rng_e,
                              float p_e, const unsigned long long* rng_p, float p_p, hipStream_t st) {
  const long long slices = (per / 4 + 255) / 256;
  const dim3 grid((unsigned)(slices * B));
  const uintptr_t al = 4 * sizeof(T) - 1;
  const bool vec = !(((uintptr_t)x | (uintptr_t)y | (uintptr_t)resid) & al);
  const T* xp = static_cast<const T*>(x);
  const T* rp = static_cast<const T*>(resid);
  const uint32_t te = E ? drop_threshold(p_e) : 0u, tp = P ? drop_threshold(p_p) : 0u;
  const float se = E ? drop_scale(p_e) : 1.f, sp = P ? drop_scale(p_p) : 1.f;
  if (vec) hipLaunchKernelGGL((branch_drop_kernel<T, true, E, P>), grid, dim3(256), 0, st, xp, rp, static_cast<T*>(y), per, (int)slices, rng_e, te, se, rng_p, tp, sp);
  else hipLaunchKernelGGL((branch_drop_kernel<T, false, E, P>), grid, dim3(256), 0, st, xp, rp, static_cast<T*>(y), per, (int)slices, rng_e, te, se, rng_p, tp, sp);
  VITPE_CHECK_LAUNCH();
}

template <typename T>
static int dispatch_branch_drop(const void* x, const void* resid, void* y, int B, long long per, const unsigned long long* rng_e,
                                float p_e, const unsigned long long* rng_p, float p_p, hipStream_t st) {
  if (rng_e && rng_p) return launch_branch_drop<T, true, true>(x, resid, y, B, per, rng_e, p_e, rng_p, p_p, st);
  if (rng_e) return launch_branch_drop<T, true, false>(x, resid, y, B, per, rng_e, p_e, rng_p, p_p, st);
  return launch_branch_drop<T, false, true>(x, resid, y, B, per, rng_e, p_e, rng_p, p_p, st);
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

extern "C" int vitpe_branch_drop_fwd(int dtype, const void* x, const void* resid, void* y, int B, long long per,
                                     const unsigned long long* rng_elem, float p_elem, const unsigned long long* rng_path,
                                     float p_path, hipStream_t st) {
  VITPE_REQUIRE(x && y && (rng_elem || rng_path) && B >= 0 && B <= (1 << 24) && per >= 0 && per % 4 == 0 &&
                (dtype == 0 || dtype == 1));
  VITPE_REQUIRE((!rng_elem || drop_p_ok(p_elem)) && (!rng_path || drop_p_ok(p_path)));
  if (B == 0 || per == 0) return 0;
  VITPE_REQUIRE(((per / 4 + 255) / 256) * B <= 0x7fffffffLL);   // one grid dimension
  return dtype == 1 ? dispatch_branch_drop<bf16>(x, resid, y, B, per, rng_elem, p_elem, rng_path, p_path, st)
                    : dispatch_branch_drop<float>(x, resid, y, B, per, rng_elem, p_elem, rng_path, p_path, st);
}

extern "C" int vitpe_branch_drop_bwd(int dtype, const void* dy, void* dx, int B, long long per,
                                     const unsigned long long* rng_elem, float p_elem, const unsigned long long* rng_path,
                                     float p_path, hipStream_t st) {
  return vitpe_branch_drop_fwd(dtype, dy, nullptr, dx, B, per, rng_elem, p_elem, rng_path, p_path, st);   // the forward without a residual
}

extern "C" int vitpe_rng_advance(unsigned long long* table, int n_sites, unsigned long long inc, hipStream_t st) {
  VITPE_REQUIRE(n_sites >= 0 && (table || n_sites == 0));
  if (n_sites == 0) return 0;
  hipLaunchKernelGGL(rng_advance_kernel, dim3((unsigned)((n_sites + 255) / 256)), dim3(256), 0, st, table, n_sites, inc);
  VITPE_CHECK_LAUNCH();
}
