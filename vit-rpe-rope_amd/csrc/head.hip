// Classifier head (reference models/vit.py:284-285) and its loss (train.py:113,119-121): LayerNorm of the class row,
// Linear(d, classes), mean cross-entropy, accuracy, and their backward -- as three stand-alone kernels (head_fwd, ce,
// head_bwd) and as the train step's fused launch pair (head_step + head_bwd_params).
#include "common.h"

namespace vitpe {

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

}  // namespace vitpe

using namespace vitpe;

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
// the parameter gradients of both head backwards: batch chunks of 32 images; per_image / out2 / metric_acc / hp_tick are
// vitpe_head_step's (null from vitpe_head_bwd)
static int head_bwd_params_launch(const float* dlogits, const float* ws_yn, const float* ws_dyn, const float* ws_xhat,
                                  float* dWh, float* dbh, float* dgamma, float* dbeta, int B, int D, int Cn,
                                  const float* per_image, float* out2, float* metric_acc, float* hp_tick, hipStream_t st) {
  hipLaunchKernelGGL(head_bwd_params_kernel, dim3((Cn * D + Cn + D + 255) / 256, (B + 31) / 32), dim3(256), 0, st,
                     dlogits, ws_yn, ws_dyn, ws_xhat, dWh, dbh, dgamma, dbeta, B, D, Cn, 32, per_image, out2, metric_acc,
                     hp_tick);
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
  return head_bwd_params_launch(dlogits, ws_yn, ws_dyn, ws_xhat, dWh, dbh, dgamma, dbeta, B, D, Cn, nullptr, nullptr, nullptr,
                                nullptr, st);
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
  return head_bwd_params_launch(dlogits, ws_yn, ws_dyn, ws_xhat, dWh, dbh, dgamma, dbeta, B, D, Cn, per_image, out2, metric_acc,
                                hp_tick, st);
}
