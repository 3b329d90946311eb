// Fused patch embedding (reference models/vit.py:164,245-258 + positional_encoding.py:37-40 + the first block's
// norm1 statistics, vit.py:113):
//
//   image -> unfold (Conv2d k = s = p  ==  patch matrix x W^T) -> + bias -> + absolute PE -> class token in row 0
//         -> tokens [B, P+1, D]  (+ LayerNorm statistics of every token row for the first attention kernel)
//
// in ONE kernel for the small-K geometries (K = C p^2 <= 64, P <= 64, D <= 256: the CIFAR / MNIST shapes), one workgroup
// (4 waves) per image.  The unfold is the A-operand staging: the image's pixels go global -> registers -> LDS in patch
// order (from fp32 images, or gathered + ToTensor + Normalize'd from the resident uint8 dataset, train.py:69-92); the
// [P, K] patch matrix never makes an HBM round trip on the way to the MFMAs.  It is still written out once (3 MB at
// batch 512) because the patch-embed WEIGHT gradient needs it as its X operand in the backward pass.
// The product runs on the matrix core (4 token tiles x D/16 feature tiles x K/32 chunks); bias / PE add, the row
// statistics and the stores happen on the accumulators (a lane owns four consecutive features of one token per tile).
// Replaces three launches (vitpe_unfold[_u8] + vitpe_gemm_nt(EPI_PATCH) + vitpe_layernorm_fwd statistics).
//
// AUG (vitpe_patch_embed_aug, uint8 path only): the gather also applies the augmentation stream of augment.h -- one draw per
// workgroup (= image), the crop and the flip are address arithmetic of the same loads.  The p == 4 row of a cropped patch
// is unaligned and may straddle the image border: it is cut out of the two ALIGNED dwords of the source row that cover it
// (a dword outside the row is the constant 0 == the zero padding), byte-reversed under a flip.
#include "common.h"
#include "augment.h"

namespace vitpe {

struct EmbedArgs {
  const float* img;            // [B,C,S,S] fp32, or null when data is set
  const unsigned char* data;   // resident uint8 dataset [Ndata,C,S,S] or null
  const long long* index;      // [B] sample indices into data (null: record b)
  const float* nmean;          // [C] Normalize constants (uint8 path)
  const float* nstd;
  const void* W;               // patch_embed.weight [D, K] T (Conv2d weight flattened: k = c p^2 + ky p + kx)
  const float* bias;           // [D]
  const float* cls;            // [D]
  const float* ape;            // [P, D] rows of the absolute PE table, or null
  void* tokens;                // [B, P+1, D] T
  void* patches;               // [B*P, K] T (for the weight gradient), nullable
  float* mean;                 // [B*(P+1)] LayerNorm statistics of the token rows, nullable (both or neither)
  float* rstd;
  int B, C, S, p, D;
  float eps;
  const unsigned long long* rng;   // AUG only: the site's (seed, offset) pair; crop padding; flip enabled
  int pad, hflip;
};

constexpr int EMB_KP = 64;     // padded K
constexpr int EMB_MP = 64;     // padded patches per image
constexpr int EMB_DMAX = 256;

// One workgroup = one image = 4 waves, wave w owns the 16-token tile w through ALL feature tiles.  Swapped MFMA
// orientation (A = weight rows, B = patch rows): acc[nt][r] = out[token 16w + c][feature 16nt + 4g + r], so a lane holds
// four consecutive features of ONE token per tile: the row statistics are an in-lane sum over the tiles plus a
// cross-group (g) reduction with two permlane swaps, and the stores are 8 B per lane -- no fp32 staging of the result.
template <typename T, bool AUG>
__global__ __launch_bounds__(256) void patch_embed_kernel(EmbedArgs a) {
  constexpr int LDA = EMB_KP + 2 * Pad<T>::elems;    // operand rows: 10 (bf16) slots, == 2 mod 4: conflict-free fragment reads
  constexpr int CHN = CH<T>::n, NTMAX = EMB_DMAX / 16, KSM = EMB_KP / 32;
  __shared__ __attribute__((aligned(16))) T sA[EMB_MP * LDA];
  __shared__ __attribute__((aligned(16))) T sW[EMB_DMAX * LDA];

  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;
  const int C = a.C, S = a.S, p = a.p, D = a.D;
  const int G = S / p, P = G * G, K = C * p * p;
  const T* Wg = reinterpret_cast<const T*>(a.W);
  const Chunk16 zero = {0u, 0u, 0u, 0u};

  // ---- stage W rows (16-B chunks; the K padding zeroed) and the image's patches (the unfold) ---------------------------
  {
    constexpr int CPR = EMB_KP / CHN;              // chunks per padded row
    const int cpr = K / CHN;                       // real chunks per row (K % CHN == 0: support check)
    for (int q = tid; q < D * CPR; q += 256) {
      const int row = q / CPR, cc = q % CPR;
      *reinterpret_cast<Chunk16*>(sW + row * LDA + cc * CHN) =
          cc < cpr ? *reinterpret_cast<const Chunk16*>(Wg + (size_t)row * K + cc * CHN) : zero;
    }
    for (int q = tid; q < EMB_MP * CPR; q += 256) {   // K padding of every patch row, all of the rows past P
      const int row = q / CPR, cc = q % CPR;
      if (cc >= cpr || row >= P) *reinterpret_cast<Chunk16*>(sA + row * LDA + cc * CHN) = zero;
    }
  }
  const long long rec = a.data != nullptr ? (a.index != nullptr ? a.index[b] : (long long)b) : 0;
  T* pout = a.patches != nullptr ? reinterpret_cast<T*>(a.patches) + (size_t)b * P * K : nullptr;
  AugDraw aug = {0, 0, 0};
  if (AUG) aug = aug_draw(a.rng, (unsigned long long)b, a.pad, a.hflip);   // uniform over the workgroup
  for (int q = tid; q < P * C * p; q += 256) {           // (patch n, channel, row ky): p contiguous pixels
    const int ky = q % p, ch = (q / p) % C, n = q / (p * C);
    const int gy = n / G, gx = n % G;
    const size_t pix = ((size_t)ch * S + gy * p + ky) * S + gx * p;
    const int k0 = ch * p * p + ky * p;
    if (p == 4) {   // the CIFAR / MNIST patch: one 16-B (fp32) or 4-B (uint8) load, one 8-B / 16-B store each way
      float v[4];
      if (AUG) {
        const int sy = gy * p + ky + aug.oy - a.pad;
        const int lo = (aug.flip ? S - 4 - gx * p : gx * p) + aug.ox - a.pad;   // leftmost source column of the four
        const int d0 = lo >> 2, sh = 8 * (lo & 3);                              // (floor / non-negative remainder)
        const bool rowok = sy >= 0 && sy < S;                                   // (S % 4 == 0: a dword never straddles the row end)
        const uint32_t* row =
            reinterpret_cast<const uint32_t*>(a.data + (size_t)rec * C * S * S + ((size_t)ch * S + (rowok ? sy : 0)) * S);
        const uint32_t w0 = rowok && d0 >= 0 && 4 * d0 < S ? row[d0] : 0u;
        const uint32_t w1 = rowok && d0 + 1 >= 0 && 4 * (d0 + 1) < S ? row[d0 + 1] : 0u;
        uint32_t u = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
        if (aug.flip) u = __builtin_bswap32(u);
        const float m = a.nmean[ch], sd = a.nstd[ch];
        v[0] = ((float)(u & 0xffu) / 255.0f - m) / sd; v[1] = ((float)((u >> 8) & 0xffu) / 255.0f - m) / sd;
        v[2] = ((float)((u >> 16) & 0xffu) / 255.0f - m) / sd; v[3] = ((float)(u >> 24) / 255.0f - m) / sd;
      } else if (a.data != nullptr) {
        const uchar4 u = *reinterpret_cast<const uchar4*>(a.data + (size_t)rec * C * S * S + pix);
        const float m = a.nmean[ch], sd = a.nstd[ch];   // ToTensor then Normalize, IEEE division (as vitpe_unfold_u8)
        v[0] = ((float)u.x / 255.0f - m) / sd; v[1] = ((float)u.y / 255.0f - m) / sd;
        v[2] = ((float)u.z / 255.0f - m) / sd; v[3] = ((float)u.w / 255.0f - m) / sd;
      } else {
        const f32x4 f = *reinterpret_cast<const f32x4*>(a.img + (size_t)b * C * S * S + pix);
        v[0] = f[0]; v[1] = f[1]; v[2] = f[2]; v[3] = f[3];
      }
      st4(sA + n * LDA + k0, v[0], v[1], v[2], v[3]);
      if (pout != nullptr) st4(pout + (size_t)n * K + k0, v[0], v[1], v[2], v[3]);
    } else {
      for (int kx = 0; kx < p; ++kx) {
        float v;
        if (AUG) {
          const int sy = gy * p + ky + aug.oy - a.pad;
          const int sx = (aug.flip ? S - 1 - (gx * p + kx) : gx * p + kx) + aug.ox - a.pad;
          const bool in = sy >= 0 && sy < S && sx >= 0 && sx < S;
          unsigned char u = 0;   // the zero padding
          if (in) u = a.data[(size_t)rec * C * S * S + ((size_t)ch * S + sy) * S + sx];
          v = ((float)u / 255.0f - a.nmean[ch]) / a.nstd[ch];
        } else if (a.data != nullptr)
          v = ((float)a.data[(size_t)rec * C * S * S + pix + kx] / 255.0f - a.nmean[ch]) / a.nstd[ch];
        else
          v = a.img[(size_t)b * C * S * S + pix + kx];
        const T t = from_f32<T>(v);
        sA[n * LDA + k0 + kx] = t;
        if (pout != nullptr) pout[(size_t)n * K + k0 + kx] = t;
      }
    }
  }
  __syncthreads();

  T* tok = reinterpret_cast<T*>(a.tokens) + (size_t)b * (P + 1) * D;
  const float invD = 1.0f / (float)D;
  const int NTL = D / 16, KS = (K + 31) / 32;
  if (16 * wave < P) {
    const int n = 16 * wave + c;                      // this lane's patch (token n + 1)
    Frag<T> fa[KSM];
#pragma unroll
    for (int ks = 0; ks < KSM; ++ks) fa[ks] = ld_frag(sA + n * LDA + 32 * ks + 8 * g);
    float s1 = 0.f, s2 = 0.f;
    f32x4 keep[NTMAX];
#pragma unroll
    for (int nt = 0; nt < NTMAX; ++nt) {
      if (nt < NTL) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KSM; ++ks)
          if (ks < KS) mma(ld_frag(sW + (16 * nt + c) * LDA + 32 * ks + 8 * g), fa[ks], acc);
        const int gn = 16 * nt + 4 * g;
        const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + gn);
        acc += bv;
        if (a.ape != nullptr && n < P) acc += *reinterpret_cast<const f32x4*>(a.ape + (size_t)n * D + gn);
        // statistics of the values as stored
#pragma unroll
        for (int r = 0; r < 4; ++r) { acc[r] = to_f32(from_f32<T>(acc[r])); s1 += acc[r]; }
        keep[nt] = acc;
        if (n < P) st4(tok + (size_t)(n + 1) * D + gn, acc[0], acc[1], acc[2], acc[3]);
      }
    }
    if (a.mean != nullptr) {   // two-pass variance on the register-resident row (as the LayerNorm kernels)
      auto xg = [](float v) {
        auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
        auto q2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        return __uint_as_float(q2[0]) + __uint_as_float(q2[1]);
      };
      const float mean = xg(s1) * invD;
#pragma unroll
      for (int nt = 0; nt < NTMAX; ++nt)
        if (nt < NTL) {
#pragma unroll
          for (int r = 0; r < 4; ++r) { const float d = keep[nt][r] - mean; s2 += d * d; }
        }
      const float var = xg(s2) * invD;
      if (g == 0 && n < P) {
        a.mean[(size_t)b * (P + 1) + n + 1] = mean;
        a.rstd[(size_t)b * (P + 1) + n + 1] = 1.0f / sqrtf(var + a.eps);
      }
    }
  }
  // ---- class-token row (reference vit.py:253-254; APE skips it): the last wave, 8 columns per lane -----------------------
  if (wave == 3) {
    const int gn = lane * 8;
    float v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) v[t] = 0.f;
    if (gn < D) {
#pragma unroll
      for (int t = 0; t < 8; ++t) v[t] = a.cls[gn + t];
#pragma unroll
      for (int h = 0; h < 8 / CHN; ++h) {
        const Chunk16 ch = f32_to_chunk<T>(v + h * CHN);
        *reinterpret_cast<Chunk16*>(tok + gn + h * CHN) = ch;
        chunk_to_f32<T>(ch, v + h * CHN);
      }
    }
    if (a.mean != nullptr) {
      float s = 0.f;
#pragma unroll
      for (int t = 0; t < 8; ++t) s += v[t];
      const float mean = wave_sum(s) * invD;
      float sq = 0.f;
      if (gn < D) {
#pragma unroll
        for (int t = 0; t < 8; ++t) { const float d = v[t] - mean; sq += d * d; }
      }
      sq = wave_sum(sq);
      if (lane == 0) {
        a.mean[(size_t)b * (P + 1)] = mean;
        a.rstd[(size_t)b * (P + 1)] = 1.0f / sqrtf(sq * invD + a.eps);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// The un-fused route (geometries outside vitpe_patch_embed_supported, VITPE_FUSE_EMBED=0) and the embedding's backward:
// the unfold as a launch of its own in front of the patch GEMM, from fp32 images or from the resident uint8 dataset
// (with the same augmentation stream), and embed_bwd.
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
// ERASE (vitpe_unfold_u8_erase, on top of AUG): the erasing stream, drawn per thread with the same rule.
struct EraseArgs {
  unsigned long long thr;
  int mode;
  float smin, smax, lmin, lmax;
};
template <typename T, bool AUG, bool ERASE>
__global__ void unfold_u8_kernel(const unsigned char* __restrict__ data, const long long* __restrict__ index,
                                 const float* __restrict__ mean, const float* __restrict__ stdv, T* __restrict__ patches,
                                 float* __restrict__ img_out, int B, int Cc, int S, int p,
                                 const unsigned long long* __restrict__ rng, int pad, int hflip, EraseArgs ea) {
  static_assert(AUG || !ERASE, "the erasing stream runs on top of the augmented gather");
  const int g = S / p, P = g * g, Kp = Cc * p * p;
  const long long total = (long long)B * P * Cc * p;
  EraseDraw er = {0, 0, 0, 0, 0};
  EraseFill fill = {};
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
      if (b != aug_b) {
        aug = aug_draw(rng, (unsigned long long)b, pad, hflip);
        aug_b = b;
        if (ERASE) {
          er = erase_draw(rng, (unsigned long long)b, S, ea.thr, ea.smin, ea.smax, ea.lmin, ea.lmax);
          if (er.on) fill = erase_fill(rng, (unsigned long long)b, ea.mode);
        }
      }
      const int sy = gy * p + ky + aug.oy - pad;
      const bool rowok = sy >= 0 && sy < S;
      const unsigned char* row = data + (size_t)rec * Cc * S * S + ((size_t)ch * S + (rowok ? sy : 0)) * S;
      for (int kx = 0; kx < p; ++kx) {
        const int sx = (aug.flip ? S - 1 - (gx * p + kx) : gx * p + kx) + aug.ox - pad;
        unsigned char u = 0;   // the zero padding
        if (rowok && sx >= 0 && sx < S) u = row[sx];
        float v = ((float)u / 255.0f - m) / sd;
        if (ERASE && erase_inside(er, gy * p + ky, gx * p + kx))
          v = erase_value(fill, (unsigned long long)b, S, gy * p + ky, gx * p + kx, ch);
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

// the erasing draws of the first B batch slots (tests): out [B,5] = (on, i, j, h, w)
__global__ void erase_params_kernel(const unsigned long long* __restrict__ rng, int* __restrict__ out, int B, int S,
                                    EraseArgs ea) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const EraseDraw d = erase_draw(rng, (unsigned long long)b, S, ea.thr, ea.smin, ea.smax, ea.lmin, ea.lmax);
  out[5 * b] = d.on; out[5 * b + 1] = d.i; out[5 * b + 2] = d.j; out[5 * b + 3] = d.h; out[5 * b + 4] = d.w;
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

}  // namespace vitpe

using namespace vitpe;

static const EraseArgs ERASE_OFF = {0ull, ERASE_CONST, 0.02f, 0.33f, 0.0f, 0.0f};   // (valid arguments, switch off)

extern "C" int vitpe_patch_embed_supported(int dtype, int C, int S, int p, int D) {
  if (!(dtype == 0 || dtype == 1) || C < 1 || p < 1 || S < p || S % p != 0) return 0;
  const int G = S / p, P = G * G, K = C * p * p;
  return K <= EMB_KP && K % (dtype == 1 ? 8 : 4) == 0 && P <= EMB_MP && D >= 16 && D <= EMB_DMAX && D % 16 == 0;
}

static int launch_patch_embed(int dtype, const float* img, const unsigned char* data, const long long* index,
                              const float* nmean, const float* nstd, const void* W, const float* bias, const float* cls,
                              const float* ape, void* tokens, void* patches, float* mean, float* rstd, int B, int C, int S,
                              int p, int D, float eps, const unsigned long long* rng, int pad, int hflip, hipStream_t stream) {
  VITPE_REQUIRE(W && bias && cls && tokens && B >= 0);
  VITPE_REQUIRE((img != nullptr) != (data != nullptr));
  VITPE_REQUIRE(data == nullptr || (nmean && nstd));
  VITPE_REQUIRE((mean == nullptr) == (rstd == nullptr));
  VITPE_REQUIRE(rng == nullptr || (img == nullptr && pad >= 0 && pad <= S));
  VITPE_REQUIRE(rng == nullptr || p != 4 || ((uintptr_t)data & 3) == 0);   // the aligned dwords of the p == 4 rows
  if (!vitpe_patch_embed_supported(dtype, C, S, p, D)) return (int)hipErrorNotSupported;
  if (B == 0) return 0;
  EmbedArgs a{};
  a.img = img; a.data = data; a.index = index; a.nmean = nmean; a.nstd = nstd; a.W = W; a.bias = bias; a.cls = cls; a.ape = ape;
  a.tokens = tokens; a.patches = patches; a.mean = mean; a.rstd = rstd; a.B = B; a.C = C; a.S = S; a.p = p; a.D = D; a.eps = eps;
  a.rng = rng; a.pad = pad; a.hflip = hflip;
  if (rng != nullptr) {
    if (dtype == 1) hipLaunchKernelGGL((patch_embed_kernel<bf16, true>), dim3(B), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((patch_embed_kernel<float, true>), dim3(B), dim3(256), 0, stream, a);
  } else {
    if (dtype == 1) hipLaunchKernelGGL((patch_embed_kernel<bf16, false>), dim3(B), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((patch_embed_kernel<float, false>), dim3(B), dim3(256), 0, stream, a);
  }
  VITPE_CHECK_LAUNCH();
}

// img XOR data: fp32 images [B,C,S,S], or the resident uint8 dataset + sample indices (as vitpe_unfold_u8).
extern "C" int vitpe_patch_embed(int dtype, const float* img, const unsigned char* data, const long long* index,
                                 const float* nmean, const float* nstd, const void* W, const float* bias, const float* cls,
                                 const float* ape, void* tokens, void* patches, float* mean, float* rstd, int B, int C, int S,
                                 int p, int D, float eps, hipStream_t stream) {
  return launch_patch_embed(dtype, img, data, index, nmean, nstd, W, bias, cls, ape, tokens, patches, mean, rstd, B, C, S, p, D,
                            eps, nullptr, 0, 0, stream);
}

// the same with the augmentation stream on the uint8 path (rng NULL: exactly vitpe_patch_embed)
extern "C" int vitpe_patch_embed_aug(int dtype, const float* img, const unsigned char* data, const long long* index,
                                     const float* nmean, const float* nstd, const void* W, const float* bias,
                                     const float* cls, const float* ape, void* tokens, void* patches, float* mean,
                                     float* rstd, int B, int C, int S, int p, int D, float eps, const unsigned long long* rng,
                                     int pad, int hflip, hipStream_t stream) {
  return launch_patch_embed(dtype, img, data, index, nmean, nstd, W, bias, cls, ape, tokens, patches, mean, rstd, B, C, S, p, D,
                            eps, rng, pad, hflip, stream);
}

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
                            const unsigned long long* rng, int pad, int hflip, const EraseArgs& ea, hipStream_t st) {
  VITPE_REQUIRE(data && mean && stdv && patches && B >= 0 && C > 0 && p > 0 && S % p == 0 && (dtype == 0 || dtype == 1));
  VITPE_REQUIRE(rng == nullptr || erase_args_ok(ea.thr, ea.mode, C, ea.smin, ea.smax, ea.lmin, ea.lmax));
  VITPE_REQUIRE(rng == nullptr || (pad >= 0 && pad <= S));
  const long long total = (long long)B * (S / p) * (S / p) * C * p;
  if (total == 0) return 0;
  const unsigned blocks = (unsigned)min((total + 255) / 256, (long long)8192);
  if (rng != nullptr && ea.thr != 0) {
    if (dtype == 1)
      hipLaunchKernelGGL((unfold_u8_kernel<bf16, true, true>), dim3(blocks), dim3(256), 0, st, data, index, mean, stdv, (bf16*)patches, img_out, B, C, S, p, rng, pad, hflip, ea);
    else
      hipLaunchKernelGGL((unfold_u8_kernel<float, true, true>), dim3(blocks), dim3(256), 0, st, data, index, mean, stdv, (float*)patches, img_out, B, C, S, p, rng, pad, hflip, ea);
  } else if (rng != nullptr) {
    if (dtype == 1)
      hipLaunchKernelGGL((unfold_u8_kernel<bf16, true, false>), dim3(blocks), dim3(256), 0, st, data, index, mean, stdv, (bf16*)patches, img_out, B, C, S, p, rng, pad, hflip, ea);
    else
      hipLaunchKernelGGL((unfold_u8_kernel<float, true, false>), dim3(blocks), dim3(256), 0, st, data, index, mean, stdv, (float*)patches, img_out, B, C, S, p, rng, pad, hflip, ea);
  } else {
    if (dtype == 1)
      hipLaunchKernelGGL((unfold_u8_kernel<bf16, false, false>), dim3(blocks), dim3(256), 0, st, data, index, mean, stdv, (bf16*)patches, img_out, B, C, S, p, rng, 0, 0, ea);
    else
      hipLaunchKernelGGL((unfold_u8_kernel<float, false, false>), dim3(blocks), dim3(256), 0, st, data, index, mean, stdv, (float*)patches, img_out, B, C, S, p, rng, 0, 0, ea);
  }
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_unfold_u8(int dtype, const unsigned char* data, const long long* index, const float* mean,
                               const float* stdv, void* patches, float* img_out, int B, int C, int S, int p,
                               hipStream_t st) {
  return launch_unfold_u8(dtype, data, index, mean, stdv, patches, img_out, B, C, S, p, nullptr, 0, 0, ERASE_OFF, st);
}

// the same with the augmentation stream (rng NULL: exactly vitpe_unfold_u8)
extern "C" int vitpe_unfold_u8_aug(int dtype, const unsigned char* data, const long long* index, const float* mean,
                                   const float* stdv, void* patches, float* img_out, int B, int C, int S, int p,
                                   const unsigned long long* rng, int pad, int hflip, hipStream_t st) {
  return launch_unfold_u8(dtype, data, index, mean, stdv, patches, img_out, B, C, S, p, rng, pad, hflip, ERASE_OFF, st);
}

// the same with the erasing stream on top (erase_thr 0: exactly vitpe_unfold_u8_aug; rng NULL: exactly vitpe_unfold_u8)
extern "C" int vitpe_unfold_u8_erase(int dtype, const unsigned char* data, const long long* index, const float* mean,
                                     const float* stdv, void* patches, float* img_out, int B, int C, int S, int p,
                                     const unsigned long long* rng, int pad, int hflip, unsigned long long erase_thr,
                                     int erase_mode, float smin, float smax, float lmin, float lmax, hipStream_t st) {
  return launch_unfold_u8(dtype, data, index, mean, stdv, patches, img_out, B, C, S, p, rng, pad, hflip,
                          EraseArgs{erase_thr, erase_mode, smin, smax, lmin, lmax}, st);
}

extern "C" int vitpe_augment_params(const unsigned long long* rng, int* out, int B, int pad, int hflip, hipStream_t st) {
  VITPE_REQUIRE(rng && B >= 0 && (out || B == 0) && pad >= 0);
  if (B == 0) return 0;
  hipLaunchKernelGGL(augment_params_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, rng, out, B, pad, hflip);
  VITPE_CHECK_LAUNCH();
}

// the erasing draws: on the device, and the same function on the host (rng and out in host memory, no stream)
extern "C" int vitpe_erase_params(const unsigned long long* rng, int* out, int B, int S, unsigned long long thr, float smin,
                                  float smax, float lmin, float lmax, hipStream_t st) {
  VITPE_REQUIRE(rng && B >= 0 && (out || B == 0) && S >= 1 && erase_args_ok(thr, ERASE_CONST, 1, smin, smax, lmin, lmax));
  if (B == 0) return 0;
  hipLaunchKernelGGL(erase_params_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, rng, out, B, S,
                     EraseArgs{thr, ERASE_CONST, smin, smax, lmin, lmax});
  VITPE_CHECK_LAUNCH();
}

extern "C" int vitpe_erase_params_host(const unsigned long long* rng, int* out, int B, int S, unsigned long long thr,
                                       float smin, float smax, float lmin, float lmax) {
  VITPE_REQUIRE(rng && B >= 0 && (out || B == 0) && S >= 1 && erase_args_ok(thr, ERASE_CONST, 1, smin, smax, lmin, lmax));
  for (int b = 0; b < B; ++b) {
    const EraseDraw d = erase_draw(rng, (unsigned long long)b, S, thr, smin, smax, lmin, lmax);
    out[5 * b] = d.on; out[5 * b + 1] = d.i; out[5 * b + 2] = d.j; out[5 * b + 3] = d.h; out[5 * b + 4] = d.w;
  }
  return 0;
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
