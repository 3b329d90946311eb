// transforms.Resize(S) of reference train.py:69-70,78-79 on the resident uint8 dataset: PIL's 8-bit antialiased
// bilinear resample (img.resize((S, S), Image.BILINEAR)) restated as integer arithmetic on fixed-point coefficients,
// so the result is the reference's bytes, not an approximation of them.
//
//   vitpe_resize_coeffs   host: the coefficient tables of one pass (doubles, PIL's order of operations)
//   vitpe_resize_u8       device: horizontal pass to a uint8 intermediate, vertical pass, one plane per workgroup
#include <math.h>

#include <vector>

#include "common.h"

namespace vitpe {

constexpr int RSZ_PRECISION_BITS = 32 - 8 - 2;   // PIL: 8-bit samples, 2 guard bits in a 32-bit accumulator
constexpr int RSZ_S0_MIN = 8, RSZ_S0_MAX = 64, RSZ_S_MIN = 4, RSZ_S_MAX = 512;
constexpr int RSZ_THREADS = 256;
constexpr size_t RSZ_LDS_MAX = 64 * 1024;        // static limit of a launch without an attribute

// Everything below that feeds an int() truncation is one IEEE double operation per statement and is compiled without
// contraction: a host with FMA must not be able to change a coefficient.
#pragma clang fp contract(off)

static int resize_ksize(int in, int out) {
  double fs = (double)in / (double)out;
  if (fs < 1.0) fs = 1.0;
  const double support = 1.0 * fs;               // bilinear: filter support 1
  return (int)ceil(support) * 2 + 1;
}

static double bilinear_filter(double t) {
  if (t < 0.0) t = -t;
  if (t < 1.0) return 1.0 - t;
  return 0.0;
}

// bounds[out][2] = (xmin, n), kk[out][ksize] (entries past n are 0); -> ksize
static int resize_coeffs(int in, int out, int* bounds, int* kk, int ksize_cap) {
  const double scale = (double)in / (double)out;
  double fs = scale;
  if (fs < 1.0) fs = 1.0;
  const double support = 1.0 * fs;
  const int ksize = (int)ceil(support) * 2 + 1;
  if (ksize > ksize_cap) return -ksize;
  std::vector<double> w((size_t)ksize);
  for (int xx = 0; xx < out; ++xx) {
    const double xh = (double)xx + 0.5;
    const double center = xh * scale;
    const double lo = center - support;
    const double hi = center + support;
    int xmin = (int)(lo + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(hi + 0.5);
    if (xmax > in) xmax = in;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      const double pos = (double)(x + xmin);
      const double d = pos - center;
      const double dh = d + 0.5;
      const double t = dh / fs;
      w[x] = bilinear_filter(t);
      ww = ww + w[x];
    }
    int* k = kk + (size_t)xx * ksize;
    for (int x = 0; x < ksize; ++x) {
      if (x < n) {
        double wn = w[x];
        if (ww != 0.0) wn = wn / ww;
        const double scaled = wn * (double)(1 << RSZ_PRECISION_BITS);
        const double rounded = scaled + 0.5;      // the bilinear weights are >= 0
        k[x] = (int)rounded;
      } else {
        k[x] = 0;
      }
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = n;
  }
  return ksize;
}

VITPE_DEV unsigned clip8(int acc) {
  const int v = acc >> RSZ_PRECISION_BITS;
  return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One workgroup walks planes blockIdx.x, blockIdx.x + gridDim.x, ...  LDS: both coefficient tables (staged once), the
// source plane [S0][S0] and the horizontal pass's intermediate [S0][ST] (ST = S rounded up to 4), so a source byte is
// read from HBM once and nothing but the result is written.  Both passes produce four neighbouring output bytes per
// thread: the vertical pass reads the intermediate one dword per lane along a row (consecutive lanes, consecutive
// banks: no conflict for the column walk) and, where VEC, stores uchar4.
template <bool VEC>
__global__ void __launch_bounds__(RSZ_THREADS)
resize_u8_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, long long planes, int S0, int S,
                 const int* __restrict__ bounds_h, const int* __restrict__ kk_h, const int* __restrict__ bounds_v,
                 const int* __restrict__ kk_v, int ksize) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rsz_lds[];
  const int tid = threadIdx.x;
  const int ST = (S + 3) & ~3, Q = ST / 4;
  int* sBh = reinterpret_cast<int*>(rsz_lds);          // [S][2]
  int* sBv = sBh + 2 * S;                              // [S][2]
  int* sKh = sBv + 2 * S;                              // [S][ksize]
  int* sKv = sKh + S * ksize;                          // [S][ksize]
  unsigned* sTmp = reinterpret_cast<unsigned*>(sKv + S * ksize);   // [S0][Q] dwords
  unsigned char* sSrc = reinterpret_cast<unsigned char*>(sTmp + S0 * Q);   // [S0][S0]

  // (xmin, n) are clamped into the source so that a bad table can give a wrong image but never a read outside the tile
  for (int i = tid; i < S; i += RSZ_THREADS) {
    int n = bounds_h[2 * i + 1];
    n = n < 0 ? 0 : (n > ksize ? ksize : (n > S0 ? S0 : n));
    int x0 = bounds_h[2 * i];
    sBh[2 * i] = x0 < 0 ? 0 : (x0 > S0 - n ? S0 - n : x0);
    sBh[2 * i + 1] = n;
    n = bounds_v[2 * i + 1];
    n = n < 0 ? 0 : (n > ksize ? ksize : (n > S0 ? S0 : n));
    x0 = bounds_v[2 * i];
    sBv[2 * i] = x0 < 0 ? 0 : (x0 > S0 - n ? S0 - n : x0);
    sBv[2 * i + 1] = n;
  }
  for (int i = tid; i < S * ksize; i += RSZ_THREADS) {
    sKh[i] = kk_h[i];
    sKv[i] = kk_v[i];
  }

  const int src_bytes = S0 * S0;
  const size_t dst_bytes = (size_t)S * S;
  for (long long plane = blockIdx.x; plane < planes; plane += gridDim.x) {
    __syncthreads();                                   // tables staged / the previous plane's tiles consumed
    const unsigned char* sp = src + (size_t)plane * src_bytes;
    if (VEC) {                                         // src_bytes % 4 == 0 and a 4-byte aligned base (host check)
      for (int i = tid; i < src_bytes / 4; i += RSZ_THREADS)
        reinterpret_cast<unsigned*>(sSrc)[i] = reinterpret_cast<const unsigned*>(sp)[i];
    } else {
      for (int i = tid; i < src_bytes; i += RSZ_THREADS) sSrc[i] = sp[i];
    }
    __syncthreads();

    // horizontal: sTmp[y][xx] = clip((2^21 + sum_x src[y][xmin + x] * k[xx][x]) >> 22)
    for (int i = tid; i < S0 * Q; i += RSZ_THREADS) {
      const int y = i / Q, q = i - y * Q;
      const unsigned char* row = sSrc + y * S0;
      unsigned packed = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int xx = 4 * q + j;
        if (xx < S) {
          const int x0 = sBh[2 * xx], n = sBh[2 * xx + 1];
          const int* k = sKh + xx * ksize;
          int acc = 1 << (RSZ_PRECISION_BITS - 1);
          for (int x = 0; x < n; ++x) acc += (int)row[x0 + x] * k[x];
          packed |= clip8(acc) << (8 * j);
        }
      }
      sTmp[i] = packed;
    }
    __syncthreads();

    // vertical: dst[yy][x] = clip((2^21 + sum_y tmp[ymin + y][x] * k[yy][y]) >> 22), four x per thread
    unsigned char* dp = dst + (size_t)plane * dst_bytes;
    for (int i = tid; i < S * Q; i += RSZ_THREADS) {
      const int yy = i / Q, q = i - yy * Q;
      const int y0 = sBv[2 * yy], n = sBv[2 * yy + 1];
      const int* k = sKv + yy * ksize;
      int a0 = 1 << (RSZ_PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
      for (int y = 0; y < n; ++y) {
        const unsigned t = sTmp[(y0 + y) * Q + q];
        const int c = k[y];
        a0 += (int)(t & 0xffu) * c;
        a1 += (int)((t >> 8) & 0xffu) * c;
        a2 += (int)((t >> 16) & 0xffu) * c;
        a3 += (int)(t >> 24) * c;
      }
      if (VEC) {                                       // S % 4 == 0: the four bytes lie in one row, 4-byte aligned
        uchar4 o;
        o.x = (unsigned char)clip8(a0); o.y = (unsigned char)clip8(a1);
        o.z = (unsigned char)clip8(a2); o.w = (unsigned char)clip8(a3);
        *reinterpret_cast<uchar4*>(dp + (size_t)yy * S + 4 * q) = o;
      } else {
        unsigned char* o = dp + (size_t)yy * S + 4 * q;
        const int left = S - 4 * q;
        o[0] = (unsigned char)clip8(a0);
        if (left > 1) o[1] = (unsigned char)clip8(a1);
        if (left > 2) o[2] = (unsigned char)clip8(a2);
        if (left > 3) o[3] = (unsigned char)clip8(a3);
      }
    }
  }
}

__global__ void __launch_bounds__(RSZ_THREADS)
resize_copy_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, size_t bytes) {
  for (size_t i = (size_t)blockIdx.x * RSZ_THREADS + threadIdx.x; i < bytes; i += (size_t)gridDim.x * RSZ_THREADS)
    dst[i] = src[i];
}

static size_t resize_lds_bytes(int S0, int S, int ksize) {
  const size_t ST = (size_t)((S + 3) & ~3);
  return sizeof(int) * (4 * (size_t)S + 2 * (size_t)S * ksize) + (size_t)S0 * ST + (size_t)S0 * S0;
}

}  // namespace vitpe

using namespace vitpe;

extern "C" int vitpe_resize_coeffs(int in, int out, int* bounds, int* kk, int ksize_cap) {
  if (!bounds || !kk || in < 1 || out < 1 || in > (1 << 16) || out > (1 << 16)) return -1;
  return resize_coeffs(in, out, bounds, kk, ksize_cap);
}

extern "C" int vitpe_resize_u8_supported(int S0, int S) {
  if (S0 < RSZ_S0_MIN || S0 > RSZ_S0_MAX || S < RSZ_S_MIN || S > RSZ_S_MAX) return 0;
  return resize_lds_bytes(S0, S, resize_ksize(S0, S)) <= RSZ_LDS_MAX;
}

extern "C" int vitpe_resize_u8(const unsigned char* src, unsigned char* dst, long long planes, int S0, int S,
                               const int* bounds_h, const int* kk_h, const int* bounds_v, const int* kk_v, int ksize,
                               hipStream_t stream) {
  VITPE_REQUIRE(src && dst && planes >= 0);
  if (!vitpe_resize_u8_supported(S0, S)) return (int)hipErrorNotSupported;
  if (planes == 0) return 0;
  if (S == S0) {                                       // PIL: a resize to the same size is a copy
    const size_t bytes = (size_t)planes * S0 * S0;
    const unsigned blocks = (unsigned)((bytes + RSZ_THREADS - 1) / RSZ_THREADS < 16384 ? (bytes + RSZ_THREADS - 1) / RSZ_THREADS : 16384);
    hipLaunchKernelGGL(resize_copy_kernel, dim3(blocks), dim3(RSZ_THREADS), 0, stream, src, dst, bytes);
    VITPE_CHECK_LAUNCH();
  }
  VITPE_REQUIRE(bounds_h && kk_h && bounds_v && kk_v && ksize == resize_ksize(S0, S));
  const size_t lds = resize_lds_bytes(S0, S, ksize);
  const unsigned blocks = (unsigned)(planes < 4096 ? planes : 4096);
  const bool vec = S % 4 == 0 && S0 % 2 == 0 && (uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0;
  if (vec)
    hipLaunchKernelGGL(resize_u8_kernel<true>, dim3(blocks), dim3(RSZ_THREADS), lds, stream, src, dst, planes, S0, S,
                       bounds_h, kk_h, bounds_v, kk_v, ksize);
  else
    hipLaunchKernelGGL(resize_u8_kernel<false>, dim3(blocks), dim3(RSZ_THREADS), lds, stream, src, dst, planes, S0, S,
                       bounds_h, kk_h, bounds_v, kk_v, ksize);
  VITPE_CHECK_LAUNCH();
}
