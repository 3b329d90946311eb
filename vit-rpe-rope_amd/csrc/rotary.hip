// Backward of the stand-alone rotate-half (reference models/rope_utils.py:3-37 under autograd) and the fixed-order
// reduction of partial rows that the rotary-table gradients use (here and in the attention core's table backward).
//
// The table gradients sum over the batch (and over the heads for a 2-D table).  They are not accumulated with float
// atomics: a workgroup owns a slice of the reduced dimension for a block of table entries, writes the slice's sum once,
// and a second pass adds the slices in order -- the same bits on every run.
#include "common.h"

namespace vitpe {

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

// one thread per table entry `col` of [L] (L = (per_head ? H : 1) * P * half) and slice blockIdx.y of the R = B (per head)
// or B * H (shared table) rows of x that use it: dx of those rows, and the slice's partial d cos / d sin
//   dx1 = g1 c + g2 s ,  dx2 = g2 c - g1 s ,  dcos += g1 x1 + g2 x2 ,  dsin += g2 x1 - g1 x2
// part (nullable) [S][2][L]: the slice's partials.  Row r of x holds (L / half) pairs of rows for this column layout:
// pair row = r * (L / half) + col / half (per head: r = b, col = (h P + n) half + f; shared: r = b H + h, col = n half + f).
__global__ __launch_bounds__(256) void rotary_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                         const float* __restrict__ cosv, const float* __restrict__ sinv,
                                                         float* __restrict__ dx, float* __restrict__ part, int R, int chunk,
                                                         long long L, int half) {
  const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
  if (col >= L) return;
  const int r0 = blockIdx.y * chunk, r1 = min(R, r0 + chunk);
  const long long rows = L / half;
  const int f = (int)(col % half);
  const float c = cosv[col], s = sinv[col];
  float dc = 0.f, ds = 0.f;
  for (int r = r0; r < r1; ++r) {
    const size_t o = (size_t)(r * rows + col / half) * 2 * half + f;
    const float g1 = dy[o], g2 = dy[o + half];
    if (part) {
      const float x1 = x[o], x2 = x[o + half];
      dc += g1 * x1 + g2 * x2;
      ds += g2 * x1 - g1 * x2;
    }
    if (dx) {
      dx[o] = g1 * c + g2 * s;
      dx[o + half] = g2 * c - g1 * s;
    }
  }
  if (part) {
    part[(size_t)blockIdx.y * 2 * L + col] = dc;
    part[(size_t)blockIdx.y * 2 * L + L + col] = ds;
  }
}

// Fixed-order sum of rows: workgroup (64-column block, slice s) sums rows [s chunk, min(R, (s + 1) chunk)) of src (row
// stride rstride) for its 64 columns -- four row groups of 64 lanes take every fourth row, their sums are added in a fixed
// order through LDS.  out != null: the slice's sum goes to out[s * ostride + col] (in place over the slice's first row
// is fine: only this workgroup reads those entries); out == null: dst0[col] += sum (col < L), dst1[col - L] += sum.
constexpr int RS_COLS = 64, RS_GROUPS = 4;
__global__ __launch_bounds__(RS_COLS * RS_GROUPS) void rows_sum_kernel(const float* __restrict__ src, size_t rstride, int R,
                                                                       int chunk, long long W, float* out, size_t ostride,
                                                                       float* __restrict__ dst0, float* __restrict__ dst1,
                                                                       long long L) {
  __shared__ float red[RS_GROUPS][RS_COLS];
  const int cl = threadIdx.x % RS_COLS, grp = threadIdx.x / RS_COLS;
  const long long col = (long long)blockIdx.x * RS_COLS + cl;
  const int r0 = blockIdx.y * chunk, r1 = min(R, r0 + chunk);
  float s = 0.f;
  if (col < W)
    for (int r = r0 + grp; r < r1; r += RS_GROUPS) s += src[(size_t)r * rstride + col];
  red[grp][cl] = s;
  __syncthreads();
  if (grp != 0 || col >= W) return;
#pragma unroll
  for (int k = 1; k < RS_GROUPS; ++k) s += red[k][cl];
  if (out) {
    out[(size_t)blockIdx.y * ostride + col] = s;
  } else if (col < L) {
    if (dst0) dst0[col] += s;
  } else if (dst1) {
    dst1[col - L] += s;
  }
}

// slices for R rows of W-wide work: about 2048 workgroups in flight, at most `cap` slices; -> (S, chunk)
static void plan_slices(int R, long long W, int cap, int& S, int& chunk) {
  const long long gx = W > RS_COLS ? (W + RS_COLS - 1) / RS_COLS : 1;
  long long want = (2048 + gx - 1) / gx;
  want = want < 1 ? 1 : want;
  want = want > cap ? cap : want;
  want = want > R ? R : want;
  chunk = (int)((R + want - 1) / want);
  S = (R + chunk - 1) / chunk;
}

// the S slice sums (rows 0, stride, 2 stride, ... of part) in order, added to dst0 | dst1 (each L wide)
static int add_slices(const float* part, int S, size_t stride, long long L, float* dst0, float* dst1, hipStream_t stream) {
  const unsigned gx = (unsigned)((2 * L + RS_COLS - 1) / RS_COLS);
  hipLaunchKernelGGL(rows_sum_kernel, dim3(gx, 1), dim3(RS_COLS * RS_GROUPS), 0, stream, part, stride, S, S, 2 * L,
                     nullptr, (size_t)0, dst0, dst1, L);
  VITPE_CHECK_LAUNCH();
}

int reduce_parts(float* part, int R, long long L, float* dst0, float* dst1, hipStream_t stream) {
  if (R <= 0 || L <= 0) return 0;
  const long long W = 2 * L;
  int S, chunk;
  plan_slices(R, W, 256, S, chunk);
  if (S == 1) return add_slices(part, R, (size_t)W, L, dst0, dst1, stream);   // (wide enough: one pass)
  if (chunk > 1) {   // pass 1: every slice into its first row
    hipLaunchKernelGGL(rows_sum_kernel, dim3((unsigned)((W + RS_COLS - 1) / RS_COLS), (unsigned)S), dim3(RS_COLS * RS_GROUPS),
                       0, stream, part, (size_t)W, R, chunk, W, part, (size_t)chunk * W, nullptr, nullptr, L);
    const int e = (int)hipGetLastError();
    if (e) return e;
  }
  return add_slices(part, S, (size_t)chunk * W, L, dst0, dst1, stream);   // pass 2
}

}  // namespace vitpe

using namespace vitpe;

extern "C" int vitpe_apply_rotary(const float* x, float* y, const float* cosv, const float* sinv, int B, int H, int P,
                                  int HD, int per_head, hipStream_t st) {
  VITPE_REQUIRE(x && y && cosv && sinv && B >= 0 && H > 0 && P > 0 && HD > 0 && HD % 2 == 0);
  const long long total = (long long)B * H * P * (HD / 2);
  if (total == 0) return 0;
  hipLaunchKernelGGL(rotary_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, y, cosv, sinv, total, H, P, HD / 2, per_head);
  VITPE_CHECK_LAUNCH();
}

static constexpr int ROTARY_BWD_MAX_SLICES = 64;   // include/vitpe.h: workspace of vitpe_apply_rotary_bwd

extern "C" int vitpe_apply_rotary_bwd(const float* dy, const float* x, const float* cosv, const float* sinv, float* dx,
                                      float* dcos, float* dsin, float* workspace, int B, int H, int P, int HD, int per_head,
                                      hipStream_t st) {
  VITPE_REQUIRE(dy && cosv && sinv && B >= 0 && H > 0 && P > 0 && HD > 0 && HD % 2 == 0);
  const bool tables = dcos || dsin;
  VITPE_REQUIRE(!tables || (x && workspace));
  if (B == 0 || !(dx || tables)) return 0;
  const int half = HD / 2;
  const int R = per_head ? B : B * H;
  const long long L = (long long)(per_head ? H : 1) * P * half;
  int S, chunk;
  plan_slices(R, (L + 3) / 4, ROTARY_BWD_MAX_SLICES, S, chunk);   // (256-column blocks here, 64 in plan_slices)
  hipLaunchKernelGGL(rotary_bwd_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)S), dim3(256), 0, st, dy, x, cosv, sinv,
                     dx, tables ? workspace : nullptr, R, chunk, L, half);
  if (!tables) VITPE_CHECK_LAUNCH();
  const int e = (int)hipGetLastError();
  if (e) return e;
  return add_slices(workspace, S, (size_t)2 * L, L, dcos, dsin, st);   // (one row per slice already: the final pass alone)
}
