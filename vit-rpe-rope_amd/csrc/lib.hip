// The library's version and the self-tests of the primitives every kernel relies on.
#include "common.h"

namespace vitpe {

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
