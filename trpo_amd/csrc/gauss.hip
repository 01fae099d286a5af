// The log-std blocks of a diagonal-Gaussian engine's flat vectors (include/trpo_engine.h, TRPO_DIST_GAUSSIAN).
//
// The network blocks of g and Hv come out of the per-layer launches and the slab reduction, exactly as for the
// categorical policy.  The last A entries, the log-std block, are written here into the reduced vector, as this
// rank's partial, before the all-reduce:
//
//   g_s[d]  = -(1/N) sum_n adv_n r_n (z_nd^2 - 1)     the prepare head leaves the rows adv r (z^2 - 1) [n][ld] in f32;
//                                                     their column sums are taken in f64 in a fixed order
//   Hv_s[d] = 2 v_s[d] (n / N)                        KL_ff's Hessian in s is 2 I per row
//
// The column reduction is two launches: kGaussColBlocks blocks (fewer for small n: a function of n alone) sum
// contiguous row ranges, thread (ty, c) the rows r0 + ty, r0 + ty + RT, ... of column c, then one thread per column
// adds the RT row-thread sums in index order; the finish adds the block partials in index order.  No float atomics,
// so two runs on the same feed give the same bits, and nothing waits on the host, so it is captured with the update.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <stdexcept>

namespace trpo {
namespace {

constexpr int kColThreads = 256, kColLd = 128;   // threads per block; columns of a partial row

// cw: a power of two >= A, <= 128 (the column threads); the block's other kColThreads / cw thread rows stride its rows
__global__ void __launch_bounds__(kColThreads) gauss_colsum_partials_kernel(const float* src, int64_t n, int A, int ld,
                                                                            int cw, int64_t rows_per_block,
                                                                            double* part) {
  __shared__ double sh[kColThreads];
  const int c = threadIdx.x % cw, ty = threadIdx.x / cw, rt = kColThreads / cw;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
  double acc = 0.0;
  if (c < A) {
#pragma unroll 4
    for (int64_t r = r0 + ty; r < r1; r += rt) acc += (double)src[r * ld + c];
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  if (ty == 0 && c < A) {
    double t = 0.0;
    for (int k = 0; k < rt; ++k) t += sh[k * cw + c];
    part[(size_t)blockIdx.x * kColLd + c] = t;
  }
}

__global__ void __launch_bounds__(kColLd) gauss_colsum_finish_kernel(const double* part, int blocks, int A, double scale,
                                                                     float* out_tail, const int* skip) {
  if (skip && *skip) return;
  const int c = threadIdx.x;
  if (c >= A) return;
  double t = 0.0;
  for (int b = 0; b < blocks; ++b) t += part[(size_t)b * kColLd + c];
  out_tail[c] = (float)(scale * t);
}

__global__ void __launch_bounds__(kColLd) gauss_scale_tail_kernel(const float* v_tail, int A, double scale,
                                                                  float* out_tail, const int* skip) {
  if (skip && *skip) return;
  const int c = threadIdx.x;
  if (c < A) out_tail[c] = (float)(scale * (double)v_tail[c]);
}

void check_width(int A, int ld) {
  if (A < 1 || A > kColLd || ld < A) throw std::runtime_error("gauss: act_dim must be in [1, 128] and <= the row stride");
}

}  // namespace

int launch_gauss_colsum_partials(const float* src, int64_t n, int A, int ld, double* part, hipStream_t s) {
  check_width(A, ld);
  if (n <= 0) throw std::runtime_error("gauss: no rows to reduce");
  int cw = 1;
  while (cw < A) cw *= 2;
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(kGaussColBlocks, (n + 1023) / 1024));
  const int64_t rows_per_block = (n + blocks - 1) / blocks;
  hipLaunchKernelGGL(gauss_colsum_partials_kernel, dim3(blocks), dim3(kColThreads), 0, s, src, n, A, ld, cw,
                     rows_per_block, part);
  return blocks;
}

void launch_gauss_colsum_finish(const double* part, int blocks, int A, double scale, float* out_tail, const int* skip,
                                hipStream_t s) {
  check_width(A, A);
  if (blocks < 1 || blocks > kGaussColBlocks) throw std::runtime_error("gauss: bad partial count");
  hipLaunchKernelGGL(gauss_colsum_finish_kernel, dim3(1), dim3(kColLd), 0, s, part, blocks, A, scale, out_tail, skip);
}

void launch_gauss_scale_tail(const float* v_tail, int A, double scale, float* out_tail, const int* skip,
                             hipStream_t s) {
  check_width(A, A);
  hipLaunchKernelGGL(gauss_scale_tail_kernel, dim3(1), dim3(kColLd), 0, s, v_tail, A, scale, out_tail, skip);
}

}  // namespace trpo
