// The Fisher feed's gather (trpo_set_fvp_subsample[_global]): rows first, first + k, first + 2k, ... of the feed into
// the Fisher sub-engine's buffers, device to device, every array in one launch.  `first` is 0 in the local mode and
// the shard's phase (k - row0 % k) % k in the global one; rows are padded to 4 floats, so any first row is 16-byte
// aligned in the wide arrays.
//
// The wide arrays (X, the old distribution / mean, a Gaussian engine's actions) have rows of q 16-byte units at a
// 16-byte-aligned base (row widths are padded to 4 floats, hipMalloc aligns to 256 bytes): one lane moves one unit
// with a 16-byte load and a 16-byte store, consecutive lanes consecutive units of the destination, so a wave writes
// 1 KiB contiguously and reads whole rows.  The per-row scalars (the advantage, a categorical engine's action) are
// 4 bytes a row: one lane gathers four rows with stride k and stores them as one 16-byte unit; the last, partial
// group of four is stored element by element.  The old log-std vector is copied whole.  Every row offset is 64-bit:
// at 8M rows of 128 floats X alone is 4.3 GB.
#include "kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace trpo {

namespace {

__global__ __launch_bounds__(256) void gather_feed_kernel(GatherArgs a) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int s = 0; s < a.nwide; ++s) {
    const GatherWide g = a.wide[s];
    const uint4* __restrict__ src = static_cast<const uint4*>(g.src);
    uint4* __restrict__ dst = static_cast<uint4*>(g.dst);
    const int64_t q = g.q, total = a.n_sub * q, src_step = a.stride * q, src_first = a.first * q;
    for (int64_t u = tid; u < total; u += nthreads) {   // u = row * q + c: the guard of the last tile
      const int64_t row = u / q, c = u - row * q;
      dst[u] = src[src_first + row * src_step + c];
    }
  }
  const int64_t groups = (a.n_sub + 3) / 4;
  for (int s = 0; s < a.nscalar; ++s) {
    const unsigned* __restrict__ src = static_cast<const unsigned*>(a.scalar[s].src) + a.first;
    unsigned* __restrict__ dst = static_cast<unsigned*>(a.scalar[s].dst);
    for (int64_t gi = tid; gi < groups; gi += nthreads) {
      const int64_t r0 = gi * 4;
      if (r0 + 4 <= a.n_sub) {
        uint4 v;
        v.x = src[r0 * a.stride];
        v.y = src[(r0 + 1) * a.stride];
        v.z = src[(r0 + 2) * a.stride];
        v.w = src[(r0 + 3) * a.stride];
        *reinterpret_cast<uint4*>(dst + r0) = v;
      } else {
        for (int64_t r = r0; r < a.n_sub; ++r) dst[r] = src[r * a.stride];
      }
    }
  }
  for (int64_t i = tid; i < a.whole_n; i += nthreads) a.whole_dst[i] = a.whole_src[i];
}

}  // namespace

void launch_gather_feed(const GatherArgs& a, int num_cus, hipStream_t s) {
  if (a.n_sub <= 0) return;
  int64_t units = (a.n_sub + 3) / 4;
  for (int i = 0; i < a.nwide; ++i) units = std::max<int64_t>(units, a.n_sub * a.wide[i].q);
  // eight workgroups of four waves per CU keep 16-byte loads in flight on every SIMD; fewer when the feed is small
  const int64_t want = (units + 255) / 256;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)num_cus * 8));
  hipLaunchKernelGGL(gather_feed_kernel, dim3(grid), dim3(256), 0, s, a);
}

}  // namespace trpo
