// GAE(lambda) advantage estimation: a two-channel segmented reverse scan.
//
// Per path (paths concatenated, starts[t] = 1 marks a path's first step), all float64:
//   end_t   = t + 1 == n or starts[t+1]
//   vnext_t = end_t ? (tail ? tail[t] : 0) : v_{t+1}
//   delta_t = (r_t + gamma vnext_t) - v_t
//   A_t     = end_t ? delta_t            : delta_t + (gamma lambda) A_{t+1}
//   R_t     = end_t ? r_t + gamma vnext_t : r_t + gamma R_{t+1}
// R is scan.hip's discounted return plus the bootstrap tail; A is the GAE advantage (Schulman et al.,
// "High-Dimensional Continuous Control Using Generalized Advantage Estimation", eq. 16).
//
// Each row is a pair of affine maps of the carry (R_{t+1}, A_{t+1}), coefficient gamma for R and
// gamma lambda for A, both cut (coefficient 0) at end_t; pairs compose channel by channel as scan.hip's
// single map does.  The same three passes: (1) per-thread chunks -> thread maps -> block map; (2) one block
// scans the block maps; (3) each thread re-walks its chunk from its carry-in, i.e. inside a chunk the
// arithmetic is exactly the recurrence above.  Every pass reads rewards, values and starts once (tail
// values only at the path-end rows); pass 3 writes both outputs.
//
// Two tiles (rewards, values) are staged in LDS, so the chunk is 8 where scan.hip's is 16: 2048-row tiles,
// 2 x (2048 + 256 pad) x 8 B = 36.9 KB per block, four blocks (16 waves) per CU.  scan.hip's 4096-row tile
// would need 69.7 KB, past the 64 KB a block may allocate statically.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace trpo {

namespace {

constexpr int kChunk = 8;
constexpr int kGaeThreads = 256;
constexpr int kTile = kChunk * kGaeThreads;

// (R, A) channel maps: c -> B + A c
struct Aff2 {
  double Ar, Br, Aa, Ba;
};

constexpr Aff2 kIdentity{1.0, 0.0, 1.0, 0.0};

// F covers earlier rows, G later ones: (F o G)(c) = F(G(c))
__device__ __forceinline__ Aff2 compose(Aff2 F, Aff2 G) {
  return Aff2{F.Ar * G.Ar, F.Br + F.Ar * G.Br, F.Aa * G.Aa, F.Ba + F.Aa * G.Ba};
}

__device__ __forceinline__ Aff2 shfl_down2(Aff2 m, int off) {
  return Aff2{__shfl_down(m.Ar, off, 64), __shfl_down(m.Br, off, 64), __shfl_down(m.Aa, off, 64),
              __shfl_down(m.Ba, off, 64)};
}

// Tiles go through LDS as in scan.hip: loaded and stored by consecutive threads, walked by each thread over
// its own kChunk rows.  A pad double every kChunk puts thread j's chunk at 8 (kChunk + 1) j = 72 j bytes:
// 18 j mod 64 runs over the 32 even banks once per 32 lanes, so the walk's ds_read_b64 is conflict-free.
// The value tile has one more slot, the halo v[T0 + kTile] that its last row's delta reads.
constexpr int kPadT = kTile + kTile / kChunk;
__device__ __forceinline__ int sidx(int i) { return i + i / kChunk; }

__device__ void tiles_load(const double* r, const double* v, int64_t T0, int64_t n, double* sr, double* sv) {
  for (int i = threadIdx.x; i < kTile; i += blockDim.x) {
    const bool in = T0 + i < n;
    sr[sidx(i)] = in ? r[T0 + i] : 0.0;
    sv[sidx(i)] = in && v ? v[T0 + i] : 0.0;
  }
  if (threadIdx.x == 0) sv[sidx(kTile)] = v && T0 + kTile < n ? v[T0 + kTile] : 0.0;
  __syncthreads();
}

// bit i: row t0 + i ends its path (rows at or past n count as ends: they cut the carry and are never stored)
__device__ __forceinline__ unsigned end_mask(const uint8_t* starts, int64_t t0, int64_t n) {
  unsigned m = 0;
#pragma unroll
  for (int i = 0; i < kChunk; ++i) {
    const int64_t t = t0 + i;
    const bool end = t + 1 >= n || (starts && starts[t + 1]);
    m |= (end ? 1u : 0u) << i;
  }
  return m;
}

// One row of the recurrence from the carry (cR, cA) = (R_{t+1}, A_{t+1}); vn = v_{t+1}.
struct Row {
  double R, A;
};
__device__ __forceinline__ Row row_step(double r, double v, double vn, bool end, double tailv, double gamma,
                                        double gl, double cR, double cA) {
  const double vnext = end ? tailv : vn;
  const double rv = r + gamma * vnext;
  const double delta = rv - v;
  return Row{end ? rv : r + gamma * cR, end ? delta : delta + gl * cA};
}

// thread map of rows [t0, t0 + kChunk) (tiles in LDS from T0; i0 = t0 - T0)
__device__ Aff2 chunk_map(const double* sr, const double* sv, int i0, int64_t t0, int64_t n, unsigned ends,
                          const double* tail, double gamma, double gl) {
  Aff2 m = kIdentity;
  double vn = sv[sidx(i0 + kChunk)];
#pragma unroll
  for (int i = kChunk - 1; i >= 0; --i) {
    const bool end = (ends >> i) & 1u;
    const double r = sr[sidx(i0 + i)], v = sv[sidx(i0 + i)];
    const double tailv = end && tail && t0 + i < n ? tail[t0 + i] : 0.0;
    const Row b = row_step(r, v, vn, end, tailv, gamma, gl, m.Br, m.Ba);
    m = Aff2{end ? 0.0 : gamma * m.Ar, b.R, end ? 0.0 : gl * m.Aa, b.A};
    vn = v;
  }
  return m;
}

// Block-wide reverse exclusive scan of maps: S_j = G_{j+1} o ... o G_{T-1} (identity for the last thread)
// and the block total G_0 o ... o G_{T-1}.
__device__ void block_rscan(Aff2 g, Aff2& excl, Aff2& total) {
  __shared__ Aff2 wtot[kGaeThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = blockDim.x >> 6;
  Aff2 inc = g;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const Aff2 o = shfl_down2(inc, off);
    if (lane + off < 64) inc = compose(inc, o);
  }
  Aff2 ex = shfl_down2(inc, 1);
  if (lane == 63) ex = kIdentity;
  if (lane == 0) wtot[wave] = inc;
  __syncthreads();
  Aff2 later = kIdentity;
  for (int w = nw - 1; w > wave; --w) later = compose(wtot[w], later);
  excl = compose(ex, later);
  Aff2 tot = kIdentity;
  for (int w = nw - 1; w >= 0; --w) tot = compose(wtot[w], tot);
  total = tot;
  __syncthreads();
}

__global__ void __launch_bounds__(kGaeThreads)
gae_pass1(const double* r, const double* v, const uint8_t* starts, const double* tail, int64_t n, double gamma,
          double gl, Aff2* blockmaps) {
  __shared__ double sr[kPadT];
  __shared__ double sv[kPadT + 1];
  const int64_t T0 = (int64_t)blockIdx.x * kTile;
  tiles_load(r, v, T0, n, sr, sv);
  const int i0 = threadIdx.x * kChunk;
  const int64_t t0 = T0 + i0;
  const Aff2 g = t0 < n ? chunk_map(sr, sv, i0, t0, n, end_mask(starts, t0, n), tail, gamma, gl) : kIdentity;
  Aff2 ex, tot;
  block_rscan(g, ex, tot);
  if (threadIdx.x == 0) blockmaps[blockIdx.x] = tot;
}

// one block: carry[b] = (G_{b+1} o ... o G_{nb-1})(0, 0), [nb][2]
__global__ void __launch_bounds__(kGaeThreads)
gae_pass2(const Aff2* blockmaps, int64_t nb, double* carry) {
  const int64_t per = (nb + blockDim.x - 1) / blockDim.x;
  const int64_t b0 = (int64_t)threadIdx.x * per;
  const int64_t b1 = b0 + per < nb ? b0 + per : nb;
  Aff2 g = kIdentity;
  for (int64_t b = b1 - 1; b >= b0; --b) g = compose(blockmaps[b], g);
  Aff2 ex, tot;
  block_rscan(g, ex, tot);
  double cR = ex.Br, cA = ex.Ba;   // (suffix)(0, 0)
  for (int64_t b = b1 - 1; b >= b0; --b) {
    carry[2 * b] = cR;
    carry[2 * b + 1] = cA;
    const Aff2 m = blockmaps[b];
    cR = m.Br + m.Ar * cR;
    cA = m.Ba + m.Aa * cA;
  }
}

__global__ void __launch_bounds__(kGaeThreads)
gae_pass3(const double* r, const double* v, const uint8_t* starts, const double* tail, int64_t n, double gamma,
          double gl, const double* carry, double* returns, double* adv) {
  __shared__ double sr[kPadT];
  __shared__ double sv[kPadT + 1];
  const int64_t T0 = (int64_t)blockIdx.x * kTile;
  tiles_load(r, v, T0, n, sr, sv);
  const int i0 = threadIdx.x * kChunk;
  const int64_t t0 = T0 + i0;
  const unsigned ends = end_mask(starts, t0, n);
  // the halo is read here, before any thread's walk replaces its values with advantages
  double vn = sv[sidx(i0 + kChunk)];
  const Aff2 g = t0 < n ? chunk_map(sr, sv, i0, t0, n, ends, tail, gamma, gl) : kIdentity;
  Aff2 ex, tot;
  block_rscan(g, ex, tot);
  double cR = ex.Br + ex.Ar * carry[2 * (int64_t)blockIdx.x];
  double cA = ex.Ba + ex.Aa * carry[2 * (int64_t)blockIdx.x + 1];
  if (t0 < n) {
    // R replaces r and A replaces v in this thread's own LDS slots
#pragma unroll
    for (int i = kChunk - 1; i >= 0; --i) {
      const bool end = (ends >> i) & 1u;
      const double rr = sr[sidx(i0 + i)], vv = sv[sidx(i0 + i)];
      const double tailv = end && tail && t0 + i < n ? tail[t0 + i] : 0.0;
      const Row b = row_step(rr, vv, vn, end, tailv, gamma, gl, cR, cA);
      cR = b.R;
      cA = b.A;
      sr[sidx(i0 + i)] = cR;
      sv[sidx(i0 + i)] = cA;
      vn = vv;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTile && T0 + i < n; i += blockDim.x) {
    if (returns) returns[T0 + i] = sr[sidx(i)];
    if (adv) adv[T0 + i] = sv[sidx(i)];
  }
}

inline int64_t gae_blocks(int64_t n) { return (n + kTile - 1) / kTile; }

}  // namespace

size_t gae_workspace_bytes(int64_t n) {
  const int64_t nb = gae_blocks(n);
  return (size_t)(nb > 0 ? nb : 1) * (sizeof(Aff2) + 2 * sizeof(double)) + 256;
}

void launch_gae(const double* rewards, const double* values, const uint8_t* starts, const double* tail_values,
                int64_t n, double gamma, double lambda, double* adv, double* returns, void* workspace,
                hipStream_t s) {
  if (n <= 0) return;
  const int64_t nb = gae_blocks(n);
  Aff2* maps = reinterpret_cast<Aff2*>(workspace);
  double* carry = reinterpret_cast<double*>(maps + nb);
  const double gl = gamma * lambda;
  hipLaunchKernelGGL(gae_pass1, dim3((unsigned)nb), dim3(kGaeThreads), 0, s, rewards, values, starts, tail_values,
                     n, gamma, gl, maps);
  hipLaunchKernelGGL(gae_pass2, dim3(1), dim3(kGaeThreads), 0, s, maps, nb, carry);
  hipLaunchKernelGGL(gae_pass3, dim3((unsigned)nb), dim3(kGaeThreads), 0, s, rewards, values, starts, tail_values,
                     n, gamma, gl, carry, returns, adv);
}

}  // namespace trpo
