// Device primitives of the split-precision kernels (gfx950), one definition each: the vector types, the scaled
// f16 hi + lo split and its three-product MFMA, the exact bf16 three-way split and its six-product MFMA, the
// running-max slots' two ends (commit, scale exponent), tanh and its derivative, the buffer load as float, the
// LDS-DMA instructions and the 32-lane reductions.
// Free functions in an anonymous namespace (internal linkage per translation unit).
#pragma once
#include "common.h"
#include "kernels.h"

#ifndef TRPO_FAST_TANH
#define TRPO_FAST_TANH 1   // 0: the device library's tanhf in the forward epilogues (A/B builds only)
#endif
#ifndef TRPO_HEAD_DPP
#define TRPO_HEAD_DPP 1    // 0: the row epilogues' head row reductions by ds_bpermute shuffles (A/B builds only)
#endif
#ifndef TRPO_TAIL_DPP
#define TRPO_TAIL_DPP 1    // 0: tail.hip's R-softmax row sums by ds_bpermute shuffles (A/B builds only)
#endif

namespace trpo {

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));   // v_cvt_pkrtz_f16_f32's result type
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));   // ds_read_b64_tr_b16 results
typedef short s16x8 __attribute__((ext_vector_type(8)));

namespace {

__device__ __forceinline__ float one_minus_sq(float h) { return (1.0f - h) * (1.0f + h); }

// tanh for the forward epilogues (trpo_inksci.py:38 `tanh` layers), branch-free: both forms are
// evaluated and one selected, where the device library's tanhf branches per lane (a wave runs both
// sides under exec masks, ~35 VALU per element, which made the tanh epilogue ~2 ms of a 256-wide
// C4 forward GEMM).  |x| < 0.625: x + x^3 P(x^2), the minimax odd polynomial of the device library's
// own small-argument branch; otherwise (1 - t) / (1 + t) with t = 2^(-2|x| log2 e) from v_exp_f32
// and v_rcp_f32 (a few ulp; t underflows to 0 past |x| ~ 44, giving 1).  Sign restored last.
__device__ __forceinline__ float tanh_fast(float x) {
#if TRPO_FAST_TANH
  const float ax = fabsf(x);
  const float x2 = x * x;
  float p = __builtin_fmaf(-0.005700020585209131f, x2, 0.02063407190144062f);   // 0xbbbac73d, 0x3ca908c9
  p = __builtin_fmaf(p, x2, -0.053737930953502655f);                        // 0xbd5c1c4e
  p = __builtin_fmaf(p, x2, 0.13331416249275208f);                         // 0x3e088382
  p = __builtin_fmaf(p, x2, -0.3333328068256378f);                        // 0xbeaaaa99
  const float small = __builtin_fmaf(x2, ax * p, ax);
  const float t = __builtin_amdgcn_exp2f(ax * -2.8853900817779268f);   // 2^(-2|x| log2 e) = e^(-2|x|)
  const float r = __builtin_amdgcn_rcpf(1.0f + t);
  const float big = __builtin_fmaf(-t, r, r);                          // (1 - t) / (1 + t)
  return __builtin_copysignf(ax < 0.625f ? small : big, x);
#else
  return tanhf(x);
#endif
}

// ---- f16 split: an f32 operand x, scaled by a power of two so that its tensor's max lands in [2^11, 2^12)
// (kernels.h f16_scale_exp), is hi + lo with hi = f16(x) and lo = f16(x - hi), and a b ~= ah bh + (ah bl + al bh);
// the dropped al bl is ~2^-22 relative.  f16 MFMA runs at the bf16 rate, so 3 products instead of the bf16
// split's 6 halve the MFMA work; the scales keep every piece a normal f16 down to 2^-15 of the operand's max
// (below that the error is absolute, 2^-36 of the max).

// (a, b) -> {hi pair, lo pair} as packed f16, two elements per conversion (v_cvt_pkrtz_f16_f32).  Round toward
// zero: a - hi is exact in f32 and below ulp16(a), so hi + lo is within 2^-21 |a|.
__device__ __forceinline__ u32x2 split2(float a, float b) {
  const fp16x2 hp = __builtin_amdgcn_cvt_pkrtz(a, b);
  const fp16x2 lp = __builtin_amdgcn_cvt_pkrtz(a - (float)hp[0], b - (float)hp[1]);
  return u32x2{__builtin_bit_cast(unsigned, hp), __builtin_bit_cast(unsigned, lp)};
}
// 8 values times s -> hi and lo, pair by pair
__device__ __forceinline__ void split8(const float* x, float s, f16x8& hi, f16x8& lo) {
  u32x4 H, L;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u32x2 p = split2(x[2 * i] * s, x[2 * i + 1] * s);
    H[i] = p[0];
    L[i] = p[1];
  }
  hi = __builtin_bit_cast(f16x8, H);
  lo = __builtin_bit_cast(f16x8, L);
}
// The same split rounding to nearest, one value at a time (plain conversions): x - hi is exact here too, but may
// be negative and is at most half an ulp16, so hi + lo is within 2^-22 |x|.  Not bit-identical to split2: the
// register-staged k-loops (gemm.hip's split kernels, rbwd0.hip), gemm.hip's weight-plane kernel and tail.hip's
// head-plane pack use it.
__device__ __forceinline__ void split2_rn(float x, unsigned short& h, unsigned short& l) {
  const _Float16 hh = (_Float16)x;
  const _Float16 ll = (_Float16)(x - (float)hh);
  h = __builtin_bit_cast(unsigned short, hh);
  l = __builtin_bit_cast(unsigned short, ll);
}

// c += al bh + ah bl + ah bh, smallest terms first: v_mfma_f32_32x32x16_f16 (f32x16 accumulator; operands as four
// planes or as {hi, lo} arrays) and v_mfma_f32_16x16x32_f16 (f32x4)
__device__ __forceinline__ f32x16 mfma3(const f16x8& ah, const f16x8& al, const f16x8& bh, const f16x8& bl,
                                        f32x16 c) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma3(const f16x8 (&a)[2], const f16x8 (&b)[2], f32x16 c) {
  return mfma3(a[0], a[1], b[0], b[1], c);
}
__device__ __forceinline__ f32x4 mfma3(const f16x8 (&a)[2], const f16x8 (&b)[2], f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[1], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0], b[1], c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a[0], b[0], c, 0, 0, 0);
}

// ---- bf16 split.  CDNA4 has no reduced-precision f32 MFMA, but bf16 MFMA runs at 16x the f32 rate.  Each f32
// operand x is split exactly into three bf16 pieces x = h + m + l + O(2^-27 |x|) (h = bf16(x), m = bf16(x - h),
// l = bf16(x - h - m); both differences are exact in f32) and
//     a b ~= ah bh + (ah bm + am bh) + (ah bl + al bh + am bm)
// keeps every product term down to 2^-18 relative; the dropped ones (am bl, al bm, al bl) are < 2^-26 relative,
// below the f32 rounding of the sum.  The pieces' products are exact in the MFMA's f32 accumulation, so the
// result matches an f32 GEMM to f32 rounding at 16/6 = 2.7x its MFMA peak.
__device__ __forceinline__ unsigned short bf16_bits(float x) { return __builtin_bit_cast(unsigned short, (__bf16)x); }
__device__ __forceinline__ float bf16_val(unsigned short b) { return __builtin_bit_cast(float, (unsigned)b << 16); }
__device__ __forceinline__ void split3(float x, unsigned short& h, unsigned short& m, unsigned short& l) {
  h = bf16_bits(x);
  const float r1 = x - bf16_val(h);
  m = bf16_bits(r1);
  const float r2 = r1 - bf16_val(m);
  l = bf16_bits(r2);
}
// c += a b over the {h, m, l} planes, smallest terms first (the 6 products with plane(a) + plane(b) <= 2):
// v_mfma_f32_32x32x16_bf16 (f32x16 accumulator) and v_mfma_f32_16x16x32_bf16 (f32x4)
__device__ __forceinline__ f32x16 mfma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16 c) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], c, 0, 0, 0);
}

// ---- scales.  The max of a running-max slot (its kAmaxSub counters, kAmaxSub / 64 per lane) -> power-of-two
// scale exponent; all lanes of the wave must call it
__device__ __forceinline__ int amax_exp(const unsigned* amax) {
  if (!amax) return f16_scale_exp(1.0f);
  const int lane = threadIdx.x & 63;
  float v = 0.0f;
#pragma unroll
  for (int i = 0; i < kAmaxSub / 64; ++i) v = fmaxf(v, __uint_as_float(amax[(lane + 64 * i) * kAmaxStride]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return f16_scale_exp(v);
}
// workgroup max of v[i] >= 0 for the non-NULL slots, one atomicMax per slot per workgroup (float bits
// order as unsigned for v >= 0) into the slot's counter for this block (kernels.h, kAmaxSub).
// Every thread of the block must call it.
// (`ext`, when given, is 48 floats of the caller's LDS to use instead of a static array: kernels whose
// one LDS array already takes the whole 160 KB.)
template <bool EXT = false>
__device__ __forceinline__ void amax_commit3(unsigned* s0, float v0, unsigned* s1, float v1, unsigned* s2, float v2,
                                             float (*ext)[16] = nullptr) {
  if (!s0 && !s1 && !s2) return;
  float(*red)[16];
  if constexpr (EXT) {
    red = ext;
  } else {
    __shared__ float red_own[3][16];
    red = red_own;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    v0 = fmaxf(v0, __shfl_xor(v0, off, 64));
    v1 = fmaxf(v1, __shfl_xor(v1, off, 64));
    v2 = fmaxf(v2, __shfl_xor(v2, off, 64));
  }
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wave] = v0;
    red[1][wave] = v1;
    red[2][wave] = v2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned* slot = threadIdx.x == 0 ? s0 : (threadIdx.x == 1 ? s1 : s2);
    if (slot) {
      float m = 0.0f;
      for (int w = 0; w < nw; ++w) m = fmaxf(m, red[threadIdx.x][w]);
      const unsigned bid = blockIdx.x + blockIdx.y * 7919u + blockIdx.z * 104729u;
      if (m > 0.0f) atomicMax(slot + (bid % kAmaxSub) * kAmaxStride, __float_as_uint(m));
    }
  }
}

template <int TM, int TN>
__device__ __forceinline__ void scale_acc(f32x16 (&acc)[TM][TN], int e) {
  if (e == 0) return;
  const float f = __builtin_ldexpf(1.0f, e);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] *= f;
}

// one buffer_load_dword as float: descriptor, per-lane byte offset, scalar byte offset
__device__ __forceinline__ float ldbuf(__amdgpu_buffer_rsrc_t r, int vo, int so) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, vo, so, 0));
}

// LDS images of [row][16 k] 16-bit values (32-B rows, no padding): the two 16-B k-chunks of a row swap places
// where bit 2 ^ bit 3 of the row is set.  The ds_read_b128 fragment reads, serviced in the lane groups
// {0-3,12-15,20-27}, {4-11,16-19,28-31} (+32), then put their 16 rows on 16 distinct 16-B bank slots, and so do
// the weight-gradient staging stores -- ds_write_b128, 8 lanes per LDS cycle on 32 banks, 8 consecutive rows of
// one chunk -- which a bit-3-only flip left 2-way conflicted, rows r and r+4 on the same banks.
__device__ __forceinline__ int swz16(int row, int chunk) {
  return row * 16 + ((chunk ^ (((row >> 2) ^ (row >> 3)) & 1)) << 3);
}

// ---- LDS-DMA: one instruction moves 16 B per lane into LDS at the wave-uniform byte address `lds` + 16 * lane
// (M0; the destination is lane-linear).  Inline asm, opaque to hipcc's s_waitcnt bookkeeping (the builtin form
// makes hipcc drain vmcnt(0) before every later LDS read), so the caller counts completion itself.  M0 is saved
// and restored around it: the compiler owns M0.
// Global form (global_load_lds_dwordx4) from the per-lane pointer `src`.
__device__ __forceinline__ void glds16(const void* src, const void* lds) {
  unsigned keep;
  const unsigned dst = (unsigned)(uintptr_t)lds;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(src), "s"(__builtin_amdgcn_readfirstlane(dst))
               : "memory");
}
// Buffer form (buffer_load_dwordx4 ... offen lds) from the descriptor `rsrc` at the per-lane byte offset `voff`
// plus the scalar one `soff`.  No "memory" clobber: the DMA writes a ring slot that no LDS read of the stage
// in flight touches, the callers' barriers order it against the reads of other stages, and a clobber would pin
// every address-taken local to the stack.
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff, unsigned lds) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %4 offen lds\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(rsrc), "s"(lds), "s"(soff));
}

// ---- 32-lane (wave-half) reductions: DPP moves + one lane swap (common.h), or, for A/B builds, ds_bpermute
// shuffles.  DPP is the caller's switch: TRPO_HEAD_DPP (rowepi.h) or TRPO_TAIL_DPP (tail.hip), one thing under
// two names so that either file can be switched alone.
template <bool DPP, class T>
__device__ __forceinline__ T sum32(T v) {
  if constexpr (DPP) return sum32_dpp(v);
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 32);
  return v;
}
template <bool DPP>
__device__ __forceinline__ float max32(float v) {
  if constexpr (DPP) return max32_dpp(v);
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 32));
  return v;
}

}  // namespace
}  // namespace trpo
