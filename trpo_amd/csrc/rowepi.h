// The fused row epilogues of the row-GEMM kernels (gemm.hip, plane.hip, rbwd0.hip) and their running-max
// bookkeeping.  Everything is in an anonymous namespace (internal linkage per translation unit).
#pragma once
#include "split.h"

#ifndef TRPO_EPI_PIPE
#define TRPO_EPI_PIPE 1    // 0: epilogue operand loads chunk by chunk (A/B builds only)
#endif
#ifndef TRPO_EPI_TRACK
#define TRPO_EPI_TRACK 1   // ablation builds only (tools): 0 drops the f16 running-max tracking
#endif
#ifndef TRPO_PREP_HEAD64
#define TRPO_PREP_HEAD64 0 // 1: the prepare head's KL / surr logit deltas in f64 (round-4 form; A/B only)
#endif
#ifndef TRPO_HEAD_LOG64
#define TRPO_HEAD_LOG64 0  // 1: the loss heads' logs in f64 (round-1 form; A/B only)
#endif

namespace trpo {
namespace {

// ---------------------------------------------------------------------------
// element-wise epilogues (one accumulator element at (row, col))
// ---------------------------------------------------------------------------
template <int EPI>
__device__ __forceinline__ void epi_elem(const RowEpiArgs& e, int row, int col, bool real, float v) {
  const size_t idx = (size_t)row * e.ldo + col;
  if constexpr (EPI == (int)RowEpi::kTanh) {
    e.out0[idx] = real ? tanh_fast(v + e.bias[col]) : 0.0f;
  } else if constexpr (EPI == (int)RowEpi::kRHidden) {
    e.out0[idx] = real ? one_minus_sq(e.H[idx]) * (v + e.bias[col]) : 0.0f;
  } else if constexpr (EPI == (int)RowEpi::kRZ) {
    e.out0[idx] = real ? v + e.bias[col] : 0.0f;
  } else if constexpr (EPI == (int)RowEpi::kPrepBwd) {
    if (real) {
      const float h = e.H[idx];
      e.out0[idx] = v * one_minus_sq(h);
      e.out1[idx] = -2.0f * v * h;
    } else {
      e.out0[idx] = 0.0f;
      e.out1[idx] = 0.0f;
    }
  } else if constexpr (EPI == (int)RowEpi::kPrepBwdE) {
    e.out0[idx] = real ? -2.0f * v * e.H[idx] : 0.0f;
  } else if constexpr (EPI == (int)RowEpi::kPgBwd) {
    e.out0[idx] = real ? v * one_minus_sq(e.H[idx]) : 0.0f;
  } else if constexpr (EPI == (int)RowEpi::kRBwd) {
    e.out0[idx] = real ? fmaf(e.E[idx], e.RH[idx], v * one_minus_sq(e.H[idx])) : 0.0f;
  } else if constexpr (EPI == (int)RowEpi::kRelu) {
    e.out0[idx] = real ? fmaxf(v + e.bias[col], 0.0f) : 0.0f;
  } else if constexpr (EPI == (int)RowEpi::kReluBwd) {
    e.out0[idx] = (real && e.H[idx] > 0.0f) ? v : 0.0f;
  }
}

// value part (loads + math) and store part of the element-wise epilogues.
// No column predicate: padding columns (col >= N) have zero accumulators (zero
// weight padding), zero bias and zero H/E/RH padding, so every formula below
// already yields exactly 0 there.  Loads are therefore unconditional and hipcc
// keeps them all in flight (a `cond ? load : 0` becomes a branch per load).
template <int EPI>
__device__ __forceinline__ void epi_elem_v(const RowEpiArgs& e, size_t idx, bool /*real*/, float v, float bv,
                                           float& o0, float& o1) {
  if constexpr (EPI == (int)RowEpi::kTanh) {
    o0 = tanh_fast(v + bv);
  } else if constexpr (EPI == (int)RowEpi::kRHidden) {
    o0 = one_minus_sq(e.H[idx]) * (v + bv);
  } else if constexpr (EPI == (int)RowEpi::kRZ) {
    o0 = v + bv;
  } else if constexpr (EPI == (int)RowEpi::kPrepBwd) {
    const float h = e.H[idx];
    o0 = v * one_minus_sq(h);
    o1 = -2.0f * v * h;
  } else if constexpr (EPI == (int)RowEpi::kPrepBwdE) {
    o0 = -2.0f * v * e.H[idx];
  } else if constexpr (EPI == (int)RowEpi::kPgBwd) {
    o0 = v * one_minus_sq(e.H[idx]);
  } else if constexpr (EPI == (int)RowEpi::kRBwd) {
    o0 = fmaf(e.E[idx], e.RH[idx], v * one_minus_sq(e.H[idx]));
  } else if constexpr (EPI == (int)RowEpi::kRelu) {
    o0 = fmaxf(v + bv, 0.0f);
  } else if constexpr (EPI == (int)RowEpi::kReluBwd) {
    o0 = e.H[idx] > 0.0f ? v : 0.0f;
  }
}
template <int EPI>
__device__ __forceinline__ void epi_store(const RowEpiArgs& e, size_t idx, float o0, float o1) {
  e.out0[idx] = o0;
  if constexpr (EPI == (int)RowEpi::kPrepBwd) e.out1[idx] = o1;
}


// ---------------------------------------------------------------------------
// row-wise softmax-head epilogues.  The row's columns live on the 32 lanes of one wave half, TN
// per lane (col = 32 t + (lane & 31), t < TN): n_actions <= 32 TN.  Row reductions sum the TN
// values of a lane first, then xor-shuffle over the 32 lanes.
// ---------------------------------------------------------------------------
template <int EPI, int TN>
__device__ __forceinline__ void epi_row(const RowEpiArgs& e, int row, bool rowvalid, int lr, int A,
                                        const float (&v)[TN], float& m0, float& m1, float& m2) {
  // `row` is already clamped into [0, M); loads go to clamped (valid) addresses
  // unconditionally and are masked by selects, so hipcc keeps them in flight.
  bool real[TN];
  size_t idx[TN];
  bool st[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const int col = 32 * t + lr;
    real[t] = col < A;
    const int colc = col < e.ldo ? col : e.ldo - 1;
    idx[t] = (size_t)row * e.ldo + colc;
    st[t] = rowvalid && col < e.ldo;
  }
  if constexpr (EPI == (int)RowEpi::kPrepHead || EPI == (int)RowEpi::kLossHead) {
    const int av = e.act[row];
    const float advv = e.adv[row];
    float z[TN], oldv[TN];
    float zm = -INFINITY;
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const float bias = e.bias[real[t] ? 32 * t + lr : 0];
      oldv[t] = e.old[idx[t]];
      // p = softmax(z)   (trpo_inksci.py:40)
      z[t] = real[t] ? v[t] + bias : -INFINITY;
      zm = fmaxf(zm, z[t]);
    }
    const float m = max32<TRPO_HEAD_DPP>(zm);
    float ex[TN], es = 0.0f;
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      ex[t] = real[t] ? expf(z[t] - m) : 0.0f;
      es += ex[t];
    }
    const float ssum = sum32<TRPO_HEAD_DPP>(es);
    const int a = rowvalid ? av : 0;
    float p[TN], old[TN];
    float pa_l = 0.0f, olda_l = 0.0f;
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      p[t] = ex[t] / ssum;
      old[t] = (rowvalid && real[t]) ? oldv[t] : 0.0f;
      if (t == (a >> 5)) {
        pa_l = p[t];
        olda_l = old[t];
      }
    }
    const float pa = __shfl(pa_l, a & 31, 32);
    const float olda = __shfl(olda_l, a & 31, 32);
    const float adv = rowvalid ? advv : 0.0f;
    // row loss terms (:46-51)
#if TRPO_HEAD_LOG64
    double klp = 0.0, enp = 0.0;
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const double pd = p[t], od = old[t];
      klp += real[t] ? od * log((od + (double)kEps) / (pd + (double)kEps)) : 0.0;
      enp += real[t] ? -pd * log(pd + (double)kEps) : 0.0;
    }
    const double klt = sum32<TRPO_HEAD_DPP>(klp);
    const double ent = sum32<TRPO_HEAD_DPP>(enp);
#else
    // the reference's own precision (f32 tensors, trpo_inksci.py:50-51): f32 logs and f32 row sums of <= 32 TN
    // terms; the sums over rows are f64 (rowterms)
    float klp = 0.0f, enp = 0.0f;
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const float lk = logf((old[t] + kEps) / (p[t] + kEps)), le = logf(p[t] + kEps);
      klp += real[t] ? old[t] * lk : 0.0f;
      enp += real[t] ? -p[t] * le : 0.0f;
    }
    const double klt = sum32<TRPO_HEAD_DPP>(klp);
    const double ent = sum32<TRPO_HEAD_DPP>(enp);
#endif
    const double sur = rowvalid ? (double)pa / (double)olda * (double)adv : 0.0;
    if (rowvalid && lr == 0) {
      e.rowterms[4 * (size_t)row + 0] = sur;
      e.rowterms[4 * (size_t)row + 1] = klt;
      e.rowterms[4 * (size_t)row + 2] = ent;
      e.rowterms[4 * (size_t)row + 3] = 0.0;
    }
    if constexpr (EPI == (int)RowEpi::kPrepHead) {
      // KL_ff plain logit delta (:56-57), cancellation-free, in f32 (f64 took 40 % of this launch at C4; the
      // O(eps) terms it feeds reach Hv only through D and E, far below f32 rounding of Hv):
      //   d_j = (p_j/N) (B_j - sum_k p_k B_k),  B = eps/(p+eps)
#if TRPO_PREP_HEAD64
      typedef double T;
#else
      typedef float T;
#endif
      const T invN = (T)e.invN;
      T B[TN], spBp = 0, restp = 0;
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const T pd = p[t];
#if TRPO_PREP_HEAD64
        B[t] = real[t] ? (T)kEps / (pd + (T)kEps) : T(0);
#else
        B[t] = real[t] ? kEps * __builtin_amdgcn_rcpf(pd + kEps) : 0.0f;   // O(eps) term: 1-ulp v_rcp_f32
#endif
        spBp += pd * B[t];
        restp += (real[t] && 32 * t + lr != a) ? pd : T(0);
      }
      const T spB = sum32<TRPO_HEAD_DPP>(spBp);
      const T rest = sum32<TRPO_HEAD_DPP>(restp);   // 1 - p_a
      // surr logit delta (:54): -(adv/(N old_a)) p_a (1[j=a] - p_j)
      const T coef = -(T)adv * invN / (T)olda * (T)pa;
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const int col = 32 * t + lr;
        const T pd = p[t];
        const float dl = real[t] ? (float)(pd * invN * (B[t] - spB)) : 0.0f;
        const float ds = real[t] ? (float)(coef * (col == a ? rest : -pd)) : 0.0f;
        if (st[t]) {
          const size_t sidx = (size_t)row * e.ldo + col;
          e.out0[sidx] = real[t] ? p[t] : 0.0f;
          e.out1[sidx] = (float)dl;
          e.out2[sidx] = (float)ds;
          m1 = fmaxf(m1, fabsf((float)dl));
          m2 = fmaxf(m2, fabsf((float)ds));
        }
      }
    }
  } else if constexpr (EPI == (int)RowEpi::kRHead) {
    // R-softmax + R-reverse of the KL_ff head:
    //   Rp   = p (Rz - <p,Rz>)
    //   RD_j = (1/N)[Rp_j (B_j - sum p B) + Rp_j A_j^2 + p_j sum_k Rp_k A_k B_k]
    //   A = p/(p+eps), B = eps/(p+eps)
    double rz[TN], pd[TN], przp = 0.0;
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const float bias = e.bias[real[t] ? 32 * t + lr : 0];
      const float pv = e.P[idx[t]];
      rz[t] = real[t] ? (double)(v[t] + bias) : 0.0;
      pd[t] = (rowvalid && real[t]) ? (double)pv : 0.0;
      przp += pd[t] * rz[t];
    }
    const double prz = sum32<TRPO_HEAD_DPP>(przp);
    double Rp[TN], Aa[TN], B[TN], spBp = 0.0, sRABp = 0.0;
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      Rp[t] = pd[t] * (rz[t] - prz);
      const double den = pd[t] + (double)kEps;
      Aa[t] = real[t] ? pd[t] / den : 0.0;
      B[t] = real[t] ? (double)kEps / den : 0.0;
      spBp += pd[t] * B[t];
      sRABp += Rp[t] * Aa[t] * B[t];
    }
    const double spB = sum32<TRPO_HEAD_DPP>(spBp);
    const double sRAB = sum32<TRPO_HEAD_DPP>(sRABp);
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const double rd = e.invN * (Rp[t] * (B[t] - spB) + Rp[t] * Aa[t] * Aa[t] + pd[t] * sRAB);
      if (st[t]) {
        e.out0[(size_t)row * e.ldo + 32 * t + lr] = real[t] ? (float)rd : 0.0f;
        if (real[t]) m0 = fmaxf(m0, fabsf((float)rd));
      }
    }
  }
}

// ---------------------------------------------------------------------------
// row-wise diagonal-Gaussian head epilogues (include/trpo_engine.h, TRPO_DIST_GAUSSIAN), in the softmax heads'
// lane layout.  The mean is the f32 accumulator plus bias; everything formed from it (z, z0, the log-ratio, the KL
// and entropy terms) is f64: the KL and the log-ratio are differences of near-equal terms.  What depends on the
// column alone is computed once per thread (gauss_cols), not per row.
// ---------------------------------------------------------------------------
template <int TN>
struct GaussCols {
  float bias[TN];
  double s[TN], s0[TN];      // log-std, old log-std
  double is[TN], is0[TN];    // 1 / sigma, 1 / sigma0
  double k[TN];              // prep / loss: sigma0^2 / sigma^2 ; R head: 1 / (sigma^2 N)
};
template <int EPI, int TN>
__device__ __forceinline__ GaussCols<TN> gauss_cols(const RowEpiArgs& e, int lr, int A) {
  GaussCols<TN> c;
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const int col = 32 * t + lr;
    const int cc = col < A ? col : 0;
    c.bias[t] = e.bias[cc];
    c.s[t] = (double)e.logstd[cc];
    c.is[t] = exp(-c.s[t]);
    if constexpr (EPI == (int)RowEpi::kGaussRHead) {
      c.s0[t] = c.s[t];
      c.is0[t] = c.is[t];
      c.k[t] = c.is[t] * c.is[t] * e.invN;
    } else {
      c.s0[t] = (double)e.logstd0[cc];
      c.is0[t] = exp(-c.s0[t]);
      c.k[t] = exp(2.0 * (c.s0[t] - c.s[t]));
    }
  }
  return c;
}

template <int EPI, int TN>
__device__ __forceinline__ void epi_row_gauss(const RowEpiArgs& e, const GaussCols<TN>& c, int row, bool rowvalid,
                                              int lr, int A, const float (&v)[TN], float& m0, float& m2) {
  // `row` is clamped into [0, M) by the caller, columns into [0, ldo): loads are unconditional, masked by selects
  bool real[TN], st[TN];
  size_t idx[TN];
#pragma unroll
  for (int t = 0; t < TN; ++t) {
    const int col = 32 * t + lr;
    real[t] = col < A;
    const int colc = col < e.ldo ? col : e.ldo - 1;
    idx[t] = (size_t)row * e.ldo + colc;
    st[t] = rowvalid && col < e.ldo;
  }
  if constexpr (EPI == (int)RowEpi::kGaussRHead) {
    // RD_L = R{mu} / (sigma^2 N), R{mu} = acc + c (the tangent bias)
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const float rd = real[t] ? (float)((double)(v[t] + c.bias[t]) * c.k[t]) : 0.0f;
      if (st[t]) {
        e.out0[(size_t)row * e.ldo + 32 * t + lr] = rd;
        m0 = fmaxf(m0, fabsf(rd));
      }
    }
  } else {
    const float advv = e.adv[row];
    float mu[TN];
    double z[TN], lrp = 0.0, klp = 0.0, enp = 0.0;
#pragma unroll
    for (int t = 0; t < TN; ++t) {
      const float av = e.actf[idx[t]], m0v = e.old[idx[t]];
      mu[t] = v[t] + c.bias[t];
      const bool on = rowvalid && real[t];
      const double a = (double)av, mud = (double)mu[t], mu0 = (double)m0v;
      z[t] = on ? (a - mud) * c.is[t] : 0.0;
      const double z0 = on ? (a - mu0) * c.is0[t] : 0.0;
      const double dm = on ? (mu0 - mud) * c.is[t] : 0.0;
      // log r = sum_d (s0 - s) + (z0^2 - z^2)/2 ; KL(old || new) ; entropy
      lrp += on ? (c.s0[t] - c.s[t]) + 0.5 * (z0 * z0 - z[t] * z[t]) : 0.0;
      klp += on ? (c.s[t] - c.s0[t]) + 0.5 * (c.k[t] + dm * dm) - 0.5 : 0.0;
      enp += on ? c.s[t] + 1.4189385332046727 : 0.0;   // 0.5 ln(2 pi e)
    }
    const double logr = sum32<TRPO_HEAD_DPP>(lrp);
    const double klt = sum32<TRPO_HEAD_DPP>(klp);
    const double ent = sum32<TRPO_HEAD_DPP>(enp);
    const double ar = rowvalid ? (double)advv * exp(logr) : 0.0;   // adv_n r_n
    if (rowvalid && lr == 0) {
      e.rowterms[4 * (size_t)row + 0] = ar;
      e.rowterms[4 * (size_t)row + 1] = klt;
      e.rowterms[4 * (size_t)row + 2] = ent;
      e.rowterms[4 * (size_t)row + 3] = 0.0;
    }
    if constexpr (EPI == (int)RowEpi::kGaussPrepHead) {
      // DS_L = -(adv r / N) z / sigma ; the rows of g_s: adv r (z^2 - 1)
      const double coef = -ar * e.invN;
#pragma unroll
      for (int t = 0; t < TN; ++t) {
        const float ds = real[t] ? (float)(coef * z[t] * c.is[t]) : 0.0f;
        const float gs = real[t] ? (float)(ar * (z[t] * z[t] - 1.0)) : 0.0f;
        if (st[t]) {
          const size_t sidx = (size_t)row * e.ldo + 32 * t + lr;
          e.out0[sidx] = real[t] ? mu[t] : 0.0f;
          e.out1[sidx] = gs;
          e.out2[sidx] = ds;
          m2 = fmaxf(m2, fabsf(ds));
        }
      }
    }
  }
}

// Linear block id -> (m-tile, n-tile).  The n-tiles of one row tile are adjacent in
// the swizzled order and land on one XCD (blocks b and b+8 share an XCD under the
// observed round-robin dispatch: speed only, never correctness), so the second
// n-tile re-reads the A rows from that XCD's L2.
__device__ __forceinline__ void tile_of(int ntn, int& mt, int& nt) {
  const int id = blockIdx.x, nwg = gridDim.x;
  int swz = id;
  if ((nwg & 7) == 0) swz = (id & 7) * (nwg >> 3) + (id >> 3);
  mt = swz / ntn;
  nt = swz - mt * ntn;
}

// Full-width tile of the element-wise epilogues: every epilogue operand goes through a per-block buffer
// descriptor (base = row m0, num_records = the rows this tile owns), so a load/store is one buffer op with
// a lane-constant voffset and a per-row SGPR soffset; rows past M fall outside the descriptor (loads read
// 0, stores are dropped) -- no per-element predicate, no 64-bit address math, and all 16 loads of a chunk
// stay in flight.
template <int WM, int WN, int TM, int TN, int EPI>
__device__ __forceinline__ void row_epi_full(const RowGemmArgs& args, f32x16 (&acc)[TM][TN], int m0, int n0, int wm,
                                             int wn, int lr, int lh, float& mx0, float& mx1) {
  constexpr int BM = WM * TM * 32;
  const int M = args.M;
  const RowEpiArgs& e = args.ea;
  const int ldo = e.ldo;
  const int Mt = M - m0 < BM ? M - m0 : BM;
  const int tile_bytes = Mt * ldo * 4;
  auto mk = [&](const float* ptr) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(ptr + (size_t)m0 * ldo), 0, tile_bytes, 0x00020000);
  };
  constexpr bool kUsesH = EPI == (int)RowEpi::kRHidden || EPI == (int)RowEpi::kPrepBwd ||
                          EPI == (int)RowEpi::kPrepBwdE || EPI == (int)RowEpi::kPgBwd ||
                          EPI == (int)RowEpi::kRBwd || EPI == (int)RowEpi::kReluBwd;
  constexpr bool kRB = EPI == (int)RowEpi::kRBwd;
  constexpr bool kPB = EPI == (int)RowEpi::kPrepBwd;
  constexpr bool kPE = EPI == (int)RowEpi::kPrepBwdE;
  // descriptors of operands an epilogue does not use alias out0 and are never touched
  const __amdgpu_buffer_rsrc_t rO0 = mk(e.out0);
  const __amdgpu_buffer_rsrc_t rH = mk(kUsesH ? e.H : e.out0);
  const __amdgpu_buffer_rsrc_t rE = mk(kRB ? e.E : e.out0);
  const __amdgpu_buffer_rsrc_t rRH = mk(kRB ? e.RH : e.out0);
  const __amdgpu_buffer_rsrc_t rO1 = mk(kPB ? e.out1 : e.out0);
  const int vbase = ((wm * TM * 32 + 4 * lh) * ldo + n0 + wn * TN * 32 + lr) * 4;
  auto st = [&](float v, __amdgpu_buffer_rsrc_t r, int vo, int so) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, vo, so, 0);
  };
  // Operand loads run one (tm, tn) chunk ahead of the chunk being computed and stored: the
  // chunk's loads are issued before the previous chunk's stores in program order (hipcc cannot
  // prove the descriptors disjoint, so it would not hoist them itself), which leaves one chunk
  // of loads in flight behind every chunk of math instead of a full round trip per chunk.
  constexpr int NL = kRB ? 3 : (kUsesH ? 1 : 0);
  constexpr int NCH = TM * TN;
  float pre[2][NL > 0 ? NL : 1][16];
  auto load_chunk = [&](int c, float (&dst)[NL > 0 ? NL : 1][16]) {
    if constexpr (NL > 0) {
      const int tn = c / TM, tm = c % TM;
      const int vo = vbase + tn * 128;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int so = (tm * 32 + (r & 3) + 8 * (r >> 2)) * ldo * 4;
        dst[0][r] = ldbuf(rH, vo, so);
        if constexpr (NL == 3) {
          dst[1][r] = ldbuf(rE, vo, so);
          dst[2][r] = ldbuf(rRH, vo, so);
        }
      }
    }
  };
  if constexpr (TRPO_EPI_PIPE) load_chunk(0, pre[0]);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int tn = c / TM, tm = c % TM;
    const int col = n0 + wn * TN * 32 + tn * 32 + lr;
    float bv = 0.0f;
    if constexpr (EPI == (int)RowEpi::kTanh || EPI == (int)RowEpi::kRHidden || EPI == (int)RowEpi::kRelu ||
                  EPI == (int)RowEpi::kRZ)
      bv = e.bias[col < args.N ? col : 0] * (col < args.N ? 1.0f : 0.0f);
    const int vo = vbase + tn * 128;
    if constexpr (TRPO_EPI_PIPE) {
      if (c + 1 < NCH) load_chunk(c + 1, pre[(c + 1) & 1]);
    } else {
      load_chunk(c, pre[c & 1]);
    }
    const float (&op)[NL > 0 ? NL : 1][16] = pre[c & 1];
    {
      float o0[16], o1[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = acc[tm][tn][r];
        if constexpr (EPI == (int)RowEpi::kTanh) {
          o0[r] = tanh_fast(v + bv);
        } else if constexpr (EPI == (int)RowEpi::kRHidden) {
          o0[r] = one_minus_sq(op[0][r]) * (v + bv);
        } else if constexpr (EPI == (int)RowEpi::kRZ) {
          o0[r] = v + bv;
        } else if constexpr (kPB) {
          const float h = op[0][r];
          o0[r] = v * one_minus_sq(h);
          o1[r] = -2.0f * v * h;
        } else if constexpr (kPE) {
          o0[r] = -2.0f * v * op[0][r];
        } else if constexpr (EPI == (int)RowEpi::kPgBwd) {
          o0[r] = v * one_minus_sq(op[0][r]);
        } else if constexpr (EPI == (int)RowEpi::kRelu) {
          o0[r] = fmaxf(v + bv, 0.0f);
        } else if constexpr (EPI == (int)RowEpi::kReluBwd) {
          o0[r] = op[0][r] > 0.0f ? v : 0.0f;
        } else {
          o0[r] = fmaf(op[1][r], op[2][r], v * one_minus_sq(op[0][r]));
        }
        // running max for the f16 operand scales (rows past M -- dropped stores -- hold 0 or,
        // for kRHidden, the tangent bias: harmless in a max)
        if constexpr (TRPO_EPI_TRACK && EPI != (int)RowEpi::kTanh && EPI != (int)RowEpi::kRelu &&
                      EPI != (int)RowEpi::kReluBwd && EPI != (int)RowEpi::kPrepBwdE) {
          mx0 = fmaxf(mx0, fabsf(o0[r]));
          if constexpr (kPB) mx1 = fmaxf(mx1, fabsf(o1[r]));
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int so = (tm * 32 + (r & 3) + 8 * (r >> 2)) * ldo * 4;
        st(o0[r], rO0, vo, so);
        if constexpr (kPB) st(o1[r], rO1, vo, so);
      }
    }
  }
}

// Fused epilogue of a row-GEMM tile.  The accumulator layout (col = lane&31,
// row = (r&3) + 8(r>>2) + 4(lane>>5)) is the same for the f32 (32x32x2) and the
// bf16 (32x32x16) MFMA, so both row-GEMM kernels share it.
template <int WM, int WN, int TM, int TN, int EPI, bool EXT_RED = false>
__device__ __forceinline__ void row_epilogue(const RowGemmArgs& args, f32x16 (&acc)[TM][TN], int m0, int n0,
                                             int wm, int wn, int lr, int lh, float (*red)[16] = nullptr) {
  constexpr int BN = WN * TN * 32;
  const int M = args.M;
  const RowEpiArgs& e = args.ea;
  float mx0 = 0.0f, mx1 = 0.0f, mx2 = 0.0f;   // max |stored output| for the f16 operand scales
  if constexpr (epi_is_head(EPI)) {
    static_assert(WN == 1, "row-wise head epilogue needs the whole row in one wave half");
    if constexpr (epi_is_gauss(EPI)) {
      const GaussCols<TN> gc = gauss_cols<EPI, TN>(e, lr, args.N);
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m0 + wm * TM * 32 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          float v[TN];
#pragma unroll
          for (int t = 0; t < TN; ++t) v[t] = acc[tm][t][r];
          epi_row_gauss<EPI, TN>(e, gc, row < M ? row : 0, row < M, lr, args.N, v, mx0, mx2);
        }
    } else {
#pragma unroll
      for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m0 + wm * TM * 32 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          float v[TN];
#pragma unroll
          for (int t = 0; t < TN; ++t) v[t] = acc[tm][t][r];
          epi_row<EPI, TN>(e, row < M ? row : 0, row < M, lr, args.N, v, mx0, mx1, mx2);
        }
    }
  } else {
    const bool fulln = (n0 + BN <= args.Npad);
    if (fulln) {
      row_epi_full<WM, WN, TM, TN, EPI>(args, acc, m0, n0, wm, wn, lr, lh, mx0, mx1);
    } else {
      // partial-width tile (odd layer widths): predicated path
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) {
        const int col = n0 + wn * TN * 32 + tn * 32 + lr;
        const bool real = col < args.N;
        const bool colv = col < args.Npad;
        const int colc = colv ? col : 0;
        float bv = 0.0f;
        if constexpr (EPI == (int)RowEpi::kTanh || EPI == (int)RowEpi::kRHidden || EPI == (int)RowEpi::kRelu ||
                      EPI == (int)RowEpi::kRZ)
          bv = e.bias[real ? col : 0];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = m0 + wm * TM * 32 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (row < M && colv) {
              float o0, o1 = 0.0f;
              epi_elem_v<EPI>(e, (size_t)row * e.ldo + colc, real, acc[tm][tn][r], real ? bv : 0.0f, o0, o1);
              epi_store<EPI>(e, (size_t)row * e.ldo + col, o0, o1);
              mx0 = fmaxf(mx0, fabsf(o0));
              mx1 = fmaxf(mx1, fabsf(o1));
            }
          }
      }
    }
  }
  amax_commit3<EXT_RED>(e.amax0, mx0, e.amax1, mx1, e.amax2, mx2, red);
}

}  // namespace
}  // namespace trpo
