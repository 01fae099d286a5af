// Host-side launch interface of the HIP kernels (gemm.hip, vec.hip, scan.hip).
//
// Everything here is stream-ordered and allocation-free, so a caller may capture
// it into a hipGraph.  Pointers are device pointers.  Row-major activation
// arrays have a leading dimension that is a multiple of 4 floats (16-B rows)
// and zero-filled padding columns.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace trpo {

// Kernel-variant switches.  Names, environment variables (TRPO_<NAME>) and defaults are the rows of
// options.cpp's table; runtime-settable through trpo_set_option for A/B and parity tests.
struct Options {
  int split_mfma;  // row GEMMs with N > 128 on the split MFMA: 0 off (f32 MFMA), 5 = 256 x 256 tile at
                   // BK 32 on f16 planes (default), 6 = 256 x 256 at BK 16, any other value = 128 x 256
  int split_wg;    // weight gradients with fan_out > 128 on the split MFMA: 0 off (f32 MFMA), 1 on
  int chain;       // FVP R-forward + R-backward as one fused kernel (chain.hip): 0 off, 1 auto, 2..4 variant
  int split_f16;   // split GEMMs on f16 MFMA: operands scaled by powers of two and split hi+lo (3 products)
  int split_min_k; // row GEMMs whose every segment has K < split_min_k stay on f32 MFMA (epilogue-bound)
  int graphs;      // engine: replay the update's sync-free prefix as a captured hipGraph
  int tail;        // engine: fused last-layer FVP tail (tail.hip) where eligible: 0 off, 1 on
  int fused;       // engine: whole small-width FVP in one launch (fused.hip): 0 off, 1 = 8 waves, 2 = 4 waves,
                   // 3 (default) = on the f16 split (fused16.hip) where it applies, else 2
  int low_seg;     // f16 split GEMMs: a segment whose product scale sits >= low_seg binades below the other
                   // segment's runs on one product (hi x hi) instead of three; 0 = off (gemm.hip)
  int planes;      // engine: row GEMMs whose operands have pre-split k-blocked f16 planes take the LDS-DMA
                   // plane kernel (plane.hip): 0 off, 1 on
  int rbwd0;       // engine: layer 1's R-backward (and the policy gradient's backward into layer 0) fused
                   // with layer 0's weight gradient where eligible (rbwd0.hip): 0 off, 1 on
  int hbwd2;       // engine: the prepare pass's and the policy gradient's backward through the head layer in one
                   // launch that reads H once (hbwd.hip), with D_1's hi plane under rbwd0: 0 off, 1 on VALU fmaf
                   // chains, 2 (default) on f32 MFMA
  int head_fwd;    // engine: softmax head forwards with one state per lane on f32 FMAs (hbwd.hip) instead of the
                   // f32 MFMA row GEMM with its 32-lane row epilogue: 0 off, 1 (default) prepare + line search,
                   // 2 line search, and the prepare head when the head has <= 8 actions
  int splits;      // engine: weight-gradient split-K slabs of the FVP launches (0 = auto: 512 at C4)
  int pg_splits;   // engine: the policy gradient's split-K slabs (0 = auto: 4 x splits, at most 2048)
  int ls_fused;    // engine: the policy forwards in one launch (fused16.hip fwd_loss16) where the FVP runs on
                   // fused16: 1 (default) the prepare pass's and the line search's, 2 the line search's only,
                   // 0 neither (per-layer row GEMMs + head_fwd)
  int cg_fuse_reduce;  // engine: single rank with the one-launch FVP: each CG iteration's slab reduction fused with
                       // its z = Hv + damping p (vec.hip reduce_slab_kernel<true>): 1 (default) on, 0 off; the p.z
                       // partials are grouped differently, so 1 and 0 are not bit-identical to each other; 2 the
                       // rest of the iteration and the next V image in the same launch, run by the workgroup that
                       // finishes last (cg_step_slabs_kernel, bit-identical to 1; measured slower: DESIGN.md §6)
  int cg_p_img;        // engine, fused16 path: each CG iteration's p update and the next FVP's V images in one launch
                       // (fused16.hip cg_p_img16_kernel, bit-identical): 1 (default) on, 0 off
  int rfwd01;          // engine: the FVP's R-forward through layers 0 and 1 in one launch (rfwd.hip) where eligible
  int fwd01;           // engine: the prepare / line-search forward through layers 0 and 1 in one launch (rfwd.hip)
                       // (two hidden layers of 256, obs <= 128, the fused tail, X planes): 1 (default) on, 0 off
  int rh1_planes;      // engine: under rfwd01 + rbwd0 on the f16 split, RH1 (per FVP, written by rfwd01) is kept as
                       // row-paired f16 hi / lo planes (PairPlane below); its readers, the layer-1 weight gradient
                       // and the fused R-backward's epilogue, fetch the hi plane alone where their low_seg test
                       // fires and both planes where it does not: 1 (default) on, 0 off
  int rbwd0_bdma;      // rbwd0.hip: the k-loop's weight planes reach LDS by LDS-DMA into a ring of three slots
                       // instead of through registers (bit-identical): 1 (default) on, 0 off
};

// A running-max slot is kAmaxSub counters, each on its own 128-B line: producers reduce within the
// workgroup and atomicMax into counter (block id mod kAmaxSub), so the device-scope atomics of a
// launch are few and spread; consumers take the max of the kAmaxSub counters (a few loads per lane).
constexpr int kAmaxSub = 256, kAmaxStride = 32, kAmaxSlot = kAmaxSub * kAmaxStride;   // in unsigned

// Power-of-two scale exponent for the f16 split: max|x| * 2^e lands in [2^11, 2^12).
__host__ __device__ inline int f16_scale_exp(float m) {
  if (!(m > 0.0f) || !(m < 3.0e38f)) return 0;
  int q = 0;
  (void)frexpf(m, &q);
  int e = 12 - q;
  return e < -100 ? -100 : (e > 100 ? 100 : e);
}
extern Options g_options;
int* option_slot(const char* name);   // the field of g_options called `name`; NULL: no such option

// ---------------------------------------------------------------------------
// Row GEMM:  C[M x N] = sum_seg A_seg[M x K_seg] * B_seg[K_seg x Npad]  -> epilogue
// ---------------------------------------------------------------------------
struct GemmSeg {
  const float* A;  // [M][lda]
  const float* B;  // [K][ldb]
  int lda, ldb, K; // K multiple of 4
  // split GEMM only: B as bf16 planes (hi, mid, lo) [3][Npad][ldk] or, with RowGemmArgs::f16,
  // scaled f16 planes (hi, lo) [2][Npad][ldk]; k contiguous, zero for k >= K (launch_split_b);
  // plane = elements per plane
  const uint16_t* B3 = nullptr;
  int ldk = 0, plane = 0;
  // f16 split only: running max |A| / max |B| (float bits, atomicMax'd by their producers) that
  // set the power-of-two operand scales; NULL means "bounded by 1"
  const unsigned* amaxA = nullptr;
  const unsigned* amaxB = nullptr;
  // f16 split, pre-split operands (plane.hip): A = (Ah + Al) * 2^-(*eAp), f16 planes written once by their
  // producer, k-blocked: element (r, k) at ((k / 32) * mpad + r) * 32 + k % 32, k padded to ldp (a multiple of
  // 64) and rows to mpad (a multiple of 256), zero-filled; Bb = B's split planes k-blocked the same way,
  // [2][ldk / 32][Npad][32] (plane = ldk * Npad elements).  Ah != NULL selects the planes path.
  const uint16_t* Ah = nullptr;
  const uint16_t* Al = nullptr;
  int ldp = 0, mpad = 0;
  const int* eAp = nullptr;
  const uint16_t* Bb = nullptr;
};

enum class RowEpi : int {
  kTanh = 0,      // out = tanh(acc + bias)                      (policy forward, hidden)
  kRHidden = 1,   // RH = (1-H^2)(acc + bias)                    (R-forward, hidden)
  kPrepBwd = 2,   // D = acc(1-H^2); E = -2 acc H                (KL_ff plain backward)
  kPgBwd = 3,     // DS = acc(1-H^2)                             (surr backward)
  kRBwd = 4,      // RD = acc(1-H^2) + E RH                      (R-backward)
  kPrepHead = 5,  // softmax head: P, D_L, DS_L, row loss terms  (prepare)
  kLossHead = 6,  // softmax head: row loss terms only           (line search)
  kRHead = 7,     // R-softmax head: RD_L                        (FVP)
  kRelu = 8,      // out = max(acc + bias, 0)                    (VF forward, utils.py:60-61)
  kReluBwd = 9,   // out = acc * (H > 0), H = the ReLU output    (VF backward)
  kPrepBwdE = 10, // E = -2 acc H only                           (KL_ff plain backward into the first
                  //                                              hidden layer: D_0 has no reader)
  kRZ = 11,       // RZ = acc + bias                             (R-forward pre-activation of the last
                  //                                              hidden layer: the fused tail applies
                  //                                              (1-H^2) as it loads H, so H is read once)
  // the diagonal-Gaussian heads (include/trpo_engine.h, TRPO_DIST_GAUSSIAN), in the softmax heads' lane layout
  kGaussPrepHead = 12,  // mean, DS_L, adv r (z^2 - 1) rows, row loss terms  (prepare)
  kGaussLossHead = 13,  // row loss terms only                               (line search)
  kGaussRHead = 14,     // RD_L = (acc + c) / (sigma^2 N)                    (FVP)
};
// the row-wise heads (one output row per 32-lane wave half, up to kMaxHeadTiles 32-column tiles)
constexpr int kMaxHeadTiles = 4;
constexpr bool epi_is_gauss(int e) { return e >= (int)RowEpi::kGaussPrepHead && e <= (int)RowEpi::kGaussRHead; }
constexpr bool epi_is_head(int e) {
  return (e >= (int)RowEpi::kPrepHead && e <= (int)RowEpi::kRHead) || epi_is_gauss(e);
}

struct RowEpiArgs {
  const float* bias;   // [N] (kTanh, kRHidden, heads)
  const float* H;      // [M][ldo] tanh activation at the output position
  const float* E;      // [M][ldo]
  const float* RH;     // [M][ldo]
  float* out0;         // tanh: H ; RHidden: RH ; PrepBwd: D ; PgBwd: DS ; RBwd: RD ; heads: P/RD_L
  float* out1;         // PrepBwd: E ; PrepHead: D_L
  float* out2;         // PrepHead: DS_L
  int ldo;             // leading dim of outputs/aux (multiple of 4)
  // heads
  const float* P;      // kRHead: cached softmax [M][ldo]
  const float* old;    // [M][ldo]
  const int* act;      // [M]
  const float* adv;    // [M]
  double* rowterms;    // [M][4] (surr*N, kl*N, ent*N, -)
  double invN;         // 1 / N_global
  // optional running max |out0| / |out1| / |out2| over the valid rows (float bits, atomicMax), the
  // operand scales of the f16 split GEMMs that consume these outputs
  unsigned* amax0 = nullptr;
  unsigned* amax1 = nullptr;
  unsigned* amax2 = nullptr;
  // Gaussian heads: `old` is the old mean, out0 the mean, out1 the rows adv r (z^2 - 1), out2 DS_L
  const float* actf = nullptr;     // [M][ldo] actions (kGaussPrepHead, kGaussLossHead)
  const float* logstd = nullptr;   // [N] log-std at the evaluated parameters
  const float* logstd0 = nullptr;  // [N] old log-std (kGaussPrepHead, kGaussLossHead)
};

struct RowGemmArgs {
  int M, N, Npad;      // rows; real output columns; padded output columns (<= ldb)
  int nseg;
  GemmSeg seg[2];
  const int* skip;     // optional device flag: launch is a no-op when *skip != 0
  RowEpi epi;
  RowEpiArgs ea;
  int f16 = 0;         // split path: 1 = two scaled f16 planes / 3 products, 0 = three bf16 planes / 6
  int low_seg = 0;     // f16: binade gap that puts the smaller segment on one product (0 = off; set at launch)
};

void launch_rowgemm(const RowGemmArgs& a, hipStream_t s);
// the pre-split-plane form (plane.hip); launch_rowgemm dispatches to it when seg[0].Ah is set
void launch_rowgemm_planes(const RowGemmArgs& a, hipStream_t s);
// f32 A [M][lda] -> scaled f16 planes hi/lo, k-blocked (GemmSeg::Ah; lo may be NULL: hi only); scale exponent
// f16_scale_exp(max |A|) from the running-max slot `amax` (NULL: |A| <= 1), written to *e_out
void launch_split_planes(const float* A, int M, int Mpad, int K, int lda, uint16_t* hi, uint16_t* lo, int ldp,
                         const unsigned* amax, int* e_out, hipStream_t s);
// k-block P planes [P][R][ld] (k contiguous) into [P][ld / 32][R][32] (GemmSeg::Bb)
void launch_block_planes(const uint16_t* src, int P, int R, int ld, uint16_t* dst, hipStream_t s);
// true when launch_rowgemm will take the split-bf16 path for this shape (the segments' B3 must be set)
bool rowgemm_uses_split(int Npad, RowEpi epi);

// Split fp32 matrices B [K][ldb] (columns [0, Npad)) into bf16 planes B3 [3][Npad][ldk]
// (hi = bf16(b), mid = bf16(b - hi), lo = bf16(b - hi - mid); k >= K zero-filled).
struct SplitJob {
  const float* B;
  uint16_t* B3;
  int K, Npad, ldb, ldk;
  const unsigned* amax = nullptr;   // f16: max |B| (float bits) that sets the plane scale
};
constexpr int kMaxSplitJobs = 16;
struct SplitArgs {
  int n;
  SplitJob job[kMaxSplitJobs];
  int f16 = 0;
};
void launch_split_b(const SplitArgs& a, const int* skip, hipStream_t s);

// ---------------------------------------------------------------------------
// Weight-gradient GEMM (split-K over rows):
//   slab[split][off_w + i*Nb + j] = sum_seg sum_rows A_seg[r][i] B_seg[r][j]
//   slab[split][off_b + j]        = sum_rows B_{colsum_seg}[r][j]
// ---------------------------------------------------------------------------
// Where a split-K launch puts one layer's block of a flat parameter-shaped gradient: split s covers rows
// [s * rows_per_split, (s + 1) * rows_per_split) and writes slab[s * slab_stride + ...] (the header above)
struct SlabDst {
  int splits = 0, rows_per_split = 0;
  float* slab = nullptr;
  int64_t slab_stride = 0;   // floats between consecutive splits
  int64_t off_w = 0, off_b = 0;
};

// Row-paired f16 planes of a [rows][256] operand (option rh1_planes): the dword at (row >> 1) * 256 + col holds
// rows 2p (low half) and 2p + 1 (high half) of one column, value * 2^(*e) rounded toward zero (hi) and the f16 of
// the exact remainder (lo).  A plane is pair_plane_dwords(rows) dwords; a row past the operand's last in the last
// pair holds zeros.  Readers take 4 B per lane, 32 consecutive columns in one 128-B run.
struct PairPlane {
  const unsigned* hi = nullptr;   // NULL: no planes (the f32 operand is read)
  const unsigned* lo = nullptr;
  const int* e = nullptr;
};
constexpr int kPairLd = 256;   // columns of a paired plane
constexpr int64_t pair_plane_dwords(int64_t rows) { return (rows + 1) / 2 * kPairLd; }

struct WSeg {
  const float* A;  // [rows][lda]
  const float* B;  // [rows][ldb]
  int lda, ldb;
  const unsigned* amaxA = nullptr;   // f16 split: max |A|, max |B| (float bits; NULL = bounded by 1)
  const unsigned* amaxB = nullptr;
  // f16 split: A as row-paired planes (lda = 256): staged straight into the LDS image, no f32 load and no split;
  // on the one-product path the lo plane is not read.  The segment's A scale is 2^(*Ap.e); the low_seg test keeps
  // reading amaxA.
  PairPlane Ap{};
};

struct WGradArgs {
  int rows;
  int Ma, Nb;          // real output dims (fan_in, fan_out)
  int Mpad, Npad;      // padded widths of A / B rows
  int nseg;
  WSeg seg[2];
  int colsum_seg;      // B of this segment is column-summed into the bias slot
  SlabDst dst;         // rows_per_split multiple of 16
  const int* skip;
  int f16 = 0;         // split path: scaled f16 (3 products) instead of bf16 (6 products)
  int low_seg = 0;     // f16: as RowGemmArgs::low_seg (set at launch)
};

void launch_wgrad(const WGradArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------
// vector / scalar kernels (vec.hip)
// ---------------------------------------------------------------------------
struct LayerPack {
  int64_t off_w;   // offset of W_l [a x b] in the flat vector
  int a, b, apad, bpad;
  float* WF;       // [2*apad][bpad]: rows [0,a) = W ; rows [apad, apad+a) = V
  float* WB;       // [2*bpad][apad]: rows [0,b) = W^T ; rows [bpad, bpad+b) = V^T
  unsigned* amax = nullptr;   // optional: atomicMax of max |W_l| (float bits)
};
constexpr int kMaxLayers = 8;
struct PackArgs {
  int nl;
  LayerPack L[kMaxLayers];
};
// which = 0: source is theta -> W halves ; which = 1: source is a tangent -> V halves
void launch_pack(const PackArgs& pa, const float* src, int which, const int* skip, hipStream_t s);

// out[p] = sum_{s<S} slab[s*stride + p]
void launch_reduce_slab(const float* slab, int S, int64_t stride, int64_t P, float* out,
                        const int* skip, hipStream_t s);

// Device scalar state of one update (CG, step scaling, line search).
struct UpdScalars {
  float rdotr[2];     // CG ping-pong (utils.py:189,198)
  float alpha, mu;
  int iters;          // CG iterations run
  int pad0;
  float tol;
  float damping;
  // step scaling (trpo_inksci.py:148-151)
  float sdotz;        // stepdir . fvp(stepdir)
  float gdots;        // g . stepdir
  double shs, lm, rate;
  // losses (f32 like session.run)
  float loss_before[3];
  float loss_trial[3];
  float loss_after[3];
  int accepted, k, reverted, pad1;
  double max_kl;
};
constexpr int kMaxCG = 64;
struct CGFlags {
  int done[kMaxCG + 2];  // done[i] is read by iteration i, written by iteration i-1
};

void launch_dot_partials(const float* a, const float* b, int64_t n, double* partials,
                         const int* skip, hipStream_t s);
// CG of utils.py:185-201.  init: x = 0, r = b, p = b, rdotr = f32(b.b), flags cleared.
// iter `it` (no-op once done[it] is set): z = hv + damping p ; alpha = rdotr/(p.z) ;
// x += alpha p ; r -= alpha z ; mu = (r.r)/rdotr ; p = r + mu p ; done[it+1] = r.r < tol.
void launch_cg_init(const float* b, float* x, float* r, float* p, int64_t n, double* partials,
                    UpdScalars* sc, CGFlags* fl, float tol, float damping, hipStream_t s);
void launch_cg_iter(const float* hv, float* x, float* r, float* p, float* z, int64_t n, UpdScalars* sc,
                    double* partials, double* partials2, CGFlags* fl, int it, hipStream_t s);
// single rank, the one-launch FVP: its slab reduction fused with the iteration's z = Hv + damping p and p.z
// (vec.hip), then the x / r and p updates; P up to kRedBlocks x 64 parameters
bool cg_fused_reduce_ok(int64_t P);
// (p_update = false: the caller runs the p update itself, e.g. launch_cg_p_img16)
void launch_cg_iter_slabs(const float* slab, int S, int64_t stride, float* hv, float* x, float* r, float* p, float* z,
                          int64_t n, UpdScalars* sc, double* partials, double* partials2, CGFlags* fl, int it,
                          hipStream_t s, bool p_update = true);
// cg_fuse_reduce = 2: the whole iteration in one launch (vec.hip cg_step_slabs_kernel): the slab reduction and
// z / p.z as above, then, in the workgroup that finishes last (an agent-scope ticket that it resets), the x / r and
// p updates of launch_cg_iter_slabs with bit-identical results, and, when `img` has jobs (the fused16 path), the next
// FVP's V images and exponents (launch_fused16_img(..., which = 1) of the new p)
struct CgStepArgs {
  const float* slab;
  int S, it;
  int64_t stride, P;
  float *hv, *x, *r, *p, *z;
  UpdScalars* sc;
  double* partials;
  CGFlags* fl;
  unsigned* ticket;   // zero between launches
};
struct ChainImgArgs;
void launch_cg_step_slabs(const CgStepArgs& a, const ChainImgArgs* img, int* img_e, hipStream_t s);
struct CGScalarsD {
  double rdotr[2];
  double alpha, mu;
  int iters, pad;
  double tol, damping;
};
void launch_cg_init_d(const double* b, double* x, double* r, double* p, int64_t n, double* partials,
                      CGScalarsD* sc, CGFlags* fl, double tol, hipStream_t s);
void launch_cg_iter_d(const double* hv, double* x, double* r, double* p, double* z, int64_t n,
                      CGScalarsD* sc, double* partials, double* partials2, CGFlags* fl, int it,
                      hipStream_t s);

// z = hv + damping*stepdir; partials = stepdir.z ; partials2 = g.stepdir
void launch_shs_partials(const float* hv, const float* stepdir, const float* g, int64_t n,
                         const UpdScalars* sc, double* partials, double* partials2, hipStream_t s);
// shs, lm, rate (single block)
void launch_shs_finish(const double* partials, const double* partials2, UpdScalars* sc, hipStream_t s);
// fullstep = stepdir / f32(lm)
void launch_fullstep(const float* stepdir, float* fullstep, int64_t n, const UpdScalars* sc, hipStream_t s);
// trial = prev + f32(0.5^k) * fullstep (no-op when accepted)
void launch_ls_trial(const float* prev, const float* fullstep, float* trial, int64_t n, int k,
                     const UpdScalars* sc, hipStream_t s);

// row loss terms -> kRedBlocks partial triples
void launch_rowterms_partials(const double* rowterms, int64_t n, double* partials3,
                              const int* skip, hipStream_t s);
// local[0..2] = ordered sum of the partial triples
void launch_rowterms_finish(const double* partials3, double* local3, const int* skip, hipStream_t s);
// which: 0 -> loss_before, 1 -> loss_trial ; out3 = f32(-sum_surr/N, sum_kl/N, sum_ent/N)
void launch_losses_store(const double* global3, double invN, UpdScalars* sc, int which,
                         const int* skip, hipStream_t s);
// line search decision for backtrack k (utils.py:176-181)
void launch_ls_decide(UpdScalars* sc, int k, hipStream_t s);
// theta = accepted ? prev + 0.5^k fullstep : prev ; revert if kl > 2 max_kl (trpo_inksci.py:153-158)
void launch_ls_finalize(const float* prev, const float* fullstep, float* theta, float* theta_ls,
                        int64_t n, UpdScalars* sc, hipStream_t s);

void launch_axpby(float* y, const float* x, float alpha, float beta, int64_t n, hipStream_t s);  // y = alpha*x + beta*y
void launch_scale_copy(const float* x, float* y, float alpha, int64_t n, hipStream_t s);          // y = alpha*x
void launch_i64_to_i32(const int64_t* src, int* dst, int64_t n, int* bad, int hi, hipStream_t s);
void launch_f64_to_f32(const double* src, float* dst, int64_t n, hipStream_t s);
// out = max(out, max |A[r][c]|) over r < n, c < w (float bits via atomicMax)
void launch_amax(const float* A, int64_t n, int w, int ld, unsigned* out, hipStream_t s);
void launch_copy_rows(const float* src, int64_t n, int w, int ld_src, float* dst, int ld_dst, hipStream_t s);

// ---------------------------------------------------------------------------
// the Fisher feed's gather (gather.hip): dst row i = src row i * stride, i < n_sub, for every array in one launch
// ---------------------------------------------------------------------------
struct GatherWide {
  const void* src;   // rows of q 16-byte units, 16-byte-aligned base
  void* dst;
  int q, pad;
};
struct GatherScalar {
  const void* src;   // one 4-byte element per row
  void* dst;
};
struct GatherArgs {
  GatherWide wide[3];
  GatherScalar scalar[2];
  int nwide, nscalar;
  int64_t n_sub, stride;
  int64_t first;            // the first source row (the global mode's phase; 0 in the local mode)
  const float* whole_src;   // copied whole (the old log-std vector), whole_n floats
  float* whole_dst;
  int64_t whole_n;
};
// grid sized from num_cus; the caller guarantees first + (n_sub - 1) * stride < the source's rows
void launch_gather_feed(const GatherArgs& a, int num_cus, hipStream_t s);

// ---------------------------------------------------------------------------
// discount scan + standardisation (scan.hip)
// ---------------------------------------------------------------------------
// out[t] = x[t] + gamma*out[t+1] within episodes (starts[t] = 1 begins an episode)
size_t discount_workspace_bytes(int64_t n);
void launch_discount(const double* x, const uint8_t* starts, int64_t n, double gamma, double* out,
                     void* workspace, hipStream_t s);
// adv = returns - baseline ; partials = sum adv
void launch_adv_center_partials(const double* returns, const double* baseline, double* adv,
                                int64_t n, double* partials, hipStream_t s);
void launch_sum_finish(const double* partials, double* out, hipStream_t s);  // out[0] = ordered sum
// partials = sum (adv - mean)^2 with mean = global_sum[0] * inv_n
void launch_adv_sq_partials(const double* adv, int64_t n, const double* global_sum, double inv_n,
                            double* partials, hipStream_t s);
// adv = (adv - mean)/(sqrt(sq*inv_n) + 1e-8) ; adv32 = f32(adv)
void launch_adv_normalize(double* adv, float* adv32, int64_t n, const double* global_sum,
                          const double* global_sq, double inv_n, hipStream_t s);

// ---------------------------------------------------------------------------
// GAE(lambda) two-channel scan (gae.hip)
// ---------------------------------------------------------------------------
// returns[t] = r[t] + gamma*returns[t+1], adv[t] = delta[t] + gamma*lambda*adv[t+1] within episodes, with
// delta[t] = (r[t] + gamma*v[t+1]) - v[t]; at a path's last row v[t+1] is tail_values[t] (0 when NULL) and
// both carries are cut.  values, starts (one path), tail_values and either output may be NULL.
size_t gae_workspace_bytes(int64_t n);
void launch_gae(const double* rewards, const double* values, const uint8_t* starts, const double* tail_values,
                int64_t n, double gamma, double lambda, double* adv, double* returns, void* workspace,
                hipStream_t s);

}  // namespace trpo

namespace trpo {
// ---------------------------------------------------------------------------
// Fused row-local FVP chain (chain.hip): R-forward through every layer, the
// R-softmax head and the R-backward down to layer 1 in one launch, 16 states
// per wave with activations carried in MFMA accumulator layout; writes RH_l and
// RD_l for the weight-gradient GEMMs.  Eligible when hidden widths <= 256 and
// n_actions <= 32.
// ---------------------------------------------------------------------------
struct ChainArgs {
  int n, L;                          // rows of this shard; layers
  int w[kMaxLayers + 1];             // widths [obs, hidden..., A]
  int ld[kMaxLayers + 1];            // row strides pad4(w)
  const float* X;
  const float* H[kMaxLayers];        // H[l], l = 1..L-1
  float* RH[kMaxLayers];             // RH[l], l = 1..L-1 (written)
  const float* P;                    // softmax at theta
  const float* D[kMaxLayers];        // D[l], l = 0..L-1 (width w[l+1])
  const float* E[kMaxLayers];        // E[l], l = 0..L-2 (width w[l+1])
  float* RD[kMaxLayers];             // RD[l], l = 0..L-1 (written)
  const float* v;                    // tangent (flat), for the tangent biases
  int64_t offb[kMaxLayers];          // bias offsets in the flat vector
  const void* img;                   // weight images (16-B units)
  const int* tab;                    // per chunk (offset, size) in 16-B units, consumption order
  int nchunks;
  double invN;                       // 1 / N_global
  const int* skip;
};

// One weight image segment: a K x O block of W_l (trans = 0: W(o,k) = W_l[k][o],
// forward) or W_l^T (trans = 1: W(o,k) = W_l[o][k], backward), split into bf16
// hi/mid/lo planes in 32-deep k-chunks, k permuted to the accumulator pairing,
// rows swizzled for conflict-free ds_read_b128.  which: 0 = from theta, 1 = tangent.
struct ChainImgJob {
  int64_t src_off, dst_off;          // flat-vector offset of W_l; u16 offset in the image
  int K, O, ldw, trans, kc, otp, which, pad;
};
constexpr int kMaxChainJobs = 4 * kMaxLayers;
struct ChainImgArgs {
  int n;
  ChainImgJob job[kMaxChainJobs];
  unsigned short* img;
};
int chain_max_tiles(int max_hidden);   // register tiles for a max hidden width (0: not eligible)
void launch_fvp_chain(const ChainArgs& a, int otm, hipStream_t s);
void launch_chain_img(const ChainImgArgs& a, const float* theta, const float* v, int which, const int* skip,
                      hipStream_t s);

// ---------------------------------------------------------------------------
// Fused small-width FVP (fused.hip): the chain above plus the weight R-gradients in one
// persistent launch, for one or two hidden layers of width <= 64, obs <= 128, <= 32 actions.
// Reads the chain's ChainArgs (the RH / RD pointers are not used) and writes one partial Hv per
// workgroup to slab[blockIdx.x] (all P entries); launch_reduce_slab over `grid` slabs finishes it.
// variant 1: 8 waves, 128 states per group (one workgroup per CU); 2: 4 waves, 64 states.
// ---------------------------------------------------------------------------
struct FusedArgs {
  ChainArgs c;
  float* slab;
  int64_t slab_stride;
  int64_t offW[kMaxLayers];
  int ngroups;                       // ceil(n / states per group)
};
bool fused_fvp_eligible(int L, const int* w);
int fused_fvp_states_per_group(int variant);
void launch_fvp_fused(const FusedArgs& a, int grid, int variant, hipStream_t s);

// The same one-launch FVP on the f16 split (fused16.hip) for one or two hidden layers of width <= 64, obs <= 128
// and <= 32 actions (C1, C2, C3; hidden dimensions padded to 64 in the images).  Weight images: the chain's job list (ChainImgJob; kc = fused16_obs_chunks(obs) for
// V_0) as 32-deep chunks of [2 f16 planes (hi, lo)][otp rows][32], each job scaled by a power of two whose
// exponent launch_fused16_img writes to img_e[job]; jobs in the order V_0 | W_1 V_1 | W_2 V_2 | W_2^T V_2^T |
// W_1^T V_1^T (one hidden layer: V_0 | W_1 V_1 | W_1^T V_1^T; hidden K padded to 2 chunks, hidden O to 64 rows).  X, D_1 and D_2 are scaled from the engine's running-max slots.
constexpr int kFused16Jobs = 9;
struct Fused16Args {
  FusedArgs f;                       // f.c.img / f.c.tab / f.c.nchunks: the f16 images and their chunk table
  const int* img_e;                  // [kFused16Jobs] scale exponents of the images
  const unsigned* am_x;              // running-max slots: X, D_1, D_2
  const unsigned* am_d1;
  const unsigned* am_d2;
  const float* DS;                   // policy gradient only: the head's surr logit delta DS_2 [n][ld 3] and its slot
  const unsigned* am_ds2;
  float* D1out;                      // with the prepare backward (launch_prep_pg_fused16): D_1, E_1 [n][ld 2], E_0
  float* E1out;                      // [n][ld 1] and D_1's running-max slot
  float* E0out;
  unsigned* am_d1_out;
};
bool fused16_eligible(int L, const int* w);
int fused16_obs_chunks(int obs);     // 32-deep k-chunks of V_0's image (obs rounded to 32, 64 or 128)
int fused16_states_per_group();
int fused16_groups_per_cu();
// the CG's p update (cg_p_kernel, bit-identical) into p_new with the V images of p_new (fused16_img_kernel, which = 1)
void launch_cg_p_img16(const ChainImgArgs& a, const float* r, const float* p_old, float* p_new, int64_t n,
                       UpdScalars* sc, const double* partials2, CGFlags* fl, int it, int* img_e, hipStream_t s);
void launch_fused16_img(const ChainImgArgs& a, const float* theta, const float* v, int which, const int* skip,
                        int* img_e, hipStream_t s);
void launch_fvp_fused16(const Fused16Args& a, int grid, hipStream_t s);
// The policy gradient of the same shapes in one launch (fused16.hip, PG form): DS_1, DS_0 by the backward chain
// over W_2^T / W_1^T's image chunks and g's blocks H_l^T DS_l + colsum DS_l into the slabs, as the FVP's.
void launch_pg_fused16(const Fused16Args& a, int grid, hipStream_t s);
// ... and with it, on the same weight chunks, the prepare pass's backward below the head: D_1, E_1, E_0 and D_1's
// running max (engine.cpp prepare())
void launch_prep_pg_fused16(const Fused16Args& a, int grid, hipStream_t s);
// Line-search loss forward for the same shapes (fused16.hip fwd_loss16_kernel): the row terms of
// trpo_inksci.py:46-53 at a trial theta, from that theta's W_0 | W_1 | W_2 images (ChainImgJob, which = 0, the
// order here; img_e per job) resident in LDS, one wave per 16 states, no barrier in the loop.
struct FwdLoss16Args {
  int64_t n;
  int L = 3;                         // layers (2: one hidden layer, w = [obs, h1, A])
  int w[4], ld[4];                   // widths [obs, h1, h2, A]; row strides
  const float* X;
  const float* theta;                // the trial vector (biases)
  int64_t offb[3];
  const void* img;                   // W_0 | W_1 | W_2 images (16-B units)
  const int* tab;                    // per chunk (offset, size) in 16-B units
  int nchunks;
  const int* img_e;                  // [3]
  const unsigned* am_x;
  const float* old;                  // [n][ld[3]]
  const int* act;
  const float* adv;
  double* rowterms;                  // [n][4]
  const int* skip;
  // the prepare pass (H1 != NULL): H_1, H_2 [n][ld[1|2]], P / D_2 / DS_2 [n][ld[3]] and the maxima of D_2, DS_2
  float* H1 = nullptr;
  float* H2 = nullptr;
  float* P = nullptr;
  float* D = nullptr;
  float* DS = nullptr;
  unsigned* am_d = nullptr;
  unsigned* am_ds = nullptr;
  double invN = 0.0;
};
void launch_fwd_loss16(const FwdLoss16Args& a, int num_cus, hipStream_t s);
}  // namespace trpo

namespace trpo {
// ---------------------------------------------------------------------------
// Fused last-layer FVP tail (tail.hip), for the f16-split engine when the last hidden width is
// in (128, 256] (a multiple of 32) and n_actions <= 32.  Per 32-row tile of a split-K slab:
//   RZ = RH W + H V + c ; RD_L = R-softmax-reverse(RZ)             (head R-forward, kRHead)
//   RD_out = (RD_L W^T + D_L V^T)(1-H^2) - 2 (D_L W^T) H RH        (R-backward, E recomputed)
//   slab  += RH^T D_L + H^T RD_L ; bias += colsum RD_L              (weight R-gradient)
// reading RH and H once.  All products on the scaled f16 hi+lo split.
// ---------------------------------------------------------------------------
constexpr int kTailK = 256;   // max hidden width of the tail (head planes are [2][2][32][kTailK])
struct TailArgs {
  int rows, a, b, apad, bpad;
  const float* RH;            // [rows][apad]  R{h} of the last hidden layer, or with rz its pre-activation RZ
  const float* H;             // [rows][apad]  its tanh activations
  int rz = 0;                 // 1: RH holds RZ (kRZ); R{h} = (1-H^2) RZ is formed on load (same f32 ops as kRHidden)
  const float* P;             // [rows][bpad]  softmax at theta
  const float* DL;            // [rows][bpad]  KL_ff plain logit delta D_{L-1}
  const float* c;             // [b]           tangent bias of the last layer
  const uint16_t* WV16;       // head planes [mat W,V][plane hi,lo][32 j][kTailK k] (launch_tail_pack)
  const uint16_t* WT16;       // R-backward planes of W^T: [plane][apad n][32 k], plane stride bplane
  const uint16_t* VT16;       // ... of V^T
  int64_t bplane;
  const unsigned *am_rh, *am_d, *am_w, *am_v;   // running-max slots of RH, D_L, W, V
  unsigned* am_out;           // running max |RD_out|
  float* RDout;               // [rows][apad]  R-delta into the last hidden layer (RD_{L-2})
  double invN;
  SlabDst dst;                // rows_per_split % 32 == 0
  const int* skip;
};
struct TailPackArgs {
  const float* theta;
  const float* v;
  int64_t off_w;              // flat offset of W_{L-1} [a][b]
  int a, b;
  const unsigned *am_w, *am_v;
  uint16_t* out;              // [2][2][32][kTailK]
};
bool tail_eligible(int apad, int bpad);   // (128, kTailK] multiple of 32; bpad in (16, 32]

// ---------------------------------------------------------------------------
// R-backward into the first hidden layer fused with layer 0's weight R-gradient (rbwd0.hip).
// Per 128-row tile of a split-K slab (trpo_inksci.py:56-70):
//   RD_0  = ([RD_1 | D_1] [W_1^T ; V_1^T]) (1 - H_1^2) + E_0 RH_1      (kept in registers, never stored)
//   slab += X^T RD_0 ;  bias += colsum RD_0                            (Hv's W_0 / b_0 blocks)
// With nseg = 1, no E and no RH it is the policy gradient's DS_0 = (DS_1 W_1^T)(1 - H_1^2) and X^T DS_0
// (trpo_inksci.py:54).  Hidden width <= 256 (wave w owns output columns [32w, 32w + 32)), obs <= 128 on
// X's pre-split k-blocked f16 planes; products on the scaled f16 hi+lo split.
// ---------------------------------------------------------------------------
struct RBwd0Args {
  int rows;                 // rows of this rank's shard
  int K, lda;               // per-segment K (the layer-1 output width) and A's leading dimension
  int N, Npad;              // layer-1 input width (RD_0's columns), padded (<= 256, multiple of 32)
  int obs;                  // X's real columns (<= 128)
  int nseg;                 // 2: [RD_1 | D_1] ; 1: DS_1 alone
  const float* A0;          // [rows][lda] RD_1 (or DS_1)
  const float* A1;          // [rows][lda] D_1
  const uint16_t* A1h;      // D_1's k-blocked f16 hi plane (GemmSeg::Ah layout, scale 2^(*eA1p)); NULL: none
  const int* eA1t = nullptr;   // ... or, when set, one scale 2^eA1t[r / 32] per 32-row tile (hbwd.hip)
  int a1_mpad;
  const int* eA1p;
  const uint16_t* B0;       // f16 hi/lo planes of W_1^T: [2][Npad][ldk] (plane stride `plane`)
  const uint16_t* B1;       // ... of V_1^T
  int ldk;
  int64_t plane;
  const unsigned *am_a0, *am_b0, *am_a1, *am_b1;   // running-max slots of the segment operands
  const float* H;           // [rows][Npad] H_1
  const float* E;           // [rows][Npad] E_0 (NULL: no E RH term)
  const float* RH;          // [rows][Npad] RH_1
  // RH_1 as row-paired planes (Npad = 256): the epilogue reads the hi plane when the launch's low_seg test fires
  // (whether or not A1h is attached), hi + lo otherwise; RH is then not read
  PairPlane RHp{};
  const uint16_t* Xh;       // X's k-blocked f16 planes (GemmSeg::Ah layout), scale 2^(*eX)
  const uint16_t* Xl;
  int x_mpad, x_ldp;
  const int* eX;
  SlabDst dst;
  const int* skip;
  int low_seg = 0;          // f16: segment 1 on one product when it sits >= low_seg binades under (set at launch)
};
// The prepare pass's and the policy gradient's backward through the head layer in one read of H (hbwd.hip):
//   D1 = (D2 W^T)(1 - H^2), DS1 = (DS2 W^T)(1 - H^2)  (K = n_actions <= 32), the policy gradient's head-layer
// weight gradient H^T DS2 (+ bias colsum) into the slabs, optionally D1's f16 hi plane
// (GemmSeg::Ah layout, row stride d1_mpad, scale 2^eD1t[r / 32] per 32-row tile)
struct HeadBwd2Args {
  int rows;
  int A, Apad;              // actions; leading dimension of D2 / DS2
  int N, Npad;              // last hidden width; leading dimension of H / D1 / DS1
  const float* WB;          // W^T rows [0, A) of the packed backward operand, [.][Npad]
  const float* D2;
  const float* DS2;
  const float* H;
  float* D1;
  float* DS1;
  unsigned* am_d1;
  unsigned* am_ds1;
  uint16_t* D1h = nullptr;
  int d1_mpad = 0;
  int* eD1t = nullptr;
  float* E1 = nullptr;       // E_{L-2} = -2 (D_{L-1} W^T) H (the kPrepBwd epilogue's second output), when read
  // workgroup s takes the rows of split s (the weight-gradient slab partition); dst.slab != NULL: it also writes
  // the policy gradient's last-layer weight gradient (H^T DS2, W block [N][A] at off_w, bias colsum DS2 at off_b)
  // of its rows into slab s
  SlabDst dst;
};
bool head_bwd2_eligible(int A, int Npad);
// The softmax head forward with one state per lane (hbwd.hip): z = H W + b (K = last hidden width, A <= 32 actions),
// p = softmax(z), the surr / kl / ent row terms, and with prep also P, D_L, DS_L (gemm.hip kPrepHead semantics)
struct HeadFwdArgs {
  int64_t rows;
  int A, Apad;              // actions; leading dimension of old / P / D / DS and of W's rows
  int K, Kpad;              // last hidden width; leading dimension of H
  const float* H;
  const float* W;           // [K][Apad] (the packed forward operand's W half)
  const float* bias;        // [A]
  const float* old;
  const int* act;
  const float* adv;
  double* rowterms;         // [rows][4]
  double invN;
  int prep = 0;
  float* P = nullptr;
  float* D = nullptr;
  float* DS = nullptr;
  unsigned* am_d = nullptr;
  unsigned* am_ds = nullptr;
};
bool head_fwd_eligible(int A, int K);
void launch_head_fwd(const HeadFwdArgs& a, int num_cus, hipStream_t s);
void launch_head_bwd2(const HeadBwd2Args& a, int num_cus, hipStream_t s);
// The R-forward through layers 0 and 1 in one launch (rfwd.hip, option rfwd01): RH1 = (1 - H1^2)(X V0 + c0)
// (stored) and RZ2 = RH1 W1 + H1 V1 + c1 (stored, the fused tail's pre-activation) for two hidden layers of 256
// and obs <= 128, X from its pre-split planes, V0 / W1 / V1 from a per-FVP chunk image (launch_rfwd01_img).
struct Rfwd01Args {
  int64_t n;
  int obs, ldh, ldz;                 // obs; row strides of H1 / RH1 and of RZ2 (floats)
  const uint16_t *Xh, *Xl;           // X's k-blocked f16 planes (GemmSeg::Ah), x_mpad rows per 32-k block
                                     // (all four blocks are loaded whatever obs is: 128 x_mpad values per plane)
  int x_mpad;
  const int* eX;                     // their scale exponent
  const float *H1, *c0, *c1;         // H1; the tangent biases of layers 0 and 1 (v + offb[l])
  const float* V0;                   // the direction's layer-0 block, [obs][256] (v + offW[0])
  float *RH1, *RZ2;
  // set: RH1 is written as row-paired f16 planes into RH1's bytes (hi plane, then lo plane at
  // pair_plane_dwords(n) dwords) at one launch-wide exponent from the bound |RH1| <= max_s |X_s|_2 max_j |V0_j|_2
  // 1.01 + max |c0|, with max_s |X_s|_2 <= sqrt(obs) max |X| and max |X| < 2^(12 - *eX); workgroup 0 writes the
  // exponent to *e_rh1
  int* e_rh1 = nullptr;
  const uint16_t* img;               // rfwd01_img_bytes()
  const unsigned *am_v0, *am_w1, *am_v1;   // the images' running-max slots
  unsigned *am_rh1, *am_rz2;         // running max |RH1|, |RZ2| (atomicMax'd)
  const int* skip;
};
// The policy forward through layers 0 and 1 in one launch (rfwd.hip, option fwd01): H1 = tanh(X W0 + b0) (stored
// when H1 is set: the prepare pass) and H2 = tanh(H1 W1 + b1), same shapes as rfwd01, W0 / W1 from a per-forward
// chunk image (launch_fwd01_img).
struct Fwd01Args {
  int64_t n;
  int obs;
  const uint16_t *Xh, *Xl;           // X's k-blocked f16 planes, x_mpad rows per 32-k block
                                     // (four blocks, as Rfwd01Args)
  int x_mpad;
  const int* eX;
  const float *b0, *b1;              // th + offb[0], th + offb[1]
  float *H1, *H2;                    // H1: NULL = not stored (the line search)
  const uint16_t* img;               // fwd01_img_bytes()
  const unsigned *am_w0, *am_w1;     // the weights' running-max slots (the image's scales)
};
// both kernels address an X plane with signed 32-bit byte offsets: up to 4 k-blocks (obs <= 128) of x_mpad rows
// of 64 bytes must stay under 2^31 (the engine takes the per-layer plane path beyond)
constexpr bool rfwd01_rows_ok(int64_t x_mpad) { return 4 * x_mpad * 64 < (int64_t(1) << 31); }
static_assert(rfwd01_rows_ok((1 << 23) - 256) && !rfwd01_rows_ok(1 << 23), "rfwd01 / fwd01 row limit");
// the row-paired planes (option rh1_planes) are addressed per tile / per split from 64-bit bases, so they take
// every row count the producer does: one limit, shared by the engine's gate and the launchers
constexpr bool pair_planes_rows_ok(int64_t x_mpad) { return rfwd01_rows_ok(x_mpad); }
bool fwd01_eligible(int L, const int* w, const int* wp);
size_t fwd01_img_bytes();
void launch_fwd01_img(const float* th, int64_t offW0, int64_t offW1, int obs, const unsigned* am_w0,
                      const unsigned* am_w1, uint16_t* img, hipStream_t s);
void launch_fwd01(const Fwd01Args& a, int num_cus, hipStream_t s);
bool rfwd01_eligible(int L, const int* w, const int* wp);
size_t rfwd01_img_bytes();
void launch_rfwd01_img(const float* theta, const float* v, int64_t offV0, int64_t offW1, int obs,
                       const unsigned* am_v0, const unsigned* am_w1, const unsigned* am_v1, uint16_t* img,
                       const int* skip, hipStream_t s);
void launch_rfwd01(const Rfwd01Args& a, int num_cus, hipStream_t s);
bool rbwd0_eligible(int obs_pad, int x_ldp, int hid_pad, int K);
void launch_rbwd0(const RBwd0Args& a, hipStream_t s);
void launch_tail_pack(const TailPackArgs& p, hipStream_t s);
void launch_fvp_tail(const TailArgs& a, hipStream_t s);
}  // namespace trpo

namespace trpo {
// ---------------------------------------------------------------------------
// Value-function baseline (vf.hip), utils.py:48-92
// ---------------------------------------------------------------------------
size_t vf_pos_workspace_bytes(int64_t n);
// feat [n][Fp] = [obs | dist | f32(t/10)] with t the step index within each path
// (starts[r] = 1 opens a path; starts may be NULL: one path); lastpos [n] scratch.  step_index [n], when given, is t
// itself (a segment rollout's feed, whose first path may continue an episode) and starts is not read.
void launch_vf_features(const float* obs, int obs_dim, int ld_obs, const float* dist, int A, int ld_dist,
                        const uint8_t* starts, int64_t n, int64_t* lastpos, void* ws, float* feat, int Fp,
                        hipStream_t s, const int64_t* step_index = nullptr);
// feat [n_paths][Fp] = [final_obs | final_dist | f32(T/10)]: the features of s_T, the state after a path's
// T steps (row t = T of launch_vf_features)
void launch_vf_tail_features(const float* obs, int obs_dim, const float* dist, int A, const int64_t* lengths,
                             int64_t n_paths, float* feat, int Fp, hipStream_t s);
// tail[end_rows[p]] = truncated[p] ? (double)pred[p] : 0.0; rows outside [0, n) are skipped
void launch_vf_tail_scatter(const float* pred, const uint8_t* truncated, const int64_t* end_rows, int64_t n_paths,
                            int64_t n, double* tail, hipStream_t s);
struct VFPackArgs {
  int F, H1, H2, H1p, H2p;
  int64_t offW1, offW2;   // flat offsets of W1 [F][H1], W2 [H1][H2]
  float* W1p;             // [Fp][H1p]
  float* W2p;             // [H1p][H2p]
  float* W2T;             // [H2p][H1p]
};
void launch_vf_pack(const VFPackArgs& a, const float* theta, hipStream_t s);
struct VFHeadArgs {
  int64_t n;
  int H2, H2p;
  const float* Z2;        // [n][H2p]
  const float* w3;        // [H2]
  const float* b3;        // [1]
  int train;
  const float* y;         // [n]            train
  float* dout;            // [n][4]         train: col 0 = d(loss)/d(net)
  float* dZ2;             // [n][H2p]       train
  double* loss_rows;      // [n]            train: (net - y)^2
  float* out32;           // [n]            predict (if out64 == NULL)
  double* out64;          // [n]            predict
};
void launch_vf_head(const VFHeadArgs& a, hipStream_t s);
void launch_adam(float* var, const float* g, float* m, float* v, int64_t n, float alpha, float b1, float b2, float eps,
                 hipStream_t s);
}  // namespace trpo

namespace trpo {
// ---------------------------------------------------------------------------
// Batched sampling and rollouts of the built-in environments (rollout.hip): agent.act
// (trpo_inksci.py:76-87), cat_sample (utils.py:95-105), rollout (utils.py:18-45)
// ---------------------------------------------------------------------------
struct PolicyShape {
  int L;
  int w[kMaxLayers + 1];
  int64_t offW[kMaxLayers], offb[kMaxLayers];
};
// One built-in environment, from its trait in rollout.hip.  Two id tables: TRPO_ENV_* (discrete actions, rolled out
// under the categorical head) and, with `continuous`, TRPO_CENV_* (float32 actions, under the diagonal-Gaussian head).
struct EnvDims {
  int obs_dim, state_dim;
  int head_dim;             // A, the policy's output width: the number of actions, or (continuous) act_dim
  int reset_draws, time_limit;
  const char* name;
};
bool env_dims(bool continuous, int env, EnvDims* out);   // host-only; false for an unknown id
// One rollout kernel serves both heads.  The head row is the action distribution, or (continuous) the mean; the draw
// of a step is cat_sample's uniform, or (continuous) one standard normal per action component.
struct RolloutArgs {
  bool continuous;          // which id table `env` is of, and with it the policy head
  int env;                  // ps must have the environment's obs_dim and head_dim
  int state_dim;            // the environment's
  PolicyShape ps;
  const float* theta;
  const float* logstd;      // continuous: [A] the log-stds the rollout samples with (the engine's snapshot)
  int maxw;                 // max layer width (LDS slice per wave: 2 * maxw floats)
  int n_envs, max_pathlength, time_limit, train;
  int64_t budget;           // steps per environment: ceil(n_timesteps / n_envs)
  int64_t env_cap;          // rows per environment region: budget + max episode length - 1
  int max_episodes;         // second dim of reset_u
  uint64_t seed;
  const double* reset_u;    // optional [n_envs][max_episodes][reset_draws] uniforms for env.reset
  const double* draws;      // optional [n_envs][env_cap][noise_dim] draws for the act, in place of Philox's
  // per-environment regions (row = env * env_cap + i)
  double* obs;              // [.][obs_dim]
  double* env_state;        // [.][state_dim] the state obs was made from; NULL where the observation is the state
  float* head;              // [.][A]
  int64_t* acti;            // the action; NULL when continuous
  float* actf;              // continuous: [.][A] the action
  double* noise;            // [.][noise_dim] the draw of every step (continuous and train = 0: zeros)
  int noise_dim;            // 1, or (continuous) A
  double* rewards;
  uint8_t* starts;
  int64_t* counts;          // [n_envs] steps collected
  int64_t* episodes;        // [n_envs] episodes collected
  // per-environment path regions (path = env * budget + episode; an environment starts at most budget episodes)
  uint8_t* end_truncated;   // 1: the path was cut off (time limit / max_pathlength), 0: the environment terminated
  double* end_obs;          // [.][obs_dim] the observation of s_T, the state after the path's last step
  float* end_head;          // [.][A] the policy's head row at s_T of a cut-off path, zeros otherwise
  int64_t* end_len;         // T, the path's step count
  int64_t* end_row;         // the path's last row within its environment's step region
};
struct RolloutOut {         // concatenated outputs; any pointer may be NULL
  double* obs64;            // [N][obs_dim]
  double* env_state;        // [N][state_dim]
  float* X;                 // [N][ldx]   (engine batch: f32 states)
  int ldx;
  float* head;              // [N][ld_head] (engine batch: oldaction_dist, or the old mean)
  int ld_head;
  int64_t* actions64;
  int* act32;
  float* actf;              // [N][ld_actf]
  int ld_actf;
  double* noise;            // [N][noise_dim]
  double* rewards;
  uint8_t* starts;
  // the per-path end records [n_paths], in the order of the concatenated rollout; written when path_offsets
  // ([n_envs] exclusive sums of the episode counts) is given
  const int64_t* path_offsets;
  int ends_only;            // 1: skip the per-step pass
  uint8_t* end_truncated;
  double* end_obs64;        // [n_paths][obs_dim]
  float* end_obs32;
  float* end_head;          // [n_paths][A]
  int64_t* end_len;
  int64_t* end_rows;        // index of the path's last step in the concatenated rollout
};
// The fixed-horizon segment rollout (rollout_segment_kernel; include/trpo_engine.h has its definition): every
// environment takes exactly r.budget steps (r.env_cap == r.budget, so row = env * budget + k and the regions are
// already concatenated) and continues from the carry.  It has arguments of its own, so that RolloutArgs and with it
// the whole-episode kernels stay what they are.
struct SegmentArgs {
  RolloutArgs r;            // r.end_len holds a fragment's row count, r.max_episodes >= budget + (resume ? 0 : 1)
  int resume;               // 1: start from the carry; 0: reset every environment first (reset index 0)
  // the carry, per environment; read when resume, always written
  double* carry_s;          // [n_envs][state_dim]
  int64_t* carry_t;         // steps taken in the current episode
  double* carry_ret;        // the current episode's rewards so far, summed in step order
  int64_t* step_index;      // [n_envs * budget] the step's index in its episode
  // per-environment path regions, beside r.end_*
  uint8_t* end_kind;        // 0 terminated, 1 cut by time_limit / max_pathlength, 2 cut by the segment
  int64_t* end_t0;          // the episode step index of the fragment's first row
  double* end_ret;          // the episode's return at the path's end, earlier segments included
};
struct SegmentOut {         // concatenated; any pointer may be NULL
  uint8_t* end_kind;        // [n_paths]
  int64_t* end_t0;
  double* end_ret;
  int64_t* end_steps;       // end_t0 + the fragment's rows: the episode's step count at s_T
  int64_t* step_index;      // [n_envs * budget]
};
size_t rollout_lds_bytes(int maxw);
void launch_rollout(const RolloutArgs& a, hipStream_t s);
void launch_rollout_segment(const SegmentArgs& g, hipStream_t s);
// path_offsets as RolloutOut's; max_paths = the largest episode count of one environment
void launch_rollout_segment_compact(const SegmentArgs& g, const int64_t* path_offsets, const SegmentOut& o,
                                    int64_t max_paths, hipStream_t s);
void launch_rollout_compact(const RolloutArgs& a, const int64_t* offsets, const RolloutOut& o, int64_t max_count,
                            hipStream_t s);
void launch_act(const PolicyShape& ps, const float* theta, int maxw, const float* states, int64_t n, const double* r,
                int train, int64_t* actions, float* dists, hipStream_t s);
// The Gaussian policy's act on n states (one wave per state, act_dim <= 64): mean = the same wave forward without
// the softmax, actions = float32(mean + exp(logstd) * normals) in float64 (train) or the mean; `normals` [n][A] f64
// may be NULL when train = 0, either output may be NULL
void launch_act_gaussian(const PolicyShape& ps, const float* theta, const float* logstd, int maxw, const float* states,
                         int64_t n, const double* normals, int train, float* actions, float* means, hipStream_t s);
void launch_cat_sample(const float* prob, int64_t n, int k, const double* r, int64_t* out, hipStream_t s);
// state [n][state_dim], action [n] i64 or (continuous) [n][head_dim] f32 -> state_out, obs_out [n][obs_dim], reward,
// done (termination); outputs may be NULL
void launch_env_step(bool continuous, int env, const double* state, const void* action, int64_t n, double* state_out,
                     double* obs_out, double* reward, uint8_t* done, hipStream_t s);
}  // namespace trpo

namespace trpo {
// ---------------------------------------------------------------------------
// The log-std blocks of a Gaussian engine's P-long vectors (gauss.hip).  The per-layer launches write the
// network blocks into the slabs; these write the last A entries of the reduced vector, this rank's partial,
// before the all-reduce.  Fixed-order f64 sums, no float atomics, no host synchronisation.
// ---------------------------------------------------------------------------
constexpr int kGaussColBlocks = 256;   // partial rows of the column reduction (fixed: the sum order depends on n only)
// part[b][c] = sum over block b's rows of src[r][c], c < A <= 128; part holds kGaussColBlocks x 128 doubles.
// Returns the blocks used (<= kGaussColBlocks), a function of n alone.
int launch_gauss_colsum_partials(const float* src, int64_t n, int A, int ld, double* part, hipStream_t s);
// out_tail[c] = f32(scale * sum_b part[b][c]), b < blocks in order
void launch_gauss_colsum_finish(const double* part, int blocks, int A, double scale, float* out_tail, const int* skip,
                                hipStream_t s);
// out_tail[c] = f32(scale * v_tail[c])   (Hv's log-std block: scale = 2 n / N)
void launch_gauss_scale_tail(const float* v_tail, int A, double scale, float* out_tail, const int* skip,
                             hipStream_t s);
}  // namespace trpo
