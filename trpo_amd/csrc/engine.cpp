// Runtime of the TRPO update engine behind the C-ABI of include/trpo_engine.h.
//
// One engine = one GPU = one shard of the state batch.  It owns every device
// buffer of the update (HBM layout in DESIGN.md), one HIP stream, and an
// optional RCCL communicator.  The reference's session.run calls
// (trpo_inksci.py:126,129,146,156) become kernel sequences on that stream:
//
//   prepare()      policy forward at theta + the KL_ff plain backward; caches
//                  H_l, P, D_l, E_l (fixed while theta is fixed, i.e. over the
//                  whole CG solve — the reference recomputes them per call)
//   policy_grad()  surr backward + weight-gradient GEMMs (flatgrad, :54)
//   fvp()          R-forward + R-backward + weight gradients (:56-70)
//   cg()           utils.py:185-201 with scalars on device and an early-exit flag
//   update()       trpo_inksci.py:144-158
#include "../../include/trpo_engine.h"
#include "abi_util.h"
#include "common.h"
#include "kernels.h"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

using namespace trpo;

using namespace trpo_abi;

struct trpo_engine {
  int device = 0;
  int num_cus = 256;               // compute units of `device` (hipDeviceAttributeMultiprocessorCount)
  hipStream_t stream = nullptr;
  // policy shape
  int dist = TRPO_DIST_CATEGORICAL;   // the policy's distribution family, fixed at creation
  bool gauss() const { return dist == TRPO_DIST_GAUSSIAN; }
  static const char* dist_name(int d) { return d == TRPO_DIST_GAUSSIAN ? "gaussian" : "categorical"; }
  // a call that exists for one family only: a state error that names this engine's, before anything is launched
  void require_dist(int want, const char* call) const {
    if (dist != want)
      throw std::runtime_error(std::string(call) + " needs a " + dist_name(want) + " engine; this engine's distribution is " +
                               dist_name(dist));
  }
  int L = 0;                       // layers
  std::vector<int> w, wp;          // widths [obs, hidden..., A] and padded
  int64_t P = 0;                   // parameters: the layers' and, on a Gaussian engine, the A log-stds after them
  const float* logstd_of(const float* th) const { return th + (P - w[L]); }
  std::vector<int64_t> offW, offb;
  int64_t cap = 0, n = 0, n_global = 0;
  // Fisher subsampling (trpo_set_fvp_subsample): with a stride k > 1 the engine has a child engine, `fisher`, of
  // ceil(cap / k) rows that holds rows 0, k, 2k, ... of the feed and serves every Fisher-vector product (fvp(), cg());
  // k = 1: no child, nothing below runs.  The child (owner != NULL) borrows its owner's stream, so its launches fall
  // into the owner's captured update graph, and the owner's theta and CG scalar block (sc, fl), so the update's
  // statistics and step scaling read the CG's results where they always did; it owns every buffer with rows in it,
  // its weight images, its CG vectors and the scalar block of its own prepare pass's losses (loss_sc).
  // The global mode (trpo_set_fvp_subsample_global) takes the stride over global row indices: the feed's first row
  // has global index feed_row0, the Fisher rows are the local rows i with (feed_row0 + i) % k == 0, the first of them
  // is fisher_phase(), and the child's n_global is ceil(n_global / k), which every rank knows without a collective.
  // The child then also borrows its owner's transport (transport()): communicator, host callback and slots.
  int64_t fvp_stride = 1;
  bool fvp_global = false;
  int64_t row0_next = 0;   // trpo_set_row_offset: the global index of the next feeds' first row
  int64_t feed_row0 = 0;   // ... and of the current feed's (recorded in every mode, read in the global one only)
  trpo_engine* fisher = nullptr;
  trpo_engine* owner = nullptr;
  std::string tag_prefix;   // of the child's profile tags ("sub."), in its owner's table
  // multi-GPU
  ncclComm_t comm = nullptr;
  int rank = 0, world = 1;
  trpo_allreduce_cb host_ar = nullptr;   // test transport (trpo_comm_set_host_allreduce)
  void* host_ar_ctx = nullptr;
  std::vector<uint8_t> host_ar_buf;

  // ---- device buffers ----
  std::vector<void*> allocs;
  float *theta = nullptr, *theta_prev = nullptr, *theta_trial = nullptr, *theta_ls = nullptr;
  float *g = nullptr, *bneg = nullptr, *x = nullptr, *r = nullptr, *p = nullptr, *z = nullptr;
  float* p2 = nullptr;   // the CG's second direction buffer (p ping-pongs when the p update writes a new buffer)
  float *hv = nullptr, *stepdir = nullptr, *fullstep = nullptr, *vin = nullptr, *vout = nullptr;
  std::vector<float*> WF, WB, WFt;   // packed [W;V], [W^T;V^T], trial forward weights
  float* WBt_scratch = nullptr;
  // bf16 (hi, mid, lo) planes of the packed matrices for the split-bf16 row GEMM:
  // [part][3][Npad][r16(K)], part 0 = W half, 1 = V half (WF3t: W half only)
  std::vector<uint16_t*> WF3, WB3, WFt3;
  float* X = nullptr;
  float* stage = nullptr;   // staging for host inputs / compact outputs: cap rows of max(pad4(obs), pad4(A), 2) floats
  int* act = nullptr;
  float *adv32 = nullptr, *old = nullptr;   // old: the old distribution, or on a Gaussian engine the old mean
  // Gaussian engine only: the actions [cap][pad4(A)], the old log-std [A] and the partials of g's log-std block
  float *actf = nullptr, *logstd0 = nullptr;
  double* gs_part = nullptr;
  double *rewards = nullptr, *returns = nullptr, *adv64 = nullptr, *baseline = nullptr;
  uint8_t* starts = nullptr;
  bool have_baseline = false, have_rewards = false;
  // advantage estimator (trpo_set_advantage_estimator) and the feed's optional tail values (GAE's V(s_T) of
  // cut-off paths, allocated on first use)
  int adv_kind = TRPO_ADV_RETURNS;
  double adv_lambda = 1.0;
  double* tail = nullptr;
  bool have_tail = false;
  double* ev_tmp = nullptr;   // explained_variance scratch
  std::vector<float*> H, D, E, RH, RD;   // indexed as in DESIGN.md
  float *Pm = nullptr, *DSL = nullptr;
  double* rowterms = nullptr;
  float* slab = nullptr;
  int S = 1, rows_per_split = 16;
  int S_pg = 1, S_cur = 1;
  int64_t slab_stride = 0;
  double *partA = nullptr, *partB = nullptr, *part3 = nullptr, *local3 = nullptr, *dscal = nullptr;
  void* scan_ws = nullptr;
  UpdScalars* sc = nullptr;
  UpdScalars* loss_sc = nullptr;   // where reduce_losses() stores: sc, or a child's own block
  CGFlags* fl = nullptr;
  int* dbad = nullptr;
  UpdScalars* hsc = nullptr;   // pinned host mirror

  // What the device buffers hold beyond their raw contents.  Every host flag that update_prefix() leaves behind
  // lives here: a replayed hipGraph runs no host code, so run_prefix() copies this record after the capture
  // (upd_state = cache) and puts it back after every replay (cache = upd_state).
  struct CacheState {
    bool prepared = false;        // prepare()'s outputs match theta, the batch and the advantages
    bool w3_valid = false;        // W halves of WF3/WB3 match WF/WB
    bool chain_w_valid = false;   // theta parts of the chain images match theta
    bool f16_w_valid = false;     // theta parts of the f16 images match theta
    bool have_returns = false;    // `returns` holds the current rewards' returns
    bool prep_e_top = true;       // prepare() wrote E_{L-2}
    bool prep_fused16 = false;    // prepare() took the fused16 branch (D_1 / E_1 / E_0 and the pg slabs from bwd_pg)
    // the prepare pass also produced the policy gradient's DS_{L-2} (hbwd.hip, in RD[L-2]) and its head-layer block
    // of the slabs
    bool ds_ready = false;
    // fused16.hip's prepare launch also left the policy gradient's blocks in the first pg_grid slabs
    bool pg_ready = false;
    int pg_grid = 0;
    bool d1_plane = false;   // D1h holds the current D_1 (row stride d1_mpad = round256(n))
    bool d1_tiled = false;   // ... with one scale per 32-row tile (eD1t, hbwd.hip) instead of pl_e[1]
    int d1_mpad = 0;
    // the Fisher child (fvp_stride > 1): its feed holds the current feed's rows and advantages; its prepare cache
    // was told of the current theta (fisher_ready())
    bool fisher_fed = false;
    bool fisher_theta = false;

    // theta changed: what prepare() derived from it is stale
    void theta_changed() { prepared = fisher_theta = false; }
    // the batch changed: prepare()'s outputs and the returns belong to the old rows
    void batch_changed() { prepared = have_returns = fisher_fed = false; }
    // new rewards: the returns are the old ones'
    void rewards_changed() { have_returns = false; }
    // the advantages (and with them the returns) were recomputed: the prepare head's DS_L and losses are stale
    void advantages_computed() {
      prepared = fisher_fed = false;
      have_returns = true;
    }
    // prepare() starts over from freshly packed weights: their planes and images are rebuilt on demand, nothing
    // of an earlier pass is left for the policy gradient or the FVP, and this pass serves the given path
    void prepare_begins(bool e_top, bool fused16) {
      w3_valid = chain_w_valid = f16_w_valid = false;
      ds_ready = pg_ready = d1_plane = d1_tiled = false;
      prep_e_top = e_top;
      prep_fused16 = fused16;
    }
    // a launch wrote the slabs: the prepare pass's policy-gradient blocks are gone, except the head-layer block
    // when the writer is the policy gradient's own lower layers (keeps_pg_head)
    void slabs_written(bool keeps_pg_head = false) {
      pg_ready = false;
      if (!keeps_pg_head) ds_ready = false;
    }
    // a launch wrote RD: DS_{L-2} lived in RD[L-2]
    void rd_written() { ds_ready = false; }
  } cache;

  // f16 split GEMMs: running max |operand| slots (float bits) that set the power-of-two scales,
  // grouped by kind, kMaxLayers slots per group (see am_*)
  bool f16 = false;
  unsigned* amax = nullptr;
  unsigned* am(int group, int l) const {
    return f16 ? amax + (size_t)(1 + group * kMaxLayers + l) * kAmaxSlot : nullptr;
  }
  unsigned* am_x() const { return f16 ? amax : nullptr; }
  unsigned* am_w(int l) const { return am(0, l); }
  unsigned* am_v(int l) const { return am(1, l); }
  // group 2: the trial weights' W halves (trial_set)
  unsigned* am_d(int l) const { return am(3, l); }
  unsigned* am_ds(int l) const { return am(4, l); }
  unsigned* am_rh(int l) const { return am(5, l); }
  unsigned* am_rd(int l) const { return am(6, l); }
  void am_reset(unsigned* first, int count) {
    if (first && count > 0)
      HIPCHECK(hipMemsetAsync(first, 0, (size_t)count * kAmaxSlot * sizeof(unsigned), stream));
  }
  // pre-split k-blocked f16 planes for the plane row GEMM (plane.hip): X's hi/lo planes, refreshed with X's
  // running max whenever X changes (layout stride x_mpad = round256(n)), and blocked copies of layer 0's
  // W / V weight planes, re-blocked from WF3 / WFt3 before each use
  uint16_t *Xh = nullptr, *Xl = nullptr, *W0b = nullptr, *V0b = nullptr;
  int* pl_e = nullptr;   // scale exponents published by the plane producers: [0] = X, [1] = D_1, [2] = RH_1
  // D_1's f16 hi plane (k-blocked like Xh, stride cache.d1_mpad), written by prepare() for the fused
  // R-backward's one-product D_1 V_1^T segment (rbwd0.hip), and its per-tile scale exponents
  uint16_t* D1h = nullptr;
  int d1_ldp = 0;
  int* eD1t = nullptr;
  bool use_hbwd2() const {
    // a hidden layer below the head layer, wider than 128 (one thread per column: at 64 columns three
    // quarters of its lanes idle, and C3 ran 3 % slower than on the row GEMMs); E_{L-2} is written too
    // where the FVP path reads it (no fused tail)
    return !gauss() && g_options.hbwd2 != 0 && L >= 3 && wp[L - 1] > 128 && head_bwd2_eligible(w[L], wp[L - 1]);
  }
  int x_mpad = 0, x_ldp = 0;
  bool x_planes = false;   // Xh/Xl hold the current X
  bool planes_geom_l0() const {   // layer 0's row GEMMs fit the plane kernel
    return L >= 2 && wp[1] % 256 == 0 && r16(wp[0]) % 64 == 0;
  }
  bool f16_split() const { return f16 && split_on(); }
  bool x_planes_on() const { return x_planes && g_options.planes != 0 && split_on(); }
  bool planes_l0() const { return x_planes_on() && planes_geom_l0() && rowgemm_uses_split(wp[1], RowEpi::kTanh); }
  // X's planes also feed the fused layer-1 R-backward + layer-0 weight gradient (rbwd0.hip)
  bool rbwd0_geom() const { return L >= 2 && rbwd0_eligible(wp[0], (wp[0] + 63) / 64 * 64, wp[1], wp[2]); }
  // attach X's planes and the blocked copy (into `dst`) of the segment's 2 weight planes to a layer-0 segment
  void attach_x_planes(GemmSeg& sg, uint16_t* dst) {
    launch_block_planes(sg.B3, 2, wp[1], r16(wp[0]), dst, stream);
    sg.Ah = Xh;
    sg.Al = Xl;
    sg.ldp = x_ldp;
    sg.mpad = x_mpad;
    sg.eAp = pl_e;
    sg.Bb = dst;
  }
  uint16_t* tail_planes = nullptr;   // head planes of the fused FVP tail (tail.hip), [2][2][32][kTailK]
  // the fused last-layer tail: f16 split, last hidden width in (128, 256], 17..32 actions
  bool use_tail() const {
    return !gauss() && g_options.tail != 0 && f16_split() && L >= 2 && tail_eligible(wp[L - 1], wp[L]) && w[L] <= 32;
  }
  // whether the FVP path reads E_{L-2} (the plain tanh'' term under the last hidden layer): every path
  // but the fused tail, which recomputes it (tail.hip)
  bool e_top_needed() const { return L < 2 || !use_tail() || use_fused() || use_chain(); }
  // prepare()'s outputs belong to the other kernel path when option fused / split_f16 changed after it ran
  void reprepare_if_path_changed() {
    if (cache.prepared && ((e_top_needed() && !cache.prep_e_top) || cache.prep_fused16 != use_fused16()))
      cache.prepared = false;
  }

  // weight images in the order a fused kernel consumes their chunks, with the chunk table
  struct ImageSet {
    uint16_t* img = nullptr;
    int* tab = nullptr;
    int* e = nullptr;   // f16 images: one scale exponent per job
    int nchunks = 0;
    ChainImgArgs jobs{};
  };
  // fused FVP chain (chain.hip)
  int chain_otm = 0;         // register tiles per hidden layer; 0 = shape not eligible
  ImageSet chain_set;
  // auto (option 1) takes the chain up to 8 register tiles (hidden widths <= 128), where it
  // beats the per-layer row GEMMs; at 16 tiles its per-128-state weight re-streaming
  // (~2 MB of bf16 planes per workgroup tile) costs more than the fusion saves
  // whole FVP (R-forward, head, R-backward and weight gradients) in one launch (fused.hip): one or
  // two hidden layers of width <= 64, obs <= 128, <= 32 actions; reuses the chain's weight images
  bool use_fused() const { return !gauss() && g_options.fused != 0 && chain_otm > 0 && fused_fvp_eligible(L, w.data()); }
  // the same launch on the f16 split (fused16.hip, option fused = 3): two hidden layers of width 49..64; its
  // own weight images (2 f16 planes, one scale exponent per job) and chunk table
  ImageSet f16_set;
  bool f16_v_img_ready = false;   // cg(): the V images of the next fvp_fused16 were built by the CG step launch
  unsigned* cg_ticket = nullptr;  // cg_step_slabs_kernel's arrival ticket (zero between launches)
  // the line-search loss forward's images (W_0 | W_1 | W_2 of the trial vector, fwd_loss16)
  ImageSet f16_loss_set;
  bool use_fused16() const { return !gauss() && g_options.fused == 3 && f16 && f16_set.img && fused16_eligible(L, w.data()); }
  // layer 1's R-backward (and the policy gradient's backward into layer 0) fused with layer 0's weight
  // gradient (rbwd0.hip): f16 split with X's planes, obs <= 128, first hidden width <= 256
  uint16_t* rf_img = nullptr;   // rfwd.hip's chunk image (V0^T, W1, V1 in the kernel's LDS order), per FVP
  uint16_t* fw_img = nullptr;   // rfwd.hip's forward image (W0^T, W1), per forward
  // the R-forward through layers 0 and 1 in one launch: X's planes, the fused tail (RZ2 is its pre-activation)
  bool use_rfwd01() const {
    return g_options.rfwd01 != 0 && rf_img && f16_split() && use_tail() && planes_l0() &&
           rfwd01_eligible(L, w.data(), wp.data()) && rfwd01_rows_ok(x_mpad);
  }
  // the forward's layers 0 and 1 in one launch (rfwd.hip fwd01_kernel): tanh layers of 256, X on its planes
  bool use_fwd01() const {
    return g_options.fwd01 != 0 && fw_img && f16_split() && planes_l0() && fwd01_eligible(L, w.data(), wp.data()) &&
           rfwd01_rows_ok(x_mpad);
  }
  bool use_rbwd0() const {
    return g_options.rbwd0 != 0 && f16 && x_planes_on() && rbwd0_geom() && rowgemm_uses_split(wp[1], RowEpi::kRBwd);
  }
  // RH1 as row-paired f16 planes in RH[1]'s bytes (option rh1_planes): rfwd01 writes them, and its two readers, the
  // fused R-backward's epilogue and the layer-1 weight gradient on the split kernel, both take planes; decided
  // per fvp() call, which holds the producer and both readers, so no state outlives the call
  bool use_rh1_planes() const {
    return g_options.rh1_planes != 0 && use_rfwd01() && use_rbwd0() && g_options.split_wg != 0 &&
           wp[1] == kPairLd && pair_planes_rows_ok(x_mpad);
  }
  PairPlane rh1_planes() const {
    const unsigned* hi = reinterpret_cast<const unsigned*>(RH[1]);
    return PairPlane{hi, hi + pair_plane_dwords(n), pl_e + 2};
  }
  RBwd0Args rbwd0_args(const int* skip) const {
    RBwd0Args a{};
    a.rows = (int)n;
    a.K = wp[2];
    a.lda = wp[2];
    a.N = w[1];
    a.Npad = wp[1];
    a.obs = w[0];
    a.B0 = WB3[1];
    a.B1 = WB3[1] + 3 * plane3_b(1);
    a.ldk = r16(wp[2]);
    a.plane = (int64_t)plane3_b(1);
    a.am_b0 = am_w(1);
    a.am_b1 = am_v(1);
    a.H = H[1];
    a.Xh = Xh;
    a.Xl = Xl;
    a.x_mpad = x_mpad;
    a.x_ldp = x_ldp;
    a.eX = pl_e;
    a.dst = slab_dst(0);
    a.skip = skip;
    return a;
  }
  bool use_chain() const {
    return !gauss() && chain_otm > 0 && (g_options.chain >= 2 || (g_options.chain == 1 && chain_otm <= 8));
  }

  // rollout (rollout.hip): per-environment regions, reallocated when a rollout needs more
  struct RollBufs {
    std::vector<void*> mem;
    int64_t rows = 0;      // capacity in region rows
    int envs = 0;
    double* obs = nullptr;
    double* env_state = nullptr;   // [rows][state_cap]; only for an environment whose observation is not its state
    int state_cap = 0;
    int64_t* actions = nullptr;   // categorical
    float* dist = nullptr;
    double* noise = nullptr;      // [rows] cat_sample uniforms, or (Gaussian) [rows][A] normals
    double* rewards = nullptr;
    uint8_t* starts = nullptr;
    int64_t *counts = nullptr, *episodes = nullptr, *offsets = nullptr;
    double *reset_u = nullptr, *act_u = nullptr;
    int64_t reset_u_n = 0, act_u_n = 0;
    // how each path ended: per-environment path regions (n_envs * budget paths), the path offsets of the
    // compaction, and the concatenated records the tail view hands out (trpo_rollout_to_batch fills them)
    int64_t paths = 0;     // capacity in region paths
    uint8_t* end_truncated = nullptr;
    double* end_obs = nullptr;
    float* end_dist = nullptr;
    int64_t *end_len = nullptr, *end_row = nullptr, *path_offsets = nullptr;
    uint8_t* cat_truncated = nullptr;
    float *cat_obs32 = nullptr, *cat_dist = nullptr;
    int64_t *cat_len = nullptr, *cat_rows = nullptr;
    // a Gaussian engine's rollout (trpo_rollout_gaussian): dist, end_dist and cat_dist hold means; the actions
    // [rows][A] f32 and the log-std vector [A] the rollout sampled with
    float* actf = nullptr;
    float* logstd = nullptr;
    // a segment rollout's columns (allocated with the rest once a segment rollout asks): step_index [rows], the
    // path regions' kind / t0 / episode return, and for the tail view the episode's step count at s_T
    int64_t* step_index = nullptr;
    uint8_t* end_kind = nullptr;
    int64_t* end_t0 = nullptr;
    double* end_ret = nullptr;
    int64_t* cat_steps = nullptr;
  } roll;
  RolloutArgs roll_args{};   // the last rollout (roll_valid)
  int64_t roll_n = 0, roll_paths = 0, roll_maxcount = 0, roll_maxpaths = 0;
  bool roll_valid = false;
  bool roll_segment = false;      // the last rollout was a segment rollout (seg_args holds roll_args and the rest)
  SegmentArgs seg_args{};
  bool feed_is_rollout = false;   // the feed is the one trpo_rollout_to_batch loaded (trpo_get_tail_view)
  // The segment rollouts' carry, apart from RollBufs: it outlives every rollout, whole-episode ones included, and
  // trpo_set_flat.  Reallocated only when a carry of more environments or a wider state is stored.
  struct Carry {
    double* s = nullptr;       // [n_envs][state_dim]
    int64_t* t = nullptr;
    double* ret = nullptr;
    int64_t cap = 0;           // doubles s holds
    int cap_envs = 0;
    bool valid = false;
    bool continuous = false;
    int env = 0, n_envs = 0, state_dim = 0;
  } carry;
  // the feed's step_index [cap] (a segment rollout's feed; trpo_feed_view.step_index), allocated on first use
  int64_t* feed_step = nullptr;
  bool feed_has_step = false;

  // profiling
  bool prof = false;
  struct Ev {
    std::string tag;
    hipEvent_t a, b;
  };
  std::vector<Ev> ev_live;
  std::vector<hipEvent_t> ev_pool;
  std::map<std::string, std::pair<long, double>> prof_acc;

  // ------------------------------------------------------------------------
  template <class T>
  T* dalloc(size_t count) {
    void* ptr = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    HIPCHECK(hipMalloc(&ptr, bytes));
    HIPCHECK(hipMemsetAsync(ptr, 0, bytes, stream));
    allocs.push_back(ptr);
    return static_cast<T*>(ptr);
  }

  void use() {
    HIPCHECK(hipSetDevice(device));
    if (!har_slots.empty()) rewind_har();
  }

  const float* act_in(int l) const { return l == 0 ? X : H[l]; }

  hipEvent_t take_event() {
    if (!ev_pool.empty()) {
      hipEvent_t e = ev_pool.back();
      ev_pool.pop_back();
      return e;
    }
    hipEvent_t e;
    HIPCHECK(hipEventCreate(&e));
    return e;
  }
  struct Scope {
    trpo_engine* e;
    int idx = -1;
    Scope(trpo_engine* eng, const char* tag) : e(eng) {
      if (e->prof) begin(tag);
    }
    // "<prefix><suffix>", and the per-layer tags "<prefix>_l<l>"
    Scope(trpo_engine* eng, const char* prefix, const char* suffix) : e(eng) {
      if (e->prof) begin(std::string(prefix) + suffix);
    }
    Scope(trpo_engine* eng, const char* prefix, int l) : e(eng) {
      if (e->prof) begin(std::string(prefix) + "_l" + std::to_string(l));
    }
    void begin(const std::string& tag) {
      Ev ev{e->tag_prefix + tag, e->take_event(), e->take_event()};
      HIPCHECK(hipEventRecord(ev.a, e->stream));
      e->ev_live.push_back(ev);
      idx = (int)e->ev_live.size() - 1;
    }
    ~Scope() {
      if (idx >= 0) (void)hipEventRecord(e->ev_live[idx].b, e->stream);
    }
  };
  void prof_collect() {
    if (fisher) {   // the child's launches, in the same table under their own tags
      fisher->prof_collect();
      for (auto& kv : fisher->prof_acc) {
        auto& acc = prof_acc[kv.first];
        acc.first += kv.second.first;
        acc.second += kv.second.second;
      }
      fisher->prof_acc.clear();
    }
    if (ev_live.empty()) return;
    HIPCHECK(hipStreamSynchronize(stream));
    for (auto& ev : ev_live) {
      float ms = 0.f;
      HIPCHECK(hipEventElapsedTime(&ms, ev.a, ev.b));
      auto& acc = prof_acc[ev.tag];
      acc.first += 1;
      acc.second += ms;
      ev_pool.push_back(ev.a);
      ev_pool.push_back(ev.b);
    }
    ev_live.clear();
  }

  // ------------------------------------------------------------------------
  // parent != NULL builds a Fisher child: no stream, theta or CG scalar block of its own (see `fisher`)
  void init(int dist_id, int obs, const int* hidden, int nh, int A, int64_t max_rows, int dev,
            trpo_engine* parent = nullptr) {
    REQUIRE(dist_id == TRPO_DIST_CATEGORICAL || dist_id == TRPO_DIST_GAUSSIAN,
            "dist must be TRPO_DIST_CATEGORICAL or TRPO_DIST_GAUSSIAN");
    dist = dist_id;
    REQUIRE(obs > 0 && A > 0 && nh >= 0 && max_rows > 0, "invalid policy dimensions");
    REQUIRE(nh + 1 <= kMaxLayers, "too many layers");
    REQUIRE(A <= 32 * kMaxHeadTiles, gauss() ? "act_dim must be <= 128 (head rows of up to 4 x 32 lanes)"
                                             : "n_actions must be <= 128 (softmax rows of up to 4 x 32 lanes)");
    REQUIRE(max_rows < (int64_t(1) << 31), "max_rows must fit in int32 row indices");
    for (int i = 0; i < nh; ++i) REQUIRE(hidden[i] > 0, "hidden widths must be positive");
    device = dev;
    use();
    HIPCHECK(hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, device));
    owner = parent;
    if (parent) {
      stream = parent->stream;
      tag_prefix = "sub.";
    } else {
      HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    }
    w.push_back(obs);
    for (int i = 0; i < nh; ++i) w.push_back(hidden[i]);
    w.push_back(A);
    L = (int)w.size() - 1;
    for (int v : w) wp.push_back(pad4(v));
    P = 0;
    for (int l = 0; l < L; ++l) {
      offW.push_back(P);
      P += (int64_t)w[l] * w[l + 1];
      offb.push_back(P);
      P += w[l + 1];
    }
    if (gauss()) P += A;   // the log-std vector, last in the flat layout
    cap = max_rows;

    if (parent) theta = parent->theta;
    else theta = dalloc<float>(P);
    for (float** v : {&theta_prev, &theta_trial, &theta_ls, &g, &bneg, &x, &r, &p, &p2, &z, &hv, &stepdir, &fullstep,
                      &vin, &vout})
      *v = dalloc<float>(P);
    int maxpad = 4;
    for (int l = 0; l < L; ++l) {
      WF.push_back(dalloc<float>((size_t)2 * wp[l] * wp[l + 1]));
      WB.push_back(dalloc<float>((size_t)2 * wp[l + 1] * wp[l]));
      WFt.push_back(dalloc<float>((size_t)2 * wp[l] * wp[l + 1]));
      maxpad = std::max<int>(maxpad, 2 * wp[l] * wp[l + 1]);
    }
    WBt_scratch = dalloc<float>(maxpad);
    for (int l = 0; l < L; ++l) {
      WF3.push_back(dalloc<uint16_t>(2 * plane3_f(l) * 3));
      WB3.push_back(dalloc<uint16_t>(2 * plane3_b(l) * 3));
      WFt3.push_back(dalloc<uint16_t>(plane3_f(l) * 3));
    }
    X = dalloc<float>((size_t)cap * wp[0]);
    act = dalloc<int>(cap);
    adv32 = dalloc<float>(cap);
    old = dalloc<float>((size_t)cap * wp[L]);
    rewards = dalloc<double>(cap);
    returns = dalloc<double>(cap);
    adv64 = dalloc<double>(cap);
    baseline = dalloc<double>(cap);
    starts = dalloc<uint8_t>(cap);
    H.assign(L + 1, nullptr);
    RH.assign(L + 1, nullptr);
    D.assign(L, nullptr);
    RD.assign(L, nullptr);
    E.assign(L, nullptr);
    for (int l = 1; l < L; ++l) {
      H[l] = dalloc<float>((size_t)cap * wp[l]);
      // (an even row count: RH[1] also holds RH1's row-paired planes, two planes of ceil(n / 2) row pairs)
      RH[l] = dalloc<float>((size_t)(cap + (cap & 1)) * wp[l]);
    }
    for (int l = 0; l < L; ++l) {
      D[l] = dalloc<float>((size_t)cap * wp[l + 1]);
      RD[l] = dalloc<float>((size_t)cap * wp[l + 1]);
      if (l < L - 1) E[l] = dalloc<float>((size_t)cap * wp[l + 1]);
    }
    Pm = dalloc<float>((size_t)cap * wp[L]);
    DSL = dalloc<float>((size_t)cap * wp[L]);
    rowterms = dalloc<double>((size_t)cap * 4);
    // split-K slabs for the weight gradients
    int tiles_max = 1;
    for (int l = 0; l < L; ++l)
      tiles_max = std::max(tiles_max, ((w[l] + 255) / 256) * ((w[l + 1] + 255) / 256));
    slab_stride = (P + 63) / 64 * 64;
    int s_target = std::max(1, std::min(512, 1024 / tiles_max));
    // narrow layers (one output tile each): a 512-split launch is 1-4 waves per CU, too few to stream
    // the activations at HBM rate; small policies take up to 2048 splits while the slabs fit 128 MB
    if (tiles_max == 1)
      s_target = (int)std::max<int64_t>(s_target, std::min<int64_t>(2048, (int64_t(128) << 20) / (slab_stride * 4)));
    // a split accumulates its rows in f32 MFMA accumulators, whose error grows with the rows per split (DESIGN.md
    // §6, numerics at full size): at least one FVP split per 16k rows (wide layers: C5 64 -> 245), and for the
    // policy gradient (once per update; its layer-0/1 blocks are sums of adv_n s_n with mean-zero advantages) 4x
    // that and one per 4k rows, up to 2048; slabs within 2 GB / 8 GB
    const int64_t slab_bytes = (int64_t)slab_stride * 4;
    auto fit = [&](int64_t bytes) { return std::max<int64_t>(1, bytes / slab_bytes); };
    s_target = (int)std::max<int64_t>(s_target, std::min<int64_t>(fit(int64_t(2) << 30), (cap + 16383) / 16384));
    // wide single-tile layers (C4) with few rows (a rank of a 2-8 GPU run): one split per CU when the rows allow it,
    // i.e. one round of the one-workgroup-per-CU split kernels and half the slab reduction (1M rows: 58.3 -> 57.2
    // ms per update, 2M: 111.1 -> 110.4; 128 splits lose half the CUs, profiles/r5u)
    if (tiles_max == 1 && s_target == 512 && num_cus < 512 && (cap + 16383) / 16384 <= num_cus) s_target = num_cus;
    if (g_options.splits > 0) s_target = std::min(g_options.splits, 8192);
    int s_pg = (int)std::max<int64_t>(
        s_target, std::min<int64_t>({2048, std::max<int64_t>(4 * (int64_t)s_target, (cap + 4095) / 4096),
                                     fit(int64_t(8) << 30)}));
    if (g_options.pg_splits > 0) s_pg = std::min(g_options.pg_splits, 8192);
    slab = dalloc<float>((size_t)std::max(s_target, s_pg) * slab_stride);
    S = s_target;
    S_pg = s_pg;
    S_cur = S;
    partA = dalloc<double>(kRedBlocks * 3);
    partB = dalloc<double>(kRedBlocks * 3);
    part3 = dalloc<double>(kRedBlocks * 3);
    local3 = dalloc<double>(4);
    dscal = dalloc<double>(8);
    scan_ws = dalloc<uint8_t>(std::max(discount_workspace_bytes(cap), gae_workspace_bytes(cap)));
    if (parent) {
      sc = parent->sc;
      fl = parent->fl;
      loss_sc = dalloc<UpdScalars>(1);
    } else {
      sc = dalloc<UpdScalars>(1);
      fl = dalloc<CGFlags>(1);
      loss_sc = sc;
    }
    cg_ticket = dalloc<unsigned>(1);
    dbad = dalloc<int>(1);
    f16 = g_options.split_f16 != 0;
    amax = dalloc<unsigned>((size_t)(1 + 8 * kMaxLayers) * kAmaxSlot);
    if (L >= 2 && tail_eligible(wp[L - 1], wp[L])) tail_planes = dalloc<uint16_t>((size_t)2 * 2 * 32 * kTailK);
    if (rfwd01_eligible(L, w.data(), wp.data())) rf_img = dalloc<uint16_t>(rfwd01_img_bytes() / 2);
    if (fwd01_eligible(L, w.data(), wp.data())) fw_img = dalloc<uint16_t>(fwd01_img_bytes() / 2);
    // allocated last: the big activation buffers keep the placement the kernels were tuned on
    stage = dalloc<float>((size_t)cap * std::max(std::max(wp[0], wp[L]), 2));
    if (f16 && (planes_geom_l0() || rbwd0_geom())) {
      x_ldp = (wp[0] + 63) / 64 * 64;
      // rfwd01 / fwd01 load all four 32-column k-blocks of an X plane whatever obs is (rfwd.hip xload: 8 k-steps
      // through a descriptor with no size; the weight image's rows past obs are zero), so the planes hold four
      // blocks there: with x_ldp = 64 the loads ran 2 x_mpad rows past the end of the allocation
      const int x_cols = rfwd01_eligible(L, w.data(), wp.data()) ? std::max(x_ldp, 128) : x_ldp;
      const size_t xp = (size_t)((cap + 255) / 256 * 256) * x_cols;
      Xh = dalloc<uint16_t>(xp);
      Xl = dalloc<uint16_t>(xp);
      W0b = dalloc<uint16_t>(2 * plane3_f(0));
      V0b = dalloc<uint16_t>(2 * plane3_f(0));
      pl_e = dalloc<int>(8);
    }
    if (f16 && L >= 2 && rbwd0_geom()) {
      d1_ldp = (wp[2] + 31) / 32 * 32;
      D1h = dalloc<uint16_t>((size_t)((cap + 255) / 256 * 256) * d1_ldp);
      eD1t = dalloc<int>((size_t)(cap + 31) / 32 + 8);
    }
    if (gauss()) {
      actf = dalloc<float>((size_t)cap * wp[L]);
      logstd0 = dalloc<float>(wp[L]);
      gs_part = dalloc<double>((size_t)kGaussColBlocks * 128);
    }
    if (!parent) {   // (a child never fetches scalars: its owner does)
      HIPCHECK(hipHostMalloc((void**)&hsc, sizeof(UpdScalars), hipHostMallocDefault));
      std::memset(hsc, 0, sizeof(UpdScalars));
    }
    if (!gauss()) {   // the fused FVP kernels embed the softmax head
      setup_chain();
      setup_fused16();
    }
    HIPCHECK(hipStreamSynchronize(stream));
  }

  // One image job: W_l (which = 0) or V_l (1), transposed or not, as K x O
  struct ImgJob {
    int l, trans, which;
  };
  struct ImgGeom {
    int kc, otp, csz;   // k-chunks, padded output rows, 16-B units per chunk
  };
  // the order the FVP kernels consume chunks: R-forward F_0 (V_0), F_l (W_l, V_l) for l = 1..L-1, then
  // R-backward B_l (W_l^T, V_l^T) for l = L-1..1
  std::vector<ImgJob> fvp_image_order() const {
    std::vector<ImgJob> order = {ImgJob{0, 0, 1}};
    for (int l = 1; l < L; ++l) {
      order.push_back({l, 0, 0});
      order.push_back({l, 0, 1});
    }
    for (int l = L - 1; l >= 1; --l) {
      order.push_back({l, 1, 0});
      order.push_back({l, 1, 1});
    }
    return order;
  }
  // lay `order` out under geom(l, trans, K, O): the jobs and the chunk table, then the image, the table and
  // n_exps scale exponents (allocated in that order), the table uploaded
  template <class Geom>
  void build_images(ImageSet& is, const std::vector<ImgJob>& order, int n_exps, Geom geom) {
    REQUIRE(order.size() <= (size_t)kMaxChainJobs, "fvp chain: layout too large");
    std::vector<int> tab;
    int64_t off16 = 0;
    is.jobs.n = 0;
    for (const ImgJob& o : order) {
      const int l = o.l, K = o.trans ? w[l + 1] : w[l], O = o.trans ? w[l] : w[l + 1];
      const ImgGeom g = geom(l, o.trans, K, O);
      ChainImgJob& j = is.jobs.job[is.jobs.n++];
      j.src_off = offW[l];
      j.dst_off = off16 * 8;
      j.K = K;
      j.O = O;
      j.ldw = w[l + 1];
      j.trans = o.trans;
      j.kc = g.kc;
      j.otp = g.otp;
      j.which = o.which;
      j.pad = 0;
      for (int c = 0; c < g.kc; ++c) {
        tab.push_back((int)(off16 + (int64_t)c * g.csz));
        tab.push_back(g.csz);
      }
      off16 += (int64_t)g.kc * g.csz;
    }
    REQUIRE(off16 < (int64_t(1) << 31), "fvp chain: layout too large");
    is.img = dalloc<uint16_t>((size_t)off16 * 8);
    is.tab = dalloc<int>(tab.size());
    if (n_exps) is.e = dalloc<int>(n_exps);
    is.jobs.img = is.img;
    HIPCHECK(hipMemcpyAsync(is.tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));   // `tab` is a local vector
    is.nchunks = (int)(tab.size() / 2);
  }

  // Weight images of the fused FVP chain: each segment is ceil(K/32) chunks of
  // [3 planes][16*ceil(O/16) rows][32] bf16.
  void setup_chain() {
    if (L < 2 || w[L] > 32) return;
    int hmax = 0;
    for (int l = 1; l < L; ++l) hmax = std::max(hmax, w[l]);
    const int otm = chain_max_tiles(hmax);
    if (!otm) return;
    build_images(chain_set, fvp_image_order(), 0, [](int, int, int K, int O) {
      const int otp = r16(O);
      return ImgGeom{(K + 31) / 32, otp, otp * 12};
    });
    chain_otm = otm;
  }

  // fused16.hip's images: the chain's job order with 2 f16 planes per chunk, V_0 padded to
  // fused16_obs_chunks(obs) chunks and every hidden dimension to 64 (2 chunks of K, 64 rows of O: the kernel's
  // hidden layers are 4 tiles of 16 whatever the width, the padding zeros)
  void setup_fused16() {
    if (!fused16_eligible(L, w.data())) return;
    auto geom = [this](int l, int trans, int K, int O) {
      const bool k_hidden = trans ? l + 1 < L : l > 0, o_hidden = trans ? true : l + 1 < L;
      const int kc = l == 0 && !trans ? fused16_obs_chunks(w[0]) : k_hidden ? 2 : (K + 31) / 32;
      const int otp = o_hidden ? 64 : r16(O);
      return ImgGeom{kc, otp, otp * 8};
    };
    const std::vector<ImgJob> order = fvp_image_order();
    REQUIRE((int)order.size() == (L == 3 ? kFused16Jobs : 5), "fused16: job count");
    build_images(f16_set, order, kFused16Jobs, geom);
    // the loss forward's W_0 | W_1 | W_2 (from the trial vector: which = 0, built per line-search trial)
    std::vector<ImgJob> loss_order;
    for (int l = 0; l < L; ++l) loss_order.push_back({l, 0, 0});
    build_images(f16_loss_set, loss_order, L, geom);
  }

  PolicyShape policy_shape() const {
    PolicyShape ps{};
    ps.L = L;
    for (int l = 0; l <= L; ++l) ps.w[l] = w[l];
    for (int l = 0; l < L; ++l) {
      ps.offW[l] = offW[l];
      ps.offb[l] = offb[l];
    }
    return ps;
  }
  int max_width() const {
    int m = 1;
    for (int l = 0; l <= L; ++l) m = std::max(m, w[l]);
    return m;
  }

  template <class T>
  T* ralloc(size_t count) {
    void* ptr = nullptr;
    HIPCHECK(hipMalloc(&ptr, std::max<size_t>(count * sizeof(T), 16)));
    roll.mem.push_back(ptr);
    return static_cast<T*>(ptr);
  }

  // rollout (utils.py:18-45) of n_envs instances of a built-in environment under the current policy: an environment
  // of TRPO_ENV_* under the categorical head, or (continuous) of TRPO_CENV_* under the Gaussian one.  Every check
  // comes before anything of the previous rollout is freed or overwritten, so a refused call leaves it fetchable.
  // A Gaussian rollout copies the log-std vector aside first: it samples with the copy, and the feed built from it
  // (trpo_rollout_gaussian_to_batch) takes it as the old log-std whatever theta has become since.
  void rollout(bool continuous, int env, const trpo_rollout_params& p, bool segment = false, int resume = 0) {
    EnvDims ed{};
    REQUIRE(env_dims(continuous, env, &ed),
            std::string(continuous ? "unknown continuous environment id " : "unknown environment id ") +
                std::to_string(env));
    REQUIRE(p.n_envs >= 1 && p.n_envs <= (1 << 20), "n_envs out of range");
    REQUIRE(p.n_timesteps >= 1 && p.max_pathlength >= 1 && p.time_limit >= 1, "bad rollout lengths");
    auto head = [&](int n) { return continuous ? "act_dim " + std::to_string(n) : std::to_string(n) + " actions"; };
    REQUIRE(w[0] == ed.obs_dim && w[L] == ed.head_dim,
            std::string(ed.name) + " needs obs_dim " + std::to_string(ed.obs_dim) + " and " + head(ed.head_dim) +
                "; the engine has obs_dim " + std::to_string(w[0]) + " and " + head(w[L]));
    const int obs_dim = ed.obs_dim, A = ed.head_dim, noise_dim = continuous ? A : 1;
    const int state_cap = ed.state_dim == ed.obs_dim ? 0 : ed.state_dim;   // such environments observe the state itself
    const int ep_max = std::min(p.max_pathlength, p.time_limit);
    const int64_t budget = (p.n_timesteps + p.n_envs - 1) / p.n_envs;
    // a segment rollout writes exactly budget rows per environment: its regions are the concatenated rollout
    const int64_t env_cap = segment ? budget : budget + ep_max - 1;
    const int64_t rows = env_cap * p.n_envs;
    REQUIRE(rows <= (int64_t(1) << 34), "rollout too large");
    const int64_t paths = budget * p.n_envs;   // every episode has at least one step
    if (p.reset_uniforms) {
      REQUIRE(p.max_episodes_per_env >= 1, "max_episodes_per_env required with reset_uniforms");
      // every episode an environment can start must have its uniforms; a segment resets after every step that
      // ends an episode, its last included, and once more at the start unless it resumes
      if (segment)
        REQUIRE((int64_t)p.max_episodes_per_env >= budget + (resume ? 0 : 1),
                "max_episodes_per_env must be >= ceil(n_timesteps/n_envs) + (resume ? 0 : 1)");
      else
        REQUIRE((int64_t)p.max_episodes_per_env >= budget, "max_episodes_per_env must be >= ceil(n_timesteps/n_envs)");
    }
    if (segment && resume) carry_check(continuous, env, p.n_envs, ed.state_dim, ep_max);
    if (segment) carry_reserve(p.n_envs, ed.state_dim);   // before the previous rollout is touched
    feed_is_rollout = false;   // the end records of the loaded feed and the regions are about to be overwritten
    roll_valid = false;
    if (rows > roll.rows || p.n_envs > roll.envs || paths > roll.paths || state_cap > roll.state_cap ||
        (segment && !roll.step_index)) {
      for (void* ptr : roll.mem) HIPCHECK(hipFree(ptr));
      roll = RollBufs{};
      roll.rows = rows;
      roll.envs = p.n_envs;
      roll.paths = paths;
      roll.end_truncated = ralloc<uint8_t>(paths);
      roll.end_obs = ralloc<double>((size_t)paths * obs_dim);
      roll.end_dist = ralloc<float>((size_t)paths * A);
      roll.end_len = ralloc<int64_t>(paths);
      roll.end_row = ralloc<int64_t>(paths);
      roll.cat_truncated = ralloc<uint8_t>(paths);
      roll.cat_obs32 = ralloc<float>((size_t)paths * obs_dim);
      roll.cat_dist = ralloc<float>((size_t)paths * A);
      roll.cat_len = ralloc<int64_t>(paths);
      roll.cat_rows = ralloc<int64_t>(paths);
      roll.obs = ralloc<double>((size_t)rows * obs_dim);
      roll.state_cap = state_cap;
      if (state_cap) roll.env_state = ralloc<double>((size_t)rows * state_cap);
      roll.dist = ralloc<float>((size_t)rows * A);
      roll.noise = ralloc<double>((size_t)rows * noise_dim);
      if (continuous) {
        roll.actf = ralloc<float>((size_t)rows * A);
        roll.logstd = ralloc<float>(A);
      } else {
        roll.actions = ralloc<int64_t>(rows);
      }
      roll.rewards = ralloc<double>(rows);
      roll.starts = ralloc<uint8_t>(rows);
      roll.counts = ralloc<int64_t>(p.n_envs);
      roll.episodes = ralloc<int64_t>(p.n_envs);
      roll.offsets = ralloc<int64_t>((size_t)2 * p.n_envs);
      if (segment) {
        roll.step_index = ralloc<int64_t>(rows);
        roll.end_kind = ralloc<uint8_t>(paths);
        roll.end_t0 = ralloc<int64_t>(paths);
        roll.end_ret = ralloc<double>(paths);
        roll.cat_steps = ralloc<int64_t>(paths);
      }
    }
    RolloutArgs a{};
    a.continuous = continuous;
    a.env = env;
    a.state_dim = ed.state_dim;
    a.ps = policy_shape();
    a.theta = theta;
    a.logstd = roll.logstd;
    a.maxw = max_width();
    a.n_envs = p.n_envs;
    a.max_pathlength = p.max_pathlength;
    a.time_limit = p.time_limit;
    a.train = p.train;
    a.budget = budget;
    a.env_cap = env_cap;
    a.max_episodes = p.max_episodes_per_env;
    a.seed = p.seed;
    // optional injected draws (tests): reset uniforms [n_envs][max_episodes][reset_draws], and for the act uniforms
    // [n_envs][env_cap] or (continuous) standard normals [n_envs][env_cap][A]
    auto stage_u = [&](const double* src, int64_t count, double*& buf, int64_t& cap_n) -> const double* {
      if (!src) return nullptr;
      if (p.mem == TRPO_MEM_DEVICE) return src;
      if (count > cap_n) {
        buf = ralloc<double>(count);
        cap_n = count;
      }
      copy_in(buf, src, (size_t)count * sizeof(double), TRPO_MEM_HOST);
      return buf;
    };
    a.reset_u = stage_u(p.reset_uniforms, (int64_t)p.n_envs * std::max(1, p.max_episodes_per_env) * ed.reset_draws,
                        roll.reset_u, roll.reset_u_n);
    a.draws = stage_u(p.action_uniforms, rows * noise_dim, roll.act_u, roll.act_u_n);
    if (continuous) copy_in(roll.logstd, logstd_of(theta), (size_t)A * sizeof(float), TRPO_MEM_DEVICE);
    a.obs = roll.obs;
    a.env_state = state_cap ? roll.env_state : nullptr;
    a.head = roll.dist;
    a.acti = roll.actions;
    a.actf = roll.actf;
    a.noise = roll.noise;
    a.noise_dim = noise_dim;
    a.rewards = roll.rewards;
    a.starts = roll.starts;
    a.counts = roll.counts;
    a.episodes = roll.episodes;
    a.end_truncated = roll.end_truncated;
    a.end_obs = roll.end_obs;
    a.end_head = roll.end_dist;
    a.end_len = roll.end_len;
    a.end_row = roll.end_row;
    roll_segment = segment;
    if (segment) {
      SegmentArgs g{};
      g.r = a;
      g.resume = resume ? 1 : 0;
      g.carry_s = carry.s;
      g.carry_t = carry.t;
      g.carry_ret = carry.ret;
      g.step_index = roll.step_index;
      g.end_kind = roll.end_kind;
      g.end_t0 = roll.end_t0;
      g.end_ret = roll.end_ret;
      carry.valid = false;   // until the kernel that rewrites it is enqueued
      launch_rollout_segment(g, stream);
      check_launch();
      carry.valid = true;
      carry.continuous = continuous;
      carry.env = env;
      carry.n_envs = p.n_envs;
      carry.state_dim = ed.state_dim;
      seg_args = g;
    } else {
      launch_rollout(a, stream);
      check_launch();
    }
    roll_args = a;
    rollout_offsets(p.n_envs);
  }

  // room for a carry of n_envs environments; a valid carry survives (it is only ever grown by the call that
  // replaces it, and a resumed rollout has checked that it fits already)
  void carry_reserve(int n_envs, int state_dim) {
    const int64_t need = (int64_t)n_envs * state_dim;
    if (need <= carry.cap && n_envs <= carry.cap_envs) return;
    double* s = nullptr;
    int64_t* t = nullptr;
    double* ret = nullptr;
    HIPCHECK(hipMalloc(reinterpret_cast<void**>(&s), (size_t)need * sizeof(double)));
    if (hipMalloc(reinterpret_cast<void**>(&t), (size_t)n_envs * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&ret), (size_t)n_envs * sizeof(double)) != hipSuccess) {
      (void)hipFree(s);
      (void)hipFree(t);
      throw ::trpo_abi::HipError("hipMalloc of the rollout carry failed");
    }
    HIPCHECK(hipStreamSynchronize(stream));   // nothing enqueued reads the old buffers past this point
    carry_free();
    carry.s = s;
    carry.t = t;
    carry.ret = ret;
    carry.cap = need;
    carry.cap_envs = n_envs;
  }
  void carry_free() {
    (void)hipFree(carry.s);
    (void)hipFree(carry.t);
    (void)hipFree(carry.ret);
    carry = Carry{};
  }
  // resume = 1: the carry must be this environment's, under this head, of as many environments, and every carried
  // episode must have a step left
  void carry_check(bool continuous, int env, int n_envs, int state_dim, int ep_max) {
    if (!carry.valid)
      throw std::runtime_error("resume = 1 needs a carry: no segment rollout or trpo_rollout_carry_set came before");
    if (carry.continuous != continuous || carry.env != env || carry.n_envs != n_envs || carry.state_dim != state_dim)
      throw std::runtime_error("resume = 1: the carry is of environment id " + std::to_string(carry.env) +
                               (carry.continuous ? " (continuous)" : " (discrete)") + " with n_envs " +
                               std::to_string(carry.n_envs) + ", not of this call's");
    std::vector<int64_t> t(n_envs);
    copy_out(t.data(), carry.t, t.size() * sizeof(int64_t), TRPO_MEM_HOST);
    for (int i = 0; i < n_envs; ++i)
      REQUIRE(t[i] >= 0 && t[i] < ep_max, "resume = 1: environment " + std::to_string(i) + " carries t = " +
                                              std::to_string(t[i]) + ", outside [0, min(max_pathlength, time_limit))");
  }

  // after a rollout kernel: row offsets [n_envs], then path offsets [n_envs] (one upload), and the totals
  void rollout_offsets(int n_envs) {
    std::vector<int64_t> counts(n_envs), eps(n_envs), offs((size_t)2 * n_envs);
    copy_out(counts.data(), roll.counts, counts.size() * sizeof(int64_t), TRPO_MEM_HOST);
    copy_out(eps.data(), roll.episodes, eps.size() * sizeof(int64_t), TRPO_MEM_HOST);
    int64_t tot = 0, mx = 0, ptot = 0, pmx = 0;
    for (int i = 0; i < n_envs; ++i) {
      offs[i] = tot;
      tot += counts[i];
      mx = std::max(mx, counts[i]);
      offs[n_envs + i] = ptot;
      ptot += eps[i];
      pmx = std::max(pmx, eps[i]);
    }
    copy_in(roll.offsets, offs.data(), offs.size() * sizeof(int64_t), TRPO_MEM_HOST);
    roll.path_offsets = roll.offsets + n_envs;
    roll_n = tot;
    roll_maxcount = mx;
    roll_paths = ptot;
    roll_maxpaths = pmx;
    roll_valid = true;
  }

  void rollout_compact(const RolloutOut& o) {
    REQUIRE(roll_valid, "no rollout to fetch");
    launch_rollout_compact(roll_args, roll.offsets, o, o.ends_only ? roll_maxpaths : roll_maxcount, stream);
    check_launch();
  }

  void segment_compact(const SegmentOut& o) {
    if (!(roll_valid && roll_segment)) throw std::runtime_error("the last rollout was not a segment rollout");
    launch_rollout_segment_compact(seg_args, roll.path_offsets, o, roll_maxpaths, stream);
    check_launch();
  }

  // how each path of the last rollout ended, concatenated; final_head is the distribution or the mean at s_T
  void rollout_fetch_ends(uint8_t* truncated, double* final_obs, float* final_head, int64_t* lengths,
                          int64_t* end_rows, int mem) {
    use();
    const int64_t P = roll_paths;
    const int obs_dim = w[0], A = w[L];
    RolloutOut o{};
    Staging st(mem, stream);
    o.ends_only = 1;
    o.path_offsets = roll.path_offsets;
    o.end_truncated = st.out(truncated, (size_t)P);
    o.end_obs64 = st.out(final_obs, (size_t)P * obs_dim);
    o.end_head = st.out(final_head, (size_t)P * A);
    o.end_len = st.out(lengths, (size_t)P);
    o.end_rows = st.out(end_rows, (size_t)P);
    rollout_compact(o);
    st.fetch();
    HIPCHECK(hipStreamSynchronize(stream));
  }

  // the last rollout becomes the feed: `o` names the feed's action column, the rest is the same for both heads
  void rollout_to_feed(RolloutOut o, int64_t n_glob) {
    const int64_t N = roll_n;
    REQUIRE(N <= cap, "rollout has more steps than max_rows");
    REQUIRE(n_glob >= N, "n_global must be >= the rollout's steps");
    require_fisher_feed_ok(N, n_glob);
    use();
    feed_row0 = row0_next;
    o.X = X;
    o.ldx = wp[0];
    o.head = old;
    o.ld_head = wp[L];
    o.rewards = rewards;
    o.starts = starts;
    // the paths' end records, for trpo_get_tail_view
    o.path_offsets = roll.path_offsets;
    o.end_truncated = roll.cat_truncated;
    o.end_obs32 = roll.cat_obs32;
    o.end_head = roll.cat_dist;
    o.end_len = roll.cat_len;
    o.end_rows = roll.cat_rows;
    rollout_compact(o);
    if (roll_segment) {
      // the feed's step_index, and per path the episode's step count at s_T for the tail features' time entry
      if (!feed_step) feed_step = dalloc<int64_t>(cap);
      SegmentOut so{};
      so.step_index = feed_step;
      so.end_steps = roll.cat_steps;
      segment_compact(so);
    }
    if (gauss()) copy_in(logstd0, roll.logstd, (size_t)w[L] * sizeof(float), TRPO_MEM_DEVICE);
    n = N;
    n_global = n_glob;
    update_x_amax();
    feed_loaded();
    feed_is_rollout = true;
    feed_has_step = roll_segment;
    have_rewards = true;
    have_baseline = false;
    HIPCHECK(hipStreamSynchronize(stream));
  }

  void drop_fisher() {
    if (!fisher) return;
    fisher->release();
    delete fisher;
    fisher = nullptr;
  }

  void release() {
    if (device >= 0) (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    drop_fisher();
    for (auto& ev : ev_live) {
      (void)hipEventDestroy(ev.a);
      (void)hipEventDestroy(ev.b);
    }
    for (auto e : ev_pool) (void)hipEventDestroy(e);
    for (void* ptr : allocs) (void)hipFree(ptr);
    allocs.clear();
    for (void* ptr : roll.mem) (void)hipFree(ptr);
    roll.mem.clear();
    carry_free();
    drop_graph();
    free_har_slots();
    if (hsc) (void)hipHostFree(hsc);
    if (comm) (void)ncclCommDestroy(comm);
    if (stream && !owner) (void)hipStreamDestroy(stream);
    stream = nullptr;
  }

  // the split geometry of the launches that follow: S (FVP weight gradients) or S_pg (policy gradient)
  void use_splits(int s) {
    if (s == S_cur) return;
    S_cur = s;
    set_splits();
  }
  // the policy gradient's split geometry for one scope; the FVP's comes back on every exit, a throwing launch
  // included
  struct PgSplits {
    trpo_engine* e;
    explicit PgSplits(trpo_engine* en) : e(en) { e->use_splits(e->S_pg); }
    ~PgSplits() { e->use_splits(e->S); }
  };
  void set_splits() {
    const SplitGeom sg = split_geometry(n, S_cur);
    rows_per_split = sg.rows_per_split;
    active_splits = sg.active;
  }
  int active_splits = 1;
  // where the launches that follow write layer l's weight-gradient block, under the geometry above
  SlabDst slab_dst(int l) const { return SlabDst{active_splits, rows_per_split, slab, slab_stride, offW[l], offb[l]}; }

  void copy_in(void* dst, const void* src, size_t bytes, int mem) { trpo_abi::copy_in(dst, src, bytes, mem, stream); }
  void copy_out(void* dst, const void* src, size_t bytes, int mem) {
    if (bytes == 0) return;
    trpo_abi::copy_out(dst, src, bytes, mem, stream);
    har_pending = false;
    check_har();
  }

  // Host test transport, stream-ordered: D2H into a pinned slot, a host node that calls the
  // caller's all-reduce (e.g. gloo) on it, H2D back.  No host synchronisation, so it is captured
  // into the update hipGraph like an RCCL call.  Each call site owns its own slot (a replayed graph
  // keeps the pointers it captured); a callback failure is latched and raised at the next sync.
  struct HostArSlot {
    trpo_engine* e;
    void* host;
    size_t bytes;
    int64_t count;
    int dtype;
  };
  std::vector<HostArSlot*> har_slots;
  size_t har_next = 0;          // slot cursor, rewound by every update / standalone call
  int har_failed = 0;           // written by the host node, read after a stream sync
  static void host_ar_node(void* arg) {
    HostArSlot* s = static_cast<HostArSlot*>(arg);
    if (s->e->host_ar(s->host, s->count, s->dtype, s->e->host_ar_ctx) != 0) s->e->har_failed = 1;
  }
  // whose communicator, host callback and slots this engine's collectives use: a Fisher child's owner, so that the
  // slot order of the host transport has one owner and the child's captured all-reduces keep their slots
  trpo_engine* transport() { return owner ? owner : this; }
  const trpo_engine* transport() const { return owner ? owner : this; }
  HostArSlot* har_slot(size_t bytes, int64_t count, int dtype) {
    if (har_next == har_slots.size()) {
      auto* s = new HostArSlot{this, nullptr, 0, 0, 0};
      har_slots.push_back(s);
    }
    HostArSlot* s = har_slots[har_next++];
    if (s->bytes < bytes) {
      if (s->host) HIPCHECK(hipHostFree(s->host));
      s->host = nullptr;
      HIPCHECK(hipHostMalloc(&s->host, bytes, hipHostMallocDefault));
      s->bytes = bytes;
    }
    s->count = count;
    s->dtype = dtype;
    return s;
  }
  void free_har_slots() {
    for (HostArSlot* s : har_slots) {
      if (s->host) (void)hipHostFree(s->host);
      delete s;
    }
    har_slots.clear();
    har_next = 0;
  }
  void check_har() {
    if (har_failed) {
      har_failed = 0;
      throw std::runtime_error("host all-reduce callback failed");
    }
  }
  void host_allreduce(void* buf, size_t bytes, size_t count, int dtype) {
    trpo_engine* t = transport();   // (a child's stream is its owner's)
    HostArSlot* s = t->har_slot(bytes, (int64_t)count, dtype);
    HIPCHECK(hipMemcpyAsync(s->host, buf, bytes, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipLaunchHostFunc(stream, host_ar_node, s));
    HIPCHECK(hipMemcpyAsync(buf, s->host, bytes, hipMemcpyHostToDevice, stream));
    t->har_pending = true;
  }
  bool har_pending = false;     // a host node may still read its slot
  size_t har_graph_end = 0;     // slots [0, har_graph_end) belong to the captured update graph
  // every C-ABI entry: slots are reused from the first one the update graph does not own, once no
  // enqueued host node can still read them
  void rewind_har() {
    if (har_pending) {
      HIPCHECK(hipStreamSynchronize(stream));
      har_pending = false;
    }
    check_har();
    har_next = har_graph_end;
  }
  bool multi_rank() const {   // a Fisher child answers for its owner
    const trpo_engine* t = transport();
    return t->comm != nullptr || (t->host_ar && t->world > 1);
  }
  // RCCL when a communicator exists (any world size, world = 1 included: trpo_comm_init always
  // creates one), else the host transport for world > 1, else nothing to reduce
  void allreduce_f32(float* buf, size_t count) {
    if (!multi_rank()) return;
    Scope sp(this, "allreduce");
    ncclComm_t cm = transport()->comm;
    if (!cm) return host_allreduce(buf, count * sizeof(float), count, TRPO_F32);
    NCCLCHECK(ncclAllReduce(buf, buf, count, ncclFloat32, ncclSum, cm, stream));
  }
  void allreduce_f64(double* buf, size_t count) {
    if (!multi_rank()) return;
    ncclComm_t cm = transport()->comm;
    if (!cm) return host_allreduce(buf, count * sizeof(double), count, TRPO_F64);
    NCCLCHECK(ncclAllReduce(buf, buf, count, ncclFloat64, ncclSum, cm, stream));
  }

  // ------------------------------------------------------------------------
  PackArgs pack_args(const std::vector<float*>& wf, const std::vector<float*>* wb, int am_group = -1) {
    PackArgs pa{};
    pa.nl = L;
    if (am_group >= 0) am_reset(am(am_group, 0), L);
    for (int l = 0; l < L; ++l) {
      pa.L[l].amax = am_group >= 0 ? am(am_group, l) : nullptr;
      pa.L[l].off_w = offW[l];
      pa.L[l].a = w[l];
      pa.L[l].b = w[l + 1];
      pa.L[l].apad = wp[l];
      pa.L[l].bpad = wp[l + 1];
      pa.L[l].WF = wf[l];
      pa.L[l].WB = wb ? (*wb)[l] : nullptr;
    }
    return pa;
  }

  // ---- split-bf16 planes ----
  static int r16(int k) { return (k + 15) / 16 * 16; }
  size_t plane3_f(int l) const { return (size_t)wp[l + 1] * r16(wp[l]); }   // WF part: K = wp[l], N = wp[l+1]
  size_t plane3_b(int l) const { return (size_t)wp[l] * r16(wp[l + 1]); }   // WB part: K = wp[l+1], N = wp[l]
  // A set of packed forward weights: the [W;V] matrices, their planes and the running-max group of the W halves.
  // The current set serves theta (and the tangent in its V halves), the trial set the line search's vectors
  // (W halves only).
  struct WeightSet {
    const std::vector<float*>& wf;
    const std::vector<uint16_t*>& wf3;
    int am_group;
  };
  WeightSet cur_set() const { return WeightSet{WF, WF3, 0}; }
  WeightSet trial_set() const { return WeightSet{WFt, WFt3, 2}; }
  unsigned* am_w(const WeightSet& ws, int l) const { return am(ws.am_group, l); }
  enum Part { kW = 0, kV = 1 };   // the halves of a packed matrix
  SplitJob job_f(const WeightSet& ws, int l, int part) const {
    return SplitJob{ws.wf[l] + (size_t)part * wp[l] * wp[l + 1], ws.wf3[l] + part * 3 * plane3_f(l), wp[l], wp[l + 1],
                    wp[l + 1], r16(wp[l]), part ? am_v(l) : am_w(ws, l)};
  }
  SplitJob job_b(int l, int part) const {
    return SplitJob{WB[l] + (size_t)part * wp[l + 1] * wp[l], WB3[l] + part * 3 * plane3_b(l), wp[l + 1], wp[l],
                    wp[l], r16(wp[l + 1]), part ? am_v(l) : am_w(l)};
  }
  // Row-GEMM segments: A [n][K] (running max amaxA, NULL = bounded by 1) times a half of a packed matrix, with
  // that half's planes and running max.  Forward: layer l's W_l / V_l of `ws`, K = wp[l]; backward: W_l^T / V_l^T,
  // K = wp[l+1].
  GemmSeg fwd_seg(int l, Part part, const float* A, const unsigned* amaxA, const WeightSet& ws) const {
    GemmSeg sg{A, ws.wf[l] + (size_t)part * wp[l] * wp[l + 1], wp[l], wp[l + 1], wp[l]};
    sg.B3 = ws.wf3[l] + part * 3 * plane3_f(l);
    sg.ldk = r16(wp[l]);
    sg.plane = (int)plane3_f(l);
    sg.amaxA = amaxA;
    sg.amaxB = part ? am_v(l) : am_w(ws, l);
    return sg;
  }
  GemmSeg bwd_seg(int l, Part part, const float* A, const unsigned* amaxA) const {
    GemmSeg sg{A, WB[l] + (size_t)part * wp[l + 1] * wp[l], wp[l + 1], wp[l], wp[l + 1]};
    sg.B3 = WB3[l] + part * 3 * plane3_b(l);
    sg.ldk = r16(wp[l + 1]);
    sg.plane = (int)plane3_b(l);
    sg.amaxA = amaxA;
    sg.amaxB = part ? am_v(l) : am_w(l);
    return sg;
  }
  bool split_on() const { return g_options.split_mfma != 0; }
  // split the given packed-matrix parts; only layers whose GEMM takes the split path
  void split_parts(bool fwd_w, bool fwd_v, bool bwd_w, bool bwd_v, const WeightSet& ws, const int* skip,
                   const char* tag) {
    if (!split_on()) return;
    SplitArgs sa{};
    sa.f16 = f16;
    for (int l = 0; l < L; ++l) {
      const bool f = rowgemm_uses_split(wp[l + 1], RowEpi::kTanh);   // layer l's forward output
      const bool b = l >= 1 && rowgemm_uses_split(wp[l], RowEpi::kRBwd);   // backward into layer l's input
      if (f && fwd_w) sa.job[sa.n++] = job_f(ws, l, 0);
      if (f && fwd_v) sa.job[sa.n++] = job_f(ws, l, 1);
      if (b && bwd_w) sa.job[sa.n++] = job_b(l, 0);
      if (b && bwd_v) sa.job[sa.n++] = job_b(l, 1);
      if (sa.n > kMaxSplitJobs - 4 || (l == L - 1 && sa.n)) {
        Scope sp(this, tag);
        launch_split_b(sa, skip, stream);
        sa.n = 0;
      }
    }
    check_launch();
  }
  void ensure_w3() {
    if (split_on() && !cache.w3_valid) {
      split_parts(true, false, true, false, cur_set(), nullptr, "split_w");
      cache.w3_valid = true;
    }
  }

  RowGemmArgs row_args(int l_out_width, int l_out_pad) {
    RowGemmArgs a{};
    a.f16 = f16;
    a.M = (int)n;
    a.N = l_out_width;
    a.Npad = l_out_pad;
    return a;
  }

  // forward through layers 0..L-1 with the weights of `ws` (W halves); the head
  // epilogue is `head`; hidden activations go to `hout`
  void forward(const WeightSet& ws, const float* th, const std::vector<float*>& hout, RowEpi head, const char* tag) {
    int l_first = 0;
    const bool prep = head == RowEpi::kPrepHead || head == RowEpi::kGaussPrepHead;
    if (use_fwd01()) {   // layers 0 and 1 in one launch; H1 stored by the prepare pass only (the FVP reads it)
      {
        Scope sp(this, tag, "_img");
        launch_fwd01_img(th, offW[0], offW[1], w[0], am_w(ws, 0), am_w(ws, 1), fw_img, stream);
        check_launch();
      }
      Fwd01Args fa{};
      fa.n = n;
      fa.obs = w[0];
      fa.Xh = Xh;
      fa.Xl = Xl;
      fa.x_mpad = x_mpad;
      fa.eX = pl_e;
      fa.b0 = th + offb[0];
      fa.b1 = th + offb[1];
      fa.H1 = prep ? hout[1] : nullptr;
      fa.H2 = hout[2];
      fa.img = fw_img;
      fa.am_w0 = am_w(ws, 0);
      fa.am_w1 = am_w(ws, 1);
      Scope sp(this, tag, "_l01");
      launch_fwd01(fa, num_cus, stream);
      check_launch();
      l_first = 2;
    }
    for (int l = l_first; l < L; ++l) {
      RowGemmArgs a = row_args(w[l + 1], wp[l + 1]);
      a.nseg = 1;
      // hidden activations are tanh outputs, |h| <= 1
      a.seg[0] = fwd_seg(l, kW, l == 0 ? X : hout[l], l == 0 ? am_x() : nullptr, ws);
      if (l == 0 && planes_l0()) attach_x_planes(a.seg[0], W0b);
      // head_fwd 1 (default): the prepare and the loss heads (the prepare outputs leave through LDS as coalesced
      // rows: C4 3.6 -> 3.1 ms); 2: the loss heads, and the prepare head for <= 8 actions
      const int hfo = g_options.head_fwd;
      const bool prep_hf = hfo == 1 || (hfo == 2 && w[L] <= 8);
      if (l == L - 1 && !gauss() && (hfo == 1 || hfo == 2) && head_fwd_eligible(w[L], w[L - 1]) &&
          ((head == RowEpi::kPrepHead && prep_hf) || head == RowEpi::kLossHead)) {
        // the softmax head with one state per lane (hbwd.hip): bound by its read of H_{L-1}
        HeadFwdArgs hf{};
        hf.rows = n;
        hf.A = w[L];
        hf.Apad = wp[L];
        hf.K = w[l];
        hf.Kpad = wp[l];
        hf.H = l == 0 ? X : hout[l];
        hf.W = ws.wf[l];
        hf.bias = th + offb[l];
        hf.old = old;
        hf.act = act;
        hf.adv = adv32;
        hf.rowterms = rowterms;
        hf.invN = 1.0 / (double)n_global;
        if (head == RowEpi::kPrepHead) {
          hf.prep = 1;
          hf.P = Pm;
          hf.D = D[L - 1];
          hf.DS = DSL;
          hf.am_d = am_d(L - 1);
          hf.am_ds = am_ds(L - 1);
        }
        Scope sp(this, tag, l);
        launch_head_fwd(hf, num_cus, stream);
        check_launch();
        continue;
      }
      a.ea.bias = th + offb[l];
      a.ea.ldo = wp[l + 1];
      if (l < L - 1) {
        a.epi = RowEpi::kTanh;
        a.ea.out0 = hout[l + 1];
      } else {
        a.epi = head;
        a.ea.out0 = Pm;
        a.ea.out1 = D[L - 1];
        a.ea.out2 = DSL;
        a.ea.old = old;
        a.ea.act = act;
        a.ea.adv = adv32;
        a.ea.rowterms = rowterms;
        a.ea.invN = 1.0 / (double)n_global;
        if (head == RowEpi::kPrepHead) {
          a.ea.amax1 = am_d(L - 1);
          a.ea.amax2 = am_ds(L - 1);
        }
        if (gauss()) {   // out1 (D_{L-1}'s buffer, free here) takes the rows of g's log-std block
          a.ea.actf = actf;
          a.ea.logstd = logstd_of(th);
          a.ea.logstd0 = logstd0;
          if (prep) a.ea.amax2 = am_ds(L - 1);
        }
      }
      Scope sp(this, tag, l);
      launch_rowgemm(a, stream);
      check_launch();
    }
  }

  // rowterms -> [surr, kl, ent] into sc->loss_before (which=0) or loss_trial (which=1)
  void reduce_losses(int which, const int* skip) {
    launch_rowterms_partials(rowterms, n, part3, skip, stream);
    launch_rowterms_finish(part3, local3, skip, stream);
    allreduce_f64(local3, 3);
    launch_losses_store(local3, 1.0 / (double)n_global, loss_sc, which, skip, stream);
    check_launch();
  }

  void require_batch() { REQUIRE(n > 0, "no batch: call trpo_set_batch first"); }

  // a caller's [n][width] f32 rows of the feed -> dst [n][ldp] (padding columns stay zero)
  void stage_rows(const float* src, int width, int ldp, float* dst, int mem) {
    if (width == ldp) {
      copy_in(dst, src, (size_t)n * width * sizeof(float), mem);
      return;
    }
    // (a stream-ordered hipMallocAsync temporary here lost the pageable host copy on its first
    // use in the VF runtime; persistent staging avoids the pattern)
    const float* s = src;
    if (mem != TRPO_MEM_DEVICE) {
      copy_in(stage, src, (size_t)n * width * sizeof(float), mem);
      s = stage;
    }
    launch_copy_rows(s, n, width, width, dst, ldp, stream);
    check_launch();
    HIPCHECK(hipStreamSynchronize(stream));
  }
  // the prepare head's first output (the softmax, or the Gaussian mean) of the feed's rows -> out [n][A]
  void fetch_head_rows(float* out, int mem) {
    const int A = w[L];
    float* dst = mem == TRPO_MEM_DEVICE ? out : stage;
    launch_copy_rows(Pm, n, A, wp[L], dst, A, stream);
    check_launch();
    if (mem != TRPO_MEM_DEVICE) copy_out(out, stage, (size_t)n * A * sizeof(float), mem);
    HIPCHECK(hipStreamSynchronize(stream));
  }
  // a new feed is in place: the split geometry follows its rows, nothing derived from the old feed survives
  void feed_loaded() {
    set_splits();
    cache.batch_changed();
    have_rewards = false;
    have_tail = false;
    feed_is_rollout = false;
    feed_has_step = false;
  }

  void update_x_amax() {
    if (!f16) return;
    am_reset(am_x(), 1);
    launch_amax(X, n, w[0], wp[0], am_x(), stream);
    x_planes = false;
    if (Xh && g_options.planes != 0 && n > 0) {
      x_mpad = (int)((n + 255) / 256 * 256);
      Scope sp(this, "split_x");
      launch_split_planes(X, (int)n, x_mpad, w[0], wp[0], Xh, Xl, x_ldp, am_x(), pl_e, stream);
      x_planes = true;
    }
    check_launch();
  }

  // ---- Fisher subsampling ----
  static int64_t sub_rows(int64_t rows, int64_t k) { return (rows + k - 1) / k; }
  // the global mode's first Fisher row of a feed that starts at global row `first`, and its Fisher rows
  static int64_t phase_of(int64_t first, int64_t k) { return (k - first % k) % k; }
  int64_t fisher_phase() const { return fvp_global ? phase_of(feed_row0, fvp_stride) : 0; }
  int64_t fisher_rows() const { return sub_rows(n - fisher_phase(), fvp_stride); }
  // the global mode: the shard lies inside the global batch and holds a Fisher row (an engine needs n > 0, the child
  // included)
  void require_global_feed_ok(int64_t rows, int64_t rows_global, int64_t first, int64_t k) const {
    if (first + rows > rows_global)
      throw std::runtime_error("fvp_subsample (global rows): row offset " + std::to_string(first) + " + n = " +
                               std::to_string(rows) + " exceeds n_global = " + std::to_string(rows_global));
    if (rows <= phase_of(first, k))
      throw std::runtime_error("fvp_subsample (global rows): the shard [" + std::to_string(first) + ", " +
                               std::to_string(first + rows) + ") holds no multiple of the stride " + std::to_string(k) +
                               ": a rank without a Fisher row is not supported");
  }
  // local mode, single-process only: the 1/N of a subsampled Fisher matrix over ranks would be sum_r ceil(n_r / k)
  void require_fisher_feed_ok(int64_t rows, int64_t rows_global) const {
    if (fvp_global) return require_global_feed_ok(rows, rows_global, row0_next, fvp_stride);
    if (fvp_stride > 1 && rows_global != rows)
      throw std::runtime_error("fvp_subsample = " + std::to_string(fvp_stride) + " needs n_global == n (got n = " +
                               std::to_string(rows) + ", n_global = " + std::to_string(rows_global) +
                               "): multi-rank subsampling is not supported");
  }
  void require_single_rank_for_fisher(const char* call) const {
    if (fvp_stride > 1 && !fvp_global)
      throw std::runtime_error(std::string(call) + ": the engine has fvp_subsample = " + std::to_string(fvp_stride) +
                               ", which is single-process (set it back to 1 first)");
  }
  void set_fvp_subsample(int64_t k, bool global) {
    REQUIRE(!owner, "a Fisher sub-engine takes no stride of its own");
    if (k < 1) throw std::runtime_error("fvp_subsample: the stride must be >= 1, got " + std::to_string(k));
    if (k == 1) global = false;   // one mode at k = 1: every row
    if (!global) {
      if (k > 1 && (comm || host_ar))
        throw std::runtime_error(
            "fvp_subsample > 1 is single-process: this engine has a communicator or a host all-reduce transport");
      if (k > 1 && n > 0 && n_global != n)
        throw std::runtime_error("fvp_subsample > 1 needs n_global == n: the current feed has n = " +
                                 std::to_string(n) + ", n_global = " + std::to_string(n_global));
    } else if (n > 0) {
      require_global_feed_ok(n, n_global, feed_row0, k);
    }
    if (k == fvp_stride && global == fvp_global) return;
    use();
    drop_graph();
    HIPCHECK(hipStreamSynchronize(stream));   // nothing enqueued still reads the old child's buffers
    drop_fisher();
    fvp_stride = 1;
    fvp_global = false;
    cache.fisher_fed = cache.fisher_theta = false;
    if (k == 1) return;
    auto c = std::make_unique<trpo_engine>();
    try {
      c->init(dist, w[0], w.data() + 1, L - 1, w[L], sub_rows(cap, k), device, this);
    } catch (...) {
      c->release();
      throw;
    }
    c->prof = prof;
    fisher = c.release();
    fvp_stride = k;
    fvp_global = global;
  }
  // rows phase, phase + k, phase + 2k, ... of the feed into the child (phase = 0 in the local mode), one launch on the
  // engine stream (capturable), then what a feed load runs after staging
  void gather_fisher_feed() {
    trpo_engine* c = fisher;
    const int64_t ns = fisher_rows();
    GatherArgs ga{};
    auto wide = [&](const float* src, float* dst, int ld) { ga.wide[ga.nwide++] = GatherWide{src, dst, ld / 4, 0}; };
    wide(X, c->X, wp[0]);
    wide(old, c->old, wp[L]);
    if (gauss()) wide(actf, c->actf, wp[L]);
    else ga.scalar[ga.nscalar++] = GatherScalar{act, c->act};
    ga.scalar[ga.nscalar++] = GatherScalar{adv32, c->adv32};
    ga.n_sub = ns;
    ga.stride = fvp_stride;
    ga.first = fisher_phase();
    if (gauss()) {
      ga.whole_src = logstd0;
      ga.whole_dst = c->logstd0;
      ga.whole_n = w[L];
    }
    {
      Scope sp(this, "fisher_gather");
      launch_gather_feed(ga, num_cus, stream);
      check_launch();
    }
    c->n = ns;
    c->n_global = fvp_global ? sub_rows(n_global, fvp_stride) : ns;
    c->update_x_amax();
    c->feed_loaded();
    cache.fisher_fed = true;
  }
  // the engine that serves the Fisher-vector products: this one, or the child with the current feed and theta
  trpo_engine* fisher_ready() {
    if (!fisher) return this;
    require_batch();
    if (!cache.fisher_fed) gather_fisher_feed();
    if (!cache.fisher_theta) {
      fisher->cache.theta_changed();
      cache.fisher_theta = true;
    }
    return fisher;
  }

  // policy forward + KL_ff plain backward at theta (cached over CG)
  void prepare() {
    require_batch();
    if (cache.prepared) return;
    PackArgs pa = pack_args(WF, &WB, 0);
    launch_pack(pa, theta, 0, nullptr, stream);
    // Only what the FVP path will read is written below (prep_e_top records it; fvp() re-prepares if the
    // path changes)
    cache.prepare_begins(e_top_needed(), use_fused16());
    ensure_w3();
    if (gauss()) {
      // the forward and the prepare head only: at theta = theta_old KL_ff's plain backward is exactly zero
      // (D_l = 0, E_l = 0), so nothing below the head is written and the FVP drops those terms
      am_reset(am_ds(L - 1), 1);
      forward(cur_set(), theta, H, RowEpi::kGaussPrepHead, "fwd");
      reduce_losses(0, nullptr);
      cache.prepared = true;
      return;
    }
    am_reset(am_d(0), L);
    am_reset(am_ds(L - 1), 1);
    if (use_fused16() && g_options.ls_fused == 1) fused16_forward(theta, true);   // fwd_loss16's prepare form
    else forward(cur_set(), theta, H, RowEpi::kPrepHead, "fwd");
    // KL_ff plain backward: DH_l = D_l W_l^T ; D_{l-1} = DH (1-H^2) ; E_{l-1} = -2 DH H.
    // D_0 is never written (the R-backward stops at RD_0), E_{L-2} not under the fused tail, which
    // recomputes it from H and D_{L-1}.
    const bool prep_e_top = cache.prep_e_top, hb2 = use_hbwd2();
    if (use_fused16()) {
      // D_1, E_1, E_0 and the policy gradient's slabs in one launch on the f16 weight images (fused16.hip)
      fused16_w_images();
      Fused16Args fa = fused16_args(nullptr, nullptr, cache.pg_grid);
      fa.D1out = L == 3 ? D[1] : nullptr;   // one hidden layer: E_0 only (D_1 is the head's delta)
      fa.E1out = L == 3 ? E[1] : nullptr;
      fa.E0out = E[0];
      fa.am_d1_out = L == 3 ? am_d(1) : nullptr;
      {
        Scope sp(this, "bwd_pg");
        launch_prep_pg_fused16(fa, cache.pg_grid, stream);
        check_launch();
      }
      cache.pg_ready = true;
      reduce_losses(0, nullptr);
      cache.prepared = true;
      return;
    }
    for (int l = L - 1; l >= 1; --l) {
      const bool need_d = l > 1, need_e = l < L - 1 || prep_e_top;
      if (!need_d && !need_e) continue;
      if (l == L - 1 && hb2) {
        // D_{L-2} and the policy gradient's DS_{L-2} in one read of H_{L-1} (hbwd.hip), with D_1's hi plane for
        // the fused R-backward where it runs (two hidden layers), scaled per 32-row tile
        am_reset(am_ds(L - 2), 1);
        HeadBwd2Args hb{};
        hb.rows = (int)n;
        hb.A = w[L];
        hb.Apad = wp[L];
        hb.N = w[L - 1];
        hb.Npad = wp[L - 1];
        hb.WB = WB[L - 1];
        hb.D2 = D[L - 1];
        hb.DS2 = DSL;
        hb.H = H[L - 1];
        hb.D1 = D[L - 2];
        hb.DS1 = RD[L - 2];
        hb.E1 = prep_e_top ? E[L - 2] : nullptr;
        hb.am_d1 = am_d(L - 2);
        hb.am_ds1 = am_ds(L - 2);
        PgSplits pgs(this);   // the slab block it writes is reduced with the policy gradient's
        hb.dst = slab_dst(L - 1);   // the policy gradient's W_{L-1} / b_{L-1} block, reduced by policy_grad()
        if (L == 3 && D1h && eD1t && use_rbwd0() && wp[2] % 32 == 0 && n > 0) {
          cache.d1_mpad = (int)((n + 255) / 256 * 256);
          hb.D1h = D1h;
          hb.d1_mpad = cache.d1_mpad;
          hb.eD1t = eD1t;
        }
        Scope sp(this, "bwd2_l2");
        launch_head_bwd2(hb, num_cus, stream);
        check_launch();
        cache.ds_ready = true;
        cache.d1_plane = cache.d1_tiled = hb.D1h != nullptr;
        continue;
      }
      RowGemmArgs a = row_args(w[l], wp[l]);
      a.nseg = 1;
      a.seg[0] = bwd_seg(l, kW, D[l], am_d(l));
      // both: kPrepBwd ; E only (D_0): kPrepBwdE ; D only: kPgBwd, whose epilogue is DH (1-H^2)
      a.epi = need_d ? (need_e ? RowEpi::kPrepBwd : RowEpi::kPgBwd) : RowEpi::kPrepBwdE;
      a.ea.H = H[l];
      a.ea.out0 = need_d ? D[l - 1] : E[l - 1];
      a.ea.amax0 = need_d ? am_d(l - 1) : nullptr;
      a.ea.out1 = need_d && need_e ? E[l - 1] : nullptr;
      a.ea.ldo = wp[l];
      Scope sp(this, "bwd", l);
      launch_rowgemm(a, stream);
      check_launch();
    }
    // D_1's hi plane for the fused R-backward (per update; the FVPs' D_1 V_1^T segment reads half the bytes)
    if (!cache.d1_plane && D1h && use_rbwd0() && n > 0) {
      cache.d1_mpad = (int)((n + 255) / 256 * 256);
      Scope sp(this, "split_d1");
      launch_split_planes(D[1], (int)n, cache.d1_mpad, wp[2], wp[2], D1h, nullptr, d1_ldp, am_d(1), pl_e + 1, stream);
      check_launch();
      cache.d1_plane = true;
    }
    reduce_losses(0, nullptr);
    cache.prepared = true;
  }

  // sum over splits -> out (local partial) ; all-reduce
  // Gaussian engine: the log-std block of `out` (no launch writes it into the slabs) as this rank's partial, from the
  // tangent's block (Hv_s = 2 v_s n / N) or, v_tail = NULL, from the prepare head's rows (g_s)
  void reduce_grad(float* out, const int* skip, int slabs = 0, const float* v_tail = nullptr) {
    {
      Scope sp(this, "reduce");
      launch_reduce_slab(slab, slabs > 0 ? slabs : active_splits, slab_stride, P, out, skip, stream);
      check_launch();
    }
    if (gauss()) {
      Scope sp(this, "logstd_block");
      const int A = w[L];
      float* tail = out + (P - A);
      if (v_tail) {
        launch_gauss_scale_tail(v_tail, A, 2.0 * (double)n / (double)n_global, tail, skip, stream);
      } else {
        const int blocks = launch_gauss_colsum_partials(D[L - 1], n, A, wp[L], gs_part, stream);
        launch_gauss_colsum_finish(gs_part, blocks, A, -1.0 / (double)n_global, tail, skip, stream);
      }
      check_launch();
    }
    allreduce_f32(out, (size_t)P);
  }

  // layer l's weight-gradient block into the slabs, profiled as "<tag>_l<l>"
  void wgrad_layer(int l, int nseg, WSeg s0, WSeg s1, int colsum_seg, const int* skip, const char* tag) {
    WGradArgs a{};
    a.rows = (int)n;
    a.Ma = w[l];
    a.Nb = w[l + 1];
    a.Mpad = wp[l];
    a.Npad = wp[l + 1];
    a.nseg = nseg;
    a.seg[0] = s0;
    a.seg[1] = s1;
    a.colsum_seg = colsum_seg;
    a.dst = slab_dst(l);
    a.skip = skip;
    a.f16 = f16;
    Scope sp(this, tag, l);
    launch_wgrad(a, stream);
    check_launch();
  }
  // the FVP's weight gradients of layers [l0, l1): (Hv)_W_l = RH_l^T D_l + H_l^T RD_l ; (Hv)_b_l = colsum RD_l
  // (rh1p: this FVP's rfwd01 left RH1 as planes)
  void fvp_wgrads(int l0, int l1, const int* skip, bool rh1p = false) {
    for (int l = l0; l < l1; ++l) {
      if (l == 0) {
        wgrad_layer(0, 1, WSeg{X, RD[0], wp[0], wp[1], am_x(), am_rd(0)}, WSeg{}, 0, skip, "fvp_wgrad");
      } else {
        WSeg s0{RH[l], D[l], wp[l], wp[l + 1], am_rh(l), am_d(l)};
        if (l == 1 && rh1p) s0.Ap = rh1_planes();
        wgrad_layer(l, 2, s0, WSeg{H[l], RD[l], wp[l], wp[l + 1], nullptr, am_rd(l)}, 1, skip, "fvp_wgrad");
      }
    }
  }

  // flatgrad(surr) (trpo_inksci.py:54) -> g (all ranks)
  void policy_grad() {
    reprepare_if_path_changed();
    prepare();
    if (use_fused16()) {
      if (!cache.pg_ready) pg_fused16();
      reduce_grad(g, nullptr, cache.pg_grid);
      return;
    }
    ensure_w3();
    PgSplits pgs(this);
    cache.slabs_written(/*keeps_pg_head=*/true);   // the layers below the head's write their blocks
    // surr backward: DS_{l-1} = (DS_l W_l^T)(1-H_l^2) ; DS of hidden layers lives in RD scratch
    std::vector<float*> DS(L);
    DS[L - 1] = DSL;
    for (int l = 0; l < L - 1; ++l) DS[l] = RD[l];
    const bool have_ds = cache.ds_ready;   // DS_{L-2} (and its running max) from the prepare pass (hbwd.hip)
    am_reset(am_ds(0), have_ds ? L - 2 : L - 1);
    const bool r0f = use_rbwd0();
    for (int l = have_ds ? L - 2 : L - 1; l >= 1; --l) {
      if (l == 1 && r0f) {
        // DS_0 stays in registers: X^T DS_0 and its column sums go straight to the slab (rbwd0.hip)
        RBwd0Args a = rbwd0_args(nullptr);
        a.nseg = 1;
        a.A0 = DS[1];
        a.am_a0 = am_ds(1);
        Scope sp(this, "pg_bwdwg_l1");
        launch_rbwd0(a, stream);
        check_launch();
        continue;
      }
      RowGemmArgs a = row_args(w[l], wp[l]);
      a.nseg = 1;
      a.seg[0] = bwd_seg(l, kW, DS[l], am_ds(l));
      a.epi = RowEpi::kPgBwd;
      a.ea.H = H[l];
      a.ea.out0 = DS[l - 1];
      a.ea.amax0 = am_ds(l - 1);
      a.ea.ldo = wp[l];
      Scope sp(this, "pg_bwd", l);
      launch_rowgemm(a, stream);
      check_launch();
    }
    // with DS_{L-2} from the prepare pass the head layer's weight gradient is already in the slabs
    for (int l = r0f ? 1 : 0; l < (have_ds ? L - 1 : L); ++l)
      wgrad_layer(l, 1, WSeg{act_in(l), DS[l], wp[l], wp[l + 1], l == 0 ? am_x() : nullptr, am_ds(l)}, WSeg{}, 0,
                  nullptr, "pg_wgrad");
    reduce_grad(g, nullptr);
  }

  // Hv (undamped, all ranks) for device vector v -> out ; no-op when *skip
  // defer (single rank, the one-launch FVP): the slab reduction is left to the caller (the CG iteration fuses it),
  // *defer receives the slab count; 0 when this FVP reduced into out itself
  void fvp(const float* v, float* out, const int* skip, int* defer = nullptr) {
    if (defer) *defer = 0;
    // the path changed since prepare(): E_{L-2} needed but not written, or the other side of the fused16 switch
    reprepare_if_path_changed();
    prepare();
    cache.rd_written();      // the FVP's R-backward writes RD (DS_{L-2}'s scratch)
    cache.slabs_written();   // ... and every FVP path the slabs
    if (use_fused16()) {
      fvp_fused16(v, out, skip, defer && !multi_rank() && cg_fused_reduce_ok(P) ? defer : nullptr);
      return;
    }
    if (use_fused()) {
      fvp_fused(v, out, skip);
      return;
    }
    if (use_chain()) {
      fvp_chain(v, out, skip);
      return;
    }
    {
      PackArgs pa = pack_args(WF, &WB, 1);
      launch_pack(pa, v, 1, skip, stream);
      check_launch();
    }
    ensure_w3();
    // Gaussian engine: D_l = E_l = 0, so the R-backward is the policy gradient's (RD_l W_l^T alone: no V^T planes)
    // and each weight gradient one segment, H_l^T RD_l
    const bool gs = gauss();
    split_parts(false, true, false, !gs, cur_set(), skip, "split_v");
    am_reset(am_rh(0), L);
    am_reset(am_rd(0), L);
    // R-forward (the fused tail takes the last layer's)
    const bool tail = use_tail();
    const int Lf = tail ? L - 1 : L;
    int l_first = 0;
    const bool rh1p = use_rh1_planes();
    if (use_rfwd01()) {   // layers 0 and 1 in one launch (rfwd.hip): RH1 and the tail's RZ2
      {
        Scope sp(this, "fvp_rfwd_img");
        launch_rfwd01_img(theta, v, offW[0], offW[1], w[0], am_v(0), am_w(1), am_v(1), rf_img, skip, stream);
        check_launch();
      }
      Rfwd01Args ra{};
      ra.n = n;
      ra.obs = w[0];
      ra.ldh = wp[1];
      ra.ldz = wp[2];
      ra.Xh = Xh;
      ra.Xl = Xl;
      ra.x_mpad = x_mpad;
      ra.eX = pl_e;
      ra.H1 = H[1];
      ra.c0 = v + offb[0];
      ra.c1 = v + offb[1];
      ra.V0 = v + offW[0];
      ra.RH1 = RH[1];
      ra.RZ2 = RH[2];
      ra.img = rf_img;
      ra.am_v0 = am_v(0);
      ra.am_w1 = am_w(1);
      ra.am_v1 = am_v(1);
      ra.am_rh1 = am_rh(1);
      ra.am_rz2 = am_rh(2);
      if (rh1p) ra.e_rh1 = pl_e + 2;
      ra.skip = skip;
      Scope sp(this, "fvp_rfwd01");
      launch_rfwd01(ra, num_cus, stream);
      check_launch();
      l_first = 2;
    }
    for (int l = l_first; l < Lf; ++l) {
      RowGemmArgs a = row_args(w[l + 1], wp[l + 1]);
      if (l == 0) {
        a.nseg = 1;
        a.seg[0] = fwd_seg(0, kV, X, am_x(), cur_set());
        if (planes_l0()) attach_x_planes(a.seg[0], V0b);
      } else {
        a.nseg = 2;
        a.seg[0] = fwd_seg(l, kW, RH[l], am_rh(l), cur_set());
        a.seg[1] = fwd_seg(l, kV, H[l], nullptr, cur_set());
      }
      a.skip = skip;
      a.ea.bias = v + offb[l];
      a.ea.ldo = wp[l + 1];
      if (l < L - 1) {
        // the fused tail is the only reader of RH_{L-1}: it gets the pre-activation and applies (1-H^2)
        // itself, so H_{L-1} is read once per FVP instead of twice (its max bounds max |RH_{L-1}|)
        a.epi = (tail && l == L - 2) ? RowEpi::kRZ : RowEpi::kRHidden;
        a.ea.H = H[l + 1];
        a.ea.out0 = RH[l + 1];
        a.ea.amax0 = am_rh(l + 1);
      } else {
        a.epi = gs ? RowEpi::kGaussRHead : RowEpi::kRHead;
        a.ea.P = Pm;
        a.ea.logstd = gs ? logstd_of(theta) : nullptr;
        a.ea.out0 = RD[L - 1];
        a.ea.amax0 = am_rd(L - 1);
        a.ea.invN = 1.0 / (double)n_global;
      }
      Scope sp(this, "fvp_rfwd", l);
      launch_rowgemm(a, stream);
      check_launch();
    }
    if (tail) {
      const int l = L - 1;
      TailPackArgs tp{};
      tp.theta = theta;
      tp.v = v;
      tp.off_w = offW[l];
      tp.a = w[l];
      tp.b = w[l + 1];
      tp.am_w = am_w(l);
      tp.am_v = am_v(l);
      tp.out = tail_planes;
      TailArgs ta{};
      ta.rows = (int)n;
      ta.a = w[l];
      ta.b = w[l + 1];
      ta.apad = wp[l];
      ta.bpad = wp[l + 1];
      ta.RH = RH[l];
      ta.rz = 1;
      ta.H = H[l];
      ta.P = Pm;
      ta.DL = D[l];
      ta.c = v + offb[l];
      ta.WV16 = tail_planes;
      ta.WT16 = WB3[l];
      ta.VT16 = WB3[l] + 3 * plane3_b(l);
      ta.bplane = (int64_t)plane3_b(l);
      ta.am_rh = am_rh(l);
      ta.am_d = am_d(l);
      ta.am_w = am_w(l);
      ta.am_v = am_v(l);
      ta.am_out = am_rd(l - 1);
      ta.RDout = RD[l - 1];
      ta.invN = 1.0 / (double)n_global;
      ta.dst = slab_dst(l);
      ta.skip = skip;
      Scope sp(this, "fvp_tail", l);
      launch_tail_pack(tp, stream);
      launch_fvp_tail(ta, stream);
      check_launch();
    }
    // layer 1's R-backward fused with layer 0's weight gradient when layer 1 is not inside the tail
    const bool r0f = use_rbwd0() && Lf - 1 >= 1;
    // R-backward: RDH_l = RD_l W_l^T + D_l V_l^T ; RD_{l-1} = RDH (1-H_l^2) + E_{l-1} RH_l
    for (int l = Lf - 1; l >= 1; --l) {
      if (l == 1 && r0f && gs) {
        RBwd0Args a = rbwd0_args(skip);   // the nseg = 1 form: RD_0 = (RD_1 W_1^T)(1 - H_1^2), X^T RD_0 to the slab
        a.nseg = 1;
        a.A0 = RD[1];
        a.am_a0 = am_rd(1);
        Scope sp(this, "fvp_rbwdwg_l1");
        launch_rbwd0(a, stream);
        check_launch();
        continue;
      }
      if (gs) {
        RowGemmArgs a = row_args(w[l], wp[l]);
        a.nseg = 1;
        a.seg[0] = bwd_seg(l, kW, RD[l], am_rd(l));
        a.skip = skip;
        a.epi = RowEpi::kPgBwd;
        a.ea.H = H[l];
        a.ea.out0 = RD[l - 1];
        a.ea.amax0 = am_rd(l - 1);
        a.ea.ldo = wp[l];
        Scope sp(this, "fvp_rbwd", l);
        launch_rowgemm(a, stream);
        check_launch();
        continue;
      }
      if (l == 1 && r0f) {
        RBwd0Args a = rbwd0_args(skip);
        a.nseg = 2;
        a.A0 = RD[1];
        a.A1 = D[1];
        if (cache.d1_plane) {
          a.A1h = D1h;
          a.a1_mpad = cache.d1_mpad;
          a.eA1p = pl_e + 1;
          if (cache.d1_tiled) a.eA1t = eD1t;
        }
        a.am_a0 = am_rd(1);
        a.am_a1 = am_d(1);
        a.E = E[0];
        a.RH = RH[1];
        if (rh1p) a.RHp = rh1_planes();
        Scope sp(this, "fvp_rbwdwg_l1");
        launch_rbwd0(a, stream);
        check_launch();
        continue;
      }
      RowGemmArgs a = row_args(w[l], wp[l]);
      a.nseg = 2;
      a.seg[0] = bwd_seg(l, kW, RD[l], am_rd(l));
      a.seg[1] = bwd_seg(l, kV, D[l], am_d(l));
      a.skip = skip;
      a.epi = RowEpi::kRBwd;
      a.ea.H = H[l];
      a.ea.E = E[l - 1];
      a.ea.RH = RH[l];
      a.ea.out0 = RD[l - 1];
      a.ea.amax0 = am_rd(l - 1);
      a.ea.ldo = wp[l];
      Scope sp(this, "fvp_rbwd", l);
      launch_rowgemm(a, stream);
      check_launch();
    }
    if (gs) {
      for (int l = r0f ? 1 : 0; l < L; ++l)
        wgrad_layer(l, 1, WSeg{act_in(l), RD[l], wp[l], wp[l + 1], l == 0 ? am_x() : nullptr, am_rd(l)}, WSeg{}, 0, skip,
                    "fvp_wgrad");
      reduce_grad(out, skip, 0, v + (P - w[L]));
      return;
    }
    fvp_wgrads(r0f ? 1 : 0, Lf, skip, rh1p);
    reduce_grad(out, skip);
  }

  ChainArgs chain_args(const ImageSet& is, const float* v, const int* skip) const {
    ChainArgs ca{};
    ca.n = (int)n;
    ca.L = L;
    for (int l = 0; l <= L; ++l) {
      ca.w[l] = w[l];
      ca.ld[l] = wp[l];
    }
    ca.X = X;
    for (int l = 0; l < L; ++l) {
      ca.H[l] = H[l];
      ca.RH[l] = RH[l];
      ca.D[l] = D[l];
      ca.E[l] = E[l];
      ca.RD[l] = RD[l];
      ca.offb[l] = offb[l];
    }
    ca.P = Pm;
    ca.v = v;
    ca.img = is.img;
    ca.tab = is.tab;
    ca.nchunks = is.nchunks;
    ca.invN = 1.0 / (double)n_global;
    ca.skip = skip;
    return ca;
  }
  // the chain images of theta (when stale) and of the tangent v
  void chain_w_images(const float* v) {
    if (cache.chain_w_valid) return;
    Scope sp(this, "fvp_img_w");
    launch_chain_img(chain_set.jobs, theta, v, 0, nullptr, stream);
    check_launch();
    cache.chain_w_valid = true;
  }
  void chain_images(const float* v, const int* skip) {
    chain_w_images(v);
    Scope sp(this, "fvp_img_v");
    launch_chain_img(chain_set.jobs, theta, v, 1, skip, stream);
    check_launch();
  }

  // the whole Hv in one launch (fused.hip) + the slab reduction
  void fvp_fused(const float* v, float* out, const int* skip) {
    chain_images(v, skip);
    const int variant = g_options.fused == 1 ? 1 : 2;   // 3 (f16) where fused16.hip does not apply: 4 waves
    const int rb = fused_fvp_states_per_group(variant);
    FusedArgs fa{};
    fa.c = chain_args(chain_set, v, skip);
    fa.slab = slab;
    fa.slab_stride = slab_stride;
    for (int l = 0; l < L; ++l) fa.offW[l] = offW[l];
    fa.ngroups = (int)((n + rb - 1) / rb);
    // one persistent workgroup per CU (8 waves) or two (4 waves), at most one per slab
    const int per_cu = variant == 2 ? 2 : 1;
    const int grid =
        (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)fa.ngroups, (int64_t)S, (int64_t)num_cus * per_cu}));
    {
      Scope sp(this, "fvp_fused");
      launch_fvp_fused(fa, grid, variant, stream);
      check_launch();
    }
    reduce_grad(out, skip, grid);
  }

  // fused16.hip's arguments for the tangent v (the FVP) or none (the policy gradient), and its grid: persistent
  // workgroups, at most one per slab, as few as take the same number of group rounds (fewer slabs to reduce)
  Fused16Args fused16_args(const float* v, const int* skip, int& grid) {
    const int rb = fused16_states_per_group();
    Fused16Args fa{};
    fa.f.c = chain_args(f16_set, v, skip);
    fa.f.slab = slab;
    fa.f.slab_stride = slab_stride;
    for (int l = 0; l < L; ++l) fa.f.offW[l] = offW[l];
    fa.f.ngroups = (int)((n + rb - 1) / rb);
    fa.img_e = f16_set.e;
    fa.am_x = am_x();
    fa.am_d1 = am_d(1);
    fa.am_d2 = L == 3 ? am_d(2) : nullptr;
    fa.DS = DSL;
    fa.am_ds2 = am_ds(L - 1);
    const int64_t slots = std::max<int64_t>(
        1, std::min<int64_t>({(int64_t)fa.f.ngroups, (int64_t)S, (int64_t)num_cus * fused16_groups_per_cu()}));
    const int64_t rounds = (fa.f.ngroups + slots - 1) / slots;
    grid = (int)std::max<int64_t>(1, (fa.f.ngroups + rounds - 1) / rounds);
    return fa;
  }
  void fused16_w_images() {
    if (cache.f16_w_valid) return;
    Scope sp(this, "fvp_img_w");
    launch_fused16_img(f16_set.jobs, theta, nullptr, 0, nullptr, f16_set.e, stream);
    check_launch();
    cache.f16_w_valid = true;
  }

  // the whole Hv in one launch on the f16 split (fused16.hip) + the slab reduction
  void fvp_fused16(const float* v, float* out, const int* skip, int* defer = nullptr) {
    fused16_w_images();
    if (!f16_v_img_ready) {   // else the previous CG step's launch built v's images (cg())
      Scope sp(this, "fvp_img_v");
      launch_fused16_img(f16_set.jobs, theta, v, 1, skip, f16_set.e, stream);
      check_launch();
    }
    f16_v_img_ready = false;
    int grid = 1;
    const Fused16Args fa = fused16_args(v, skip, grid);
    {
      Scope sp(this, "fvp_fused");
      launch_fvp_fused16(fa, grid, stream);
      check_launch();
    }
    if (defer) {
      *defer = grid;
      return;
    }
    reduce_grad(out, skip, grid);
  }

  // g's slabs in one launch on the same machinery (fused16.hip, PG form): the surr backward from DS_2 and every
  // block of g (when the prepare launch's are gone)
  void pg_fused16() {
    fused16_w_images();
    cache.slabs_written();
    const Fused16Args fa = fused16_args(nullptr, nullptr, cache.pg_grid);
    {
      Scope sp(this, "pg_fused");
      launch_pg_fused16(fa, cache.pg_grid, stream);
      check_launch();
    }
    cache.pg_ready = true;
  }

  // the same Hv with the row-local part (R-forward, R-head, R-backward) in one fused launch
  void fvp_chain(const float* v, float* out, const int* skip) {
    chain_images(v, skip);
    const ChainArgs ca = chain_args(chain_set, v, skip);
    {
      Scope sp(this, "fvp_chain");
      launch_fvp_chain(ca, chain_otm, stream);
      check_launch();
    }
    bool split_wg_used = false;   // a weight gradient on the split path reads RH / RD scales
    for (int l = 0; l < L; ++l) split_wg_used |= g_options.split_wg != 0 && w[l + 1] > 128;
    if (f16 && split_wg_used) {
      // the chain writes RH / RD without running maxima; the split weight gradients need them
      am_reset(am_rh(0), L);
      am_reset(am_rd(0), L);
      for (int l = 0; l < L; ++l) {
        if (l >= 1) launch_amax(RH[l], n, w[l], wp[l], am_rh(l), stream);
        launch_amax(RD[l], n, w[l + 1], wp[l + 1], am_rd(l), stream);
      }
      check_launch();
    }
    fvp_wgrads(0, L, skip);
    reduce_grad(out, skip);
  }

  // conjugate_gradient(fvp, b) (utils.py:185-201): b, x device vectors
  void cg(const float* b, float* xo, int iters, float tol, float damping) {
    REQUIRE(iters >= 0 && iters <= kMaxCG, "cg_iters out of range");
    prepare();
    launch_cg_init(b, xo, r, p, P, partA, sc, fl, tol, damping, stream);
    check_launch();
    f16_v_img_ready = false;
    float* pc = p;    // this iteration's direction; cg_p_img16 writes the next one into the other buffer
    float* pn = p2;
    for (int it = 0; it < iters; ++it) {
      int slabs = 0;
      fvp(pc, hv, &fl->done[it], g_options.cg_fuse_reduce ? &slabs : nullptr);
      Scope sp(this, "cg_vec");
      if (slabs > 0 && g_options.cg_fuse_reduce == 2) {
        // the rest of the iteration in the slab reduction's launch; on the fused16 path it also builds the next
        // iteration's V image, which that FVP then does not launch (fvp_fused16)
        const CgStepArgs ca{slab, slabs, it, slab_stride, P, hv, xo, r, pc, z, sc, partA, fl, cg_ticket};
        const bool img = use_fused16() && it + 1 < iters;
        launch_cg_step_slabs(ca, img ? &f16_set.jobs : nullptr, f16_set.e, stream);
        f16_v_img_ready = img;
      } else if (slabs > 0 && g_options.cg_p_img != 0 && use_fused16() && it + 1 < iters) {
        // the p update and the next FVP's V images in one launch (the next p in the other buffer)
        launch_cg_iter_slabs(slab, slabs, slab_stride, hv, xo, r, pc, z, P, sc, partA, partB, fl, it, stream, false);
        launch_cg_p_img16(f16_set.jobs, r, pc, pn, P, sc, partB, fl, it, f16_set.e, stream);
        f16_v_img_ready = true;
        std::swap(pc, pn);
      } else if (slabs > 0) {
        launch_cg_iter_slabs(slab, slabs, slab_stride, hv, xo, r, pc, z, P, sc, partA, partB, fl, it, stream);
      } else {
        launch_cg_iter(hv, xo, r, pc, z, P, sc, partA, partB, fl, it, stream);
      }
      check_launch();
    }
    f16_v_img_ready = false;
  }

  void fetch_scalars() {
    HIPCHECK(hipMemcpyAsync(hsc, sc, sizeof(UpdScalars), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    har_pending = false;
    check_har();
  }

  // loss(th) at a device parameter vector, without touching the prepared cache
  // the policy forward in one launch from th's f16 weight images (fused16.hip fwd_loss16_kernel): the line search's
  // row loss terms, or (prep) the prepare pass's H_1, H_2, P, D_2, DS_2, their maxima and the row terms
  void fused16_forward(const float* th, bool prep) {
    {
      Scope sp(this, prep ? "fwd_img" : "ls_img");
      launch_fused16_img(f16_loss_set.jobs, th, nullptr, 0, nullptr, f16_loss_set.e, stream);
      check_launch();
    }
    FwdLoss16Args la{};
    la.n = n;
    la.L = L;
    for (int l = 0; l <= L; ++l) {
      la.w[l] = w[l];
      la.ld[l] = wp[l];
    }
    la.X = X;
    la.theta = th;
    for (int l = 0; l < L; ++l) la.offb[l] = offb[l];
    la.img = f16_loss_set.img;
    la.tab = f16_loss_set.tab;
    la.nchunks = f16_loss_set.nchunks;
    la.img_e = f16_loss_set.e;
    la.am_x = am_x();
    la.old = old;
    la.act = act;
    la.adv = adv32;
    la.rowterms = rowterms;
    if (prep) {
      la.H1 = H[1];
      la.H2 = L == 3 ? H[2] : nullptr;
      la.P = Pm;
      la.D = D[L - 1];
      la.DS = DSL;
      la.am_d = am_d(L - 1);
      la.am_ds = am_ds(L - 1);
      la.invN = 1.0 / (double)n_global;
    }
    Scope sp(this, prep ? "fwd" : "ls_fwd");
    launch_fwd_loss16(la, num_cus, stream);
    check_launch();
  }

  void eval_losses_dev(const float* th) {
    require_batch();
    if (use_fused16() && g_options.ls_fused != 0) {
      fused16_forward(th, false);
      reduce_losses(1, nullptr);
      return;
    }
    PackArgs pa = pack_args(WFt, nullptr, 2);
    launch_pack(pa, th, 0, nullptr, stream);
    split_parts(true, false, false, false, trial_set(), nullptr, "split_t");
    forward(trial_set(), th, RH, gauss() ? RowEpi::kGaussLossHead : RowEpi::kLossHead, "ls_fwd");
    reduce_losses(1, nullptr);
  }

  // tail values belong to GAE; the returns estimator would silently drop them
  void check_estimator_state() const {
    if (have_tail && adv_kind == TRPO_ADV_RETURNS)
      throw std::runtime_error(
          "tail values are set but the advantage estimator is TRPO_ADV_RETURNS: select TRPO_ADV_GAE or clear them");
  }

  // Two-pass moments of c = y - sub (sub may be NULL) over all ranks: c to centered_out (may alias y), its sum to
  // *mean_slot, then the sum of (c - mean)^2 to *sumsq_slot, mean = *mean_slot * inv_n.  `part` holds kRedBlocks
  // partials; without an engine (one process) nothing is all-reduced.
  static void moments(trpo_engine* e, hipStream_t s, double* part, const double* y, const double* sub,
                      double* centered_out, int64_t count, double inv_n, double* mean_slot, double* sumsq_slot) {
    launch_adv_center_partials(y, sub, centered_out, count, part, s);
    launch_sum_finish(part, mean_slot, s);
    if (e) e->allreduce_f64(mean_slot, 1);
    launch_adv_sq_partials(centered_out, count, mean_slot, inv_n, part, s);
    launch_sum_finish(part, sumsq_slot, s);
    if (e) e->allreduce_f64(sumsq_slot, 1);
  }

  void compute_advantages(double gamma) {
    REQUIRE(have_rewards, "no rewards: call trpo_set_rewards first");
    check_estimator_state();
    const double inv_n = 1.0 / (double)n_global;
    if (adv_kind == TRPO_ADV_GAE) {
      // one scan writes the returns and the raw advantages; the standardisation then runs in place, the
      // launches of standardize()
      launch_gae(rewards, have_baseline ? baseline : nullptr, starts, have_tail ? tail : nullptr, n, gamma,
                 adv_lambda, adv64, returns, scan_ws, stream);
      moments(this, stream, partA, adv64, nullptr, adv64, n, inv_n, dscal, dscal + 1);
    } else {
      launch_discount(rewards, starts, n, gamma, returns, scan_ws, stream);
      moments(this, stream, partA, returns, have_baseline ? baseline : nullptr, adv64, n, inv_n, dscal, dscal + 1);
    }
    launch_adv_normalize(adv64, adv32, n, dscal, dscal + 1, inv_n, stream);
    check_launch();
    cache.advantages_computed();
  }

  // adv = (adv - mean)/(std + 1e-8) over all ranks (trpo_inksci.py:115-117), device arrays on this
  // engine's stream; the same kernels and sums as compute_advantages
  void standardize(double* adv, float* adv32, int64_t cnt, int64_t cnt_global) {
    const double inv_n = 1.0 / (double)cnt_global;
    moments(this, stream, partA, adv, nullptr, adv, cnt, inv_n, dscal + 6, dscal + 7);
    launch_adv_normalize(adv, adv32, cnt, dscal + 6, dscal + 7, inv_n, stream);
    check_launch();
  }

  // 1 - var(y - ypred)/var(y) with y = returns, ypred = baseline (utils.py:208-211), f64 over all ranks
  double explained_variance() {
    REQUIRE(cache.have_returns, "no returns: compute the advantages first");
    if (!ev_tmp) ev_tmp = dalloc<double>(cap);
    const double inv_n = 1.0 / (double)n_global;
    moments(this, stream, partA, returns, nullptr, ev_tmp, n, inv_n, dscal + 2, dscal + 3);
    moments(this, stream, partA, returns, have_baseline ? baseline : nullptr, ev_tmp, n, inv_n, dscal + 4, dscal + 5);
    check_launch();
    double h[6];
    copy_out(h, dscal, sizeof h, TRPO_MEM_HOST);
    const double vary = h[3] * inv_n, vard = h[5] * inv_n;
    return vary == 0.0 ? std::nan("") : 1.0 - vard / vary;
  }

  // The update's sync-free prefix: advantages .. CG .. step scaling .. the first line-search trial
  // (trpo_inksci.py:102-153 up to the first `loss(xnew)` of utils.py:176).  Nothing in it waits on
  // the host, so it is replayed as one captured hipGraph (update()).
  void update_prefix(const trpo_update_params& prm) {
    if (prm.compute_advantages) {
      Scope sp(this, "advantages");
      compute_advantages(prm.gamma);
    }
    prepare();
    // thprev = self.gf()  (:144)
    HIPCHECK(hipMemcpyAsync(theta_prev, theta, P * sizeof(float), hipMemcpyDeviceToDevice, stream));
    // g = session.run(pg)  (:146)
    policy_grad();
    // stepdir = conjugate_gradient(fisher_vector_product, -g)  (:147)
    launch_scale_copy(g, bneg, -1.0f, P, stream);
    // the Fisher matrix of the CG and of shs: over every row, or (fvp_stride > 1) over the child's rows, gathered
    // here, after the advantages
    trpo_engine* fe = fisher_ready();
    fe->cg(bneg, stepdir, prm.cg_iters, prm.residual_tol, prm.cg_damping);
    // shs = .5 * stepdir.dot(fisher_vector_product(stepdir)) ; lm ; fullstep ; rate  (:148-151)
    fe->fvp(stepdir, hv, nullptr);
    {
      Scope sp(this, "step_scale");
      launch_shs_partials(hv, stepdir, g, P, sc, partA, partB, stream);
      launch_shs_finish(partA, partB, sc, stream);
      launch_fullstep(stepdir, fullstep, P, sc, stream);
      check_launch();
    }
    // theta = linesearch(loss, thprev, fullstep, neggdotstepdir / lm)  (:153): trial k = 0
    launch_ls_trial(theta_prev, fullstep, theta_trial, P, 0, sc, stream);
    eval_losses_dev(theta_trial);
    launch_ls_decide(sc, 0, stream);
    check_launch();
  }

  // hipGraph of update_prefix: keyed on everything that shapes its launches (rows, the update
  // parameters that become kernel arguments, the baseline switch, the kernel-variant options).
  // The first update with a key runs eagerly (lazy allocations happen there), the second captures
  // and replays, later ones replay.  The cache state the prefix leaves behind is restored after a replay.
  struct GraphKey {
    int64_t n, n_global;
    int64_t fvp_stride;   // the Fisher child's rows follow from it: its launches are part of the graph
    int64_t fvp_global, fisher_phase;   // ... and from the mode and the gather's first row
    const void* comm;   // the communicator / host transport the all-reduces were captured with
    const void* host_ar;
    int rank, world;
    int cg_iters, adv, baseline;
    int adv_kind, tail;   // the estimator's kind and whether the feed has tail values: they pick the captured scan
    int x_planes;   // X's planes hold the current batch: the captured plane kernels read them (set_batch
                    // writes them outside the graph, so a replay must not outlive a change of this flag)
    float tol, damping;
    double gamma;
    double lambda;   // GAE's lambda is a kernel argument of the captured scan
    Options opt;
  };
  static_assert(offsetof(GraphKey, opt) ==
                    5 * sizeof(int64_t) + 2 * sizeof(void*) + 8 * sizeof(int) + 2 * sizeof(float) + 2 * sizeof(double),
                "GraphKey is compared with memcmp: keep it free of padding");
  GraphKey graph_key(const trpo_update_params& prm) const {
    GraphKey k;
    std::memset(&k, 0, sizeof k);
    k.n = n;
    k.n_global = n_global;
    k.fvp_stride = fvp_stride;
    k.fvp_global = fvp_global ? 1 : 0;
    k.fisher_phase = fisher_phase();
    k.comm = comm;
    k.host_ar = (const void*)host_ar;
    k.rank = rank;
    k.world = world;
    k.cg_iters = prm.cg_iters;
    k.adv = prm.compute_advantages != 0;
    k.baseline = have_baseline;
    k.adv_kind = adv_kind;
    k.tail = have_tail ? 1 : 0;
    k.lambda = adv_lambda;
    k.x_planes = x_planes ? 1 : 0;
    k.tol = prm.residual_tol;
    k.damping = prm.cg_damping;
    k.gamma = prm.compute_advantages ? prm.gamma : 0.0;
    k.opt = g_options;
    return k;
  }
  hipGraphExec_t upd_exec = nullptr;
  GraphKey upd_key{};
  bool upd_key_seen = false, graphs_broken = false;
  CacheState upd_state{};   // `cache` as the captured prefix left it
  CacheState upd_state_fisher{};   // ... and the Fisher child's
  void drop_graph() {
    if (upd_exec) {
      if (har_graph_end) (void)hipStreamSynchronize(stream);   // its host nodes may still be pending
      (void)hipGraphExecDestroy(upd_exec);
    }
    upd_exec = nullptr;
    upd_key_seen = false;
    har_graph_end = 0;
  }
  void run_prefix(const trpo_update_params& prm) {
    // multi-rank engines capture their all-reduces too (RCCL calls or the host transport's nodes)
    const bool graphable = g_options.graphs != 0 && !prof && !graphs_broken;
    if (!graphable) {
      update_prefix(prm);
      return;
    }
    const GraphKey key = graph_key(prm);
    const bool same = upd_key_seen && std::memcmp(&key, &upd_key, sizeof key) == 0;
    if (same && upd_exec) {
      HIPCHECK(hipGraphLaunch(upd_exec, stream));
      if (har_graph_end) har_pending = true;
      cache = upd_state;
      if (fisher) fisher->cache = upd_state_fisher;
      return;
    }
    if (!same) {
      drop_graph();
      har_next = 0;
      update_prefix(prm);
      upd_key = key;
      upd_key_seen = true;
      return;
    }
    // capture (the cache is rebuilt inside the graph, so the prefix must not skip prepare(), nor the Fisher
    // child's gather, whose feed_loaded() makes the child prepare again)
    cache.prepared = cache.fisher_fed = false;
    hipGraph_t graph = nullptr;
    har_next = 0;
    HIPCHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    try {
      update_prefix(prm);
    } catch (...) {
      (void)hipStreamEndCapture(stream, &graph);
      if (graph) (void)hipGraphDestroy(graph);
      graphs_broken = true;
      throw;
    }
    HIPCHECK(hipStreamEndCapture(stream, &graph));
    const hipError_t ie = hipGraphInstantiate(&upd_exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ie != hipSuccess) {
      upd_exec = nullptr;
      graphs_broken = true;
      (void)hipGetLastError();
      cache.prepared = cache.fisher_fed = false;
      update_prefix(prm);
      return;
    }
    upd_state = cache;
    if (fisher) upd_state_fisher = fisher->cache;
    har_graph_end = har_next;   // the graph's host nodes own these slots from now on
    HIPCHECK(hipGraphLaunch(upd_exec, stream));
    if (har_graph_end) har_pending = true;
  }

  void update(const trpo_update_params& prm, trpo_update_stats* st) {
    require_batch();
    REQUIRE(prm.cg_iters >= 0 && prm.cg_iters <= kMaxCG, "cg_iters out of range");
    REQUIRE(!prm.compute_advantages || have_rewards, "no rewards: call trpo_set_rewards first");
    if (prm.compute_advantages) check_estimator_state();   // before any capture begins
    // max_kl goes to the scalar block before shs_finish reads it (no prefix kernel writes it)
    HIPCHECK(hipMemcpyAsync(&sc->max_kl, &prm.max_kl, sizeof(double), hipMemcpyHostToDevice, stream));
    run_prefix(prm);
    fetch_scalars();
    for (int k = 1; k < 10 && !hsc->accepted; ++k) {
      launch_ls_trial(theta_prev, fullstep, theta_trial, P, k, sc, stream);
      eval_losses_dev(theta_trial);
      launch_ls_decide(sc, k, stream);
      check_launch();
      fetch_scalars();
    }
    // sff(theta) ; losses ; revert if kl > 2 max_kl  (:154-158)
    launch_ls_finalize(theta_prev, fullstep, theta, theta_ls, P, sc, stream);
    check_launch();
    cache.theta_changed();
    fetch_scalars();
    if (st) {
      st->cg_iters = hsc->iters;
      st->k = hsc->accepted ? hsc->k : -1;
      st->reverted = hsc->reverted;
      st->shs = hsc->shs;
      st->lm = hsc->lm;
      st->rate = hsc->rate;
      st->surr_before = hsc->loss_before[0];
      st->kl_before = hsc->loss_before[1];
      st->ent_before = hsc->loss_before[2];
      st->surr_after = hsc->loss_after[0];
      st->kl_after = hsc->loss_after[1];
      st->ent_after = hsc->loss_after[2];
      st->rdotr = hsc->rdotr[hsc->iters & 1];
      st->gdotstepdir = hsc->gdots;
    }
  }
};

// =============================================================================
// C-ABI
// =============================================================================
extern "C" {

const char* trpo_last_error(void) { return g_last_error.c_str(); }

int trpo_create_dist(trpo_engine** out, int dist, int obs_dim, const int* hidden, int n_hidden, int act_dim,
                     int64_t max_rows, int device) {
  return guarded([&] {
    REQUIRE(out, "out is NULL");
    REQUIRE(n_hidden == 0 || hidden, "hidden is NULL");
    auto e = std::make_unique<trpo_engine>();
    try {
      e->init(dist, obs_dim, hidden, n_hidden, act_dim, max_rows, device);
    } catch (...) {
      e->release();
      throw;
    }
    *out = e.release();
  });
}

int trpo_create(trpo_engine** out, int obs_dim, const int* hidden, int n_hidden, int n_actions,
                int64_t max_rows, int device) {
  return trpo_create_dist(out, TRPO_DIST_CATEGORICAL, obs_dim, hidden, n_hidden, n_actions, max_rows, device);
}

int trpo_get_dist(trpo_engine* e, int* dist) {
  return guarded([&] {
    REQUIRE(e && dist, "NULL argument");
    *dist = e->dist;
  });
}

void trpo_destroy(trpo_engine* e) {
  if (!e) return;
  e->release();
  delete e;
}

int64_t trpo_num_params(const trpo_engine* e) { return e ? e->P : -1; }

int trpo_synchronize(trpo_engine* e) {
  return guarded([&] {
    REQUIRE(e, "engine is NULL");
    e->use();
    HIPCHECK(hipStreamSynchronize(e->stream));
    e->har_pending = false;
    e->check_har();
  });
}

void* trpo_stream(trpo_engine* e) { return e ? (void*)e->stream : nullptr; }

int trpo_comm_unique_id(uint8_t out_id[128]) {
  return guarded([&] {
    REQUIRE(out_id, "out_id is NULL");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId id;
    NCCLCHECK(ncclGetUniqueId(&id));
    std::memcpy(out_id, &id, sizeof id);
  });
}

int trpo_comm_init(trpo_engine* e, const uint8_t id[128], int rank, int world) {
  return guarded([&] {
    REQUIRE(e && id, "NULL argument");
    REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank/world");
    e->require_single_rank_for_fisher("trpo_comm_init");
    e->use();
    if (e->comm) {
      NCCLCHECK(ncclCommDestroy(e->comm));
      e->comm = nullptr;
    }
    e->drop_graph();
    e->rank = rank;
    e->world = world;
    e->host_ar = nullptr;
    // world = 1 creates a one-rank communicator as well: every all-reduce then runs through RCCL
    // (an identity), which exercises that path on a single GPU
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof uid);
    NCCLCHECK(ncclCommInitRank(&e->comm, world, uid, rank));
  });
}

int trpo_comm_set_host_allreduce(trpo_engine* e, trpo_allreduce_cb cb, void* ctx, int rank, int world) {
  return guarded([&] {
    REQUIRE(e && cb, "NULL argument");
    REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank/world");
    e->require_single_rank_for_fisher("trpo_comm_set_host_allreduce");
    e->use();
    e->drop_graph();
    if (e->comm) {
      NCCLCHECK(ncclCommDestroy(e->comm));
      e->comm = nullptr;
    }
    e->host_ar = cb;
    e->host_ar_ctx = ctx;
    e->rank = rank;
    e->world = world;
  });
}

int trpo_comm_info(trpo_engine* e, trpo_comm_info_t* out) {
  return guarded([&] {
    REQUIRE(e && out, "NULL argument");
    e->use();
    trpo_comm_info_t ci{};
    ci.transport = e->comm ? 1 : (e->host_ar ? 2 : 0);
    ci.rank = e->rank;
    ci.world = e->world;
    ci.comm_count = ci.comm_rank = ci.comm_device = -1;
    if (e->comm) {
      NCCLCHECK(ncclCommCount(e->comm, &ci.comm_count));
      NCCLCHECK(ncclCommUserRank(e->comm, &ci.comm_rank));
      NCCLCHECK(ncclCommCuDevice(e->comm, &ci.comm_device));
    }
    ci.device = e->device;
    HIPCHECK(hipDeviceGetPCIBusId(ci.pci_bus_id, (int)sizeof ci.pci_bus_id, e->device));
    *out = ci;
  });
}

int trpo_set_flat(trpo_engine* e, const float* theta, int mem) {
  return guarded([&] {
    REQUIRE(e && theta, "NULL argument");
    e->use();
    e->copy_in(e->theta, theta, e->P * sizeof(float), mem);
    e->cache.theta_changed();
  });
}

int trpo_get_flat(trpo_engine* e, float* out, int mem) {
  return guarded([&] {
    REQUIRE(e && out, "NULL argument");
    e->use();
    e->copy_out(out, e->theta, e->P * sizeof(float), mem);
  });
}

int trpo_get_vector(trpo_engine* e, int which, float* out, int mem) {
  return guarded([&] {
    REQUIRE(e && out, "NULL argument");
    e->use();
    const float* src = nullptr;
    switch (which) {
      case TRPO_VEC_THETA: src = e->theta; break;
      case TRPO_VEC_THETA_PREV: src = e->theta_prev; break;
      case TRPO_VEC_G: src = e->g; break;
      case TRPO_VEC_STEPDIR: src = e->stepdir; break;
      case TRPO_VEC_FULLSTEP: src = e->fullstep; break;
      case TRPO_VEC_THETA_LS: src = e->theta_ls; break;
      default: throw ArgError("unknown vector id");
    }
    e->copy_out(out, src, e->P * sizeof(float), mem);
  });
}

int trpo_set_batch(trpo_engine* e, int64_t n, int64_t n_global, const float* states,
                   const int64_t* actions, const float* advant, const float* old_dist, int mem) {
  return guarded([&] {
    REQUIRE(e && states && actions && old_dist, "NULL argument");
    e->require_dist(TRPO_DIST_CATEGORICAL, "trpo_set_batch");
    REQUIRE(n > 0 && n <= e->cap, "n out of range (0 < n <= max_rows)");
    REQUIRE(n_global >= n, "n_global must be >= n");
    e->require_fisher_feed_ok(n, n_global);
    e->use();
    e->n = n;
    e->n_global = n_global;
    e->feed_row0 = e->row0_next;
    const int obs = e->w[0], A = e->w[e->L];
    // states -> [n][pad4(obs)], old_dist -> [n][pad4(A)] (padding zero)
    e->stage_rows(states, obs, e->wp[0], e->X, mem);
    e->stage_rows(old_dist, A, e->wp[e->L], e->old, mem);
    e->update_x_amax();
    const int64_t* acts = actions;
    if (mem != TRPO_MEM_DEVICE) {
      e->copy_in(e->stage, actions, (size_t)n * sizeof(int64_t), mem);
      acts = reinterpret_cast<const int64_t*>(e->stage);
    }
    HIPCHECK(hipMemsetAsync(e->dbad, 0, sizeof(int), e->stream));
    launch_i64_to_i32(acts, e->act, n, e->dbad, A, e->stream);
    check_launch();
    int bad = 0;
    e->copy_out(&bad, e->dbad, sizeof(int), TRPO_MEM_HOST);
    REQUIRE(!bad, "action index out of range [0, n_actions)");
    if (advant) e->copy_in(e->adv32, advant, (size_t)n * sizeof(float), mem);
    e->feed_loaded();
  });
}

int trpo_set_batch_gaussian(trpo_engine* e, int64_t n, int64_t n_global, const float* states, const float* actions,
                            const float* advant, const float* old_mean, const float* old_logstd, int mem) {
  return guarded([&] {
    REQUIRE(e && states && actions && old_mean && old_logstd, "NULL argument");
    e->require_dist(TRPO_DIST_GAUSSIAN, "trpo_set_batch_gaussian");
    REQUIRE(n > 0 && n <= e->cap, "n out of range (0 < n <= max_rows)");
    REQUIRE(n_global >= n, "n_global must be >= n");
    e->require_fisher_feed_ok(n, n_global);
    e->use();
    e->n = n;
    e->n_global = n_global;
    e->feed_row0 = e->row0_next;
    const int A = e->w[e->L], ldA = e->wp[e->L];
    e->stage_rows(states, e->w[0], e->wp[0], e->X, mem);
    e->stage_rows(actions, A, ldA, e->actf, mem);
    e->stage_rows(old_mean, A, ldA, e->old, mem);
    e->copy_in(e->logstd0, old_logstd, (size_t)A * sizeof(float), mem);
    e->update_x_amax();
    if (advant) e->copy_in(e->adv32, advant, (size_t)n * sizeof(float), mem);
    e->feed_loaded();
  });
}

int trpo_set_rewards(trpo_engine* e, const double* rewards, const uint8_t* starts,
                     const double* baseline, int mem) {
  return guarded([&] {
    REQUIRE(e && rewards && starts, "NULL argument");
    e->require_batch();
    e->use();
    e->copy_in(e->rewards, rewards, (size_t)e->n * sizeof(double), mem);
    e->copy_in(e->starts, starts, (size_t)e->n, mem);
    e->have_baseline = baseline != nullptr;
    if (baseline) e->copy_in(e->baseline, baseline, (size_t)e->n * sizeof(double), mem);
    e->have_rewards = true;
    e->cache.rewards_changed();
    e->have_tail = false;
    e->feed_is_rollout = false;
    e->feed_has_step = false;   // the new path starts are not the segment's
  });
}

int trpo_set_advantage_estimator(trpo_engine* e, int kind, double lambda) {
  return guarded([&] {
    REQUIRE(kind == TRPO_ADV_RETURNS || kind == TRPO_ADV_GAE, "kind must be TRPO_ADV_RETURNS or TRPO_ADV_GAE");
    REQUIRE(kind != TRPO_ADV_GAE || (lambda >= 0.0 && lambda <= 1.0), "lambda must be in [0, 1]");   // NaN fails
    REQUIRE(e, "engine is NULL");
    e->adv_kind = kind;
    e->adv_lambda = kind == TRPO_ADV_GAE ? lambda : 1.0;
  });
}

int trpo_get_advantage_estimator(trpo_engine* e, int* kind, double* lambda) {
  return guarded([&] {
    REQUIRE(e, "engine is NULL");
    if (kind) *kind = e->adv_kind;
    if (lambda) *lambda = e->adv_lambda;
  });
}

int trpo_set_tail_values(trpo_engine* e, const double* tail_values, int mem) {
  return guarded([&] {
    REQUIRE(e, "engine is NULL");
    if (!tail_values) {
      e->have_tail = false;
      return;
    }
    e->require_batch();
    e->use();
    if (!e->tail) e->tail = e->dalloc<double>(e->cap);
    // the engine's own buffer (trpo_get_tail_view's tail, written in place) is marked set without a copy
    if (tail_values != e->tail) e->copy_in(e->tail, tail_values, (size_t)e->n * sizeof(double), mem);
    e->have_tail = true;
  });
}

int trpo_get_tail_values(trpo_engine* e, double* out, int mem) {
  return guarded([&] {
    REQUIRE(e && out, "NULL argument");
    e->require_batch();
    e->use();
    if (e->have_tail) {
      e->copy_out(out, e->tail, (size_t)e->n * sizeof(double), mem);
    } else if (mem == TRPO_MEM_DEVICE) {
      HIPCHECK(hipMemsetAsync(out, 0, (size_t)e->n * sizeof(double), e->stream));
      HIPCHECK(hipStreamSynchronize(e->stream));
    } else {
      std::fill(out, out + e->n, 0.0);
    }
  });
}

int trpo_compute_advantages(trpo_engine* e, double gamma, double* returns_out, double* advant_out,
                            int mem) {
  return guarded([&] {
    REQUIRE(e, "engine is NULL");
    e->use();
    e->compute_advantages(gamma);
    if (returns_out) e->copy_out(returns_out, e->returns, (size_t)e->n * sizeof(double), mem);
    if (advant_out) e->copy_out(advant_out, e->adv64, (size_t)e->n * sizeof(double), mem);
  });
}

int trpo_standardize(trpo_engine* e, double* adv, int64_t n, int64_t n_global, float* adv32_out, int mem) {
  return guarded([&] {
    REQUIRE(adv, "adv is NULL");
    REQUIRE(n >= 0 && n_global >= n, "need 0 <= n <= n_global");
    REQUIRE(e || n_global == n, "n_global != n needs an engine (its communicator sums the ranks)");
    if (e) e->use();
    if (n_global == 0) return;
    hipStream_t s = e ? e->stream : nullptr;
    Staging st(mem, s);
    double* da = st.inout(adv, (size_t)n);
    float* d32 = st.out(adv32_out, (size_t)n);
    if (e) {
      e->standardize(da, d32, n, n_global);
    } else {
      double* part = st.tmp<double>(kRedBlocks);
      double* sums = st.tmp<double>(2);
      const double inv_n = 1.0 / (double)n;
      trpo_engine::moments(nullptr, s, part, da, nullptr, da, n, inv_n, sums, sums + 1);
      launch_adv_normalize(da, d32, n, sums, sums + 1, inv_n, s);
      check_launch();
    }
    st.fetch();
    HIPCHECK(hipStreamSynchronize(s));
    if (e) {
      // the host all-reduce callbacks of the two sums ran during the sync: a failure there means the
      // mean / std were rank-local, so it is this call's error (as fetch_scalars / copy_out report it)
      e->har_pending = false;
      e->check_har();
    }
  });
}

int trpo_losses(trpo_engine* e, float out3[3]) {
  return guarded([&] {
    REQUIRE(e && out3, "NULL argument");
    e->use();
    e->prepare();
    e->fetch_scalars();
    std::memcpy(out3, e->hsc->loss_before, 3 * sizeof(float));
  });
}

int trpo_eval_losses(trpo_engine* e, const float* theta, float out3[3], int mem) {
  return guarded([&] {
    REQUIRE(e && theta && out3, "NULL argument");
    e->use();
    e->copy_in(e->theta, theta, e->P * sizeof(float), mem);   // sff(th), trpo_inksci.py:128
    e->cache.theta_changed();
    e->eval_losses_dev(e->theta);
    e->fetch_scalars();
    std::memcpy(out3, e->hsc->loss_trial, 3 * sizeof(float));
  });
}

int trpo_action_dist(trpo_engine* e, float* out, int mem) {
  return guarded([&] {
    REQUIRE(e && out, "NULL argument");
    e->require_dist(TRPO_DIST_CATEGORICAL, "trpo_action_dist");
    e->use();
    e->prepare();
    e->fetch_head_rows(out, mem);
  });
}

int trpo_action_mean(trpo_engine* e, float* mean_out, float* logstd_out, int mem) {
  return guarded([&] {
    REQUIRE(e, "engine is NULL");
    e->require_dist(TRPO_DIST_GAUSSIAN, "trpo_action_mean");
    e->use();
    e->prepare();
    if (mean_out) e->fetch_head_rows(mean_out, mem);
    if (logstd_out) e->copy_out(logstd_out, e->logstd_of(e->theta), (size_t)e->w[e->L] * sizeof(float), mem);
  });
}

int trpo_policy_grad(trpo_engine* e, float* g_out, int mem) {
  return guarded([&] {
    REQUIRE(e && g_out, "NULL argument");
    e->use();
    e->policy_grad();
    e->copy_out(g_out, e->g, e->P * sizeof(float), mem);
  });
}

int trpo_fvp(trpo_engine* e, const float* v, float* out, float damping, int mem) {
  return guarded([&] {
    REQUIRE(e && v && out, "NULL argument");
    e->use();
    e->copy_in(e->vin, v, e->P * sizeof(float), mem);
    e->fisher_ready()->fvp(e->vin, e->hv, nullptr);
    // out = fvp + damping * v  (float32, trpo_inksci.py:126)
    HIPCHECK(hipMemcpyAsync(e->vout, e->hv, e->P * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    if (damping != 0.0f) {
      float* tmp = e->z;
      launch_scale_copy(e->vin, tmp, damping, e->P, e->stream);
      launch_axpby(e->vout, tmp, 1.0f, 1.0f, e->P, e->stream);
      check_launch();
    }
    e->copy_out(out, e->vout, e->P * sizeof(float), mem);
  });
}

int trpo_cg(trpo_engine* e, const float* b, float* x_out, int cg_iters, float residual_tol,
            float damping, int* iters_out, int mem) {
  return guarded([&] {
    REQUIRE(e && b && x_out, "NULL argument");
    e->use();
    e->copy_in(e->bneg, b, e->P * sizeof(float), mem);
    e->fisher_ready()->cg(e->bneg, e->stepdir, cg_iters, residual_tol, damping);
    e->copy_out(x_out, e->stepdir, e->P * sizeof(float), mem);
    e->fetch_scalars();
    if (iters_out) *iters_out = e->hsc->iters;
  });
}

int trpo_cg_callback(trpo_fax_cb f_Ax, void* ctx, const void* b, void* x_out, int64_t n, int dtype,
                     int cg_iters, double residual_tol, int* iters_out) {
  return guarded([&] {
    REQUIRE(f_Ax && b && x_out, "NULL argument");
    REQUIRE(n > 0, "n must be positive");
    REQUIRE(dtype == TRPO_F32 || dtype == TRPO_F64, "dtype must be TRPO_F32 or TRPO_F64");
    REQUIRE(cg_iters >= 0 && cg_iters <= kMaxCG, "cg_iters out of range");
    const size_t es = dtype == TRPO_F64 ? 8 : 4;
    const size_t bytes = (size_t)n * es;
    hipStream_t s = nullptr;
    HIPCHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    std::vector<void*> bufs;
    auto alloc = [&](size_t by) {
      void* p = nullptr;
      HIPCHECK(hipMalloc(&p, std::max<size_t>(by, 16)));
      HIPCHECK(hipMemsetAsync(p, 0, std::max<size_t>(by, 16), s));
      bufs.push_back(p);
      return p;
    };
    try {
      void *db = alloc(bytes), *dx = alloc(bytes), *dr = alloc(bytes), *dp = alloc(bytes),
           *dz = alloc(bytes), *dhv = alloc(bytes);
      double* pa = (double*)alloc(kRedBlocks * sizeof(double));
      double* pb = (double*)alloc(kRedBlocks * sizeof(double));
      CGFlags* fl = (CGFlags*)alloc(sizeof(CGFlags));
      void* sc = alloc(std::max(sizeof(UpdScalars), sizeof(CGScalarsD)));
      std::vector<uint8_t> ph(bytes), zh(bytes);
      HIPCHECK(hipMemcpyAsync(db, b, bytes, hipMemcpyHostToDevice, s));
      if (dtype == TRPO_F64)
        launch_cg_init_d((double*)db, (double*)dx, (double*)dr, (double*)dp, n, pa, (CGScalarsD*)sc, fl,
                         residual_tol, s);
      else
        launch_cg_init((float*)db, (float*)dx, (float*)dr, (float*)dp, n, pa, (UpdScalars*)sc, fl,
                       (float)residual_tol, 0.0f, s);
      HIPCHECK(hipGetLastError());
      int iters = 0;
      for (int it = 0; it < cg_iters; ++it) {
        int done = 0;
        HIPCHECK(hipMemcpyAsync(&done, &fl->done[it], sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHECK(hipMemcpyAsync(ph.data(), dp, bytes, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        if (done) break;
        REQUIRE(f_Ax(ph.data(), zh.data(), ctx) == 0, "f_Ax callback failed");
        HIPCHECK(hipMemcpyAsync(dhv, zh.data(), bytes, hipMemcpyHostToDevice, s));
        if (dtype == TRPO_F64)
          launch_cg_iter_d((double*)dhv, (double*)dx, (double*)dr, (double*)dp, (double*)dz, n,
                           (CGScalarsD*)sc, pa, pb, fl, it, s);
        else
          launch_cg_iter((float*)dhv, (float*)dx, (float*)dr, (float*)dp, (float*)dz, n, (UpdScalars*)sc,
                         pa, pb, fl, it, s);
        HIPCHECK(hipGetLastError());
        iters = it + 1;
      }
      HIPCHECK(hipMemcpyAsync(x_out, dx, bytes, hipMemcpyDeviceToHost, s));
      HIPCHECK(hipStreamSynchronize(s));
      if (iters_out) *iters_out = iters;
    } catch (...) {
      (void)hipStreamSynchronize(s);
      for (void* p : bufs) (void)hipFree(p);
      (void)hipStreamDestroy(s);
      throw;
    }
    for (void* p : bufs) (void)hipFree(p);
    HIPCHECK(hipStreamDestroy(s));
  });
}

int trpo_linesearch(trpo_engine* e, const float* x, const float* fullstep, double rate,
                    float* theta_out, int* k_out, int mem) {
  return guarded([&] {
    REQUIRE(e && x && fullstep && theta_out, "NULL argument");
    e->use();
    const int64_t P = e->P;
    e->copy_in(e->theta_prev, x, P * sizeof(float), mem);
    e->copy_in(e->fullstep, fullstep, P * sizeof(float), mem);
    // fval = f(x)  (utils.py:173)
    e->eval_losses_dev(e->theta_prev);
    e->fetch_scalars();
    UpdScalars init = *e->hsc;
    init.loss_before[0] = init.loss_trial[0];
    init.loss_before[1] = init.loss_trial[1];
    init.loss_before[2] = init.loss_trial[2];
    init.rate = rate;
    init.accepted = 0;
    init.k = -1;
    *e->hsc = init;
    HIPCHECK(hipMemcpyAsync(e->sc, e->hsc, sizeof(UpdScalars), hipMemcpyHostToDevice, e->stream));
    int k_acc = -1;
    for (int k = 0; k < 10; ++k) {
      launch_ls_trial(e->theta_prev, e->fullstep, e->theta_trial, P, k, e->sc, e->stream);
      e->eval_losses_dev(e->theta_trial);
      launch_ls_decide(e->sc, k, e->stream);
      check_launch();
      e->fetch_scalars();
      HIPCHECK(hipMemcpyAsync(e->theta, e->theta_trial, P * sizeof(float), hipMemcpyDeviceToDevice,
                              e->stream));   // loss() leaves sff(xnew) behind
      if (e->hsc->accepted) {
        k_acc = k;
        break;
      }
    }
    e->cache.theta_changed();
    e->copy_out(theta_out, k_acc >= 0 ? e->theta_trial : e->theta_prev, P * sizeof(float), mem);
    if (k_out) *k_out = k_acc;
  });
}

int trpo_update(trpo_engine* e, const trpo_update_params* p, trpo_update_stats* stats) {
  return guarded([&] {
    REQUIRE(e, "engine is NULL");
    e->use();
    trpo_update_params prm;
    trpo_default_params(&prm);
    if (p) prm = *p;
    e->update(prm, stats);
  });
}

int trpo_rollout_env(trpo_engine* e, int env, const trpo_rollout_params* p, int64_t* n_steps_out,
                     int64_t* n_paths_out) {
  return guarded([&] {
    REQUIRE(e && p, "NULL argument");
    e->require_dist(TRPO_DIST_CATEGORICAL, "trpo_rollout_env");
    e->use();
    e->rollout(false, env, *p);
    if (n_steps_out) *n_steps_out = e->roll_n;
    if (n_paths_out) *n_paths_out = e->roll_paths;
  });
}

int trpo_rollout_cartpole(trpo_engine* e, const trpo_rollout_params* p, int64_t* n_steps_out, int64_t* n_paths_out) {
  return trpo_rollout_env(e, TRPO_ENV_CARTPOLE_V0, p, n_steps_out, n_paths_out);
}

int trpo_rollout_fetch_states(trpo_engine* e, double* env_states, int mem) {
  return guarded([&] {
    REQUIRE(e, "NULL argument");
    e->require_dist(TRPO_DIST_CATEGORICAL, "trpo_rollout_fetch_states");
    if (!e->roll_valid) throw std::runtime_error("no rollout to fetch");
    REQUIRE(env_states, "NULL argument");
    e->use();
    RolloutOut o{};
    Staging st(mem, e->stream);
    o.env_state = st.out(env_states, (size_t)e->roll_n * e->roll_args.state_dim);
    e->rollout_compact(o);
    st.fetch();
    HIPCHECK(hipStreamSynchronize(e->stream));
  });
}

int trpo_rollout_fetch(trpo_engine* e, double* obs, float* obs32, int64_t* actions, float* action_dists,
                       double* rewards, uint8_t* episode_starts, double* uniforms, int mem) {
  return guarded([&] {
    REQUIRE(e, "NULL argument");
    e->require_dist(TRPO_DIST_CATEGORICAL, "trpo_rollout_fetch");
    REQUIRE(e->roll_valid, "no rollout to fetch");
    e->use();
    const int64_t N = e->roll_n;
    const int obs_dim = e->w[0], A = e->w[e->L];
    RolloutOut o{};
    Staging st(mem, e->stream);
    o.obs64 = st.out(obs, (size_t)N * obs_dim);
    o.X = st.out(obs32, (size_t)N * obs_dim);
    o.ldx = obs_dim;
    o.actions64 = st.out(actions, (size_t)N);
    o.head = st.out(action_dists, (size_t)N * A);
    o.ld_head = A;
    o.rewards = st.out(rewards, (size_t)N);
    o.starts = st.out(episode_starts, (size_t)N);
    o.noise = st.out(uniforms, (size_t)N);
    e->rollout_compact(o);
    st.fetch();
    HIPCHECK(hipStreamSynchronize(e->stream));
  });
}

int trpo_rollout_to_batch(trpo_engine* e, int64_t n_global) {
  return guarded([&] {
    REQUIRE(e, "NULL argument");
    e->require_dist(TRPO_DIST_CATEGORICAL, "trpo_rollout_to_batch");
    REQUIRE(e->roll_valid, "no rollout to load");
    RolloutOut o{};
    o.act32 = e->act;
    e->rollout_to_feed(o, n_global);
  });
}

int trpo_get_feed_view(trpo_engine* e, trpo_feed_view* v) {
  return guarded([&] {
    REQUIRE(e && v, "NULL argument");
    e->require_batch();
    e->use();
    HIPCHECK(hipStreamSynchronize(e->stream));   // other streams read these buffers next
    v->n = e->n;
    v->n_global = e->n_global;
    v->obs_dim = e->w[0];
    v->n_actions = e->w[e->L];
    v->states = e->X;
    v->ld_states = e->wp[0];
    v->old_dist = e->old;
    v->ld_old = e->wp[e->L];
    v->episode_starts = e->have_rewards ? e->starts : nullptr;
    v->returns = e->cache.have_returns ? e->returns : nullptr;   // stale until the advantages are computed
    v->baseline = e->baseline;
    v->step_index = e->have_rewards && e->feed_has_step ? e->feed_step : nullptr;
  });
}

int trpo_rollout_fetch_ends(trpo_engine* e, uint8_t* truncated, double* final_obs, float* final_dists,
                            int64_t* lengths, int64_t* end_rows, int mem) {
  return guarded([&] {
    REQUIRE(e, "NULL argument");
    e->require_dist(TRPO_DIST_CATEGORICAL, "trpo_rollout_fetch_ends");
    if (!e->roll_valid) throw std::runtime_error("no rollout to fetch");
    e->rollout_fetch_ends(truncated, final_obs, final_dists, lengths, end_rows, mem);
  });
}

int trpo_get_tail_view(trpo_engine* e, trpo_tail_view* v) {
  return guarded([&] {
    REQUIRE(e && v, "NULL argument");
    if (!(e->feed_is_rollout && e->roll_valid && e->n > 0))
      throw std::runtime_error("the feed is not the one trpo_rollout_to_batch loaded");
    e->use();
    if (!e->tail) e->tail = e->dalloc<double>(e->cap);
    HIPCHECK(hipMemsetAsync(e->tail, 0, (size_t)e->n * sizeof(double), e->stream));
    e->have_tail = false;
    HIPCHECK(hipStreamSynchronize(e->stream));   // other streams read and write these buffers next
    v->n = e->n;
    v->n_paths = e->roll_paths;
    v->obs_dim = e->w[0];
    v->n_actions = e->w[e->L];
    v->final_obs32 = e->roll.cat_obs32;
    v->final_dist = e->roll.cat_dist;
    // the time entry of s_T's features is the episode's step count there: of a segment's fragment, t0 + rows
    v->lengths = e->roll_segment ? e->roll.cat_steps : e->roll.cat_len;
    v->truncated = e->roll.cat_truncated;
    v->end_rows = e->roll.cat_rows;
    v->tail = e->tail;
  });
}

int trpo_set_baseline(trpo_engine* e, const double* baseline, int mem) {
  return guarded([&] {
    REQUIRE(e && baseline, "NULL argument");
    e->require_batch();
    e->use();
    if (baseline != e->baseline) e->copy_in(e->baseline, baseline, (size_t)e->n * sizeof(double), mem);
    e->have_baseline = true;
  });
}

int trpo_explained_variance(trpo_engine* e, double* out) {
  return guarded([&] {
    REQUIRE(e && out, "NULL argument");
    e->use();
    *out = e->explained_variance();
  });
}

int trpo_act(trpo_engine* e, const float* states, int64_t n, const double* uniforms, int train, int64_t* actions_out,
             float* dists_out, int mem) {
  return guarded([&] {
    REQUIRE(e && states && n >= 0, "bad argument");
    e->require_dist(TRPO_DIST_CATEGORICAL, "trpo_act");
    REQUIRE(!train || uniforms, "train = 1 needs uniforms (cat_sample's np.random.rand)");
    REQUIRE(e->w[e->L] <= 64, "act: n_actions must be <= 64 (one wave per state)");
    e->use();
    if (n == 0) return;
    const int obs = e->w[0], A = e->w[e->L];
    Staging st(mem, e->stream);
    const float* s = st.in(states, (size_t)n * obs);
    const double* r = st.in(uniforms, (size_t)n);
    int64_t* ao = st.out(actions_out, (size_t)n);
    float* dout = st.out(dists_out, (size_t)n * A);
    launch_act(e->policy_shape(), e->theta, e->max_width(), s, n, r, train, ao, dout, e->stream);
    check_launch();
    st.fetch();
    HIPCHECK(hipStreamSynchronize(e->stream));
  });
}

int trpo_act_gaussian(trpo_engine* e, const float* states, int64_t n, const double* normals, int train,
                      float* actions_out, float* mean_out, float* logstd_out, int mem) {
  return guarded([&] {
    REQUIRE(e && states && n >= 0, "bad argument");
    e->require_dist(TRPO_DIST_GAUSSIAN, "trpo_act_gaussian");
    REQUIRE(!train || normals, "train = 1 needs normals [n][act_dim]");
    REQUIRE(e->w[e->L] <= 64, "act_gaussian: act_dim must be <= 64 (one wave per state)");
    e->use();
    const int obs = e->w[0], A = e->w[e->L];
    if (logstd_out) e->copy_out(logstd_out, e->logstd_of(e->theta), (size_t)A * sizeof(float), mem);
    if (n == 0) return;
    Staging st(mem, e->stream);
    const float* s = st.in(states, (size_t)n * obs);
    const double* xi = st.in(normals, (size_t)n * A);
    float* ao = st.out(actions_out, (size_t)n * A);
    float* mo = st.out(mean_out, (size_t)n * A);
    launch_act_gaussian(e->policy_shape(), e->theta, e->logstd_of(e->theta), e->max_width(), s, n, xi, train, ao, mo,
                        e->stream);
    check_launch();
    st.fetch();
    HIPCHECK(hipStreamSynchronize(e->stream));
  });
}

// ---- the Gaussian engine's rollouts of the continuous-action environments ----------------------------------
int trpo_rollout_gaussian(trpo_engine* e, int cenv, const trpo_rollout_params* p, int64_t* n_steps_out,
                          int64_t* n_paths_out) {
  return guarded([&] {
    REQUIRE(e && p, "NULL argument");
    e->require_dist(TRPO_DIST_GAUSSIAN, "trpo_rollout_gaussian");
    REQUIRE(e->w[e->L] <= 64, "rollout_gaussian: act_dim must be <= 64 (one wave per environment)");
    e->use();
    e->rollout(true, cenv, *p);
    if (n_steps_out) *n_steps_out = e->roll_n;
    if (n_paths_out) *n_paths_out = e->roll_paths;
  });
}

int trpo_rollout_gaussian_fetch(trpo_engine* e, double* obs, float* obs32, float* actions, float* means,
                                float* logstd, double* rewards, uint8_t* episode_starts, double* normals,
                                double* env_states, int mem) {
  return guarded([&] {
    REQUIRE(e, "NULL argument");
    e->require_dist(TRPO_DIST_GAUSSIAN, "trpo_rollout_gaussian_fetch");
    if (!e->roll_valid) throw std::runtime_error("no rollout to fetch");
    e->use();
    const int64_t N = e->roll_n;
    const int obs_dim = e->w[0], A = e->w[e->L];
    RolloutOut o{};
    Staging st(mem, e->stream);
    o.obs64 = st.out(obs, (size_t)N * obs_dim);
    o.X = st.out(obs32, (size_t)N * obs_dim);
    o.ldx = obs_dim;
    o.actf = st.out(actions, (size_t)N * A);
    o.ld_actf = A;
    o.head = st.out(means, (size_t)N * A);
    o.ld_head = A;
    o.noise = st.out(normals, (size_t)N * A);
    o.rewards = st.out(rewards, (size_t)N);
    o.starts = st.out(episode_starts, (size_t)N);
    o.env_state = st.out(env_states, (size_t)N * e->roll_args.state_dim);
    e->rollout_compact(o);
    st.fetch();
    if (logstd) e->copy_out(logstd, e->roll.logstd, (size_t)A * sizeof(float), mem);
    HIPCHECK(hipStreamSynchronize(e->stream));
  });
}

int trpo_rollout_gaussian_fetch_ends(trpo_engine* e, uint8_t* truncated, double* final_obs, float* final_means,
                                     int64_t* lengths, int64_t* end_rows, int mem) {
  return guarded([&] {
    REQUIRE(e, "NULL argument");
    e->require_dist(TRPO_DIST_GAUSSIAN, "trpo_rollout_gaussian_fetch_ends");
    if (!e->roll_valid) throw std::runtime_error("no rollout to fetch");
    e->rollout_fetch_ends(truncated, final_obs, final_means, lengths, end_rows, mem);
  });
}

int trpo_rollout_gaussian_to_batch(trpo_engine* e, int64_t n_global) {
  return guarded([&] {
    REQUIRE(e, "NULL argument");
    e->require_dist(TRPO_DIST_GAUSSIAN, "trpo_rollout_gaussian_to_batch");
    if (!e->roll_valid) throw std::runtime_error("no rollout to load");
    RolloutOut o{};
    o.actf = e->actf;
    o.ld_actf = e->wp[e->L];
    e->rollout_to_feed(o, n_global);
  });
}

// ---- fixed-horizon segment rollouts: environments that persist across calls ---------------------------------
int trpo_rollout_env_segment(trpo_engine* e, int env, const trpo_rollout_params* p, int resume, int64_t* n_steps_out,
                             int64_t* n_paths_out) {
  return guarded([&] {
    REQUIRE(e && p, "NULL argument");
    REQUIRE(resume == 0 || resume == 1, "resume must be 0 or 1");
    e->require_dist(TRPO_DIST_CATEGORICAL, "trpo_rollout_env_segment");
    e->use();
    e->rollout(false, env, *p, true, resume);
    if (n_steps_out) *n_steps_out = e->roll_n;
    if (n_paths_out) *n_paths_out = e->roll_paths;
  });
}

int trpo_rollout_gaussian_segment(trpo_engine* e, int cenv, const trpo_rollout_params* p, int resume,
                                  int64_t* n_steps_out, int64_t* n_paths_out) {
  return guarded([&] {
    REQUIRE(e && p, "NULL argument");
    REQUIRE(resume == 0 || resume == 1, "resume must be 0 or 1");
    e->require_dist(TRPO_DIST_GAUSSIAN, "trpo_rollout_gaussian_segment");
    REQUIRE(e->w[e->L] <= 64, "rollout_gaussian_segment: act_dim must be <= 64 (one wave per environment)");
    e->use();
    e->rollout(true, cenv, *p, true, resume);
    if (n_steps_out) *n_steps_out = e->roll_n;
    if (n_paths_out) *n_paths_out = e->roll_paths;
  });
}

int trpo_rollout_segment_fetch(trpo_engine* e, uint8_t* end_kind, int64_t* t0, double* episode_returns,
                               int64_t* step_index, int mem) {
  return guarded([&] {
    REQUIRE(e, "NULL argument");
    if (!e->roll_valid) throw std::runtime_error("no rollout to fetch");
    if (!e->roll_segment) throw std::runtime_error("the last rollout was not a segment rollout");
    e->use();
    const size_t P = (size_t)e->roll_paths, N = (size_t)e->roll_n;
    SegmentOut o{};
    Staging st(mem, e->stream);
    o.end_kind = st.out(end_kind, P);
    o.end_t0 = st.out(t0, P);
    o.end_ret = st.out(episode_returns, P);
    o.step_index = st.out(step_index, N);
    e->segment_compact(o);
    st.fetch();
    HIPCHECK(hipStreamSynchronize(e->stream));
  });
}

int trpo_rollout_carry_get(trpo_engine* e, int* env_out, int* n_envs_out, double* states, int64_t* t, double* returns,
                           int mem) {
  return guarded([&] {
    REQUIRE(e, "NULL argument");
    if (!e->carry.valid) throw std::runtime_error("there is no rollout carry");
    e->use();
    const auto& c = e->carry;
    if (env_out) *env_out = c.env;
    if (n_envs_out) *n_envs_out = c.n_envs;
    if (states) e->copy_out(states, c.s, (size_t)c.n_envs * c.state_dim * sizeof(double), mem);
    if (t) e->copy_out(t, c.t, (size_t)c.n_envs * sizeof(int64_t), mem);
    if (returns) e->copy_out(returns, c.ret, (size_t)c.n_envs * sizeof(double), mem);
    HIPCHECK(hipStreamSynchronize(e->stream));
  });
}

int trpo_rollout_carry_set(trpo_engine* e, int env, int n_envs, const double* states, const int64_t* t,
                           const double* returns, int mem) {
  return guarded([&] {
    REQUIRE(e && states && t && returns, "NULL argument");
    EnvDims ed{};
    REQUIRE(env_dims(e->gauss(), env, &ed),
            std::string(e->gauss() ? "unknown continuous environment id " : "unknown environment id ") +
                std::to_string(env));
    REQUIRE(n_envs >= 1 && n_envs <= (1 << 20), "n_envs out of range");
    REQUIRE(e->w[0] == ed.obs_dim && e->w[e->L] == ed.head_dim,
            std::string(ed.name) + " does not fit this engine's obs_dim and head width");
    e->use();
    e->carry_reserve(n_envs, ed.state_dim);
    e->carry.valid = false;
    e->copy_in(e->carry.s, states, (size_t)n_envs * ed.state_dim * sizeof(double), mem);
    e->copy_in(e->carry.t, t, (size_t)n_envs * sizeof(int64_t), mem);
    e->copy_in(e->carry.ret, returns, (size_t)n_envs * sizeof(double), mem);
    HIPCHECK(hipStreamSynchronize(e->stream));
    e->carry.valid = true;
    e->carry.continuous = e->gauss();
    e->carry.env = env;
    e->carry.n_envs = n_envs;
    e->carry.state_dim = ed.state_dim;
  });
}

int trpo_rollout_carry_clear(trpo_engine* e) {
  return guarded([&] {
    REQUIRE(e, "NULL argument");
    e->carry.valid = false;
  });
}

int trpo_set_fvp_subsample(trpo_engine* e, int stride) {
  return guarded([&] {
    REQUIRE(e, "engine is NULL");
    e->set_fvp_subsample(stride, false);
  });
}

int trpo_set_fvp_subsample_global(trpo_engine* e, int stride) {
  return guarded([&] {
    REQUIRE(e, "engine is NULL");
    e->set_fvp_subsample(stride, true);
  });
}

int trpo_set_row_offset(trpo_engine* e, int64_t row0) {
  return guarded([&] {
    REQUIRE(e, "engine is NULL");
    if (row0 < 0) throw std::runtime_error("trpo_set_row_offset: row0 must be >= 0, got " + std::to_string(row0));
    e->row0_next = row0;
  });
}

int trpo_get_fvp_subsample_global(trpo_engine* e, int* global, int64_t* n_sub_global, int64_t* phase,
                                  int64_t* row0) {
  return guarded([&] {
    REQUIRE(e, "engine is NULL");
    if (global) *global = e->fvp_global ? 1 : 0;
    if (n_sub_global)
      *n_sub_global = trpo_engine::sub_rows(e->fvp_global ? e->n_global : e->n, e->fvp_stride);
    if (phase) *phase = e->fisher_phase();
    if (row0) *row0 = e->row0_next;
  });
}

int trpo_get_fvp_subsample(trpo_engine* e, int* stride, int64_t* n_sub) {
  return guarded([&] {
    REQUIRE(e, "engine is NULL");
    if (stride) *stride = (int)e->fvp_stride;
    if (n_sub) *n_sub = e->n > 0 ? e->fisher_rows() : 0;
  });
}

int trpo_fvp_subsample_fetch(trpo_engine* e, float* states, void* actions, float* old, float* advant, int mem) {
  return guarded([&] {
    REQUIRE(e, "engine is NULL");
    if (!e->fisher) throw std::runtime_error("trpo_fvp_subsample_fetch: no Fisher feed (fvp_subsample is 1)");
    e->use();
    trpo_engine* c = e->fisher_ready();
    const int64_t ns = c->n;
    const int obs = c->w[0], A = c->w[c->L];
    // padded rows -> the caller's unpadded ones, through the child's staging buffer for a host caller
    auto rows = [&](const float* src, int width, int ld, float* out) {
      if (!out) return;
      float* dst = mem == TRPO_MEM_DEVICE ? out : c->stage;
      launch_copy_rows(src, ns, width, ld, dst, width, c->stream);
      check_launch();
      if (mem != TRPO_MEM_DEVICE) e->copy_out(out, c->stage, (size_t)ns * width * sizeof(float), mem);
    };
    rows(c->X, obs, c->wp[0], states);
    rows(c->old, A, c->wp[c->L], old);
    if (c->gauss()) rows(c->actf, A, c->wp[c->L], static_cast<float*>(actions));
    else if (actions) e->copy_out(actions, c->act, (size_t)ns * sizeof(int), mem);
    if (advant) e->copy_out(advant, c->adv32, (size_t)ns * sizeof(float), mem);
    HIPCHECK(hipStreamSynchronize(e->stream));
  });
}

int trpo_profile_enable(trpo_engine* e, int enable) {
  return guarded([&] {
    REQUIRE(e, "engine is NULL");
    e->use();
    e->prof_collect();
    e->prof = enable != 0;
    if (e->fisher) e->fisher->prof = e->prof;
  });
}

int trpo_profile_reset(trpo_engine* e) {
  return guarded([&] {
    REQUIRE(e, "engine is NULL");
    e->use();
    e->prof_collect();
    e->prof_acc.clear();
  });
}

int trpo_profile_query(trpo_engine* e, char* buf, int cap) {
  std::string js;
  int rc = guarded([&] {
    REQUIRE(e, "engine is NULL");
    e->use();
    e->prof_collect();
    js = "{";
    bool first = true;
    for (auto& kv : e->prof_acc) {
      char item[256];
      std::snprintf(item, sizeof item, "%s\"%s\": [%ld, %.6f]", first ? "" : ", ", kv.first.c_str(),
                    kv.second.first, kv.second.second);
      js += item;
      first = false;
    }
    js += "}";
  });
  if (rc != TRPO_OK) return rc;
  if (buf && cap > 0) {
    std::strncpy(buf, js.c_str(), (size_t)cap - 1);
    buf[cap - 1] = '\0';
  }
  return (int)js.size();
}

}  // extern "C"
