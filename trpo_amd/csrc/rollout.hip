// Batched policy sampling and rollouts of the built-in environments on the GPU (gfx950).
//
// Restates, data-parallel over environments:
//   * agent.act (trpo_inksci.py:76-87): the policy forward on one state, then
//     cat_sample (utils.py:95-105) -- inverse CDF over the float32 cumsum of the
//     action distribution against a float64 uniform, first k with csprob > r,
//     else 0 -- or argmax when not training;
//   * rollout (utils.py:18-45): episodes of up to max_pathlength steps, each
//     recording (obs, action, action_dist, reward), until the collected steps
//     reach n_timesteps;
//   * the CartPole-v0 environment the reference runs (gym.make("CartPole-v0"),
//     trpo_inksci.py:179): Euler-integrated cart-pole, reset to U(-0.05, 0.05)^4,
//     done past |x| > 2.4 or |theta| > 12 degrees, reward 1 per step, and the
//     v0 TimeLimit of 200 steps.  gym is not vendored in the reference; this is
//     its published classic_control/cartpole.py restated in float64 (Python floats).
//   * MountainCar-v0 and Acrobot-v1, which the reference does not run: gym's classic_control tasks
//     restated the same way (include/trpo_engine.h spells out their equations).  The rollout is one
//     kernel over an environment trait (reset, step, observe and the dimensions), so that a task whose
//     state is not its observation (Acrobot) or whose reward is not constant costs no second kernel.
//   * Pendulum-v1 and MountainCarContinuous-v0 under the diagonal-Gaussian policy: the same kernel over a trait
//     with kContinuous set, which steps with the float32 action components, sampled as act_gaussian does
//     (gauss_act) from Box-Muller normals off the same Philox stream; it records action, mean and normal per
//     component, and samples with the copy of the log-std vector the engine took when the rollout began.
//
// What depends on the policy head sits behind `if constexpr (Env::kContinuous)`: the forward (softmax or mean),
// the sample, the per-step records of head row, action and draw, and the trait's step().  The head row -- the
// distribution or the mean, kHead floats -- is rerun at s_T and compacted by the same lines for both.
//
// One wave simulates one environment for its whole share of the rollout: the
// policy forward is wave-parallel over output units (activations in a per-wave
// LDS slice), the physics and sampling are computed redundantly by all 64
// lanes so every lane holds the state in registers.  Each environment collects
// episodes until its own step count reaches ceil(n_timesteps / n_envs) -- the
// reference's stopping rule applied per environment, so with n_envs = 1 it is
// exactly utils.py:23-44 and for any n_envs every started episode completes.
// Episodes land in a per-environment region; a compaction kernel concatenates
// the regions in environment order (deterministic for a given seed).
//
// The reference scores every path end alike.  Here each path also records how it
// ended, in a per-environment path region (an environment starts at most
// ceil(n_timesteps / n_envs) episodes): whether it was cut off -- its last step
// did not terminate the environment, the time limit or max_pathlength ended it --
// or terminated (a step that does both is a termination), the state s_T after the
// last step, T, the path's last row and, for a cut-off path, the policy's
// distribution (or mean) at s_T from one more forward that draws nothing.  The
// compaction kernel concatenates these records too, so that GAE can bootstrap the
// cut-off paths from V(s_T) (vf.hip: the VF's features are [obs | dist | t/10]).
// The per-step outputs and the Philox draw indices do not depend on any of it.
//
// rollout_segment_kernel collects the other way, as baselines' traj_segment_generator does: every environment
// takes exactly ceil(n_timesteps / n_envs) steps per call and continues, from a per-environment carry (state,
// episode step count, episode return so far), where the previous call left it.  Its paths are the fragments of
// episodes that lie in the segment; a fragment the segment cut is a cut-off path whose s_T is the carried state.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <stdexcept>

#pragma clang fp contract(off)

namespace trpo {
namespace {

// ---- Philox4x32-10 (counter-based; key = seed, counter = (env, stream, draw)) -------------------
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
  const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
  c[0] = hi1 ^ c[1] ^ k0;
  c[1] = lo1;
  c[2] = hi0 ^ c[3] ^ k1;
  c[3] = lo0;
}
__device__ __forceinline__ void philox(uint32_t (&c)[4], uint64_t seed) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
// uniform double in [0, 1) with 53 random bits, numpy's random_sample recipe ((a>>5)*2^26 + (b>>6)) / 2^53
__device__ __forceinline__ double uniform53(uint64_t seed, uint32_t env, uint32_t stream, uint64_t draw) {
  uint32_t c[4] = {env, stream, (uint32_t)draw, (uint32_t)(draw >> 32)};
  philox(c, seed);
  const uint32_t a = c[0] >> 5, b = c[1] >> 6;
  return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
}

// standard normal by Box-Muller off one Philox call: u1 from (c0, c1), u2 from (c2, c3), both by uniform53's recipe;
// xi = sqrt(-2 log(1 - u1)) cos(2 pi u2)  (1 - u1 is in (0, 1], so the log is finite)
__device__ __forceinline__ double normal53(uint64_t seed, uint32_t env, uint32_t stream, uint64_t draw) {
  uint32_t c[4] = {env, stream, (uint32_t)draw, (uint32_t)(draw >> 32)};
  philox(c, seed);
  const double u1 = ((double)(c[0] >> 5) * 67108864.0 + (double)(c[1] >> 6)) / 9007199254740992.0;
  const double u2 = ((double)(c[2] >> 5) * 67108864.0 + (double)(c[3] >> 6)) / 9007199254740992.0;
  return sqrt(-2.0 * log(1.0 - u1)) * cos(2 * 3.141592653589793 * u2);
}

// ---- CartPole-v0 (gym classic_control/cartpole.py), float64 ------------------------------------
constexpr double kGravity = 9.8, kMassCart = 1.0, kMassPole = 0.1;
constexpr double kTotalMass = kMassPole + kMassCart;
constexpr double kLength = 0.5;                          // half the pole's length
constexpr double kPoleMassLength = kMassPole * kLength;
constexpr double kForceMag = 10.0, kTau = 0.02;
constexpr double kThetaThreshold = 12 * 2 * 3.141592653589793 / 360;
constexpr double kXThreshold = 2.4;

__device__ __forceinline__ bool cartpole_step(double (&s)[4], int action) {
  const double x = s[0], x_dot = s[1], theta = s[2], theta_dot = s[3];
  const double force = action == 1 ? kForceMag : -kForceMag;
  const double costheta = cos(theta), sintheta = sin(theta);
  const double temp = (force + kPoleMassLength * (theta_dot * theta_dot) * sintheta) / kTotalMass;
  const double thetaacc =
      (kGravity * sintheta - costheta * temp) / (kLength * (4.0 / 3.0 - kMassPole * (costheta * costheta) / kTotalMass));
  const double xacc = temp - kPoleMassLength * thetaacc * costheta / kTotalMass;
  s[0] = x + kTau * x_dot;
  s[1] = x_dot + kTau * xacc;
  s[2] = theta + kTau * theta_dot;
  s[3] = theta_dot + kTau * thetaacc;
  return s[0] < -kXThreshold || s[0] > kXThreshold || s[2] < -kThetaThreshold || s[2] > kThetaThreshold;
}

// The rollout's view of an environment.  kObsIsState: the observation is the state itself, so the per-step
// record of the state is the record of the observation and no second array is written.  kHead: the width of the
// policy's output row, the number of actions or (kContinuous) of float32 action components step() takes.
struct CartPoleV0 {
  static constexpr int kState = 4, kObs = 4, kHead = 2, kResetDraws = 4, kTimeLimit = 200;
  static constexpr bool kObsIsState = true, kContinuous = false;
  static constexpr const char* kName = "CartPole-v0";
  // env.reset(): np_random.uniform(-0.05, 0.05, size=(4,))
  static __device__ __forceinline__ void reset(double (&s)[kState], const double* u) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = -0.05 + (0.05 - -0.05) * u[i];
  }
  static __device__ __forceinline__ bool step(double (&s)[kState], int action, double& reward) {
    reward = 1.0;
    return cartpole_step(s, action);
  }
  static __device__ __forceinline__ double observe(const double (&s)[kState], int i) { return s[i]; }
};

__device__ __forceinline__ double clampd(double x, double lo, double hi) {   // min(max(x, lo), hi)
  const double a = lo > x ? lo : x;
  return hi < a ? hi : a;
}

// ---- MountainCar-v0 (gym classic_control/mountain_car.py), float64 -----------------------------------
struct MountainCarV0 {
  static constexpr int kState = 2, kObs = 2, kHead = 3, kResetDraws = 1, kTimeLimit = 200;
  static constexpr bool kObsIsState = true, kContinuous = false;
  static constexpr const char* kName = "MountainCar-v0";
  static __device__ __forceinline__ void reset(double (&s)[kState], const double* u) {
    s[0] = -0.6 + (-0.4 - -0.6) * u[0];
    s[1] = 0.0;
  }
  static __device__ __forceinline__ bool step(double (&s)[kState], int action, double& reward) {
    double p = s[0], v = s[1];
    v = v + (double)(action - 1) * 0.001 + cos(3.0 * p) * (-0.0025);
    v = clampd(v, -0.07, 0.07);
    p = p + v;
    p = clampd(p, -1.2, 0.6);
    if (p == -1.2 && v < 0.0) v = 0.0;
    s[0] = p;
    s[1] = v;
    reward = -1.0;
    return p >= 0.5 && v >= 0.0;
  }
  static __device__ __forceinline__ double observe(const double (&s)[kState], int i) { return s[i]; }
};

// ---- Acrobot-v1 (gym classic_control/acrobot.py, "book" dynamics, one RK4 step), float64 -------------
struct AcrobotV1 {
  static constexpr int kState = 4, kObs = 6, kHead = 3, kResetDraws = 4, kTimeLimit = 500;
  static constexpr bool kObsIsState = false, kContinuous = false;
  static constexpr const char* kName = "Acrobot-v1";
  static constexpr double kPi = 3.141592653589793;
  static constexpr double m1 = 1.0, m2 = 1.0, l1 = 1.0, lc1 = 0.5, lc2 = 0.5, I1 = 1.0, I2 = 1.0, g = 9.8, dt = 0.2;
  static __device__ __forceinline__ void reset(double (&s)[kState], const double* u) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = -0.1 + (0.1 - -0.1) * u[i];
  }
  // d/dt (t1, t2, w1, w2) under torque a
  static __device__ __forceinline__ void deriv(const double (&y)[4], double a, double (&k)[4]) {
    const double t1 = y[0], t2 = y[1], w1 = y[2], w2 = y[3];
    const double c2 = cos(t2), s2 = sin(t2);
    const double d1 = m1 * (lc1 * lc1) + m2 * (l1 * l1 + lc2 * lc2 + 2 * l1 * lc2 * c2) + I1 + I2;
    const double d2 = m2 * (lc2 * lc2 + l1 * lc2 * c2) + I2;
    const double phi2 = m2 * lc2 * g * cos(t1 + t2 - kPi / 2);
    const double phi1 = -m2 * l1 * lc2 * (w2 * w2) * s2 - 2 * m2 * l1 * lc2 * w2 * w1 * s2 +
                        (m1 * lc1 + m2 * l1) * g * cos(t1 - kPi / 2) + phi2;
    const double dd2 =
        (a + d2 / d1 * phi1 - m2 * l1 * lc2 * (w1 * w1) * s2 - phi2) / (m2 * (lc2 * lc2) + I2 - (d2 * d2) / d1);
    const double dd1 = -(d2 * dd2 + phi1) / d1;
    k[0] = w1;
    k[1] = w2;
    k[2] = dd1;
    k[3] = dd2;
  }
  // while x > pi: x -= 2 pi; while x < -pi: x += 2 pi.  From a state in range one step moves an angle by a few
  // turns at most; an angle that is not finite or absurdly large (only trpo_env_step can be handed one) is
  // left as it is rather than looped on.
  static __device__ __forceinline__ double wrap(double x) {
    if (!(fabs(x) < 1e5)) return x;
    while (x > kPi) x -= 2 * kPi;
    while (x < -kPi) x += 2 * kPi;
    return x;
  }
  static __device__ __forceinline__ bool step(double (&s)[kState], int action, double& reward) {
    const double a = (double)(action - 1);
    double k1[4], k2[4], k3[4], k4[4], y[4];
    deriv(s, a, k1);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = s[i] + dt / 2 * k1[i];
    deriv(y, a, k2);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = s[i] + dt / 2 * k2[i];
    deriv(y, a, k3);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = s[i] + dt * k3[i];
    deriv(y, a, k4);
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = s[i] + dt / 6 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]);
    s[0] = wrap(s[0]);
    s[1] = wrap(s[1]);
    s[2] = clampd(s[2], -4 * kPi, 4 * kPi);
    s[3] = clampd(s[3], -9 * kPi, 9 * kPi);
    const bool done = -cos(s[0]) - cos(s[1] + s[0]) > 1.0;
    reward = done ? 0.0 : -1.0;
    return done;
  }
  // (cos t1, sin t1, cos t2, sin t2, w1, w2)
  static __device__ __forceinline__ double observe(const double (&s)[kState], int i) {
    if (i >= 4) return i == 4 ? s[2] : s[3];
    const double th = i < 2 ? s[0] : s[1];
    return (i & 1) ? sin(th) : cos(th);
  }
};

// env id (TRPO_ENV_*) -> trait; false for an unknown id
template <class F>
bool with_env(int env, F&& f) {
  switch (env) {
    case 0: f(CartPoleV0{}); return true;
    case 1: f(MountainCarV0{}); return true;
    case 2: f(AcrobotV1{}); return true;
    default: return false;
  }
}

// ---- the continuous-action environments (TRPO_CENV_*; include/trpo_engine.h spells out their equations) ----
// A trait of this kind steps with the kHead float32 action components the policy produced, widened to float64.

// Pendulum-v1 (gym classic_control/pendulum.py), float64
struct PendulumV1 {
  static constexpr int kState = 2, kObs = 3, kHead = 1, kResetDraws = 2, kTimeLimit = 200;
  static constexpr bool kObsIsState = false, kContinuous = true;
  static constexpr const char* kName = "Pendulum-v1";
  static constexpr double kPi = 3.141592653589793;
  static __device__ __forceinline__ void reset(double (&s)[kState], const double* u) {
    s[0] = -kPi + (kPi - -kPi) * u[0];
    s[1] = -1.0 + (1.0 - -1.0) * u[1];
  }
  static __device__ __forceinline__ bool step(double (&s)[kState], const float (&act)[kHead], double& reward) {
    const double th = s[0], thd = s[1];
    const double u = clampd((double)act[0], -2.0, 2.0);
    const double y = th + kPi;
    double m = fmod(y, 2 * kPi);
    if (m < 0.0) m = m + 2 * kPi;
    const double an = m - kPi;
    const double cost = an * an + 0.1 * (thd * thd) + 0.001 * (u * u);
    double thd1 = thd + (3 * 10.0 / (2 * 1.0) * sin(th) + 3.0 / (1.0 * (1.0 * 1.0)) * u) * 0.05;
    thd1 = clampd(thd1, -8.0, 8.0);
    s[0] = th + thd1 * 0.05;
    s[1] = thd1;
    reward = -cost;
    return false;
  }
  // (cos th, sin th, thd)
  static __device__ __forceinline__ double observe(const double (&s)[kState], int i) {
    return i == 0 ? cos(s[0]) : (i == 1 ? sin(s[0]) : s[1]);
  }
};

// MountainCarContinuous-v0 (gym classic_control/continuous_mountain_car.py), float64
struct MountainCarContinuousV0 {
  static constexpr int kState = 2, kObs = 2, kHead = 1, kResetDraws = 1, kTimeLimit = 999;
  static constexpr bool kObsIsState = true, kContinuous = true;
  static constexpr const char* kName = "MountainCarContinuous-v0";
  static __device__ __forceinline__ void reset(double (&s)[kState], const double* u) {
    s[0] = -0.6 + (-0.4 - -0.6) * u[0];
    s[1] = 0.0;
  }
  static __device__ __forceinline__ bool step(double (&s)[kState], const float (&act)[kHead], double& reward) {
    const double a = (double)act[0];
    double p = s[0], v = s[1];
    const double f = clampd(a, -1.0, 1.0);
    v = v + f * 0.0015 + cos(3.0 * p) * (-0.0025);
    v = clampd(v, -0.07, 0.07);
    p = p + v;
    p = clampd(p, -1.2, 0.6);
    if (p == -1.2 && v < 0.0) v = 0.0;
    s[0] = p;
    s[1] = v;
    const bool done = p >= 0.45 && v >= 0.0;
    reward = (done ? 100.0 : 0.0) - (a * a) * 0.1;   // the unclamped action, as gym's
    return done;
  }
  static __device__ __forceinline__ double observe(const double (&s)[kState], int i) { return s[i]; }
};

// continuous env id (TRPO_CENV_*) -> trait; false for an unknown id
template <class F>
bool with_cenv(int cenv, F&& f) {
  switch (cenv) {
    case 0: f(PendulumV1{}); return true;
    case 1: f(MountainCarContinuousV0{}); return true;
    default: return false;
  }
}
// either id table, by the policy head the environment is rolled out under
template <class F>
bool with_any_env(bool continuous, int env, F&& f) {
  return continuous ? with_cenv(env, f) : with_env(env, f);
}

// ---- wave-level policy forward ---------------------------------------------------------------
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_sumf(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// lane src's v in every lane; src must be the same in all lanes
__device__ __forceinline__ float wave_bcast(float v, int src) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
}

// h_{l} = tanh(h_{l-1} W_l + b_l), the last layer linear (trpo_inksci.py:38-39); `in` holds the obs (w[0]
// floats) on entry; returns the slice that holds the last layer's outputs z_L.  All lanes must call.
__device__ __forceinline__ float* wave_layers(const PolicyShape& ps, const float* theta, float* in, float* out,
                                              int lane) {
  for (int l = 0; l < ps.L; ++l) {
    const int a = ps.w[l], b = ps.w[l + 1];
    const float* W = theta + ps.offW[l];
    const float* bias = theta + ps.offb[l];
    const bool last = l == ps.L - 1;
    for (int j = lane; j < b; j += 64) {
      float acc = 0.0f;
      for (int k = 0; k < a; ++k) acc = acc + in[k] * W[(int64_t)k * b + j];
      const float z = acc + bias[j];
      out[j] = last ? z : tanhf(z);
    }
    wave_sync();
    float* t = in;
    in = out;
    out = t;
  }
  return in;
}

// ... p = softmax(z_L) (trpo_inksci.py:40); returns this lane's p (lanes >= A: 0).  All lanes must call.
__device__ float wave_policy(const PolicyShape& ps, const float* theta, float* in, float* out, int lane) {
  in = wave_layers(ps, theta, in, out, lane);
  // softmax over A <= 64 logits, now in `in`
  const int A = ps.w[ps.L];
  const float z = lane < A ? in[lane] : -INFINITY;
  const float m = wave_max(z);
  const float ex = lane < A ? expf(z - m) : 0.0f;
  const float s = wave_sumf(ex);
  return lane < A ? ex / s : 0.0f;
}

// cat_sample (utils.py:95-105) on the wave's distribution: csprob = float32 cumsum, first k with
// csprob > r (float64 comparison), 0 if none.  train = 0: argmax (trpo_inksci.py:82), first max.
__device__ __forceinline__ int wave_choose(float p, int A, double r, int train) {
  int out = 0;
  if (train) {
    float cs = 0.0f;
    for (int k = 0; k < A; ++k) {
      cs = cs + __shfl(p, k, 64);
      if ((double)cs > r) {
        out = k;
        break;
      }
    }
  } else {
    float best = __shfl(p, 0, 64);
    for (int k = 1; k < A; ++k) {
      const float pk = __shfl(p, k, 64);
      if (pk > best) {
        best = pk;
        out = k;
      }
    }
  }
  return out;
}

// the diagonal-Gaussian policy's sample of one action component (include/trpo_engine.h, TRPO_DIST_GAUSSIAN):
// a = float32(mu + exp(s) * xi), the product and the sum in float64.  act_gaussian_kernel and the Gaussian rollout
// both sample through it.
__device__ __forceinline__ float gauss_act(float mu, float logstd, double xi) {
  const double noise = exp((double)logstd) * xi;
  return (float)((double)mu + noise);
}

// this lane's entry of the policy's head row at the obs in `in` (lanes >= A: 0): its softmax probability, or
// (kContinuous) its component of the mean.  All lanes must call.
template <bool kContinuous>
__device__ __forceinline__ float wave_head(const PolicyShape& ps, const float* theta, float* in, float* out, int A,
                                           int lane) {
  if constexpr (kContinuous) {
    const float* mu = wave_layers(ps, theta, in, out, lane);
    return lane < A ? mu[lane] : 0.0f;
  } else {
    return wave_policy(ps, theta, in, out, lane);
  }
}

constexpr int kRollWaves = 4;

// The draw of an environment's step k (counted over all its episodes) is Philox (seed, env, stream 0, .): the
// uniform at k, or (kContinuous) the normal of component d at k * A + d, whether or not train.
template <class Env>
__global__ void __launch_bounds__(kRollWaves * 64) rollout_kernel(const RolloutArgs a) {
  extern __shared__ float lds[];
  constexpr int kS = Env::kState, obs_dim = Env::kObs, A = Env::kHead;   // the engine checked ps against them
  constexpr bool kCont = Env::kContinuous;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int env = blockIdx.x * kRollWaves + wv;
  if (env >= a.n_envs) return;
  float* buf0 = lds + (size_t)wv * 2 * a.maxw;
  float* buf1 = buf0 + a.maxw;
  const int64_t base = (int64_t)env * a.env_cap;
  int64_t count = 0;
  int episode = 0;
  while (count < a.budget) {
    // env.reset() from kResetDraws uniforms
    double u[Env::kResetDraws];
#pragma unroll
    for (int i = 0; i < Env::kResetDraws; ++i)
      u[i] = a.reset_u ? a.reset_u[((int64_t)env * a.max_episodes + episode) * Env::kResetDraws + i]
                       : uniform53(a.seed, (uint32_t)env, 1u, (uint64_t)episode * Env::kResetDraws + i);
    double s[kS];
    Env::reset(s, u);
    ++episode;
    bool done = false;
    int len = 0;
    for (int t = 0; t < a.max_pathlength; ++t) {
      const int64_t row = base + count;
      // act(ob): the obs fed to the float32 state placeholder, recorded as the float64 ob
      if (lane < obs_dim) {
        const double ob = Env::observe(s, lane);
        buf0[lane] = (float)ob;
        a.obs[row * obs_dim + lane] = ob;
      }
      if constexpr (!Env::kObsIsState) {
        if (lane < kS) a.env_state[row * kS + lane] = s[lane];
      }
      wave_sync();
      const float h = wave_head<kCont>(a.ps, a.theta, buf0, buf1, A, lane);
      // Where the stores sit matters to the step's latency: the compiler reloads their pointers from the kernel
      // arguments inside this loop, one wait per group of stores.
      double reward;
      if constexpr (kCont) {
        // every lane forms the whole action, as it holds the whole state; lane d records component d
        float act[A];
#pragma unroll
        for (int d = 0; d < A; ++d) {
          const float m = wave_bcast(h, d);
          double xi = 0.0;
          if (a.train)
            xi = a.draws ? a.draws[row * A + d] : normal53(a.seed, (uint32_t)env, 0u, (uint64_t)count * A + d);
          act[d] = a.train ? gauss_act(m, a.logstd[d], xi) : m;
          if (lane == d) {
            a.actf[row * A + d] = act[d];
            a.head[row * A + d] = m;
            a.noise[row * A + d] = xi;
          }
        }
        done = Env::step(s, act, reward);
      } else {
        if (lane < A) a.head[row * A + lane] = h;
        const double r = a.draws ? a.draws[row] : uniform53(a.seed, (uint32_t)env, 0u, (uint64_t)count);
        const int action = wave_choose(h, A, r, a.train);
        done = Env::step(s, action, reward);
        if (lane == 0) {
          a.acti[row] = action;
          a.noise[row] = r;
        }
      }
      if (lane == 0) {
        a.rewards[row] = reward;
        a.starts[row] = t == 0 ? 1 : 0;
      }
      ++count;
      len = t + 1;
      // the TimeLimit wrapper (CartPole-v0: max_episode_steps=200) reports done at its last step
      if (done || t + 1 >= a.time_limit) break;
      wave_sync();
    }
    wave_sync();
    // How the path ended.  It was cut off (truncated) when its last step did not terminate the environment:
    // the time limit or max_pathlength ended it, and a step that does both counts as terminated.  s is s_T;
    // its observation is recorded, and a cut-off path also records the policy's head row there (the distribution
    // is among the VF's features of s_T, vf.hip).  The extra forward draws nothing.
    const int64_t path = (int64_t)env * a.budget + (episode - 1);
    const bool truncated = !done;
    const double obT = lane < obs_dim ? Env::observe(s, lane) : 0.0;
    float hT = 0.0f;
    if (truncated) {
      if (lane < obs_dim) buf0[lane] = (float)obT;
      wave_sync();
      hT = wave_head<kCont>(a.ps, a.theta, buf0, buf1, A, lane);
      wave_sync();
    }
    if (lane < obs_dim) a.end_obs[path * obs_dim + lane] = obT;
    if (lane < A) a.end_head[path * A + lane] = hT;
    if (lane == 0) {
      a.end_truncated[path] = truncated ? 1 : 0;
      a.end_len[path] = len;
      a.end_row[path] = count - 1;
    }
  }
  if (lane == 0) {
    a.counts[env] = count;
    a.episodes[env] = episode;
  }
}

// The fixed-horizon segment rollout: every environment takes exactly a.budget steps and continues where the carry
// says the previous call left it (include/trpo_engine.h, trpo_rollout_env_segment, is the definition).  The step is
// rollout_kernel's, line for line; what differs is the bookkeeping around it: an episode's step index t and return
// live across calls, a path is the fragment of an episode that lies in this segment, and an environment is reset
// only after a step that ended its episode, the segment's last step included.  Draw k of the call is the action
// draw of the environment's step k; reset draws count this environment's resets within the call.  A kernel of
// its own rather than a flag of rollout_kernel, whose five instantiations stay what they were.
template <class Env>
__global__ void __launch_bounds__(kRollWaves * 64) rollout_segment_kernel(const SegmentArgs g) {
  extern __shared__ float lds[];
  const RolloutArgs& a = g.r;
  constexpr int kS = Env::kState, obs_dim = Env::kObs, A = Env::kHead;   // the engine checked ps against them
  constexpr bool kCont = Env::kContinuous;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int env = blockIdx.x * kRollWaves + wv;
  if (env >= a.n_envs) return;
  float* buf0 = lds + (size_t)wv * 2 * a.maxw;
  float* buf1 = buf0 + a.maxw;
  const int64_t H = a.budget, base = (int64_t)env * H;
  const int ep_max = a.max_pathlength < a.time_limit ? a.max_pathlength : a.time_limit;
  double s[kS];
  int64_t t = 0;       // steps taken in the current episode
  double ret = 0.0;    // its rewards so far
  int resets = 0;      // this environment's resets within this call
  auto reset = [&]() {
    double u[Env::kResetDraws];
#pragma unroll
    for (int i = 0; i < Env::kResetDraws; ++i)
      u[i] = a.reset_u ? a.reset_u[((int64_t)env * a.max_episodes + resets) * Env::kResetDraws + i]
                       : uniform53(a.seed, (uint32_t)env, 1u, (uint64_t)resets * Env::kResetDraws + i);
    Env::reset(s, u);
    ++resets;
    t = 0;
    ret = 0.0;
  };
  if (g.resume) {
#pragma unroll
    for (int i = 0; i < kS; ++i) s[i] = g.carry_s[(int64_t)env * kS + i];
    t = g.carry_t[env];
    ret = g.carry_ret[env];
  } else {
    reset();
  }
  int paths = 0;         // end records written
  int64_t frag0 = 0;     // the current fragment's first step of this call
  int64_t t0 = t;        // and that step's index in its episode
  bool fresh = true;     // the next row opens a path
  for (int64_t k = 0; k < H; ++k) {
    const int64_t row = base + k;
    // act(ob): the obs fed to the float32 state placeholder, recorded as the float64 ob
    if (lane < obs_dim) {
      const double ob = Env::observe(s, lane);
      buf0[lane] = (float)ob;
      a.obs[row * obs_dim + lane] = ob;
    }
    if constexpr (!Env::kObsIsState) {
      if (lane < kS) a.env_state[row * kS + lane] = s[lane];
    }
    wave_sync();
    const float h = wave_head<kCont>(a.ps, a.theta, buf0, buf1, A, lane);
    double reward;
    bool done;
    if constexpr (kCont) {
      float act[A];
#pragma unroll
      for (int d = 0; d < A; ++d) {
        const float m = wave_bcast(h, d);
        double xi = 0.0;
        if (a.train) xi = a.draws ? a.draws[row * A + d] : normal53(a.seed, (uint32_t)env, 0u, (uint64_t)k * A + d);
        act[d] = a.train ? gauss_act(m, a.logstd[d], xi) : m;
        if (lane == d) {
          a.actf[row * A + d] = act[d];
          a.head[row * A + d] = m;
          a.noise[row * A + d] = xi;
        }
      }
      done = Env::step(s, act, reward);
    } else {
      if (lane < A) a.head[row * A + lane] = h;
      const double r = a.draws ? a.draws[row] : uniform53(a.seed, (uint32_t)env, 0u, (uint64_t)k);
      const int action = wave_choose(h, A, r, a.train);
      done = Env::step(s, action, reward);
      if (lane == 0) {
        a.acti[row] = action;
        a.noise[row] = r;
      }
    }
    // step_index goes with the group of stores rollout_kernel has here (one wait for the group's pointers)
    if (lane == 0) {
      a.rewards[row] = reward;
      a.starts[row] = fresh ? 1 : 0;
      g.step_index[row] = t;
    }
    t += 1;
    ret = ret + reward;
    // the TimeLimit wrapper and max_pathlength end an episode at its step ep_max; a termination there wins
    const bool ended = done || t >= ep_max;
    fresh = ended;
    wave_sync();
    if (!ended && k + 1 < H) continue;
    // The fragment's end record, as rollout_kernel writes a path's: s is s_T, and a cut-off path -- by the limit
    // (kind 1) or by the segment (kind 2), whose s_T is the carried state -- records the head row there from one
    // more forward that draws nothing.
    const int64_t path = base + paths;   // at most one record per step: paths <= H
    const bool truncated = !done;
    const double obT = lane < obs_dim ? Env::observe(s, lane) : 0.0;
    float hT = 0.0f;
    if (truncated) {
      if (lane < obs_dim) buf0[lane] = (float)obT;
      wave_sync();
      hT = wave_head<kCont>(a.ps, a.theta, buf0, buf1, A, lane);
      wave_sync();
    }
    if (lane < obs_dim) a.end_obs[path * obs_dim + lane] = obT;
    if (lane < A) a.end_head[path * A + lane] = hT;
    if (lane == 0) {
      a.end_truncated[path] = truncated ? 1 : 0;
      a.end_len[path] = k + 1 - frag0;
      a.end_row[path] = k;
      g.end_kind[path] = done ? 0 : (ended ? 1 : 2);
      g.end_t0[path] = t0;
      g.end_ret[path] = ret;
    }
    ++paths;
    if (ended) {
      reset();
      frag0 = k + 1;
      t0 = 0;
    }
  }
  if (lane < kS) g.carry_s[(int64_t)env * kS + lane] = s[lane];
  if (lane == 0) {
    g.carry_t[env] = t;
    g.carry_ret[env] = ret;
    a.counts[env] = H;
    a.episodes[env] = paths;
  }
}

// the segment rollout's per-path columns, concatenated like rollout_compact_kernel's end records; its rows need no
// move (every environment has exactly budget of them), step_index is copied out as it lies
__global__ void __launch_bounds__(256) rollout_segment_compact_kernel(const SegmentArgs g, const int64_t* path_offsets,
                                                                      SegmentOut o) {
  const RolloutArgs& a = g.r;
  const int env = blockIdx.y;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o.step_index) {
    const int64_t r0 = (int64_t)env * a.budget;
    for (int64_t i = i0; i < a.budget; i += stride) o.step_index[r0 + i] = g.step_index[r0 + i];
  }
  const int64_t np = a.episodes[env], pdst0 = path_offsets[env], psrc0 = (int64_t)env * a.budget;
  for (int64_t i = i0; i < np; i += stride) {
    const int64_t s = psrc0 + i, d = pdst0 + i;
    if (o.end_kind) o.end_kind[d] = g.end_kind[s];
    if (o.end_t0) o.end_t0[d] = g.end_t0[s];
    if (o.end_ret) o.end_ret[d] = g.end_ret[s];
    if (o.end_steps) o.end_steps[d] = g.end_t0[s] + a.end_len[s];
  }
}

// concatenate the per-environment regions in environment order
__global__ void __launch_bounds__(256) rollout_compact_kernel(const RolloutArgs a, const int64_t* offsets,
                                                              RolloutOut o) {
  const int obs_dim = a.ps.w[0], A = a.ps.w[a.ps.L];
  const int env = blockIdx.y;
  const int64_t cnt = o.ends_only ? 0 : a.counts[env], dst0 = offsets[env], src0 = (int64_t)env * a.env_cap;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = src0 + i, d = dst0 + i;
    for (int c = 0; c < obs_dim; ++c) {
      const double v = a.obs[s * obs_dim + c];
      if (o.obs64) o.obs64[d * obs_dim + c] = v;
      if (o.X) o.X[d * o.ldx + c] = (float)v;
    }
    for (int c = 0; c < A; ++c) {
      if (o.head) o.head[d * o.ld_head + c] = a.head[s * A + c];
      if (o.actf) o.actf[d * o.ld_actf + c] = a.actf[s * A + c];
    }
    if (o.actions64) o.actions64[d] = a.acti[s];
    if (o.act32) o.act32[d] = a.acti[s];
    if (o.noise)
      for (int c = 0; c < a.noise_dim; ++c) o.noise[d * a.noise_dim + c] = a.noise[s * a.noise_dim + c];
    if (o.rewards) o.rewards[d] = a.rewards[s];
    if (o.starts) o.starts[d] = a.starts[s];
    if (o.env_state) {   // an environment whose observation is its state recorded it once, as obs
      const double* st = a.env_state ? a.env_state : a.obs;
      for (int c = 0; c < a.state_dim; ++c) o.env_state[d * a.state_dim + c] = st[s * a.state_dim + c];
    }
  }
  // the per-path end records; path offsets = exclusive sums of the environments' episode counts
  if (!o.path_offsets) return;
  const int64_t np = a.episodes[env], pdst0 = o.path_offsets[env], psrc0 = (int64_t)env * a.budget;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < np; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t s = psrc0 + i, d = pdst0 + i;
    for (int c = 0; c < obs_dim; ++c) {
      const double v = a.end_obs[s * obs_dim + c];
      if (o.end_obs64) o.end_obs64[d * obs_dim + c] = v;
      if (o.end_obs32) o.end_obs32[d * obs_dim + c] = (float)v;
    }
    if (o.end_head)
      for (int c = 0; c < A; ++c) o.end_head[d * A + c] = a.end_head[s * A + c];
    if (o.end_truncated) o.end_truncated[d] = a.end_truncated[s];
    if (o.end_len) o.end_len[d] = a.end_len[s];
    if (o.end_rows) o.end_rows[d] = dst0 + a.end_row[s];
  }
}

// act on a batch of given states (one wave per state)
__global__ void __launch_bounds__(kRollWaves * 64) act_kernel(const PolicyShape ps, const float* theta, int maxw,
                                                              const float* states, int64_t n, const double* r,
                                                              int train, int64_t* actions, float* dists) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * kRollWaves + wv;
  if (row >= n) return;
  float* buf0 = lds + (size_t)wv * 2 * maxw;
  float* buf1 = buf0 + maxw;
  const int obs_dim = ps.w[0], A = ps.w[ps.L];
  for (int c = lane; c < obs_dim; c += 64) buf0[c] = states[row * obs_dim + c];
  wave_sync();
  const float p = wave_policy(ps, theta, buf0, buf1, lane);
  const int action = wave_choose(p, A, r ? r[row] : 0.0, train);
  if (lane < A && dists) dists[row * A + lane] = p;
  if (lane == 0 && actions) actions[row] = action;
}

// the diagonal-Gaussian policy's act (one wave per state): the same wave forward without the softmax, then
// a = float32(mu + exp(s) * xi) in float64 (train) or a = mu (include/trpo_engine.h, TRPO_DIST_GAUSSIAN)
__global__ void __launch_bounds__(kRollWaves * 64) act_gaussian_kernel(const PolicyShape ps, const float* theta,
                                                                       const float* logstd, int maxw,
                                                                       const float* states, int64_t n,
                                                                       const double* normals, int train,
                                                                       float* actions, float* means) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * kRollWaves + wv;
  if (row >= n) return;
  float* buf0 = lds + (size_t)wv * 2 * maxw;
  float* buf1 = buf0 + maxw;
  const int obs_dim = ps.w[0], A = ps.w[ps.L];
  for (int c = lane; c < obs_dim; c += 64) buf0[c] = states[row * obs_dim + c];
  wave_sync();
  const float* mu = wave_layers(ps, theta, buf0, buf1, lane);
  if (lane < A) {
    const float m = mu[lane];
    if (means) means[row * A + lane] = m;
    if (actions) actions[row * A + lane] = train ? gauss_act(m, logstd[lane], normals[row * A + lane]) : m;
  }
}

__global__ void __launch_bounds__(256) cat_sample_kernel(const float* prob, int64_t n, int k, const double* r,
                                                         int64_t* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float cs = 0.0f;
    int64_t o = 0;
    for (int j = 0; j < k; ++j) {
      cs = cs + prob[i * k + j];
      if ((double)cs > r[i]) {
        o = j;
        break;
      }
    }
    out[i] = o;
  }
}

// one step per row of any environment: the state after it, its observation, reward and termination; action is
// [n] i64, or (kContinuous) [n][kHead] f32
template <class Env>
__global__ void __launch_bounds__(256) env_step_kernel(const double* state, const void* action, int64_t n,
                                                       double* state_out, double* obs_out, double* reward,
                                                       uint8_t* done) {
  constexpr int kS = Env::kState, kO = Env::kObs, kA = Env::kHead;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double s[kS];
#pragma unroll
    for (int j = 0; j < kS; ++j) s[j] = state[kS * i + j];
    double rw;
    bool d;
    if constexpr (Env::kContinuous) {
      float act[kA];
#pragma unroll
      for (int j = 0; j < kA; ++j) act[j] = static_cast<const float*>(action)[kA * i + j];
      d = Env::step(s, act, rw);
    } else {
      d = Env::step(s, (int)static_cast<const int64_t*>(action)[i], rw);
    }
    if (state_out) {
#pragma unroll
      for (int j = 0; j < kS; ++j) state_out[kS * i + j] = s[j];
    }
    if (obs_out) {
#pragma unroll
      for (int j = 0; j < kO; ++j) obs_out[kO * i + j] = Env::observe(s, j);
    }
    if (reward) reward[i] = rw;
    if (done) done[i] = d ? 1 : 0;
  }
}

inline unsigned grid1(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

size_t rollout_lds_bytes(int maxw) { return (size_t)kRollWaves * 2 * maxw * sizeof(float); }

bool env_dims(bool continuous, int env, EnvDims* out) {
  return with_any_env(continuous, env, [&](auto e) {
    using Env = decltype(e);
    *out = EnvDims{Env::kObs, Env::kState, Env::kHead, Env::kResetDraws, Env::kTimeLimit, Env::kName};
  });
}

void launch_rollout(const RolloutArgs& a, hipStream_t s) {
  const unsigned blocks = (unsigned)((a.n_envs + kRollWaves - 1) / kRollWaves);
  const bool known = with_any_env(a.continuous, a.env, [&](auto e) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(rollout_kernel<decltype(e)>), dim3(blocks), dim3(kRollWaves * 64),
                       rollout_lds_bytes(a.maxw), s, a);
  });
  if (!known) throw std::invalid_argument("launch_rollout: unknown environment id");
}

void launch_rollout_segment(const SegmentArgs& g, hipStream_t s) {
  const RolloutArgs& a = g.r;
  if (a.env_cap != a.budget) throw std::invalid_argument("launch_rollout_segment: env_cap must be the budget");
  const unsigned blocks = (unsigned)((a.n_envs + kRollWaves - 1) / kRollWaves);
  const bool known = with_any_env(a.continuous, a.env, [&](auto e) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(rollout_segment_kernel<decltype(e)>), dim3(blocks), dim3(kRollWaves * 64),
                       rollout_lds_bytes(a.maxw), s, g);
  });
  if (!known) throw std::invalid_argument("launch_rollout_segment: unknown environment id");
}

void launch_rollout_segment_compact(const SegmentArgs& g, const int64_t* path_offsets, const SegmentOut& o,
                                    int64_t max_paths, hipStream_t s) {
  const int64_t most = o.step_index ? g.r.budget : max_paths;
  const unsigned bx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((most + 255) / 256, 64));
  hipLaunchKernelGGL(rollout_segment_compact_kernel, dim3(bx, g.r.n_envs), dim3(256), 0, s, g, path_offsets, o);
}

void launch_rollout_compact(const RolloutArgs& a, const int64_t* offsets, const RolloutOut& o, int64_t max_count,
                            hipStream_t s) {
  const unsigned bx = (unsigned)std::max<int64_t>(1, std::min<int64_t>((max_count + 255) / 256, 64));
  hipLaunchKernelGGL(rollout_compact_kernel, dim3(bx, a.n_envs), dim3(256), 0, s, a, offsets, o);
}

void launch_act(const PolicyShape& ps, const float* theta, int maxw, const float* states, int64_t n, const double* r,
                int train, int64_t* actions, float* dists, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(act_kernel, dim3((unsigned)((n + kRollWaves - 1) / kRollWaves)), dim3(kRollWaves * 64),
                     rollout_lds_bytes(maxw), s, ps, theta, maxw, states, n, r, train, actions, dists);
}

void launch_act_gaussian(const PolicyShape& ps, const float* theta, const float* logstd, int maxw, const float* states,
                         int64_t n, const double* normals, int train, float* actions, float* means, hipStream_t s) {
  if (n <= 0) return;
  if (ps.w[ps.L] > 64) throw std::invalid_argument("launch_act_gaussian: act_dim must be <= 64 (one wave per state)");
  if (train && !normals) throw std::invalid_argument("launch_act_gaussian: train = 1 needs normals");
  hipLaunchKernelGGL(act_gaussian_kernel, dim3((unsigned)((n + kRollWaves - 1) / kRollWaves)), dim3(kRollWaves * 64),
                     rollout_lds_bytes(maxw), s, ps, theta, logstd, maxw, states, n, normals, train, actions, means);
}

void launch_cat_sample(const float* prob, int64_t n, int k, const double* r, int64_t* out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(cat_sample_kernel, dim3(grid1(n)), dim3(256), 0, s, prob, n, k, r, out);
}

void launch_env_step(bool continuous, int env, const double* state, const void* action, int64_t n, double* state_out,
                     double* obs_out, double* reward, uint8_t* done, hipStream_t s) {
  const bool known = with_any_env(continuous, env, [&](auto e) {
    if (n <= 0) return;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(env_step_kernel<decltype(e)>), dim3(grid1(n)), dim3(256), 0, s, state, action,
                       n, state_out, obs_out, reward, done);
  });
  if (!known) throw std::invalid_argument("launch_env_step: unknown environment id");
}

}  // namespace trpo
