// The C-ABI entries of include/trpo_engine.h that need no engine: batched sampling and CartPole steps, the
// discount and GAE scans on the current device's null stream, the parameter defaults, the device count and the
// process-wide kernel-variant options.
#include "../../include/trpo_engine.h"
#include "abi_util.h"
#include "kernels.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

using namespace trpo;
using namespace trpo_abi;

extern "C" {

void trpo_default_params(trpo_update_params* p) {
  if (!p) return;
  p->cg_iters = 10;
  p->residual_tol = 1e-10f;
  p->cg_damping = 0.1f;
  p->max_kl = 0.01;
  p->compute_advantages = 0;
  p->gamma = 0.95;
}

void trpo_default_rollout_params(trpo_rollout_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->n_envs = 1;
  p->max_pathlength = 1000;    // config["max_steps"] (trpo_inksci.py:17)
  p->n_timesteps = 1000;       // config["episodes_per_roll"] (trpo_inksci.py:17, used as a step budget)
  p->train = 1;
  p->time_limit = 200;         // CartPole-v0 TimeLimit
  p->seed = 1;
  p->mem = TRPO_MEM_HOST;
}

int trpo_env_info(int env, trpo_env_info_t* out) {
  return guarded([&] {
    REQUIRE(out, "NULL argument");
    EnvDims d{};
    REQUIRE(env_dims(false, env, &d), "unknown environment id " + std::to_string(env));
    std::memset(out, 0, sizeof *out);
    out->obs_dim = d.obs_dim;
    out->state_dim = d.state_dim;
    out->n_actions = d.head_dim;
    out->reset_draws = d.reset_draws;
    out->time_limit = d.time_limit;
    std::strncpy(out->name, d.name, sizeof out->name - 1);
  });
}

int trpo_default_rollout_params_env(int env, trpo_rollout_params* p) {
  return guarded([&] {
    REQUIRE(p, "NULL argument");
    EnvDims d{};
    REQUIRE(env_dims(false, env, &d), "unknown environment id " + std::to_string(env));
    trpo_default_rollout_params(p);
    p->time_limit = d.time_limit;
  });
}

int trpo_env_step(int env, const double* state, const int64_t* action, int64_t n, double* state_out, double* obs_out,
                  double* reward, uint8_t* done, int mem) {
  return guarded([&] {
    EnvDims d{};
    REQUIRE(env_dims(false, env, &d), "unknown environment id " + std::to_string(env));
    REQUIRE(state && action && n >= 0, "bad argument");
    if (n == 0) return;
    Staging st(mem, nullptr);
    const double* ds = st.in(state, (size_t)n * d.state_dim);
    const int64_t* da = st.in(action, (size_t)n);
    double* dso = st.out(state_out, (size_t)n * d.state_dim);
    double* dob = st.out(obs_out, (size_t)n * d.obs_dim);
    double* dr = st.out(reward, (size_t)n);
    launch_env_step(false, env, ds, da, n, dso, dob, dr, st.out(done, (size_t)n), nullptr);
    check_launch();
    st.fetch();
    HIPCHECK(hipDeviceSynchronize());
  });
}

int trpo_cont_env_info(int cenv, trpo_cont_env_info_t* out) {
  return guarded([&] {
    REQUIRE(out, "NULL argument");
    EnvDims d{};
    REQUIRE(env_dims(true, cenv, &d), "unknown continuous environment id " + std::to_string(cenv));
    std::memset(out, 0, sizeof *out);
    out->obs_dim = d.obs_dim;
    out->state_dim = d.state_dim;
    out->act_dim = d.head_dim;
    out->reset_draws = d.reset_draws;
    out->time_limit = d.time_limit;
    std::strncpy(out->name, d.name, sizeof out->name - 1);
  });
}

int trpo_default_rollout_params_cont(int cenv, trpo_rollout_params* p) {
  return guarded([&] {
    REQUIRE(p, "NULL argument");
    EnvDims d{};
    REQUIRE(env_dims(true, cenv, &d), "unknown continuous environment id " + std::to_string(cenv));
    trpo_default_rollout_params(p);
    p->time_limit = d.time_limit;
  });
}

int trpo_cont_env_step(int cenv, const double* state, const float* action, int64_t n, double* state_out,
                       double* obs_out, double* reward, uint8_t* done, int mem) {
  return guarded([&] {
    EnvDims d{};
    REQUIRE(env_dims(true, cenv, &d), "unknown continuous environment id " + std::to_string(cenv));
    REQUIRE(state && action && n >= 0, "bad argument");
    if (n == 0) return;
    Staging st(mem, nullptr);
    const double* ds = st.in(state, (size_t)n * d.state_dim);
    const float* da = st.in(action, (size_t)n * d.head_dim);
    double* dso = st.out(state_out, (size_t)n * d.state_dim);
    double* dob = st.out(obs_out, (size_t)n * d.obs_dim);
    double* dr = st.out(reward, (size_t)n);
    launch_env_step(true, cenv, ds, da, n, dso, dob, dr, st.out(done, (size_t)n), nullptr);
    check_launch();
    st.fetch();
    HIPCHECK(hipDeviceSynchronize());
  });
}

int trpo_device_count(int* out) {
  return guarded([&] {
    REQUIRE(out, "NULL argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    (void)hipGetLastError();
    *out = n;
  });
}

int trpo_cat_sample(const float* prob, int64_t n, int k, const double* r, int64_t* out, int mem) {
  return guarded([&] {
    REQUIRE(prob && r && out && n >= 0 && k >= 1, "bad argument");
    if (n == 0) return;
    Staging st(mem, nullptr);
    const float* dp = st.in(prob, (size_t)n * k);
    const double* dr = st.in(r, (size_t)n);
    launch_cat_sample(dp, n, k, dr, st.out(out, (size_t)n), nullptr);
    check_launch();
    st.fetch();
    HIPCHECK(hipDeviceSynchronize());
  });
}

int trpo_cartpole_step(const double* state, const int64_t* action, int64_t n, double* state_out, double* reward,
                       uint8_t* done, int mem) {
  return guarded([&] {
    REQUIRE(state && action && state_out && n >= 0, "bad argument");
    if (n == 0) return;
    Staging st(mem, nullptr);
    const double* ds = st.in(state, (size_t)n * 4);
    const int64_t* da = st.in(action, (size_t)n);
    double* dso = st.out(state_out, (size_t)n * 4);
    double* dr = st.out(reward, (size_t)n);
    launch_env_step(false, TRPO_ENV_CARTPOLE_V0, ds, da, n, dso, nullptr, dr, st.out(done, (size_t)n), nullptr);
    check_launch();
    st.fetch();
    HIPCHECK(hipDeviceSynchronize());
  });
}

int trpo_discount(const double* x, const uint8_t* starts, int64_t n, double gamma, double* out, int mem) {
  return guarded([&] {
    REQUIRE(x && out, "NULL argument");
    REQUIRE(n >= 0, "n < 0");
    if (n == 0) return;
    Staging st(mem, nullptr);
    const double* dx = st.in(x, (size_t)n);
    const uint8_t* ds = st.in(starts, (size_t)n);
    if (!ds) {   // one path: the scan reads a flag per row
      uint8_t* z = st.tmp<uint8_t>((size_t)n);
      HIPCHECK(hipMemset(z, 0, (size_t)n));
      ds = z;
    }
    launch_discount(dx, ds, n, gamma, st.out(out, (size_t)n), st.tmp<uint8_t>(discount_workspace_bytes(n)), nullptr);
    check_launch();
    HIPCHECK(hipDeviceSynchronize());
    st.fetch();
  });
}

int trpo_gae(const double* rewards, const double* values, const uint8_t* starts, const double* tail_values,
             int64_t n, double gamma, double lambda, double* adv_out, double* returns_out, int mem) {
  return guarded([&] {
    REQUIRE(n >= 0, "n < 0");
    REQUIRE(lambda >= 0.0 && lambda <= 1.0, "lambda must be in [0, 1]");
    if (n == 0) return;
    REQUIRE(rewards, "rewards is NULL");
    Staging st(mem, nullptr);
    const double* dr = st.in(rewards, (size_t)n);
    const double* dv = st.in(values, (size_t)n);
    const uint8_t* ds = st.in(starts, (size_t)n);
    const double* dt = st.in(tail_values, (size_t)n);
    double* da = st.out(adv_out, (size_t)n);
    double* dret = st.out(returns_out, (size_t)n);
    launch_gae(dr, dv, ds, dt, n, gamma, lambda, da, dret, st.tmp<uint8_t>(gae_workspace_bytes(n)), nullptr);
    check_launch();
    HIPCHECK(hipDeviceSynchronize());
    st.fetch();
  });
}

static int* known_option(const char* name) {
  if (int* slot = option_slot(name)) return slot;
  throw ArgError(std::string("unknown option ") + name);
}

int trpo_plane_rows_ok(int64_t x_mpad, int* rfwd01_ok, int* pair_planes_ok) {
  return guarded([&] {
    REQUIRE(rfwd01_ok && pair_planes_ok, "NULL argument");
    *rfwd01_ok = rfwd01_rows_ok(x_mpad) ? 1 : 0;
    *pair_planes_ok = pair_planes_rows_ok(x_mpad) ? 1 : 0;
  });
}

int trpo_set_option(const char* name, int value) {
  return guarded([&] {
    REQUIRE(name, "NULL argument");
    *known_option(name) = value;
  });
}

int trpo_get_option(const char* name, int* value) {
  return guarded([&] {
    REQUIRE(name && value, "NULL argument");
    *value = *known_option(name);
  });
}

}  // extern "C"
