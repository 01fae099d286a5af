// The process-wide kernel-variant options (kernels.h Options): their names, environment variables and defaults.
#include "kernels.h"

#include <cstdlib>
#include <cstring>

namespace trpo {
namespace {

// One row per field of Options: g_options starts from the defaults, each overridden by its environment variable,
// and option_slot finds a field by its name.
struct OptionRow {
  const char* name;
  const char* env;
  int Options::*field;
  int dflt;
};
constexpr OptionRow kOptionRows[] = {
    {"split_mfma", "TRPO_SPLIT_MFMA", &Options::split_mfma, 5},
    {"split_wg", "TRPO_SPLIT_WG", &Options::split_wg, 1},
    {"chain", "TRPO_CHAIN", &Options::chain, 1},
    {"split_f16", "TRPO_SPLIT_F16", &Options::split_f16, 1},
    {"split_min_k", "TRPO_SPLIT_MIN_K", &Options::split_min_k, 0},
    {"graphs", "TRPO_GRAPHS", &Options::graphs, 1},
    {"tail", "TRPO_TAIL", &Options::tail, 1},
    {"fused", "TRPO_FUSED", &Options::fused, 3},
    {"low_seg", "TRPO_LOW_SEG", &Options::low_seg, 14},
    {"planes", "TRPO_PLANES", &Options::planes, 1},
    {"rbwd0", "TRPO_RBWD0", &Options::rbwd0, 1},
    {"hbwd2", "TRPO_HBWD2", &Options::hbwd2, 2},
    {"head_fwd", "TRPO_HEAD_FWD", &Options::head_fwd, 1},
    {"splits", "TRPO_SPLITS", &Options::splits, 0},
    {"pg_splits", "TRPO_PG_SPLITS", &Options::pg_splits, 0},
    {"ls_fused", "TRPO_LS_FUSED", &Options::ls_fused, 1},
    {"cg_fuse_reduce", "TRPO_CG_FUSE_REDUCE", &Options::cg_fuse_reduce, 1},
    {"cg_p_img", "TRPO_CG_P_IMG", &Options::cg_p_img, 1},
    {"rfwd01", "TRPO_RFWD01", &Options::rfwd01, 1},
    {"fwd01", "TRPO_FWD01", &Options::fwd01, 1},
    {"rh1_planes", "TRPO_RH1_PLANES", &Options::rh1_planes, 1},
    {"rbwd0_bdma", "TRPO_RBWD0_BDMA", &Options::rbwd0_bdma, 1},
};
static_assert(sizeof kOptionRows / sizeof kOptionRows[0] == sizeof(Options) / sizeof(int),
              "every field of Options needs a row");

Options options_from_env() {
  Options o{};
  for (const OptionRow& r : kOptionRows) {
    const char* e = std::getenv(r.env);
    o.*r.field = e ? std::atoi(e) : r.dflt;
  }
  return o;
}

}  // namespace

Options g_options = options_from_env();

int* option_slot(const char* name) {
  for (const OptionRow& r : kOptionRows)
    if (!std::strcmp(name, r.name)) return &(g_options.*r.field);
  return nullptr;
}

}  // namespace trpo
