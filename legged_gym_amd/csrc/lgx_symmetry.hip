// Left-right symmetry augmentation of the PPO rollout storage (lgx.h: lgx_ppo_symmetry_augment;
// rsl_rl 2.x symmetry_cfg.use_data_augmentation; tables: envs/base/symmetry.py).
//
// One launch writes, for r in [0, rows), row dst_row + r of every array the update reads from row
// src_row + r: observations and privileged observations through their signed permutations
// (mirror(x)[c] = sign[c] * x[perm[c]]), actions and mu through the action table, sigma through the
// action permutation alone, and the four per-row scalars copied.  The update kernels then run
// unchanged over twice the rows.
//
// Shape of gather_rows_padded_kernel (lgx_gemm.hip): a row per wave, four workgroup rows, per pass of
// 256 columns four clamped (always valid) table entries and then four source values in flight per
// lane, then the predicated stores.  A copy and a sign flip: every output bit is decided by the
// tables, not by the grid.  Source and destination rows are disjoint (checked), so no row is read
// after it is written.
#include <stdio.h>

#include "lgx_device.h"
#include "lgx_internal.h"

#define SYM_TPB 256
#define SYM_ROWS (SYM_TPB / 64)   // rows per workgroup: one per wave
static_assert(sizeof(lgx_symmetry_args) == 160, "lgx_symmetry_args: sim/abi.py LgxSymmetryArgs mirrors this layout");

namespace {

// d[c] = sign[c] * s[perm[c]] for c in [0, width)
__device__ __forceinline__ void mirror_row(const float* s, float* d, const int32_t* __restrict__ perm,
                                           const float* __restrict__ sign, int width, int lane) {
  for (int c0 = 0; c0 < width; c0 += 256) {
    int p[4];
    float g[4], v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = min(c0 + 64 * i + lane, width - 1);
      p[i] = perm[c];
      g[i] = sign[c];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = s[p[i]];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = c0 + 64 * i + lane;
      if (c < width) d[c] = g[i] * v[i];
    }
  }
}

__global__ void __launch_bounds__(SYM_TPB) symmetry_augment_kernel(const lgx_symmetry_args a) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * SYM_ROWS + wave;
  if (r >= a.rows) return;
  const int64_t sr = a.src_row + r, dr = a.dst_row + r;
  const int A = a.num_actions;
  // the narrow arrays first: their loads are in flight while the wide rows are walked
  const int ca = min(lane, A - 1);
  const int pa = a.act_perm[ca];
  const float ga = a.act_sign[ca];
  const float act = a.actions[sr * A + pa], mu = a.mu[sr * A + pa], sg = a.sigma[sr * A + pa];
  float scal = 0.f;
  float* sp = lane == 0 ? a.actions_log_prob : lane == 1 ? a.advantages : lane == 2 ? a.values : a.returns;
  if (lane < 4) scal = sp[sr];
  mirror_row(a.observations + sr * a.num_obs, a.observations + dr * a.num_obs, a.obs_perm, a.obs_sign, a.num_obs,
             lane);
  if (a.privileged_observations)
    mirror_row(a.privileged_observations + sr * a.num_cobs, a.privileged_observations + dr * a.num_cobs, a.cobs_perm,
               a.cobs_sign, a.num_cobs, lane);
  if (lane < A) {
    a.actions[dr * A + lane] = ga * act;
    a.mu[dr * A + lane] = ga * mu;
    a.sigma[dr * A + lane] = sg;
  }
  if (lane < 4) sp[dr] = scal;
}

}  // namespace

extern "C" int lgx_ppo_symmetry_check_table(const int32_t* perm, const float* sign, int32_t width) {
  char msg[160];
  if (!perm || !sign) return lgx_fail(LGX_EINVAL, "lgx_ppo_symmetry_check_table: null table");
  if (width < 1 || width > LGX_MAX_PRIV_OBS)
    return lgx_fail(LGX_EINVAL, "lgx_ppo_symmetry_check_table: width outside [1, LGX_MAX_PRIV_OBS]");
  for (int32_t c = 0; c < width; ++c) {
    if (perm[c] < 0 || perm[c] >= width) {
      snprintf(msg, sizeof msg, "lgx_ppo_symmetry_check_table: perm[%d] = %d outside [0, %d)", c, perm[c], width);
      return lgx_fail(LGX_EINVAL, msg);
    }
    if (sign[c] != 1.f && sign[c] != -1.f) {
      snprintf(msg, sizeof msg, "lgx_ppo_symmetry_check_table: sign[%d] = %g is not +-1", c, (double)sign[c]);
      return lgx_fail(LGX_EINVAL, msg);
    }
  }
  return LGX_OK;
}

extern "C" int lgx_ppo_symmetry_augment(const lgx_symmetry_args* args, void* stream) {
  char msg[160];
  auto fail = [&](const char* what) {
    snprintf(msg, sizeof msg, "lgx_ppo_symmetry_augment: %s", what);
    return lgx_fail(LGX_EINVAL, msg);
  };
  if (!args) return fail("null args");
  const lgx_symmetry_args& a = *args;
  if (a.rows < 1) return fail("rows < 1");
  if (a.src_row < 0 || a.dst_row < 0) return fail("negative src_row or dst_row");
  if ((a.src_row < a.dst_row ? a.dst_row - a.src_row : a.src_row - a.dst_row) < a.rows)
    return fail("source and destination rows overlap");
  if (a.num_obs < 1 || a.num_obs > LGX_MAX_PRIV_OBS) return fail("num_obs outside [1, LGX_MAX_PRIV_OBS]");
  if (a.num_actions < 1 || a.num_actions > LGX_PPO_MAX_ACTIONS)
    return fail("num_actions outside [1, LGX_PPO_MAX_ACTIONS]");
  if (!a.observations || !a.obs_perm || !a.obs_sign) return fail("null observations or observation table");
  if (a.privileged_observations) {
    if (a.num_cobs < 1 || a.num_cobs > LGX_MAX_PRIV_OBS) return fail("num_cobs outside [1, LGX_MAX_PRIV_OBS]");
    if (!a.cobs_perm || !a.cobs_sign) return fail("privileged observations without their table");
  }
  if (!a.actions || !a.mu || !a.sigma || !a.act_perm || !a.act_sign)
    return fail("null actions, mu, sigma or action table");
  if (!a.actions_log_prob || !a.advantages || !a.values || !a.returns)
    return fail("null actions_log_prob, advantages, values or returns");
  const int64_t blocks = (a.rows + SYM_ROWS - 1) / SYM_ROWS;
  if (blocks > 0x7fffffff) return fail("too many rows for one launch");
  hipLaunchKernelGGL(symmetry_augment_kernel, dim3((uint32_t)blocks), dim3(SYM_TPB), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return lgx_hip_status("lgx_ppo_symmetry_augment");
}
