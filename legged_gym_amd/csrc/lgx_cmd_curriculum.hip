// Command curriculum on the device (legged_robot.py:165-167, 189-190, 465-474): widen lin_vel_x once
// the envs that reset in a curriculum step track their velocity command well, and give those same
// envs their new command from the widened range.  A translation unit of its own: the post-physics,
// reset and physics kernels are not touched and stay the machine code they were
// (tools/kernel_code_diff.py).
//
// Two launches, enqueued by the entry points of lgx_api.hip after their post-physics / reset launch
// on curriculum steps only (common_step_counter % max_episode_length == 0, decided on the host):
//   decide  one wave.  Re-reduces the reset count and the tracking_lin_vel row from the block
//           partials that launch left in lgx_buffers.scratch, in extras_finalize_body's order (lane l
//           takes blocks l, l + 64, ..., then the xor butterfly), so the mean is the one the episode
//           extras publish.  Compares, clips, writes `state`; on a change the device params' range
//           and the `changed` flag.  Plain stores, one writer.
//   patch   one lane per env (or per listed id).  Returns at once unless `changed`.  Redraws the
//           reset's command from the same counters (LGX_DRAW_RESET_CMD, this step, the reset's tag,
//           or the injected draws) with the new x range and resample_cmd's gate, and writes
//           commands[e, 0:2] and every published copy of them: obs columns 9, 10, the obs part of a
//           bound history row, the clean part of a bound privileged row.
// Two launches because one grid would race: one workgroup would write the range while the others
// still read the old one.  The launch boundary also makes the new range visible to every later
// launch, whose reads of the params may go through the scalar cache.
#include "lgx_device.h"
#include "lgx_internal.h"

namespace {

struct Draws {   // lgx_envlogic.hip's: the in-kernel Philox stream or the injected rows
  const lgx_env_params* P;
  const float* inj;
  int32_t stride;
  LGX_DEV float operator()(int e, int slot, int64_t step, uint32_t tag) const {
    return inj ? inj[(int64_t)e * stride + slot] : lgx_uniform(P->seed, e, slot, step, tag);
  }
  LGX_DEV void quad(int e, int q, int64_t step, uint32_t tag, float u[4]) const {
    if (inj) {
#pragma unroll
      for (int k = 0; k < 4; ++k) u[k] = 4 * q + k < stride ? inj[(int64_t)e * stride + 4 * q + k] : 0.f;
    } else {
      lgx_uniform4(P->seed, e, q, step, tag, u);
    }
  }
};

}  // namespace

__global__ void __launch_bounds__(64)
lgx_cmd_curriculum_decide_kernel(lgx_env_params* P, const float* scratch, int32_t nblocks, int32_t count_row,
                                 lgx_cmdcur_args cc) {
  const int lane = threadIdx.x;
  float cnt = 0.f, sum = 0.f;
  for (int b = lane; b < nblocks; b += 64) {
    cnt += scratch[(int64_t)b * LGX_PARTIAL_STRIDE + count_row];
    sum += scratch[(int64_t)b * LGX_PARTIAL_STRIDE + cc.row];
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    cnt += __shfl_xor(cnt, m);
    sum += __shfl_xor(sum, m);
  }
  if (lane != 0) return;
  int32_t changed = 0;
  if (cnt > 0.f) {   // len(env_ids) > 0
    // mean(episode_sums[env_ids]) / max_episode_length > 0.8 * scale, all float32 (:470)
    const float lhs = (sum / cnt) / P->max_episode_length;
    float lo = P->cmd_ranges[0][0], hi = P->cmd_ranges[0][1];
    float n = cc.state[2];
    if (lhs > cc.threshold) {   // np.clip(x, a, b) = min(max(x, a), b) (:471-472)
      const float nlo = fminf(fmaxf(lo - 0.5f, -cc.max_curriculum), 0.f);
      const float nhi = fminf(fmaxf(hi + 0.5f, 0.f), cc.max_curriculum);
      if (nlo != lo || nhi != hi) {
        changed = 1;
        lo = nlo;
        hi = nhi;
        n += 1.f;
        P->cmd_ranges[0][0] = lo;
        P->cmd_ranges[0][1] = hi;
      }
    }
    cc.state[0] = lo;
    cc.state[1] = hi;
    cc.state[2] = n;
    cc.state[3] = lhs;
  }
  *cc.changed = changed;
}

__global__ void __launch_bounds__(64)
lgx_cmd_curriculum_patch_kernel(const lgx_env_params* P, lgx_cmdcur_patch_args a) {
  if (*a.changed == 0) return;
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= a.n) return;
  int e = k;
  if (a.ids) e = a.ids[k];            // lgx_reset_idx: every listed env was reset
  else if (!a.reset[e]) return;       // the post-physics launch's reset flags
  const int nobs = P->num_obs;
  const Draws D{P, a.draws, LGX_DRAW_NOISE + nobs};
  // resample_cmd's x and y draws and its small-command gate (legged_robot.py:360-368); the yaw /
  // heading draw does not depend on the x range
  float c[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float lo = P->cmd_ranges[i][0], hi = P->cmd_ranges[i][1];
    c[i] = (hi - lo) * D(e, LGX_DRAW_RESET_CMD + i, a.step, a.tag) + lo;
  }
  const float keep = sqrtf(c[0] * c[0] + c[1] * c[1]) > 0.2f ? 1.0f : 0.0f;
  c[0] *= keep; c[1] *= keep;
  a.commands[(int64_t)e * 4 + 0] = c[0];
  a.commands[(int64_t)e * 4 + 1] = c[1];
  if (!a.obs) return;
  // the observation launch's expression for entries 9, 10 (phase C of post_physics_body): scale,
  // noise (its scale is zero here: lgx_bind_command_curriculum), clip
  const float clip = P->clip_obs, mul = P->obs_scale_lin_vel;
  const bool noise = P->add_noise != 0;
  float nz[4] = {0.5f, 0.5f, 0.5f, 0.5f};
  if (noise) D.quad(e, (LGX_DRAW_NOISE >> 2) + 2, a.step, 0u, nz);   // entries 8 .. 11
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float v = c[i];
    float o = (v - 0.f) * mul;
    if (a.priv) a.priv[(int64_t)e * a.priv_width + 9 + i] = clampf(o, -clip, clip);
    if (noise) o += (2.f * nz[1 + i] - 1.f) * P->noise_scale_vec[9 + i];
    const float w = clampf(o, -clip, clip);
    a.obs[(int64_t)e * nobs + 9 + i] = w;
    if (a.hist) a.hist[(int64_t)e * a.hist_width + 9 + i] = w;
  }
}

// state = {lo, hi, 0, 0} from the device's own range (lgx_bind_command_curriculum)
__global__ void lgx_cmd_curriculum_init_kernel(const lgx_env_params* P, float* state) {
  state[0] = P->cmd_ranges[0][0];
  state[1] = P->cmd_ranges[0][1];
  state[2] = 0.f;
  state[3] = 0.f;
}

__global__ void lgx_set_command_range_kernel(lgx_env_params* P, int32_t k, float lo, float hi, float* state) {
  P->cmd_ranges[k][0] = lo;
  P->cmd_ranges[k][1] = hi;
  if (state) { state[0] = lo; state[1] = hi; }
}

int lgx_launch_cmd_curriculum(lgx_env_params* dp, const float* scratch, int32_t nblocks, int32_t count_row,
                              const lgx_cmdcur_args& cc, const lgx_cmdcur_patch_args& pa, hipStream_t stream) {
  if (nblocks <= 0 || pa.n <= 0) return 0;
  hipLaunchKernelGGL(lgx_cmd_curriculum_decide_kernel, dim3(1), dim3(64), 0, stream, dp, scratch, nblocks, count_row, cc);
  hipLaunchKernelGGL(lgx_cmd_curriculum_patch_kernel, dim3((pa.n + 63) / 64), dim3(64), 0, stream,
                     (const lgx_env_params*)dp, pa);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int lgx_launch_cmd_curriculum_init(const lgx_env_params* dp, float* state, hipStream_t stream) {
  hipLaunchKernelGGL(lgx_cmd_curriculum_init_kernel, dim3(1), dim3(1), 0, stream, dp, state);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int lgx_launch_set_command_range(lgx_env_params* dp, int32_t k, float lo, float hi, float* state, hipStream_t stream) {
  hipLaunchKernelGGL(lgx_set_command_range_kernel, dim3(1), dim3(1), 0, stream, dp, k, lo, hi, state);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
