// Internal (non-ABI) declarations shared by the lgx HIP translation units.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "../../include/lgx.h"

#define LGX_MAX_LANE_PTS 24   // contact candidates per leg lane (Go1: 23)

// device-resident model: the ABI model + the per-lane (per-leg) contact candidate tables
struct lgx_dev_model {
  lgx_model m;
  int32_t lane_npts[4];
  int32_t max_lane_npts;
  int32_t joint_rot_eye;   // every joint frame rotation is the identity (URDF rpy = 0: the quadrupeds but ANYmal C)
  int32_t lane_pts[4][LGX_MAX_LANE_PTS];
  int32_t pad_tail[(4 - (sizeof(lgx_model) / 4 + 6 + 4 * LGX_MAX_LANE_PTS) % 4) % 4];   // 16-byte multiple
};

int lgx_launch_ground_contact(const lgx_env_params* dp, const lgx_buffers& b, const float* q, int32_t n, float* o,
                              hipStream_t stream);
int lgx_physics_pp(int32_t n_envs);   // lanes per leg of the physics launch at n_envs (LGX_PHYS_PP overrides)
// frozen != 0: only the drive inputs of `nsub` substeps (clip, targets, actuator-net history and
// model_ins rows) with the state held fixed (lgx_drive_inputs)
// pp: lanes per leg (lgx_physics_pp at lgx_sim_create)
// tm_mode: the stage-2 form of the corrected-trimesh queue (LGX_TM_STAGE2 at lgx_sim_create): the
// automatic rule, or one form for every queue length - 16 lanes per sphere, one lane per sphere, one
// lane per (sphere, cell, triangle).  Every form gives the same bits.
enum { LGX_TM_AUTO = 0, LGX_TM_ROWS = 1, LGX_TM_LANE = 2, LGX_TM_PACKED = 3 };
int lgx_launch_physics(const lgx_dev_model* dm, const lgx_env_params* dp, const lgx_buffers& b, int32_t n_envs,
                       int32_t nsub, int32_t from_actions, const float* act_src, hipStream_t stream, int32_t frozen,
                       int pp, int32_t tm_mode);
// the per-env actuator tables of a sim (lgx_bind_actuator_rand, checked there), passed by value to
// the physics launches of a sim that bound them; prev == nullptr: nothing bound.  kp_scale / kd_scale
// [N,12] and lag [N] are the caller's (each may be nullptr: 1, 1, 0), prev [N,12] is the sim's: the
// clipped actions of the last launch that took actions
struct lgx_act_rand_args {
  const float* kp_scale;
  const float* kd_scale;
  const int32_t* lag;
  float* prev;
};
// the same launch with the tables bound (ar.prev != nullptr; lgx_physics_rand.hip): the
// lgx_physics_kernel<PP, lgx_act_rand_args> instantiations
int lgx_launch_physics_rand(const lgx_dev_model* dm, const lgx_env_params* dp, const lgx_buffers& b, int32_t n_envs,
                            int32_t nsub, int32_t from_actions, const float* act_src, hipStream_t stream,
                            int32_t frozen, int pp, int32_t tm_mode, const lgx_act_rand_args& ar);
// the dense joint-space kernel (lgx_physics.hip): leg_dof == 6 robots, or any with LGX_PHYS_DENSE=1
int lgx_launch_physics_dense(const lgx_dev_model* dm, const lgx_env_params* dp, const lgx_buffers& b, int32_t n_envs,
                             int32_t nsub, int32_t from_actions, const float* act_src, hipStream_t stream,
                             int32_t frozen, int32_t num_points);
// the privileged-observation row of a sim (lgx_bind_privileged_obs, checked there), passed by value
// to the post-physics launches; buf == nullptr: nothing bound.  Term t's id is 4 bits and its first
// column 16 bits of packed words, not arrays: a kernel argument indexed by a loop variable is kept
// in scratch memory.
struct lgx_priv_args {
  float* buf;            // [N, width]
  int32_t width, num_terms;
  uint32_t ids;          // term t: bits [4t, 4t + 4)
  uint32_t pad;
  uint64_t offs_lo, offs_hi;   // term t < 4: bits [16t, 16t + 16) of offs_lo; else of offs_hi, t - 4
  float cf_scale, tq_scale;
  __host__ __device__ int id(int t) const { return (int)((ids >> (4 * t)) & 15u); }
  __host__ __device__ int off(int t) const { return (int)(((t < 4 ? offs_lo : offs_hi) >> (16 * (t & 3))) & 0xffffu); }
  void set(int t, int id_, int off_) {
    ids |= (uint32_t)id_ << (4 * t);
    (t < 4 ? offs_lo : offs_hi) |= (uint64_t)off_ << (16 * (t & 3));
  }
};
static_assert(LGX_PRIV_MAX_TERMS <= 8 && LGX_PRIV_COUNT <= 16 && LGX_MAX_PRIV_OBS < 65536, "lgx_priv_args packing");
// the observation history of a sim (lgx_bind_obs_history, checked there), passed by value to the
// post-physics launches; row == nullptr: nothing bound.  age: the sim's int32[N] (lgx.h)
struct lgx_hist_args {
  float* row;            // [N, width]: this launch's output
  const float* prev;     // [N, width]: the previous launch's row, != row
  int32_t* age;
  int32_t frames, frame_width, width;
};
// the Go1 actuator net's share of a post-physics launch: `rows` rows of `in` -> `out` on persistent
// workgroups behind the post-physics ones (lgx_actuator_mlp's arguments)
struct lgx_act_launch {
  const float* in;
  float* out;
  int64_t rows;
  const float* w;
  const float* scale;
};
// The post-physics launch, one kernel out of eight: act == nullptr: no actuator workgroups;
// pv.buf == nullptr and hv.row == nullptr: the kernels of a sim with neither bound (no other kernel
// argument or code), otherwise the instantiation with the privileged row, the history or both.
int lgx_launch_post_physics(const lgx_env_params* dp, const lgx_buffers& b, int32_t n_envs, int64_t step,
                            const float* draws, float* extras_snapshot, const lgx_act_launch* act,
                            const lgx_priv_args& pv, const lgx_hist_args& hv, hipStream_t stream);
// its choice among the four history kernels (hv.row != nullptr), which live in lgx_envlogic_hist.hip
int lgx_post_physics_hist_select(const lgx_env_params* dp, const lgx_buffers& b, int32_t n_envs, int64_t step,
                                 const float* draws, float* extras_snapshot, const lgx_act_launch* act,
                                 const lgx_priv_args& pv, const lgx_hist_args& hv, hipStream_t stream);
// hist_age: the bound history's ages (zeroed for the listed envs) or nullptr
int lgx_launch_reset_idx(const lgx_env_params* dp, const lgx_buffers& b, const int32_t* ids, int32_t n, int64_t step,
                         int32_t init_done, const float* draws, float* extras_snapshot, int32_t* hist_age,
                         hipStream_t stream);
// the command curriculum of a sim (lgx_bind_command_curriculum, checked there), passed by value to
// the decide launch; state == nullptr: nothing bound.  changed: the sim's device int32, written by
// every decide launch (1: the range moved) and read by the patch launch behind it
struct lgx_cmdcur_args {
  float* state;          // the caller's float[4]: lo, hi, number of widenings, last left-hand side
  int32_t* changed;
  float max_curriculum, threshold;
  int32_t row;           // tracking_lin_vel's row of the block partials (= of episode_sums)
};
// what the patch launch rewrites for the envs that reset in this step: n = num_envs and the reset
// flags (post-physics routes), or the n listed ids (lgx_reset_idx; reset unused); obs == nullptr:
// commands only, else obs and, where bound, the history row (hist) and the privileged row (priv)
struct lgx_cmdcur_patch_args {
  const int32_t* changed;
  const uint8_t* reset;
  const int32_t* ids;
  int32_t n;
  uint32_t tag;          // the Philox tag of the reset's draws: 0 post-physics, 1 lgx_reset_idx
  int64_t step;
  const float* draws;    // injected draws or nullptr
  float* commands;
  float* obs;
  float* hist;
  float* priv;
  int32_t hist_width, priv_width;
};
// lgx_cmd_curriculum.hip: decide (one wave over the nblocks partial rows of the launch before it;
// count_row = the reset-count row) + patch; nothing is launched for nblocks <= 0 or pa.n <= 0
int lgx_launch_cmd_curriculum(lgx_env_params* dp, const float* scratch, int32_t nblocks, int32_t count_row,
                              const lgx_cmdcur_args& cc, const lgx_cmdcur_patch_args& pa, hipStream_t stream);
int lgx_launch_cmd_curriculum_init(const lgx_env_params* dp, float* state, hipStream_t stream);
// cmd_ranges[k] = {lo, hi} in the device params, and state[0:2] when state != nullptr
int lgx_launch_set_command_range(lgx_env_params* dp, int32_t k, float lo, float hi, float* state, hipStream_t stream);
// wg_per_cu: persistent workgroups per CU of the weight-stationary kernel (2 when it owns the
// chip, 1 when it shares the CUs with concurrent work on another stream)
int lgx_launch_actuator_mlp(const float* in, float* out, int64_t rows, const float* w, const float* out_scale,
                            hipStream_t stream, int wg_per_cu = 2);
int lgx_launch_actuator_lstm(const float* x, float* h, float* c, float* tau, int64_t m, const float* w,
                             hipStream_t stream);
int lgx_launch_mlp_forward(const float* x, float* y, int64_t rows, int32_t nl, const int32_t* dims,
                           const float* const* weights, const float* const* biases, int32_t act, hipStream_t stream);

int lgx_launch_mlp_forward2(const lgx_mlp_desc* d, int32_t count, hipStream_t stream);
int lgx_launch_gae(const float* rew, const float* val, const uint8_t* dones, const float* last_val, float* ret,
                   float* adv, int32_t T, int32_t N, float gamma, float lam, hipStream_t stream);
int lgx_launch_gae_parts(const float* rew, const float* val, const uint8_t* dones, const float* last_val, float* ret,
                         float* adv, int32_t T, int32_t N, float gamma, float lam, double* parts, hipStream_t stream);
int lgx_launch_adv_norm(float* adv, int64_t n, const double* parts, int32_t nparts, hipStream_t stream);
int lgx_launch_gae_norm(const float* rew, const float* val, const uint8_t* dones, const float* last_val, float* ret,
                        float* adv, int32_t T, int32_t N, float gamma, float lam, double* scratch, hipStream_t stream);

// Kernel-tight timing for lgx_profile_*: when the caller arms a (start, stop) event pair, the
// next LGX_LAUNCH on this thread is dispatched with hipExtLaunchKernelGGL, which records the
// events on the kernel's own dispatch (no host launch latency inside the interval).
struct lgx_timing_slot { hipEvent_t start = nullptr, stop = nullptr; };
extern thread_local lgx_timing_slot lgx_timing;
#define LGX_LAUNCH(kern, grid, block, shmem, stream, ...)                                          \
  do {                                                                                           \
    if (lgx_timing.start || lgx_timing.stop) {                                                   \
      hipExtLaunchKernelGGL(kern, grid, block, shmem, stream, lgx_timing.start, lgx_timing.stop, 0, \
                            __VA_ARGS__);                                                        \
      lgx_timing = lgx_timing_slot{};                                                            \
    } else {                                                                                     \
      hipLaunchKernelGGL(kern, grid, block, shmem, stream, __VA_ARGS__);                         \
    }                                                                                            \
  } while (0)

// error reporting shared by the translation units (thread-local message, lgx_last_error)
int lgx_fail(int code, const char* msg);
// lgx_gemm_split.hip: the split-bf16 path of lgx_gemm_nt (arguments already checked)
int lgx_gemm_nt_split(const lgx_gemm_args& a, int cus, void* stream);
// lgx_gemm_x3p.hip: pipelined split-bf16 path (pre-split B, K % 32 == 0)
int lgx_gemm_nt_x3p(const lgx_gemm_args& a, int cus, void* stream);
int lgx_hip_status(const char* what);  // LGX_OK or LGX_EHIP from hipGetLastError()

// a batch of reduction jobs passed by value to one launch (lgx_reduce_slices)
struct lgx_reduce_jobs {
  lgx_reduce_job job[LGX_MAX_REDUCE_JOBS];
  int32_t tile_start[LGX_MAX_REDUCE_JOBS];    // first tile of each job in the flat grid
  int32_t tile_outputs[LGX_MAX_REDUCE_JOBS];  // outputs per tile (16 or 64)
};

// scratch layout (floats): [blocks][LGX_MAX_TERMS + 2] reduction partials
#ifndef LGX_ENV_BLOCK
#define LGX_ENV_BLOCK 16  // envs per post-physics workgroup (16 lanes each)
#endif
#define LGX_PARTIAL_STRIDE (LGX_MAX_TERMS + 2)

#ifdef __HIPCC__
// ELU (alpha 1) of the policy networks: exp(x) - 1 on v_exp_f32 for x <= 0.  Absolute error
// <= ~1.2e-7 against torch's expm1 (a few ulp of 1; relative error grows only where the output
// is tiny, |x| < 2^-8); libm's expm1f costs ~10x more VALU, which in the GEMM epilogues competes
// with the operand splits for the MFMA issue gaps (measured: layer-1 forward 54 -> 61 us with
// an expm1-accurate polynomial form).
__device__ __forceinline__ float lgx_elu(float x) { return x > 0.f ? x : __expf(x) - 1.f; }
// Normal(mu, sd).sample() from a standard-normal draw (torch.normal = normal_(0, 1) * std + mu) and
// the log-prob term of one action dimension (Normal.log_prob); shared by lgx_ppo_act and the
// rollout MLP's fused act epilogue so both write bit-identical rows.  Explicit fma, no contraction.
__device__ __forceinline__ float lgx_ppo_sample(float mu, float sd, float eps) { return __builtin_fmaf(sd, eps, mu); }
__device__ __forceinline__ float lgx_ppo_logp_term(float d, float sd) {
#pragma clang fp contract(off)
  const float half_log_2pi = 0.91893853320467274178f;
  return -(d * d) / (2.f * sd * sd) - logf(sd) - half_log_2pi;
}
// PPO.process_env_step's time-out bootstrap: rew + gamma * (V * time_out), as torch evaluates it
__device__ __forceinline__ float lgx_ppo_reward(float rew, float gamma, float value, bool time_out) {
#pragma clang fp contract(off)
  return rew + gamma * (value * (time_out ? 1.f : 0.f));
}
#endif
