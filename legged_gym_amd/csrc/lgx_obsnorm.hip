// Empirical observation normalisation (lgx.h: lgx_obs_norm_partials / lgx_obs_norm_apply): a
// running float64 (count, mean, M2) per observation column, updated from each env step's [N, D]
// batch and applied to it, for up to LGX_OBS_NORM_MAX_JOBS buffers (actor and critic rows) per launch.
//
// Two launches, no atomics, every output has exactly one writer:
//   partials: one thread per (block of LGX_OBS_NORM_ROWS rows, column) sums its rows in ascending
//             order, then their squared deviations from the block mean (the rows stay in registers
//             between the two passes; coalesced across columns, no cross-lane reduction);
//   apply:    one thread per (row tile, column) folds the partials into the state in ascending
//             order (Chan's combine, as moments_combine of lgx_rl.hip), derives the f32 mean and
//             1 / (std + eps) from those registers, and normalises its tile's rows of that column.
//             Every workgroup repeats the fold of its columns (no workgroup waits for another; the
//             weights n_b / n, which the counts alone decide, once per workgroup in LDS);
//             the first row tile writes the new state to state_out != state_in.
// Everything a result depends on is fixed by (rows, width) and the order of the partials, not by the
// grid: the same partials give the same state and the same y wherever they were computed.
#include <stdio.h>

#include "lgx_device.h"
#include "lgx_internal.h"

#define ON_TPB 256
#define ON_R LGX_OBS_NORM_ROWS
#define ON_APPLY_ROWS 32   // rows per workgroup of the apply launch
#define ON_FOLD 32         // partials whose loads are issued together in the fold

struct lgx_obs_norm_jobs {
  lgx_obs_norm_job job[LGX_OBS_NORM_MAX_JOBS];
  int32_t wg_start[LGX_OBS_NORM_MAX_JOBS + 1];   // first workgroup of each job in the flat grid
  int32_t col_chunks[LGX_OBS_NORM_MAX_JOBS];     // ceil(width / ON_TPB)
};

// part layout (doubles), per block: [0] n, [1 .. D] mean, [1 + D .. 2D] M2 (the state's layout too)
__global__ void __launch_bounds__(ON_TPB) lgx_obs_norm_partials_kernel(const lgx_obs_norm_jobs js, int32_t njobs) {
  const int j = (njobs > 1 && (int)blockIdx.x >= js.wg_start[1]) ? 1 : 0;
  const lgx_obs_norm_job jb = j ? js.job[1] : js.job[0];   // (by value: an indexed kernel argument goes to scratch)
  const int wg = (int)blockIdx.x - js.wg_start[j];
  const int chunks = js.col_chunks[j];
  const int64_t blk = wg / chunks;
  const int c = (wg % chunks) * ON_TPB + (int)threadIdx.x;
  const int D = jb.width;
  if (c >= D) return;
  const int64_t r0 = blk * ON_R;
  const int nr = (int)(jb.rows - r0 < ON_R ? jb.rows - r0 : ON_R);   // (uniform over the workgroup)
  const float* __restrict__ x = jb.x + r0 * D + c;
  float v[ON_R];
#pragma unroll
  for (int i = 0; i < ON_R; ++i) v[i] = i < nr ? x[(int64_t)i * D] : 0.f;
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < ON_R; ++i)
    if (i < nr) sum += (double)v[i];
  const double mean = sum / (double)nr;
  double m2 = 0.0;
#pragma unroll
  for (int i = 0; i < ON_R; ++i)
    if (i < nr) {
      const double d = (double)v[i] - mean;
      m2 = fma(d, d, m2);
    }
  double* __restrict__ p = jb.parts + blk * (1 + 2 * (int64_t)D);
  if (c == 0) p[0] = (double)nr;
  p[1 + c] = mean;
  p[1 + D + c] = m2;
}

// One batch of the fold: the loads of its (up to) ON_FOLD partials are issued together, so the
// serial fold pays one memory latency per batch, not per partial; the chunk's first batch (kb == 0)
// derives the chunk's weights while its loads are in flight.  s_g[ON_TPB]: the count after the chunk.
template <bool FULL>
__device__ __forceinline__ void on_fold_batch(const double* __restrict__ p, int64_t stride, int c, int D, int nk,
                                              int kb, int chunk, int t, double nb, double n, double& mean,
                                              double& m2, double* s_nb, double* s_w, double* s_g) {
  double pm[ON_FOLD], pq[ON_FOLD];
#pragma unroll
  for (int u = 0; u < ON_FOLD; ++u) {
    pm[u] = FULL || u < nk ? p[u * stride + 1 + c] : 0.0;
    pq[u] = FULL || u < nk ? p[u * stride + 1 + D + c] : 0.0;
  }
  if (kb == 0) {
    s_nb[t] = nb;
    __syncthreads();
    if (t < chunk) {
      double before = n;   // counts are integers: their float64 sums are exact in any order
      for (int i = 0; i < t; ++i) before += s_nb[i];
      const double tot = before + nb;
      const double w = tot > 0.0 ? nb / tot : 0.0;
      s_w[t] = w;
      s_g[t] = before * w;
      if (t == chunk - 1) s_g[ON_TPB] = tot;
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < ON_FOLD; ++u)
    if (FULL || u < nk) {
      const double d = pm[u] - mean;
      mean = fma(d, s_w[kb + u], mean);
      m2 = (m2 + pq[u]) + d * d * s_g[kb + u];
    }
}

// The fold's weights depend on the counts alone, so a workgroup derives them once per chunk of
// ON_TPB partials (thread t: w = n_b / n and g = n_a w of partial t, from an exact running count in
// LDS) and every column thread then folds with five float64 operations per partial and no division.
__global__ void __launch_bounds__(ON_TPB) lgx_obs_norm_apply_kernel(const lgx_obs_norm_jobs js, int32_t njobs) {
  __shared__ double s_nb[ON_TPB], s_w[ON_TPB], s_g[ON_TPB + 1];
  const int j = (njobs > 1 && (int)blockIdx.x >= js.wg_start[1]) ? 1 : 0;
  const lgx_obs_norm_job jb = j ? js.job[1] : js.job[0];   // (by value: an indexed kernel argument goes to scratch)
  const int wg = (int)blockIdx.x - js.wg_start[j];
  const int chunks = js.col_chunks[j];
  const int64_t tile = wg / chunks;
  const int t = (int)threadIdx.x;
  const int D = jb.width;
  const bool live = (wg % chunks) * ON_TPB + t < D;
  const int c = live ? (wg % chunks) * ON_TPB + t : 0;   // (idle threads stay for the barriers)
  // this thread's rows first: their loads are in flight while the partials are folded
  const int64_t r0 = tile * ON_APPLY_ROWS;
  const int nr = live ? (int)(jb.rows - r0 < ON_APPLY_ROWS ? jb.rows - r0 : ON_APPLY_ROWS) : 0;
  const float* x = jb.x + r0 * D + c;   // (x may be y: each element is read and written by one thread)
  float v[ON_APPLY_ROWS];
#pragma unroll
  for (int i = 0; i < ON_APPLY_ROWS; ++i) v[i] = i < nr ? x[(int64_t)i * D] : 0.f;
  double n = jb.state_in[0], mean = jb.state_in[1 + c], m2 = jb.state_in[1 + D + c];
  if (jb.update) {   // (uniform over the workgroup)
    const int64_t stride = 1 + 2 * (int64_t)D;
    for (int64_t k0 = 0; k0 < jb.nparts; k0 += ON_TPB) {
      const int chunk = (int)(jb.nparts - k0 < ON_TPB ? jb.nparts - k0 : ON_TPB);
      const double* __restrict__ p = jb.parts + k0 * stride;
      const double nb = t < chunk ? p[t * stride] : 0.0;
      for (int kb = 0; kb < chunk; kb += ON_FOLD, p += ON_FOLD * stride) {
        if (chunk - kb >= ON_FOLD)   // (a full batch: straight-line code, no per-partial guards)
          on_fold_batch<true>(p, stride, c, D, ON_FOLD, kb, chunk, t, nb, n, mean, m2, s_nb, s_w, s_g);
        else
          on_fold_batch<false>(p, stride, c, D, chunk - kb, kb, chunk, t, nb, n, mean, m2, s_nb, s_w, s_g);
      }
      __syncthreads();   // (every thread is past the fold before the next chunk's weights are written)
      n = s_g[ON_TPB];   // the count after this chunk
    }
    if (tile == 0 && live) {   // from the merged registers: state_in is never written by this launch
      if (c == 0) jb.state_out[0] = n;
      jb.state_out[1 + c] = mean;
      jb.state_out[1 + D + c] = m2;
    }
  }
  const float mf = n > 0.0 ? (float)mean : 0.f;
  const float inv = (float)(1.0 / ((n > 0.0 ? sqrt(m2 / n) : 1.0) + jb.eps));
  float* y = jb.y + r0 * D + c;
#pragma unroll
  for (int i = 0; i < ON_APPLY_ROWS; ++i)
    if (i < nr) y[(int64_t)i * D] = (v[i] - mf) * inv;
}

// Checks shared by the two entry points; fills the flat grid (per job: `per` rows per workgroup).
static int obs_norm_plan(const char* who, const lgx_obs_norm_job* jobs, int32_t njobs, bool apply, int per,
                         lgx_obs_norm_jobs& js, int64_t& total) {
  char msg[160];
  auto fail = [&](const char* what) {
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return lgx_fail(LGX_EINVAL, msg);
  };
  if (!jobs) return fail("null jobs");
  if (njobs < 1 || njobs > LGX_OBS_NORM_MAX_JOBS) return fail("njobs must be 1 .. LGX_OBS_NORM_MAX_JOBS");
  total = 0;
  for (int j = 0; j < njobs; ++j) {
    const lgx_obs_norm_job& jb = jobs[j];
    if (jb.rows < 1) return fail("rows < 1");
    if (jb.width < 1 || jb.width > LGX_MAX_PRIV_OBS) return fail("width outside [1, LGX_MAX_PRIV_OBS]");
    const int64_t need = (jb.rows + ON_R - 1) / ON_R;
    if (!jb.x) return fail("null x");
    if (apply) {
      if (!jb.y || !jb.state_in) return fail("null y or state_in");
      if (jb.update) {
        if (!jb.parts || !jb.state_out) return fail("null parts or state_out");
        if (jb.state_out == jb.state_in) return fail("state_out must not be state_in");
        if (jb.nparts < need) return fail("nparts does not cover rows");
      }
    } else if (!jb.parts) {
      return fail("null parts");
    }
    js.job[j] = jb;
    js.col_chunks[j] = (jb.width + ON_TPB - 1) / ON_TPB;
    js.wg_start[j] = (int32_t)total;
    total += ((jb.rows + per - 1) / per) * js.col_chunks[j];
    if (total > 0x7fffffff) return fail("too many rows for one launch");
  }
  js.wg_start[njobs] = (int32_t)total;
  return LGX_OK;
}

extern "C" int32_t lgx_obs_norm_rows_per_part(void) { return ON_R; }

extern "C" int64_t lgx_obs_norm_part_doubles(int64_t rows, int32_t width) {
  if (rows < 1 || width < 1) return 0;
  return ((rows + ON_R - 1) / ON_R) * (1 + 2 * (int64_t)width);
}

extern "C" int lgx_obs_norm_partials(const lgx_obs_norm_job* jobs, int32_t njobs, void* stream) {
  lgx_obs_norm_jobs js = {};
  int64_t total = 0;
  if (int rc = obs_norm_plan("lgx_obs_norm_partials", jobs, njobs, false, ON_R, js, total)) return rc;
  hipLaunchKernelGGL(lgx_obs_norm_partials_kernel, dim3((uint32_t)total), dim3(ON_TPB), 0,
                     reinterpret_cast<hipStream_t>(stream), js, njobs);
  return lgx_hip_status("lgx_obs_norm_partials");
}

extern "C" int lgx_obs_norm_apply(const lgx_obs_norm_job* jobs, int32_t njobs, void* stream) {
  lgx_obs_norm_jobs js = {};
  int64_t total = 0;
  if (int rc = obs_norm_plan("lgx_obs_norm_apply", jobs, njobs, true, ON_APPLY_ROWS, js, total)) return rc;
  hipLaunchKernelGGL(lgx_obs_norm_apply_kernel, dim3((uint32_t)total), dim3(ON_TPB), 0,
                     reinterpret_cast<hipStream_t>(stream), js, njobs);
  return lgx_hip_status("lgx_obs_norm_apply");
}
