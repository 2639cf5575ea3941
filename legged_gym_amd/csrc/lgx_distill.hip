// Teacher-student distillation (rsl_rl 2.x `Distillation`): the narrow end of the
// supervised update in one launch - the student's output layer, the behaviour loss against the
// teacher's stored action means, and the output layer's backward.
//
// lgx_bc_loss_bwd is ppo_loss_bwd_kernel (lgx_ppo.hip) for one network and a quadratic loss:
// BC_ROWS rows of the last hidden activations are read from HBM once into LDS (row stride H + 4
// floats) next to W4, then
//   1. output layer: BC_LPR lanes per row dot interleaved float4 columns against the W4 rows (LDS
//      broadcasts), combined across the row's lanes by xor shuffles; mu = Y3 W4^T + b4;
//   2. loss per row: the row's lanes take actions j = q, q + BC_LPR, ...: d = mu - target,
//      dmu = 2 scale d into LDS, sum d^2 per row; the workgroup's sum, rows in order, is its one
//      loss partial;
//   3. backward (thread = hidden column): dZ3 = (dmu W4) * elu'(Y3) over head_in in place, and the
//      workgroup's [A*H dW4 | A db4 | H db3] partials, rows in order.
// No atomics: every output has one writer and a fixed summation order, so two launches give the
// same bits.  All LDS is dynamic and every carve offset a multiple of 16 bytes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <cmath>

#include "lgx_internal.h"
#include "lgx_launch.h"

namespace {

constexpr int TPB = 256;
constexpr int BC_ROWS = 32;              // rows per workgroup
constexpr int BC_LPR = TPB / BC_ROWS;    // lanes per row in phases 1-2 (8)
constexpr int BC_DS = ((LGX_PPO_MAX_ACTIONS + 3) / 4) * 4;   // dmu row stride in LDS (floats)
constexpr int BC_MAX_LDS = 96 * 1024;

#define LGX_STREAM(s) reinterpret_cast<hipStream_t>(s)

__device__ __forceinline__ float elu_grad_from_out(float y) { return y > 0.f ? 1.f : y + 1.f; }

__device__ __forceinline__ float bc_rowsum(float v) {   // sum over the BC_LPR lanes of a row
#pragma unroll
  for (int m = 1; m < BC_LPR; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// floats of dynamic LDS: [BC_ROWS][H + 4] rows | [A][H] W4 | [BC_ROWS][BC_DS] dmu | [BC_ROWS] row sums
__host__ __device__ inline int64_t bc_lds_floats(int A, int H) {
  return (int64_t)BC_ROWS * (H + 4) + (int64_t)A * H + BC_ROWS * BC_DS + BC_ROWS;
}

template <int MAXA>
__global__ void __launch_bounds__(TPB)
bc_loss_bwd_kernel(float* __restrict__ head_in, const float* __restrict__ W4, const float* __restrict__ b4,
                   const float* __restrict__ target, int64_t rows, int32_t A, int32_t H, float scale,
                   float* __restrict__ loss_parts, float* __restrict__ hparts) {
  constexpr int JQ = (MAXA + BC_LPR - 1) / BC_LPR;   // actions per lane
  constexpr int DS4 = (MAXA + 3) / 4;                // float4 reads of a dmu row
  const int H4 = H >> 2, HS = H + 4;
  extern __shared__ __attribute__((aligned(16))) float bc_dyn[];
  float* ylds = bc_dyn;                        // [BC_ROWS][HS]
  float* wlds = ylds + BC_ROWS * HS;           // [A][H]
  float* dmu = wlds + A * H;                   // [BC_ROWS][BC_DS]   (A * H % 16 == 0: 16-byte aligned)
  float* rowsq = dmu + BC_ROWS * BC_DS;        // [BC_ROWS]
  const int t = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * BC_ROWS;
  const int nr = (int)min((int64_t)BC_ROWS, rows - r0);
  // ---- stage the rows (rows past M as zeros) and the head weights
  for (int i = t; i < BC_ROWS * H4; i += TPB) {
    const int rr = i / H4, c4 = i - rr * H4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rr < nr) v = reinterpret_cast<const float4*>(head_in + (r0 + rr) * H)[c4];
    *reinterpret_cast<float4*>(ylds + rr * HS + 4 * c4) = v;
  }
  for (int i = t; i < A * H4; i += TPB) reinterpret_cast<float4*>(wlds)[i] = reinterpret_cast<const float4*>(W4)[i];
  __syncthreads();
  // ---- 1. output layer
  const int rr = t / BC_LPR, q = t % BC_LPR;
  float hv[MAXA];
#pragma unroll
  for (int j = 0; j < MAXA; ++j) hv[j] = 0.f;
  {
    const float* ya = ylds + rr * HS;
    const float4* w4 = reinterpret_cast<const float4*>(wlds);
    for (int c4 = q; c4 < H4; c4 += BC_LPR) {
      const float4 x = *reinterpret_cast<const float4*>(ya + 4 * c4);
#pragma unroll
      for (int j = 0; j < MAXA; ++j)
        if (j < A) {
          const float4 w = w4[j * H4 + c4];
          hv[j] += x.x * w.x + x.y * w.y + x.z * w.z + x.w * w.w;
        }
    }
  }
#pragma unroll
  for (int j = 0; j < MAXA; ++j) hv[j] = bc_rowsum(hv[j]);
  // ---- 2. the row's loss and d loss / d mu (lane q: actions q + BC_LPR m)
  {
    const bool valid = rr < nr;
    float sq = 0.f;
#pragma unroll
    for (int m = 0; m < JQ; ++m) {
      const int j = q + BC_LPR * m;
      float h = 0.f;
#pragma unroll
      for (int jj = 0; jj < MAXA; ++jj) h = jj == j ? hv[jj] : h;
      if (j < A) {
        float d = 0.f;
        if (valid) d = (h + b4[j]) - target[(r0 + rr) * A + j];
        dmu[rr * BC_DS + j] = 2.f * scale * d;
        sq += d * d;
      } else if (j < BC_DS) {
        dmu[rr * BC_DS + j] = 0.f;
      }
    }
    sq = bc_rowsum(sq);
    if (q == 0) rowsq[rr] = sq;
  }
  __syncthreads();
  float* P = hparts + (int64_t)blockIdx.x * ((int64_t)A * H + A + H);
  if (t == 0) {   // this workgroup's sum of squared errors, rows in order
    float s = 0.f;
    for (int i = 0; i < BC_ROWS; ++i) s += rowsq[i];
    loss_parts[blockIdx.x] = s;
  }
  if (t >= 64 && t < 64 + A) {   // db4 partial (the second wave: wave 0 holds the serial loss sum)
    const int j = t - 64;
    float s = 0.f;
    for (int i = 0; i < BC_ROWS; ++i) s += dmu[i * BC_DS + j];
    P[(int64_t)A * H + j] = s;
  }
  // ---- 3. output-layer backward
  for (int c = t; c < H; c += TPB) {
    float w[MAXA], acc[MAXA];
#pragma unroll
    for (int j = 0; j < MAXA; ++j) {
      w[j] = j < A ? wlds[j * H + c] : 0.f;
      acc[j] = 0.f;
    }
    const float* ycol = ylds + c;
    float* col = head_in + r0 * H + c;
    float cs = 0.f;
    for (int i = 0; i < nr; ++i) {
      const float y = ycol[i * HS];
      float drow[4 * DS4];
#pragma unroll
      for (int u = 0; u < DS4; ++u) {
        const float4 v = *reinterpret_cast<const float4*>(dmu + i * BC_DS + 4 * u);
        drow[4 * u] = v.x; drow[4 * u + 1] = v.y; drow[4 * u + 2] = v.z; drow[4 * u + 3] = v.w;
      }
      float dA = 0.f;
#pragma unroll
      for (int j = 0; j < MAXA; ++j)
        if (j < A) { acc[j] += drow[j] * y; dA += drow[j] * w[j]; }
      const float dz = dA * elu_grad_from_out(y);
      col[(int64_t)i * H] = dz;
      cs += dz;
    }
#pragma unroll
    for (int j = 0; j < MAXA; ++j)
      if (j < A) P[(int64_t)j * H + c] = acc[j];
    P[(int64_t)A * H + A + c] = cs;
  }
}

// out[0] = scale * sum of `n` partials (one workgroup, fixed order: lane-strided chains, then the tree)
__global__ void __launch_bounds__(TPB)
bc_loss_reduce_kernel(const float* __restrict__ parts, int64_t n, float scale, float* __restrict__ out) {
  __shared__ float red[TPB];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += TPB) s += parts[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = TPB / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0] * scale;
}

bool bc_shape_ok(int64_t rows, int32_t A, int32_t H) {
  return rows >= 1 && A >= 1 && A <= LGX_PPO_MAX_ACTIONS && H >= 16 && H % 16 == 0 &&
         bc_lds_floats(A, H) * (int64_t)sizeof(float) <= BC_MAX_LDS;
}

}  // namespace

extern "C" int lgx_bc_loss_bwd_layout(int64_t rows, int32_t num_actions, int32_t hidden, int64_t* out) {
  if (!out) return lgx_fail(LGX_EINVAL, "lgx_bc_loss_bwd_layout: null out");
  if (rows < 1) return lgx_fail(LGX_EINVAL, "lgx_bc_loss_bwd_layout: rows < 1");
  if (num_actions < 1 || num_actions > LGX_PPO_MAX_ACTIONS)
    return lgx_fail(LGX_EINVAL, "lgx_bc_loss_bwd_layout: num_actions outside [1, LGX_PPO_MAX_ACTIONS]");
  if (hidden < 16 || hidden % 16)
    return lgx_fail(LGX_EINVAL, "lgx_bc_loss_bwd_layout: hidden must be a positive multiple of 16");
  if (!bc_shape_ok(rows, num_actions, hidden))
    return lgx_fail(LGX_EINVAL, "lgx_bc_loss_bwd_layout: hidden too wide for the LDS row stage (96 KB)");
  const int64_t blocks = (rows + BC_ROWS - 1) / BC_ROWS;
  out[0] = blocks;
  out[1] = blocks * ((int64_t)num_actions * hidden + num_actions + hidden);
  out[2] = bc_lds_floats(num_actions, hidden) * (int64_t)sizeof(float);
  return LGX_OK;
}

extern "C" int lgx_bc_loss_bwd(float* head_in, const float* W4, const float* b4, const float* target, int64_t rows,
                               int32_t num_actions, int32_t hidden, float scale, float* loss_partials,
                               float* head_partials, void* stream) {
  if (!head_in || !W4 || !b4 || !target || !loss_partials || !head_partials)
    return lgx_fail(LGX_EINVAL, "lgx_bc_loss_bwd: null pointer");
  if (!std::isfinite(scale)) return lgx_fail(LGX_EINVAL, "lgx_bc_loss_bwd: scale must be finite");
  int64_t lay[3];
  if (lgx_bc_loss_bwd_layout(rows, num_actions, hidden, lay) != LGX_OK) return LGX_EINVAL;   // (its message)
  if (((uintptr_t)head_in & 15) || ((uintptr_t)W4 & 15))
    return lgx_fail(LGX_EINVAL, "lgx_bc_loss_bwd: head_in and W4 must be 16-byte aligned");
  if (lay[0] >= (1ll << 31)) return lgx_fail(LGX_EINVAL, "lgx_bc_loss_bwd: too many rows for one grid");
  static const bool attr_ok =
      lgx_allow_dynamic_lds({&bc_loss_bwd_kernel<12>, &bc_loss_bwd_kernel<LGX_PPO_MAX_ACTIONS>}, BC_MAX_LDS);
  if (!attr_ok) return lgx_fail(LGX_EHIP, "lgx_bc_loss_bwd: hipFuncSetAttribute failed");
  const dim3 grid((unsigned)lay[0]), block(TPB);
  const size_t lds = (size_t)lay[2];
  if (num_actions <= 12)
    hipLaunchKernelGGL(bc_loss_bwd_kernel<12>, grid, block, lds, LGX_STREAM(stream), head_in, W4, b4, target, rows,
                       num_actions, hidden, scale, loss_partials, head_partials);
  else
    hipLaunchKernelGGL(bc_loss_bwd_kernel<LGX_PPO_MAX_ACTIONS>, grid, block, lds, LGX_STREAM(stream), head_in, W4, b4,
                       target, rows, num_actions, hidden, scale, loss_partials, head_partials);
  return lgx_hip_status("lgx_bc_loss_bwd");
}

extern "C" int lgx_bc_loss_reduce(const float* partials, int64_t count, float scale, float* out, void* stream) {
  if (!partials || !out) return lgx_fail(LGX_EINVAL, "lgx_bc_loss_reduce: null pointer");
  if (count < 1) return lgx_fail(LGX_EINVAL, "lgx_bc_loss_reduce: count < 1");
  if (!std::isfinite(scale)) return lgx_fail(LGX_EINVAL, "lgx_bc_loss_reduce: scale must be finite");
  hipLaunchKernelGGL(bc_loss_reduce_kernel, dim3(1), dim3(TPB), 0, LGX_STREAM(stream), partials, count, scale, out);
  return lgx_hip_status("lgx_bc_loss_reduce");
}
