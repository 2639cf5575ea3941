// The body of ppo_loss_bwd_kernel and ppo_loss_bwd_mirror_kernel (lgx_ppo.hip), included into both:
// the two kernels are one text, and the plain kernel's machine code does not depend on the mirror
// form's existence (a shared inline function changed its register allocation).  The including kernel
// provides `a` (lgx_ppo_loss_args), `hparts`, `ms` (ppo_mirror_args; unused without MIRROR), the
// template parameter MAXA and `constexpr bool MIRROR`.
  constexpr int JQ = (MAXA + LB_LPR - 1) / LB_LPR;   // actions per lane
  constexpr int DS = ((MAXA + 1 + 3) / 4) * 4;      // dMU row (+ dV), 16-byte LDS reads
  const int A = a.num_actions, H = a.hidden, H4 = H >> 2, HS = H + 4;
  const int NP = 2 * A + 4;
  extern __shared__ float4 lb_dyn[];
  float* ylds = reinterpret_cast<float*>(lb_dyn);            // [2][LB_ROWS][HS]
  float* wlds = ylds + 2 * LB_ROWS * HS;                      // [A + 1][H]: W4a rows, then w4c
  __shared__ __align__(16) float dmu[LB_ROWS][DS];
  __shared__ float red[LB_ROWS][2 * MAXA + 4 + 1];
  const int t = threadIdx.x;
  const int64_t half = MIRROR ? a.rows >> 1 : 0;                // (MIRROR: the real rows)
  const int64_t r0 = (int64_t)blockIdx.x * (MIRROR ? LB_PAIRS : LB_ROWS);
  const int nr = (int)min((int64_t)(MIRROR ? LB_PAIRS : LB_ROWS), (MIRROR ? half : a.rows) - r0);
  // local row -> staged at all / its minibatch row (MIRROR: nr pairs, the partner LB_PAIRS further)
  auto live = [&](int lr) { return (MIRROR ? (lr & (LB_PAIRS - 1)) : lr) < nr; };
  auto grow = [&](int lr) -> int64_t {
    if constexpr (MIRROR) return r0 + (lr & (LB_PAIRS - 1)) + (lr >= LB_PAIRS ? half : 0);
    else return r0 + lr;
  };
  float* A3 = const_cast<float*>(a.head_in);
  // ---- stage the rows (rows past M as zeros) and the head weights
  for (int i = t; i < 2 * LB_ROWS * H4; i += TPB) {
    const int nrow = i / H4, c4 = i - nrow * H4;              // nrow = net * LB_ROWS + row
    const int net = nrow >= LB_ROWS, rr = nrow - net * LB_ROWS;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (MIRROR) {
      if (live(rr)) v = reinterpret_cast<const float4*>(A3 + ((int64_t)net * a.rows + grow(rr)) * H)[c4];
    } else {
      if (rr < nr) v = reinterpret_cast<const float4*>(A3 + ((int64_t)net * a.rows + r0 + rr) * H)[c4];
    }
    *reinterpret_cast<float4*>(ylds + nrow * HS + 4 * c4) = v;
  }
  for (int i = t; i < (A + 1) * H4; i += TPB)
    reinterpret_cast<float4*>(wlds)[i] = i < A * H4 ? reinterpret_cast<const float4*>(a.W4a)[i]
                                                    : reinterpret_cast<const float4*>(a.W4c)[i - A * H4];
  __syncthreads();
  // ---- 1. output layers
  const int rr = t / LB_LPR, q = t % LB_LPR;
  float hv[MAXA + 1];
#pragma unroll
  for (int j = 0; j <= MAXA; ++j) hv[j] = 0.f;
  {
    const float* ya = ylds + rr * HS;
    const float* yc = ylds + (LB_ROWS + rr) * HS;
    const float4* w4 = reinterpret_cast<const float4*>(wlds);
    for (int c4 = q; c4 < H4; c4 += LB_LPR) {
      const float4 x = *reinterpret_cast<const float4*>(ya + 4 * c4);
      const float4 y = *reinterpret_cast<const float4*>(yc + 4 * c4);
#pragma unroll
      for (int j = 0; j < MAXA; ++j)
        if (j < A) {
          const float4 w = w4[j * H4 + c4];
          hv[j] += x.x * w.x + x.y * w.y + x.z * w.z + x.w * w.w;
        }
      const float4 w = w4[A * H4 + c4];
      hv[MAXA] += y.x * w.x + y.y * w.y + y.z * w.z + y.w * w.w;
    }
  }
#pragma unroll
  for (int j = 0; j <= MAXA; ++j) hv[j] = lb_rowsum(hv[j]);
  // ---- 2. loss per row (lane q: actions q + LB_LPR m)
  float* my = red[rr];
  const bool valid = live(rr);
  {
    const int64_t r = grow(rr);
    const bool ppo = MIRROR ? valid && r < ms.ppo_rows : valid;   // the row takes part in the PPO terms
    const int64_t g = ppo ? (a.idx ? a.idx[r] : r) : 0;
    const float invM = 1.0f / (float)(MIRROR ? ms.ppo_rows : a.rows);
    const float half_log_2pi = 0.91893853320467274178f;
    float mu[JQ], sd[JQ], act[JQ];
    float logp = 0.f, kl = 0.f;
#pragma unroll
    for (int m = 0; m < JQ; ++m) {
      const int j = q + LB_LPR * m;
      float h = 0.f;
#pragma unroll
      for (int jj = 0; jj < MAXA; ++jj) h = jj == j ? hv[jj] : h;
      mu[m] = sd[m] = 1.f;
      act[m] = 0.f;
      if (MIRROR && valid && j < A) mu[m] = h + a.b4a[j];
      if (ppo && j < A) {
        mu[m] = h + a.b4a[j];
        sd[m] = a.std[j];
        act[m] = a.actions[g * A + j];
        const float var = sd[m] * sd[m];
        const float d = act[m] - mu[m];
        logp += -(d * d) / (2.f * var) - logf(sd[m]) - half_log_2pi;
        const float so = a.old_sigma[g * A + j], mo = a.old_mu[g * A + j];
        kl += logf(sd[m] / so + 1.e-5f) + (so * so + (mo - mu[m]) * (mo - mu[m])) / (2.f * var) - 0.5f;
      }
    }
    logp = lb_rowsum(logp);
    kl = lb_rowsum(kl);
    // mirror term: the real rows publish mu, their mirrors take sign[j] mu[perm[j]] as the target
    float dsym[JQ];
#pragma unroll
    for (int m = 0; m < JQ; ++m) dsym[m] = 0.f;
    if constexpr (MIRROR) {
      __shared__ float mux[LB_PAIRS][MAXA];
      __shared__ float symsq[LB_PAIRS];
      if (rr < LB_PAIRS) {
#pragma unroll
        for (int m = 0; m < JQ; ++m)
          if (q + LB_LPR * m < A) mux[rr][q + LB_LPR * m] = mu[m];
      }
      __syncthreads();
      const float gs = 2.f * ms.coeff / ((float)half * (float)A);
      float sq = 0.f;
      if (valid && rr >= LB_PAIRS) {
#pragma unroll
        for (int m = 0; m < JQ; ++m) {
          const int j = q + LB_LPR * m;
          if (j < A) {
            const float diff = mu[m] - ms.act_sign[j] * mux[rr - LB_PAIRS][ms.act_perm[j]];
            dsym[m] = gs * diff;
            sq += diff * diff;
          }
        }
      }
      sq = lb_rowsum(sq);
      if (q == 0 && rr >= LB_PAIRS) symsq[rr - LB_PAIRS] = sq;
      __syncthreads();
      if (t == 0) {   // this workgroup's sum over its mirror rows, in row order
        float s = 0.f;
        for (int i = 0; i < LB_PAIRS; ++i) s += symsq[i];
        ms.sym_partials[blockIdx.x] = s;
      }
    }
    float dlogp = 0.f, surr = 0.f, vl = 0.f, dv = 0.f;
    if (ppo) {
      const float adv = a.advantages[g];
      const float ratio = expf(logp - a.old_logp[g]);
      const float lo = 1.f - a.clip_param, hi = 1.f + a.clip_param;
      const float rc = fminf(fmaxf(ratio, lo), hi);
      const float s1 = -adv * ratio, s2 = -adv * rc;
      const bool inside = ratio >= lo && ratio <= hi;
      float dsdr;   // torch.maximum backward: ties split the gradient; clamp passes it inside [lo, hi]
      if (s1 > s2) dsdr = -adv;
      else if (s1 < s2) dsdr = inside ? -adv : 0.f;
      else dsdr = 0.5f * (-adv) + 0.5f * (inside ? -adv : 0.f);
      surr = fmaxf(s1, s2);
      dlogp = dsdr * invM * ratio;
      const float v = hv[MAXA] + a.b4c[0];
      const float tv = a.target_values[g], ret = a.returns[g];
      if (a.use_clipped_value_loss) {
        const float dvt = v - tv;
        const float vc = tv + fminf(fmaxf(dvt, -a.clip_param), a.clip_param);
        const bool vin = dvt >= -a.clip_param && dvt <= a.clip_param;
        const float u1 = (v - ret) * (v - ret), u2 = (vc - ret) * (vc - ret);
        vl = fmaxf(u1, u2);
        const float g1 = 2.f * (v - ret), g2 = vin ? 2.f * (vc - ret) : 0.f;
        dv = u1 > u2 ? g1 : (u1 < u2 ? g2 : 0.5f * g1 + 0.5f * g2);
      } else {
        vl = (ret - v) * (ret - v);
        dv = 2.f * (v - ret);
      }
      dv *= a.value_loss_coef * invM;
    }
#pragma unroll
    for (int m = 0; m < JQ; ++m) {
      const int j = q + LB_LPR * m;
      if (j < A) {
        const float var = sd[m] * sd[m];
        const float d = act[m] - mu[m];
        float dm = ppo ? dlogp * d / var : 0.f;
        if constexpr (MIRROR) dm += dsym[m];
        dmu[rr][j] = dm;
        my[A + j] = dm;
        my[j] = ppo ? dlogp * (d * d / (var * sd[m]) - 1.f / sd[m]) : 0.f;
      }
    }
    if (q == 0) {
      dmu[rr][A] = dv;
      my[2 * A] = dv;
      my[2 * A + 1] = ppo ? kl : 0.f;
      my[2 * A + 2] = surr;
      my[2 * A + 3] = vl;
    }
  }
  __syncthreads();
  if (t < NP) {   // loss partials of this workgroup (rows in order)
    float s = 0.f;
    for (int i = 0; i < LB_ROWS; ++i) s += red[i][t];
    if (MIRROR && t > 2 * A) s *= (float)a.rows / (float)ms.ppo_rows;   // (means over ppo_rows rows)
    a.partials[(int64_t)blockIdx.x * NP + t] = s;
  }
  // ---- 3. output-layer backward (as head_bwd_kernel; A3 rows from LDS)
  float* P = hparts + (int64_t)blockIdx.x * ((A + 1) * H + 2 * H);
  for (int o = t; o < 2 * H; o += TPB) {
    const int net = o >= H, c = o - net * H;
    const int nj = net == 0 ? A : 1;
    float w[MAXA], acc[MAXA];
#pragma unroll
    for (int j = 0; j < MAXA; ++j) {
      w[j] = j < nj ? wlds[(net == 0 ? j : A) * H + c] : 0.f;
      acc[j] = 0.f;
    }
    const float* ycol = ylds + net * LB_ROWS * HS + c;
    float* col = A3 + ((int64_t)net * a.rows + r0) * H + c;
    float cs = 0.f;
    for (int i = 0; i < (MIRROR ? LB_ROWS : nr); ++i) {
      if (MIRROR && !live(i)) continue;
      const float y = ycol[i * HS];
      float drow[DS];
#pragma unroll
      for (int u = 0; u < DS / 4; ++u) {
        const float4 v = *reinterpret_cast<const float4*>(&dmu[i][4 * u]);
        drow[4 * u] = v.x; drow[4 * u + 1] = v.y; drow[4 * u + 2] = v.z; drow[4 * u + 3] = v.w;
      }
      float dA = 0.f;
      if (net == 0) {
#pragma unroll
        for (int j = 0; j < MAXA; ++j)
          if (j < nj) { acc[j] += drow[j] * y; dA += drow[j] * w[j]; }
      } else {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j <= MAXA; ++j) d = (j == A) ? drow[j] : d;   // dV column
        acc[0] += d * y;
        dA = d * w[0];
      }
      const float dz = dA * elu_grad_from_out(y);
      if constexpr (MIRROR) A3[((int64_t)net * a.rows + grow(i)) * H + c] = dz;
      else col[(int64_t)i * H] = dz;
      cs += dz;
    }
    const int jo = net == 0 ? 0 : A;
#pragma unroll
    for (int j = 0; j < MAXA; ++j)
      if (j < nj) P[(jo + j) * H + c] = acc[j];
    P[(A + 1) * H + o] = cs;
  }
