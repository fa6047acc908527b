// Cost gradient (quattro_cost_gradient_f32): the adjoint sweep of J(x0, u) = sum_t L(x_t, u_t) + Lf(x_N), x_{t+1} = f(x_t, u_t),
//   lambda_N = Lf_x(x_N);  t = N-1 .. 0:  g_t = L_u + B_t^T lambda_{t+1},  lambda_t = L_x + A_t^T lambda_{t+1}
// -> grad_u = g, grad_x0 = lambda_0, costate = lambda, all fp32.
//
// Arithmetic differentiated (reference quattro_ilqr_tf/quattro_ilqr_tf.py): simulate :127-132 and compute_total_cost :138-143.  The
// reference has no counterpart: it never forms dJ/du (its only first-order quantities are the Q_u of the backward pass).
//
// A group of LPI adjacent lanes owns one trajectory and lane j of the group owns direction j of z = (x, u), the mapping of
// linearize_rk4_kernel / user_linearize_item.  A gradient needs products with [A | B]^T only, and (A^T lambda)_j, (B^T lambda)_a are
// dot products of COLUMN j of [A | B] with lambda: the lane that pushes e_j through the step is the lane that needs the result.
//   off the chain : column j of [A_t | B_t] (the tangent of the whole integrator step along e_j; the stage points of an RK4 step
//                   are formed once per step and lane) and entry j of l_z(t) do not depend on lambda.  They are formed for
//                   QUATTRO_GRAD_BLOCK steps at a time and staged in LDS ([step][entry][lane], every access 64 consecutive floats).
//                   A group with lanes to spare linearises several steps at once (LPI / (n + m) of them: three for the cart-pole), so
//                   the lane that forms a column is not always the lane that consumes it: that is what the stage is for.
//   on the chain  : per step one n-term fmaf chain per lane over its staged column and lambda_{t+1}, which every lane of the group
//                   holds in registers, then the exchange of the n new entries inside the group through 64 floats of LDS (one
//                   write, n broadcast reads; the workgroup is one wave, so the barrier between them is a wait count).
// Rows as score_kernel takes them: a private block `own` is filled with VALUES behind wave-uniform branches, so the same code runs
// with and without rows and a trajectory's result does not depend on its place in the batch.  model_phys reaches the dynamics here.
// No global workspace, nothing allocated.
#include "grad_device.h"

namespace {

constexpr int GRAD_BLOCK = QUATTRO_GRAD_BLOCK;

template <int MODEL, bool RK4, int LPI>
__global__ __launch_bounds__(QT_WAVE) void cost_gradient_kernel(const quattro_model_params p, const float* __restrict__ x,
                                                                const float* __restrict__ u, const int B, const int N,
                                                                const float* __restrict__ model_phys,
                                                                const float* __restrict__ x_ref_rows, const int ref_rows,
                                                                const float* __restrict__ cost_rows, float* __restrict__ grad_u,
                                                                float* __restrict__ grad_x0, float* __restrict__ costate) {
  constexpr int NX = ModelDims<MODEL>::NX, NU = ModelDims<MODEL>::NU, NZ = NX + NU;
  constexpr int ROW = NX + 1;                                  // staged per step and lane: the column and l_z[j]
  static_assert(NZ <= LPI && QT_WAVE % LPI == 0, "one lane per direction of z");
  __shared__ float s_stage[GRAD_BLOCK * ROW * QT_WAVE];
  __shared__ float s_lam[QT_WAVE];
  const int lane = threadIdx.x;
  const int grp = lane / LPI, j = lane % LPI;
  // off the chain a group linearises SPP steps at once where it has lanes to spare (cart-pole: 3 steps x 5 directions on 15 of its 16
  // lanes): lane j takes direction `dir` of the pass's step `sub`; on the chain lane j < NZ reads back direction j of every step
  constexpr int SPP = LPI / NZ;
  const int sub = j / NZ, dir = j - sub * NZ;
  const long long braw = (long long)blockIdx.x * (QT_WAVE / LPI) + grp;
  const bool live = braw < B;                                  // groups past the batch recompute trajectory B - 1 and store nothing
  const size_t bb = live ? (size_t)braw : (size_t)(B - 1);

  quattro_model_params own = p;
  if (cost_rows != nullptr) {
    float w[QUATTRO_COST_ROW_FLOATS];
#pragma unroll
    for (int i = 0; i < QUATTRO_COST_ROW_FLOATS; ++i) w[i] = cost_rows[bb * QUATTRO_COST_ROW_FLOATS + i];
#pragma unroll
    for (int i = 0; i < QUATTRO_MAX_NX; ++i) {
      own.q[i] = w[i];
      own.qf[i] = w[QUATTRO_MAX_NX + i];
    }
#pragma unroll
    for (int i = 0; i < QUATTRO_MAX_NU; ++i) own.r[i] = w[2 * QUATTRO_MAX_NX + i];
  }
  if (model_phys != nullptr) {
    float ph[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) ph[i] = model_phys[bb * 8 + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) own.phys[i] = ph[i];
  }
  const float* xb = x + bb * (size_t)(N + 1) * NX;
  const float* ub = u + bb * (size_t)N * NU;
  // the reference of horizon step t (t = N: the terminal term): row min(t, ref_rows - 1), the solves' rule for a plan from step 0
  auto set_ref = [&](int t) __attribute__((always_inline)) {
    float xr[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xr[i] = p.x_ref[i];
    if (x_ref_rows != nullptr) {
      const int row = t < ref_rows - 1 ? t : ref_rows - 1;
      const float* rr = x_ref_rows + (bb * (size_t)ref_rows + (size_t)row) * NX;
#pragma unroll
      for (int i = 0; i < NX; ++i) xr[i] = rr[i];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) own.x_ref[i] = xr[i];
  };
  // the group's new lambda: lane i < NX holds entry i in v -> all NX entries in every lane
  float lam[NX];
  // (no barrier in front of the write: the workgroup is ONE wave, whose LDS operations complete in program order, so the reads of
  //  the previous exchange are done before this write lands)
  auto exchange = [&](float v) __attribute__((always_inline)) {
    if (j < NX) s_lam[grp * LPI + j] = v;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NX; ++i) lam[i] = s_lam[grp * LPI + i];
  };

  float v;
  {
    float xN[NX];
    load_vec<NX>(xb + (size_t)N * NX, xN);
    set_ref(N);
    v = grad_terminal_entry<MODEL>(own, xN, j);
    if (live && j < NX && costate != nullptr) costate[(bb * (size_t)(N + 1) + (size_t)N) * NX + j] = v;
    exchange(v);
  }
  for (int t_hi = N; t_hi > 0; t_hi -= GRAD_BLOCK) {
    const int cnt = t_hi < GRAD_BLOCK ? t_hi : GRAD_BLOCK;     // steps t_hi - 1 .. t_hi - cnt, slot s holds step t_hi - 1 - s
#pragma unroll 1
    for (int s0 = 0; s0 < cnt; s0 += SPP) {
      const int s = s0 + sub;
      const bool mine = sub < SPP && s < cnt;                  // lanes without a step of their own redo step s0 and store nothing
      const int t = t_hi - 1 - (mine ? s : s0);
      float xs[NX], us[NU], col[NX];
      load_vec<NX>(xb + (size_t)t * NX, xs);
      load_vec<NU>(ub + (size_t)t * NU, us);
      set_ref(t);
      const float lz = grad_item<MODEL, RK4>(own, xs, us, dir, col);
      if (mine) {
        float* st = s_stage + s * ROW * QT_WAVE + grp * LPI + dir;
#pragma unroll
        for (int i = 0; i < NX; ++i) st[i * QT_WAVE] = col[i];
        st[NX * QT_WAVE] = lz;
      }
    }
    __syncthreads();
    float col[NX], lz;
    {
      const float* st = s_stage + lane;
#pragma unroll
      for (int i = 0; i < NX; ++i) col[i] = st[i * QT_WAVE];
      lz = st[NX * QT_WAVE];
    }
#pragma unroll 1
    for (int s = 0; s < cnt; ++s) {
      const int t = t_hi - 1 - s;
      float coln[NX], lzn = 0.0f;
      if (s + 1 < cnt) {                                       // the next step's column is requested before anything waits
        const float* st = s_stage + (s + 1) * ROW * QT_WAVE + lane;
#pragma unroll
        for (int i = 0; i < NX; ++i) coln[i] = st[i * QT_WAVE];
        lzn = st[NX * QT_WAVE];
      }
      v = lz;
#pragma unroll
      for (int i = 0; i < NX; ++i) v = fmaf(col[i], lam[i], v);
      if (live) {
        if (j >= NX && j < NZ) grad_u[(bb * (size_t)N + (size_t)t) * NU + (j - NX)] = v;
        if (j < NX && costate != nullptr) costate[(bb * (size_t)(N + 1) + (size_t)t) * NX + j] = v;
      }
      exchange(v);
      if (s + 1 < cnt) {
#pragma unroll
        for (int i = 0; i < NX; ++i) col[i] = coln[i];
        lz = lzn;
      }
    }
    __syncthreads();                                           // the stage is rewritten by the next block of steps
  }
  if (live && j < NX && grad_x0 != nullptr) grad_x0[bb * NX + j] = v;     // lambda_0: the value costate[b][0] was given
}

template <int MODEL, int LPI>
int launch_cost_gradient(const quattro_model_params& p, const float* x, const float* u, int B, int N, const float* model_phys,
                         const float* x_ref_rows, int ref_rows, const float* cost_rows, float* grad_u, float* grad_x0,
                         float* costate, hipStream_t stream) {
  constexpr int PER = QT_WAVE / LPI;
  const dim3 grid((unsigned)((B + PER - 1) / PER)), block(QT_WAVE);
  if (p.integrator == QUATTRO_INTEGRATOR_EULER)
    hipLaunchKernelGGL((cost_gradient_kernel<MODEL, false, LPI>), grid, block, 0, stream, p, x, u, B, N, model_phys, x_ref_rows,
                       ref_rows, cost_rows, grad_u, grad_x0, costate);
  else if (p.integrator == QUATTRO_INTEGRATOR_RK4)
    hipLaunchKernelGGL((cost_gradient_kernel<MODEL, true, LPI>), grid, block, 0, stream, p, x, u, B, N, model_phys, x_ref_rows,
                       ref_rows, cost_rows, grad_u, grad_x0, costate);
  else
    return QUATTRO_ERR_UNSUPPORTED;
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

}  // namespace

int quattro_launch_cost_gradient(const quattro_model_params& p, const float* x, const float* u, int B, int N,
                                 const float* model_phys, const float* x_ref_rows, int ref_rows, const float* cost_rows,
                                 float* grad_u, float* grad_x0, float* costate, hipStream_t stream) {
  if (p.model_id == QUATTRO_MODEL_CARTPOLE)
    return launch_cost_gradient<QUATTRO_MODEL_CARTPOLE, 16>(p, x, u, B, N, model_phys, x_ref_rows, ref_rows, cost_rows, grad_u,
                                                            grad_x0, costate, stream);
  if (p.model_id == QUATTRO_MODEL_QUADROTOR)
    return launch_cost_gradient<QUATTRO_MODEL_QUADROTOR, 16>(p, x, u, B, N, model_phys, x_ref_rows, ref_rows, cost_rows, grad_u,
                                                             grad_x0, costate, stream);
#ifdef QT_USER_MODEL_HEADER
  if (p.model_id == QUATTRO_MODEL_USER) {
    constexpr int NZ = QT_USER_NX + QT_USER_NU, LPI = NZ <= 8 ? 8 : (NZ <= 16 ? 16 : 32);
    return launch_cost_gradient<QUATTRO_MODEL_USER, LPI>(p, x, u, B, N, model_phys, x_ref_rows, ref_rows, cost_rows, grad_u,
                                                         grad_x0, costate, stream);
  }
#endif
  return QUATTRO_ERR_UNSUPPORTED;
}
