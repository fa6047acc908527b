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
#include "rollout_body.h"

namespace {

constexpr int GRAD_BLOCK = QUATTRO_GRAD_BLOCK;

// entry j of Lf_x(x_N)
template <int MODEL>
__device__ __forceinline__ float grad_terminal_entry(const quattro_model_params& own, const float* xN, const int j) {
  constexpr int NX = ModelDims<MODEL>::NX;
#ifdef QT_USER_MODEL_HEADER
  if constexpr (MODEL == QUATTRO_MODEL_USER) {
    using D = qtad::Dual<float>;
    D xd[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xd[i] = D(xN[i], i == j ? 1.0f : 0.0f);
    return qt_user::final_cost<D>(own, xd).d;
  } else
#endif
  {
    float v = 0.0f;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const float g = qt_terminal_vx(own, i, xN[i]);
      v = (i == j) ? g : v;
    }
    return v;
  }
}

// l_u of ONE control (weight ra, value ua): the expression of qt_control_cost_derivs with a softplus that is accurate RELATIVE to
// itself.  qt_softplus forms log(1 + e) on the hardware v_exp_f32 / v_log_f32; the absolute error 6e-8 of forming 1 + e is harmless
// next to the cost it is added to, but away from the barrier (beta u of 3 or more) with a small r the barrier is all of l_u and, over
// a short horizon, most of g_t: 2.7e-6 of the entry on the cart-pole (beta = 3, r = 0.004, N = 2).  Here, on the same two hardware
// instructions: the rounding of x log2(e) is compensated (e (1 + r ln 2)), and log1p(e) = log(w) e / (w - 1) with w = 1 + e rounded
// (w - 1 is exact, and the quotient undoes the rounding of w).  About 25 instructions; the math library's expf / log1pf gave the
// same accuracy at about 150, which every pass of every wave runs whether its lane holds a control or not.
// NOT the bits of the l_u in the records of quattro_linearize_f32: the two agree to fp32 round-off where the barrier is active and to
// about 1e-6 relative away from it, where the record's is the less accurate one.
__device__ __forceinline__ float grad_control_lu(const quattro_model_params& own, float ra, float ua) {
#pragma clang fp contract(off)
  float lu = 2.0f * ra * ua;
  if (own.barrier_alpha != 0.0f) {
    const float bz = -own.barrier_beta * ua;
    const float a = -fabsf(bz);
    const float t = a * 1.44269504f;                                       // log2(e) = 1.44269504f + 1.92596299e-8
    const float r = fmaf(a, 1.44269504f, -t) + a * 1.92596299e-8f;
    float e = exp2f(t);
    e = fmaf(e, r * 0.693147181f, e);                                      // exp(a) = 2^t 2^r
    const float w = 1.0f + e;
    const float l1p = (w == 1.0f) ? e : __logf(w) * __fdividef(e, w - 1.0f);
    const float sp = (fmaxf(bz, 0.0f) + l1p) * (1.0f / own.barrier_beta);
    const float sg = __fdividef(bz >= 0.0f ? 1.0f : e, w);                 // logistic(bz)
    lu = fmaf(own.barrier_alpha, -2.0f * sp * sg, lu);
  }
  return lu;
}

// column j of [A | B] at (xs, us) -> col[NX], and entry j of l_z = (l_x, l_u) (returned)
template <int MODEL, bool RK4>
__device__ __forceinline__ float grad_item(const quattro_model_params& own, const float* xs, const float* us, const int j,
                                           float* col) {
  constexpr int NX = ModelDims<MODEL>::NX, NU = ModelDims<MODEL>::NU;
#ifdef QT_USER_MODEL_HEADER
  if constexpr (MODEL == QUATTRO_MODEL_USER) {
    using D = qtad::Dual<float>;
    D xd[NX], ud[NU], xn[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xd[i] = D(xs[i], i == j ? 1.0f : 0.0f);
#pragma unroll
    for (int a = 0; a < NU; ++a) ud[a] = D(us[a], NX + a == j ? 1.0f : 0.0f);
    qt_user::step<D, RK4>(own, xd, ud, xn);
#pragma unroll
    for (int i = 0; i < NX; ++i) col[i] = xn[i].d;
    return qt_user::stage_cost<D>(own, xd, ud).d;
  } else
#endif
  {
    const float dt = own.dt;
    float dx0[NX], du[NU];
#pragma unroll
    for (int i = 0; i < NX; ++i) dx0[i] = (i == j) ? 1.0f : 0.0f;
#pragma unroll
    for (int a = 0; a < NU; ++a) du[a] = (NX + a == j) ? 1.0f : 0.0f;
    if constexpr (!RK4) {
      float dk[NX];
      qt_rate_jvp<MODEL>(own, xs, us, dx0, du, dk);
#pragma unroll
      for (int i = 0; i < NX; ++i) col[i] = fmaf(dt, dk[i], dx0[i]);
    } else if constexpr (MODEL == QUATTRO_MODEL_QUADROTOR) {
      QuadStage st[4];
      quad_rk4_stages(own, own.phys, xs, us, [&](int s, const QuadStage& q) __attribute__((always_inline)) { st[s] = q; });
      rk4_tangent<NX>(dt, dx0, col, [&](int s, const float* dxs, float* dk) __attribute__((always_inline)) {
        quad_jvp_at(st[s], own, dxs, du, dk);
      });
    } else {
      float xp[4][NX];
      rk4_points<NX>(dt, xs, xp, [&](int, const float* xst, float* k) __attribute__((always_inline)) { qt_rate<MODEL>(own, xst, us, k); });
      rk4_tangent<NX>(dt, dx0, col, [&](int s, const float* dxs, float* dk) __attribute__((always_inline)) {
        qt_rate_jvp<MODEL>(own, xp[s], us, dxs, du, dk);
      });
    }
    // l_z[j]: the lane's own state entry, or its own control (quadratic term + barrier)
    float v = 0.0f, ra = own.r[0], ua = us[0];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const float g = 2.0f * own.q[i] * (xs[i] - own.x_ref[i]);
      v = (i == j) ? g : v;
    }
#pragma unroll
    for (int a = 1; a < NU; ++a) {
      ra = (NX + a == j) ? own.r[a] : ra;
      ua = (NX + a == j) ? us[a] : ua;
    }
    return j >= NX ? grad_control_lu(own, ra, ua) : v;
  }
}

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
