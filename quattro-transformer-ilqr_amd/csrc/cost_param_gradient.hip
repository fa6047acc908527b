// Cost gradient with respect to what a trajectory's rows hold (quattro_cost_param_gradient_f32): its physical parameters, its cost
// weights and its targets, given the costate lambda of the adjoint sweep (cost_gradient.hip) under the same rows.
//   grad_phys[k]     = sum_{t<N} sum_i lambda_{t+1,i} d f_i / d theta_k (x_t, u_t; theta)      f: the whole integrator step
//   grad_cost_rows   : q_i -> sum_{t<N} (x_{t,i} - ref_{t,i})^2,  qf_i -> (x_{N,i} - ref_{N,i})^2,  r_a -> sum_{t<N} u_{t,a}^2
//   grad_ref_rows    : row rho -> sum_{t<N, min(t,R-1)=rho} -2 q_i (x_{t,i} - ref_{rho,i}),  and -2 qf_i (x_{N,i} - ref_{rho,i}) where
//                      min(N, R-1) = rho (the row rule of the adjoint sweep)
// Arithmetic differentiated (reference quattro_ilqr_tf/quattro_ilqr_tf.py): simulate :127-132 and compute_total_cost :138-143 with
// respect to quantities the reference keeps inside its Python callables; it has no counterpart.
//
// No serial chain: given lambda every (trajectory, step) item stands alone.  score_kernel's mapping: one wave per trajectory, a slot
// per lane, 64 slots a pass; slot s < N is horizon step s, slot N the terminal term.  A lane forms its slot's fp32 terms -- for the
// parameters by pushing Dual<float>(theta_k, 1) through the scalar-generic step of models_generic.h, one k after the other (the
// parameter-only coefficients and their derivatives come from a table the wave fills once, lane k seeding theta_k; the arithmetic
// is GenericRate::Scalar, double for the cart-pole, and the term is rounded to fp32 once) -- and
// leaves them in LDS, one row of 64 per output entry (rows 65 floats apart: lane o walking row o meets no bank conflict).  Then lane
// o adds row o's terms to its fp64 accumulator in slot order.  So every sum runs over t = 0 .. N in that order whatever B, the
// trajectory's place in the batch or the grid: there are no atomics and no workspace, and trajectory b's results are those of a
// B = 1 call with row b in the struct, bit for bit.  Entries with a single term (qf, target rows below the last) are that term
// added to +0.0, so that a zero term comes out +0.0 like an empty sum.
// Rows as score_kernel takes them: a private block of VALUES behind wave-uniform branches, one code path with and without rows.
#include "rollout_body.h"
#include "models_generic.h"

namespace {

template <int MODEL, bool RK4>
__global__ __launch_bounds__(QT_WAVE) void cost_param_gradient_kernel(
    const quattro_model_params p, const float* __restrict__ x, const float* __restrict__ u, const int N,
    const float* __restrict__ costate, const float* __restrict__ model_phys, const float* __restrict__ x_ref_rows, const int ref_rows,
    const float* __restrict__ cost_rows, double* __restrict__ grad_phys, double* __restrict__ grad_cost_rows,
    double* __restrict__ grad_ref_rows) {
  using GR = GenericRate<MODEL>;
  using S = typename GR::Scalar;     // the arithmetic of the parameter terms: float, or double where fp32 cannot hold the bound
  using D = qtad::Dual<S>;
  constexpr int NX = GR::NX, NU = GR::NU, NP = GR::NP, NC = GR::NC;
  // output entries that are sums over slots, one LDS row and one summing lane each: phys | q | r | the last target row
  constexpr int O_Q = NP, O_R = NP + NX, O_T = NP + NX + NU, NOUT = NP + 2 * NX + NU;
  constexpr int PITCH = QT_WAVE + 1;
  static_assert(NOUT <= QT_WAVE && NP <= 8, "one summing lane per output entry");
  __shared__ float s_term[NOUT * PITCH];
  __shared__ double s_cost[QUATTRO_COST_ROW_FLOATS];
  __shared__ S s_dc[NP * NC];
  const size_t bb = blockIdx.x;
  const int lane = threadIdx.x;

  float q[NX], qf[NX], ph[8];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    q[i] = p.q[i];
    qf[i] = p.qf[i];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) ph[i] = p.phys[i];
  if (cost_rows != nullptr) {
    const float* w = cost_rows + bb * QUATTRO_COST_ROW_FLOATS;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      q[i] = w[i];
      qf[i] = w[QUATTRO_MAX_NX + i];
    }
  }
  if (model_phys != nullptr) {
#pragma unroll
    for (int i = 0; i < 8; ++i) ph[i] = model_phys[bb * 8 + i];
  }
  const int R = x_ref_rows != nullptr ? ref_rows : 1;
  const float* xb = x + bb * (size_t)(N + 1) * NX;
  const float* ub = u + bb * (size_t)N * NU;
  double* gref = grad_ref_rows != nullptr ? grad_ref_rows + bb * (size_t)R * NX : nullptr;

  if (lane < QUATTRO_COST_ROW_FLOATS) s_cost[lane] = 0.0;
  // the coefficients of the rate (GenericRate::coefs) depend on the parameters alone: lane k < NP seeds theta_k and leaves the NC
  // derivatives along it in the table, every lane keeps the NC values (they do not depend on the seed)
  S cv[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) cv[j] = S(0);
  if (grad_phys != nullptr) {
    D pd[NP], c[NC];
#pragma unroll
    for (int i = 0; i < NP; ++i) pd[i] = D(S(ph[i]), i == lane ? S(1) : S(0));
    GR::coefs(pd, c);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      cv[j] = c[j].v;
      if (lane < NP) s_dc[lane * NC + j] = c[j].d;
    }
  }
  __syncthreads();
  // target rows past the horizon, the last one included when it lies there: +0.0
  if (gref != nullptr) {
    for (int row = N + 1 + lane; row < R; row += QT_WAVE) {
#pragma unroll
      for (int i = 0; i < NX; ++i) gref[(size_t)row * NX + i] = 0.0;
    }
  }

  double acc = 0.0;
  const int slots = N + 1;
  for (int base = 0; base < slots; base += QT_WAVE) {
    const int s = base + lane;
    float term[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) term[o] = 0.0f;
    if (s < slots) {
      float xs[NX], xr[NX], d[NX], tg[NX];
      load_vec<NX>(xb + (size_t)s * NX, xs);
#pragma unroll
      for (int i = 0; i < NX; ++i) xr[i] = p.x_ref[i];
      const int row = s < R - 1 ? s : R - 1;
      if (x_ref_rows != nullptr) {
        const float* rr = x_ref_rows + (bb * (size_t)ref_rows + (size_t)row) * NX;
#pragma unroll
        for (int i = 0; i < NX; ++i) xr[i] = rr[i];
      }
#pragma unroll
      for (int i = 0; i < NX; ++i) d[i] = xs[i] - xr[i];
      if (s < N) {
        float us[NU];
        load_vec<NU>(ub + (size_t)s * NU, us);
        if (grad_phys != nullptr) {
          float lam[NX];
          S g1[GR::NG], xS[NX], uS[NU];
          load_vec<NX>(costate + (bb * (size_t)(N + 1) + (size_t)(s + 1)) * NX, lam);
#pragma unroll
          for (int i = 0; i < NX; ++i) xS[i] = S(xs[i]);
#pragma unroll
          for (int a = 0; a < NU; ++a) uS[a] = S(us[a]);
          GR::terms(xS, uS, g1);
#pragma unroll
          for (int k = 0; k < NP; ++k) {
            D c[NC], xn[NX];
#pragma unroll
            for (int j = 0; j < NC; ++j) c[j] = D(cv[j], s_dc[k * NC + j]);
            generic_step<MODEL, RK4, S, D, D>(S(p.dt), c, g1, xS, uS, xn);
            S v = S(0);
#pragma unroll
            for (int i = 0; i < NX; ++i) v = fma(S(lam[i]), xn[i].d, v);
            term[k] = (float)v;                      // the per-step term is fp32 whatever it was formed in
          }
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          term[O_Q + i] = d[i] * d[i];
          tg[i] = -2.0f * q[i] * d[i];
        }
#pragma unroll
        for (int a = 0; a < NU; ++a) term[O_R + a] = us[a] * us[a];
      } else {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          s_cost[QUATTRO_MAX_NX + i] = 0.0 + (double)(d[i] * d[i]);
          tg[i] = -2.0f * qf[i] * d[i];
        }
      }
      if (s < R - 1) {           // a row of its own: this slot is its only term
        if (gref != nullptr) {
#pragma unroll
          for (int i = 0; i < NX; ++i) gref[(size_t)s * NX + i] = 0.0 + (double)tg[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < NX; ++i) term[O_T + i] = tg[i];
      }
    }
#pragma unroll
    for (int o = 0; o < NOUT; ++o) s_term[o * PITCH + lane] = term[o];
    __syncthreads();
    const int cnt = slots - base < QT_WAVE ? slots - base : QT_WAVE;
    if (lane < NOUT) {
      const float* mine = s_term + lane * PITCH;
      for (int i = 0; i < cnt; ++i) acc += (double)mine[i];
    }
    __syncthreads();
  }

  if (lane >= O_Q && lane < O_R) s_cost[lane - O_Q] = acc;
  if (lane >= O_R && lane < O_T) s_cost[2 * QUATTRO_MAX_NX + (lane - O_R)] = acc;
  __syncthreads();
  if (grad_phys != nullptr && lane < 8) grad_phys[bb * 8 + lane] = lane < NP ? acc : 0.0;
  if (grad_cost_rows != nullptr && lane < QUATTRO_COST_ROW_FLOATS)
    grad_cost_rows[bb * QUATTRO_COST_ROW_FLOATS + lane] = s_cost[lane];
  // the last target row, where it lies inside the horizon (slot R - 1 exists): the sum of every slot from R - 1 on
  if (gref != nullptr && R - 1 <= N && lane >= O_T && lane < NOUT) gref[(size_t)(R - 1) * NX + (lane - O_T)] = acc;
}

template <int MODEL>
int launch_cost_param_gradient(const quattro_model_params& p, const float* x, const float* u, int B, int N, const float* costate,
                               const float* model_phys, const float* x_ref_rows, int ref_rows, const float* cost_rows,
                               double* grad_phys, double* grad_cost_rows, double* grad_ref_rows, hipStream_t stream) {
  const dim3 grid((unsigned)B), block(QT_WAVE);
  if (p.integrator == QUATTRO_INTEGRATOR_EULER)
    hipLaunchKernelGGL((cost_param_gradient_kernel<MODEL, false>), grid, block, 0, stream, p, x, u, N, costate, model_phys, x_ref_rows,
                       ref_rows, cost_rows, grad_phys, grad_cost_rows, grad_ref_rows);
  else if (p.integrator == QUATTRO_INTEGRATOR_RK4)
    hipLaunchKernelGGL((cost_param_gradient_kernel<MODEL, true>), grid, block, 0, stream, p, x, u, N, costate, model_phys, x_ref_rows,
                       ref_rows, cost_rows, grad_phys, grad_cost_rows, grad_ref_rows);
  else
    return QUATTRO_ERR_UNSUPPORTED;
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

}  // namespace

int quattro_launch_cost_param_gradient(const quattro_model_params& p, const float* x, const float* u, int B, int N,
                                       const float* costate, const float* model_phys, const float* x_ref_rows, int ref_rows,
                                       const float* cost_rows, double* grad_phys, double* grad_cost_rows, double* grad_ref_rows,
                                       hipStream_t stream) {
  if (p.model_id == QUATTRO_MODEL_CARTPOLE)
    return launch_cost_param_gradient<QUATTRO_MODEL_CARTPOLE>(p, x, u, B, N, costate, model_phys, x_ref_rows, ref_rows, cost_rows,
                                                              grad_phys, grad_cost_rows, grad_ref_rows, stream);
  if (p.model_id == QUATTRO_MODEL_QUADROTOR)
    return launch_cost_param_gradient<QUATTRO_MODEL_QUADROTOR>(p, x, u, B, N, costate, model_phys, x_ref_rows, ref_rows, cost_rows,
                                                               grad_phys, grad_cost_rows, grad_ref_rows, stream);
  return QUATTRO_ERR_UNSUPPORTED;
}
