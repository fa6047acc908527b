// Cost gradient with respect to what a trajectory's rows hold, for a USER-COMPILED model (quattro_cost_param_gradient_f32 of a library
// built by compile_model(..., param_grad=True); cost_param_gradient.hip is the built-in models' kernel and documents the outputs):
//   grad_phys[k]        = sum_{t<N} [ sum_i lambda_{t+1,i} d f_i / d theta_k (x_t, u_t; theta) + dL/dtheta_k (x_t, u_t) ] + dLf/dtheta_k (x_N)
//   grad_cost_rows[e]   = sum_{t<N} dL/de + dLf/de          e any of q_i, qf_i, r_a: a user's cost may read any weight in either cost
//   grad_ref_rows[rho]  = sum_{t<N, min(t,R-1)=rho} dL/dx_ref_i + [min(N,R-1)=rho] dLf/dx_ref_i   (the row rule of the adjoint sweep)
// f is the whole integrator step qt_user::step<D, RK4>, theta the trajectory's own phys.  Nothing is known about the three bodies, so
// every partial is a forward-mode derivative: the bodies are instantiated with T = Dual<float> and a parameter block whose phys, q,
// qf, r and x_ref are duals (UserParamBlock), one direction seeded at a time, x and u duals with zero tangent.  The three classes of
// direction run as separate loops that are NOT unrolled: in each only the seeded class carries a tangent that is not a literal zero,
// the weight and target directions evaluate the costs alone, and a direction's term goes to LDS as it is formed (a register array of
// terms indexed by the direction would live in scratch).
//
// The mapping and the arithmetic are cost_param_gradient_kernel's: one wave per trajectory, a slot per lane, 64 slots a pass; slot
// s < N is horizon step s, slot N the terminal term.  A lane forms each fp32 term of its slot -- for a parameter the fmaf chain over
// lambda_{t+1} plus the cost's own derivative, rounded once -- and leaves it in LDS, one row of 64 per output entry, rows 65 floats
// apart.  Then lane o adds row o to its fp64 accumulator in slot order: no atomics, no workspace, and trajectory b's results are those
// of a B = 1 call with row b in the struct, bit for bit; an output does not depend on which others are asked for.  An entry with a
// single term (a target row below the last) is that term added to +0.0.
// Only compiled into a library built with -DQT_USER_PARAM_GRAD=1 -DQT_USER_NP=len(phys).
#include "rollout_body.h"

#if !defined(QT_USER_MODEL_HEADER) || !defined(QT_USER_NP)
#error "user_param_gradient.hip is part of a user model's library built with param_grad=True"
#endif

namespace {

using D = qtad::Dual<float>;

// quattro_model_params as the generated bodies read it, with everything that is differentiated held in T
template <class T>
struct UserParamBlock {
  float dt, barrier_alpha, barrier_beta;
  T phys[8];
  T q[QUATTRO_MAX_NX];
  T qf[QUATTRO_MAX_NX];
  T x_ref[QUATTRO_MAX_NX];
  T r[QUATTRO_MAX_NU];
};

constexpr int NX = QT_USER_NX, NU = QT_USER_NU, NP = QT_USER_NP;
constexpr int NW = 2 * NX + NU;       // weight directions in the order q | qf | r

// the block of one direction: CLASS 0 phys, 1 weights, 2 targets; every other tangent is a literal zero
template <int CLASS>
__device__ __forceinline__ void seed_block(UserParamBlock<D>& pb, const quattro_model_params& p, const float* ph, const float* q,
                                           const float* qf, const float* r, const float* xr, const int dir) {
  pb.dt = p.dt;
  pb.barrier_alpha = p.barrier_alpha;
  pb.barrier_beta = p.barrier_beta;
#pragma unroll
  for (int i = 0; i < 8; ++i) pb.phys[i] = D(ph[i], (CLASS == 0 && i == dir) ? 1.0f : 0.0f);
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    pb.q[i] = D(q[i], (CLASS == 1 && i == dir) ? 1.0f : 0.0f);
    pb.qf[i] = D(qf[i], (CLASS == 1 && NX + i == dir) ? 1.0f : 0.0f);
    pb.x_ref[i] = D(xr[i], (CLASS == 2 && i == dir) ? 1.0f : 0.0f);
  }
#pragma unroll
  for (int a = 0; a < NU; ++a) pb.r[a] = D(r[a], (CLASS == 1 && 2 * NX + a == dir) ? 1.0f : 0.0f);
}

template <bool RK4>
__global__ __launch_bounds__(QT_WAVE) void user_param_gradient_kernel(
    const quattro_model_params p, const float* __restrict__ x, const float* __restrict__ u, const int N,
    const float* __restrict__ costate, const float* __restrict__ model_phys, const float* __restrict__ x_ref_rows, const int ref_rows,
    const float* __restrict__ cost_rows, double* __restrict__ grad_phys, double* __restrict__ grad_cost_rows,
    double* __restrict__ grad_ref_rows) {
  // output entries that are sums over slots, one LDS row and one summing lane each: phys | q | qf | r | the last target row
  constexpr int O_Q = NP, O_QF = NP + NX, O_R = NP + 2 * NX, O_T = NP + NW, NOUT = NP + NW + NX;
  constexpr int PITCH = QT_WAVE + 1;
  static_assert(NOUT <= QT_WAVE && NP <= 8, "one summing lane per output entry");
  __shared__ float s_term[NOUT * PITCH];
  __shared__ double s_cost[QUATTRO_COST_ROW_FLOATS];
  const size_t bb = blockIdx.x;
  const int lane = threadIdx.x;

  float q[NX], qf[NX], r[NU], ph[8];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    q[i] = p.q[i];
    qf[i] = p.qf[i];
  }
#pragma unroll
  for (int a = 0; a < NU; ++a) r[a] = p.r[a];
#pragma unroll
  for (int i = 0; i < 8; ++i) ph[i] = p.phys[i];
  if (cost_rows != nullptr) {
    const float* w = cost_rows + bb * QUATTRO_COST_ROW_FLOATS;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      q[i] = w[i];
      qf[i] = w[QUATTRO_MAX_NX + i];
    }
#pragma unroll
    for (int a = 0; a < NU; ++a) r[a] = w[2 * QUATTRO_MAX_NX + a];
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
  // target rows past the horizon, the last one included when it lies there: +0.0
  if (gref != nullptr) {
    for (int row = N + 1 + lane; row < R; row += QT_WAVE) {
#pragma unroll
      for (int i = 0; i < NX; ++i) gref[(size_t)row * NX + i] = 0.0;
    }
  }
  // the summing lane of an entry nobody asked for has nothing to add (its LDS row is never written)
  const bool sums = lane < O_Q ? grad_phys != nullptr : lane < O_T ? grad_cost_rows != nullptr : lane < NOUT && gref != nullptr;

  double acc = 0.0;
  const int slots = N + 1;
  for (int base = 0; base < slots; base += QT_WAVE) {
    const int s = base + lane;
    if (s < slots) {
      const bool stage = s < N;
      float xs[NX], xr[NX], us[NU];
      load_vec<NX>(xb + (size_t)s * NX, xs);
#pragma unroll
      for (int a = 0; a < NU; ++a) us[a] = 0.0f;
      if (stage) load_vec<NU>(ub + (size_t)s * NU, us);
#pragma unroll
      for (int i = 0; i < NX; ++i) xr[i] = p.x_ref[i];
      if (x_ref_rows != nullptr) {
        const int row = s < R - 1 ? s : R - 1;
        const float* rr = x_ref_rows + (bb * (size_t)ref_rows + (size_t)row) * NX;
#pragma unroll
        for (int i = 0; i < NX; ++i) xr[i] = rr[i];
      }
      D xd[NX], ud[NU];
#pragma unroll
      for (int i = 0; i < NX; ++i) xd[i] = D(xs[i], 0.0f);
#pragma unroll
      for (int a = 0; a < NU; ++a) ud[a] = D(us[a], 0.0f);

      if (grad_phys != nullptr) {
        float lam[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) lam[i] = 0.0f;
        if (stage) load_vec<NX>(costate + (bb * (size_t)(N + 1) + (size_t)(s + 1)) * NX, lam);
#pragma unroll 1
        for (int k = 0; k < NP; ++k) {
          UserParamBlock<D> pb;
          seed_block<0>(pb, p, ph, q, qf, r, xr, k);
          float term;
          if (stage) {
            D xn[NX];
            qt_user::step<D, RK4>(pb, xd, ud, xn);
            float v = 0.0f;
#pragma unroll
            for (int i = 0; i < NX; ++i) v = fmaf(lam[i], xn[i].d, v);
            term = v + qt_user::stage_cost<D>(pb, xd, ud).d;
          } else {
            term = qt_user::final_cost<D>(pb, xd).d;
          }
          s_term[k * PITCH + lane] = term;
        }
      }
      if (grad_cost_rows != nullptr) {
#pragma unroll 1
        for (int e = 0; e < NW; ++e) {
          UserParamBlock<D> pb;
          seed_block<1>(pb, p, ph, q, qf, r, xr, e);
          s_term[(O_Q + e) * PITCH + lane] = stage ? qt_user::stage_cost<D>(pb, xd, ud).d : qt_user::final_cost<D>(pb, xd).d;
        }
      }
      if (gref != nullptr) {
#pragma unroll 1
        for (int i = 0; i < NX; ++i) {
          UserParamBlock<D> pb;
          seed_block<2>(pb, p, ph, q, qf, r, xr, i);
          const float tg = stage ? qt_user::stage_cost<D>(pb, xd, ud).d : qt_user::final_cost<D>(pb, xd).d;
          if (s < R - 1) {           // a row of its own: this slot is its only term
            gref[(size_t)s * NX + i] = 0.0 + (double)tg;
            s_term[(O_T + i) * PITCH + lane] = 0.0f;
          } else {
            s_term[(O_T + i) * PITCH + lane] = tg;
          }
        }
      }
    }
    __syncthreads();
    const int cnt = slots - base < QT_WAVE ? slots - base : QT_WAVE;
    if (sums) {
      const float* mine = s_term + lane * PITCH;
      for (int i = 0; i < cnt; ++i) acc += (double)mine[i];
    }
    __syncthreads();
  }

  if (lane >= O_Q && lane < O_QF) s_cost[lane - O_Q] = acc;
  if (lane >= O_QF && lane < O_R) s_cost[QUATTRO_MAX_NX + (lane - O_QF)] = acc;
  if (lane >= O_R && lane < O_T) s_cost[2 * QUATTRO_MAX_NX + (lane - O_R)] = acc;
  __syncthreads();
  if (grad_phys != nullptr && lane < 8) grad_phys[bb * 8 + lane] = lane < NP ? acc : 0.0;
  if (grad_cost_rows != nullptr && lane < QUATTRO_COST_ROW_FLOATS)
    grad_cost_rows[bb * QUATTRO_COST_ROW_FLOATS + lane] = s_cost[lane];
  // the last target row, where it lies inside the horizon (slot R - 1 exists): the sum of every slot from R - 1 on
  if (gref != nullptr && R - 1 <= N && lane >= O_T && lane < NOUT) gref[(size_t)(R - 1) * NX + (lane - O_T)] = acc;
}

}  // namespace

int quattro_launch_user_param_gradient(const quattro_model_params& p, const float* x, const float* u, int B, int N,
                                       const float* costate, const float* model_phys, const float* x_ref_rows, int ref_rows,
                                       const float* cost_rows, double* grad_phys, double* grad_cost_rows, double* grad_ref_rows,
                                       hipStream_t stream) {
  const dim3 grid((unsigned)B), block(QT_WAVE);
  if (p.integrator == QUATTRO_INTEGRATOR_EULER)
    hipLaunchKernelGGL((user_param_gradient_kernel<false>), grid, block, 0, stream, p, x, u, N, costate, model_phys, x_ref_rows,
                       ref_rows, cost_rows, grad_phys, grad_cost_rows, grad_ref_rows);
  else if (p.integrator == QUATTRO_INTEGRATOR_RK4)
    hipLaunchKernelGGL((user_param_gradient_kernel<true>), grid, block, 0, stream, p, x, u, N, costate, model_phys, x_ref_rows,
                       ref_rows, cost_rows, grad_phys, grad_cost_rows, grad_ref_rows);
  else
    return QUATTRO_ERR_UNSUPPORTED;
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}
