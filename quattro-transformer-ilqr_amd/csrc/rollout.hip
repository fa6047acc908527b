// Rollout kernels: open-loop simulate + cost, closed-loop forward passes for all line-search step sizes, and
// the fused line search (evaluate every alpha, accept the first that does not increase the cost, commit it).
//
// Arithmetic replaced (reference quattro_ilqr_tf/quattro_ilqr_tf.py): simulate :127-132, compute_total_cost
// :138-143 (total_cost_kernel; term by term under per-trajectory rows: score_kernel), forward_pass :377-390, and the alpha loop + stop test of optimize :433-451, :472 (:546-563, :584).
//
// Serial in t by nature (x'_{t+1} depends on x'_t); parallel over (trajectory, alpha).  Eight lanes per
// trajectory (one per alpha, n_alpha <= 8) sit next to each other in a wave, so the loads of K_t, k_t, x_t, u_t
// they share are single broadcast requests, and "first accepted alpha" is one ballot.  The nominal data of step
// t+2 is requested while step t is computed (two register buffers, loop unrolled by two): with well under one wave
// per SIMD there is no other wave to hide the load latency behind.
// States and controls are fp32; the running sum of the cost is kept in fp64 because the accept test
// `cand_cost <= current_cost` (:444) and the stop test |dJ| < tol (:472) compare nearly equal totals.
#include "rollout_body.h"

namespace {

template <int MODEL, bool RK4>
__global__ __launch_bounds__(64) void simulate_kernel(const quattro_model_params p, const float* __restrict__ x0,
                                const float* __restrict__ u, int B, int N, float* __restrict__ x,
                                double* __restrict__ cost) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  simulate_body<MODEL, RK4>(p, x0, u, N, x, cost, b);
}

// sum_t L(x_t,u_t) + Lf(x_N) of given (x,u) sequences, which need not satisfy the dynamics
template <int MODEL>
__global__ __launch_bounds__(64) void total_cost_kernel(const quattro_model_params p, const float* __restrict__ x,
                                  const float* __restrict__ u, int B, int N, double* __restrict__ cost) {
  constexpr int NX = ModelDims<MODEL>::NX, NU = ModelDims<MODEL>::NU;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float* xb = x + (size_t)b * (N + 1) * NX;
  const float* ub = u + (size_t)b * N * NU;
  double J = 0.0;
  float xt[NX], ut[NU];
  for (int t = 0; t < N; ++t) {
    load_vec<NX>(xb + (size_t)t * NX, xt);
    load_vec<NU>(ub + (size_t)t * NU, ut);
    J += (double)qt_stage_cost<MODEL>(p, xt, ut);
  }
  load_vec<NX>(xb + (size_t)N * NX, xt);
  J += (double)qt_final_cost<MODEL>(p, xt);
  cost[b] = J;
}

// Scoring (quattro_score_f32): stage[b][s] = L(x_s, u_s) for s < S, slot S = Lf(x_S) or +0, total[b] = their fp64 sum in step order,
// each trajectory under rows of its own (phys, reference, weights; any of them NULL: the block's values).  One wave per trajectory,
// a step per lane, 64 steps a pass: the trajectory's q, qf, r, phys are wave-uniform, only x_ref and the step's (x, u) differ from lane
// to lane.  The block `own` is filled with VALUES behind wave-uniform branches (the way solve_loop.h's trajectory_params and
// set_ref_row fill theirs; code of this kernel's own), so every call runs the same cost code with or without rows.
// Lanes past the end of the last pass stay out of the branch that evaluates the cost: qt_stage_cost's __all(negligible) is then
// taken over lanes that hold a step, and its shortcut is exact whichever way it goes.  The ordered sum goes through 512 bytes of LDS
// (every lane adds the pass's terms in step order: the same J in all lanes), so it needs no global memory when stage == NULL.
template <int MODEL>
__global__ __launch_bounds__(QT_WAVE) void score_kernel(const quattro_model_params p, const float* __restrict__ x,
                                                        const float* __restrict__ u, const int S,
                                                        const float* __restrict__ model_phys, const float* __restrict__ x_ref_rows,
                                                        const int ref_rows, const int ref_hold, const float* __restrict__ cost_rows,
                                                        const int terminal, float* __restrict__ stage, double* __restrict__ total) {
  constexpr int NX = ModelDims<MODEL>::NX, NU = ModelDims<MODEL>::NU;
  __shared__ double term[QT_WAVE];
  const size_t bb = blockIdx.x;
  const int lane = threadIdx.x;
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
  const size_t steps = (size_t)S + 1;                          // slots of a trajectory: S stage costs and the terminal slot
  const float* xb = x + bb * steps * NX;
  const float* ub = u + bb * (size_t)S * NU;
  double J = 0.0;
  for (size_t base = 0; base < steps; base += QT_WAVE) {
    float c = 0.0f;
    if (base + lane < steps) {
      const int s = (int)(base + lane);
      float xs[NX], xr[NX];
      load_vec<NX>(xb + (size_t)s * NX, xs);
#pragma unroll
      for (int i = 0; i < NX; ++i) xr[i] = p.x_ref[i];
      if (x_ref_rows != nullptr) {
        const int held = (s / ref_hold) * ref_hold;
        const int row = held < ref_rows - 1 ? held : ref_rows - 1;
        const float* rr = x_ref_rows + (bb * (size_t)ref_rows + (size_t)row) * NX;
#pragma unroll
        for (int i = 0; i < NX; ++i) xr[i] = rr[i];
      }
#pragma unroll
      for (int i = 0; i < NX; ++i) own.x_ref[i] = xr[i];
      if (s < S) {
        float us[NU];
        load_vec<NU>(ub + (size_t)s * NU, us);
        c = qt_stage_cost<MODEL>(own, xs, us);
      } else if (terminal != 0) {
        c = qt_final_cost<MODEL>(own, xs);
      }
      if (stage != nullptr) stage[bb * steps + (size_t)s] = c;
    }
    term[lane] = (double)c;
    __syncthreads();
    const int cnt = steps - base < (size_t)QT_WAVE ? (int)(steps - base) : QT_WAVE;
    for (int i = 0; i < cnt; ++i) J += term[i];
    __syncthreads();
  }
  if (lane == 0) total[bb] = J;
}

// costs (and optionally trajectories) of every (trajectory, alpha): thread = b * 8 + alpha slot
template <int MODEL, bool RK4>
__global__ __launch_bounds__(64) void rollout_kernel(const quattro_model_params p, const float* __restrict__ x_nom,
                               const float* __restrict__ u_nom, const float* __restrict__ K,
                               const float* __restrict__ k, AlphaList al, int n_alpha, int B, int N,
                               float* __restrict__ x_new, float* __restrict__ u_new, double* __restrict__ cost,
                               const int32_t* __restrict__ active) {
  constexpr int NX = ModelDims<MODEL>::NX, NU = ModelDims<MODEL>::NU;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = gid >> 3, ai = gid & 7;
  if (b >= B || ai >= n_alpha) return;
  if (active != nullptr && active[b] == 0) return;
  const float* xn = x_nom + (size_t)b * (N + 1) * NX;
  const float* un = u_nom + (size_t)b * N * NU;
  const float* Kb = K + (size_t)b * N * NU * NX;
  const float* kb = k + (size_t)b * N * NU;
  double J;
  if (x_new != nullptr && u_new != nullptr) {
    float* xo = x_new + ((size_t)ai * B + b) * (N + 1) * NX;
    float* uo = u_new + ((size_t)ai * B + b) * N * NU;
    float x0[NX];
    load_vec<NX>(xn, x0);
    store_vec<NX>(xo, x0);
    J = rollout_closed<MODEL, RK4>(p, xn, un, Kb, kb, al.a[ai], N, ArrayStore<MODEL>{xo, uo});
  } else {
    J = rollout_closed<MODEL, RK4>(p, xn, un, Kb, kb, al.a[ai], N, NoStore{});
  }
  cost[(size_t)ai * B + b] = J;
}

// Fused line search: 8 lanes per trajectory (linesearch_body)
template <int MODEL, bool RK4>
__global__ __launch_bounds__(64) void linesearch_kernel(const quattro_model_params p, float* x_nom, float* u_nom,
                                  const float* __restrict__ K, const float* __restrict__ k, AlphaList al, int n_alpha,
                                  int B, int N, double tol, double* cost, int32_t* __restrict__ alpha_idx,
                                  int32_t* active, int32_t* iters, float* __restrict__ scratch) {
  linesearch_body<MODEL, RK4, 8>(p, x_nom, u_nom, K, k, al, n_alpha, B, N, tol, cost, alpha_idx, active, iters, scratch,
                                 blockIdx.x * blockDim.x + threadIdx.x, false);
}

// tracked plant steps (quattro_track_f32): one lane per trajectory; the steps themselves are track_body, the function the
// persistent MPC loops run between their solves
template <int MODEL>
__global__ __launch_bounds__(64) void track_kernel(const quattro_model_params p, const PlantSpec plant,
                                                   const float* __restrict__ plant_phys, const float* __restrict__ x0,
                                                   const float* __restrict__ x_nom, const float* __restrict__ u_nom,
                                                   const float* __restrict__ K, const int feedback, const int B, const int N,
                                                   const int n_steps, const float* __restrict__ disturbance,
                                                   float* __restrict__ x_out, float* __restrict__ u_out) {
  constexpr int NX = ModelDims<MODEL>::NX, NU = ModelDims<MODEL>::NU;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const size_t bb = b;
  float xh[NX];
  load_vec<NX>(x0 + bb * NX, xh);
  float* xrows = x_out + bb * (size_t)(n_steps + 1) * NX;
  store_vec<NX>(xrows, xh);
  track_body<MODEL>(p, plant, plant_phys, feedback != 0, x_nom + bb * (N + 1) * NX, u_nom + bb * N * NU, K + bb * N * NU * NX, xh,
                    n_steps, disturbance != nullptr ? disturbance + bb * NX : nullptr, (size_t)B * NX, xrows,
                    u_out + bb * (size_t)n_steps * NU, bb);
}

}  // namespace

// the one-lane-per-candidate kernels of this file serve the cart-pole; quadrotor calls were routed to rollout_quad.hip
// by the launchers before they get here
#ifdef QT_USER_MODEL_HEADER
#define QT_DISPATCH_USER(p, ...)                           \
  else if ((p).model_id == QUATTRO_MODEL_USER) {           \
    constexpr int MODEL = QUATTRO_MODEL_USER;              \
    QT_DISPATCH_INTEG(p, __VA_ARGS__);                     \
  }
#else
#define QT_DISPATCH_USER(p, ...)
#endif
#define QT_DISPATCH_MODEL(p, ...)                          \
  if ((p).model_id == QUATTRO_MODEL_CARTPOLE) {            \
    constexpr int MODEL = QUATTRO_MODEL_CARTPOLE;          \
    QT_DISPATCH_INTEG(p, __VA_ARGS__);                     \
  }                                                        \
  QT_DISPATCH_USER(p, __VA_ARGS__)                         \
  else {                                                   \
    return QUATTRO_ERR_UNSUPPORTED;                        \
  }

// quadrotor: lane-cooperative kernels (rollout_quad.hip)
int quattro_launch_simulate_quad(const quattro_model_params&, const float*, const float*, int, int, float*, double*,
                                 hipStream_t);
int quattro_launch_rollout_quad(const quattro_model_params&, const float*, const float*, const float*, const float*,
                                const float*, int, int, int, float*, float*, double*, const int32_t*, hipStream_t);
int quattro_launch_linesearch_quad(const quattro_model_params&, float*, float*, const float*, const float*,
                                   const float*, int, int, int, double, double*, int32_t*, int32_t*, int32_t*, float*,
                                   hipStream_t);
int quattro_launch_track_quad(const quattro_model_params&, const PlantSpec&, const float*, const float*, const float*,
                              const float*, const float*, int, int, int, int, const float*, float*, float*, hipStream_t);

size_t quattro_linesearch_scratch_bytes_impl(int n, int m, int B, int N) {
  const size_t cs = (size_t)((n + m + 3) / 4 * 4);
  return (size_t)B * 8 * (size_t)N * cs * sizeof(float);
}

int quattro_launch_simulate(const quattro_model_params& p, const float* x0, const float* u, int B, int N, float* x,
                            double* cost, hipStream_t stream) {
  if (p.model_id == QUATTRO_MODEL_QUADROTOR) return quattro_launch_simulate_quad(p, x0, u, B, N, x, cost, stream);
  const int threads = 64;
  QT_DISPATCH_MODEL(p, hipLaunchKernelGGL((simulate_kernel<MODEL, RK4>), dim3((B + threads - 1) / threads), dim3(threads),
                                          0, stream, p, x0, u, B, N, x, cost));
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

int quattro_launch_total_cost(const quattro_model_params& p, const float* x, const float* u, int B, int N,
                              double* cost, hipStream_t stream) {
  const int threads = 64;
  const dim3 grid((B + threads - 1) / threads);
  if (p.model_id == QUATTRO_MODEL_CARTPOLE)
    hipLaunchKernelGGL((total_cost_kernel<QUATTRO_MODEL_CARTPOLE>), grid, dim3(threads), 0, stream, p, x, u, B, N, cost);
  else if (p.model_id == QUATTRO_MODEL_QUADROTOR)
    hipLaunchKernelGGL((total_cost_kernel<QUATTRO_MODEL_QUADROTOR>), grid, dim3(threads), 0, stream, p, x, u, B, N, cost);
#ifdef QT_USER_MODEL_HEADER
  else if (p.model_id == QUATTRO_MODEL_USER)
    hipLaunchKernelGGL((total_cost_kernel<QUATTRO_MODEL_USER>), grid, dim3(threads), 0, stream, p, x, u, B, N, cost);
#endif
  else
    return QUATTRO_ERR_UNSUPPORTED;
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

// one wave (one workgroup) per trajectory; the quadrotor too: the generic stage and final cost, no lane-cooperative form
int quattro_launch_score(const quattro_model_params& p, const float* x, const float* u, int B, int S, const float* model_phys,
                         const float* x_ref_rows, int ref_rows, int ref_hold, const float* cost_rows, int terminal, float* stage,
                         double* total, hipStream_t stream) {
  const dim3 grid((unsigned)B), block(QT_WAVE);
  if (p.model_id == QUATTRO_MODEL_CARTPOLE)
    hipLaunchKernelGGL((score_kernel<QUATTRO_MODEL_CARTPOLE>), grid, block, 0, stream, p, x, u, S, model_phys, x_ref_rows, ref_rows,
                       ref_hold, cost_rows, terminal, stage, total);
  else if (p.model_id == QUATTRO_MODEL_QUADROTOR)
    hipLaunchKernelGGL((score_kernel<QUATTRO_MODEL_QUADROTOR>), grid, block, 0, stream, p, x, u, S, model_phys, x_ref_rows, ref_rows,
                       ref_hold, cost_rows, terminal, stage, total);
#ifdef QT_USER_MODEL_HEADER
  else if (p.model_id == QUATTRO_MODEL_USER)
    hipLaunchKernelGGL((score_kernel<QUATTRO_MODEL_USER>), grid, block, 0, stream, p, x, u, S, model_phys, x_ref_rows, ref_rows,
                       ref_hold, cost_rows, terminal, stage, total);
#endif
  else
    return QUATTRO_ERR_UNSUPPORTED;
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

int quattro_launch_rollout(const quattro_model_params& p, const float* x_nom, const float* u_nom, const float* K,
                           const float* k, const float* alphas, int n_alpha, int B, int N, float* x_new, float* u_new,
                           double* cost, const int32_t* active, hipStream_t stream) {
  if (p.model_id == QUATTRO_MODEL_QUADROTOR)
    return quattro_launch_rollout_quad(p, x_nom, u_nom, K, k, alphas, n_alpha, B, N, x_new, u_new, cost, active, stream);
  const AlphaList al = make_alpha_list(alphas, n_alpha);
  const int threads = 64;
  const long long tot = (long long)B * 8;
  QT_DISPATCH_MODEL(p, hipLaunchKernelGGL((rollout_kernel<MODEL, RK4>), dim3((unsigned)((tot + threads - 1) / threads)),
                                          dim3(threads), 0, stream, p, x_nom, u_nom, K, k, al, n_alpha, B, N, x_new,
                                          u_new, cost, active));
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

int quattro_launch_linesearch(const quattro_model_params& p, float* x_nom, float* u_nom, const float* K,
                              const float* k, const float* alphas, int n_alpha, int B, int N, double tol, double* cost,
                              int32_t* alpha_idx, int32_t* active, int32_t* iters, float* scratch,
                              hipStream_t stream) {
  if (p.model_id == QUATTRO_MODEL_QUADROTOR)
    return quattro_launch_linesearch_quad(p, x_nom, u_nom, K, k, alphas, n_alpha, B, N, tol, cost, alpha_idx, active,
                                          iters, scratch, stream);
  const AlphaList al = make_alpha_list(alphas, n_alpha);
  const int threads = 64;
  const long long tot = (long long)B * 8;
  QT_DISPATCH_MODEL(p, hipLaunchKernelGGL((linesearch_kernel<MODEL, RK4>), dim3((unsigned)((tot + threads - 1) / threads)),
                                          dim3(threads), 0, stream, p, x_nom, u_nom, K, k, al, n_alpha, B, N, tol, cost,
                                          alpha_idx, active, iters, scratch));
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

int quattro_launch_track(const quattro_model_params& p, const PlantSpec& plant, const float* plant_phys, const float* x0,
                         const float* x_nom, const float* u_nom, const float* K, int feedback, int B, int N, int n_steps,
                         const float* disturbance, float* x_out, float* u_out, hipStream_t stream) {
  if (p.model_id == QUATTRO_MODEL_QUADROTOR)
    return quattro_launch_track_quad(p, plant, plant_phys, x0, x_nom, u_nom, K, feedback, B, N, n_steps, disturbance, x_out, u_out,
                                     stream);
  const int threads = 64;
  const dim3 grid((B + threads - 1) / threads);
  if (p.model_id == QUATTRO_MODEL_CARTPOLE)
    hipLaunchKernelGGL((track_kernel<QUATTRO_MODEL_CARTPOLE>), grid, dim3(threads), 0, stream, p, plant, plant_phys, x0, x_nom, u_nom,
                       K, feedback, B, N, n_steps, disturbance, x_out, u_out);
#ifdef QT_USER_MODEL_HEADER
  else if (p.model_id == QUATTRO_MODEL_USER)
    hipLaunchKernelGGL((track_kernel<QUATTRO_MODEL_USER>), grid, dim3(threads), 0, stream, p, plant, plant_phys, x0, x_nom, u_nom, K,
                       feedback, B, N, n_steps, disturbance, x_out, u_out);
#endif
  else
    return QUATTRO_ERR_UNSUPPORTED;
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}
