// Device-resident iLQR solve loop and receding-horizon (MPC) loop for the cart-pole: ONE launch runs, for every trajectory, the
// whole `while` loop of iLQR_TF.optimize (quattro_ilqr_tf/quattro_ilqr_tf.py:428-472) and, in MPC mode, the caller's loop
// around it (examples/cartpole/cartpole_mpc.py:326-332: solve, apply u_0, shift the warm start), with no host involvement.
// Same idea as solve_quad.hip (trajectories are independent: no grid-wide dependency anywhere), smaller grain: a trajectory
// owns a 16-lane DPP row of a wave — what the sweep needs (cartpole_body.h) — so a wave carries four trajectories and the
// whole loop is WAVE-private: no workgroup barrier at all, the phases hand their data over through global memory in program
// order of one wave.
//   nominal rollout : lane 0 of the row                               (rollout_body.h: simulate_body)
//   sweep           : the row's 16 lanes                              (cartpole_body.h: sweep16_cartpole_body)
//   line search     : lanes 0..5 of the row roll the candidates out, all 16 copy the accepted one
//                                                                     (rollout_body.h: linesearch_body<.., 16>)
// BASELINE configs[1] (B = 1024) is 256 such waves on 1024 SIMDs: every wave runs alone, an iteration costs the sum of its
// chains and nothing else — no launch, no kernel boundary, no host call.
#include "cartpole_body.h"
#include "rollout_body.h"
#include "solve_loop.h"

namespace {

struct CpSolveArgs {
  quattro_model_params p;
  SolveLoop c;          // x [B][N+1][4], u [B][N][1], K [B][N][1][4], k [B][N][1]
};

// PLANT: the loop of quattro_mpc_run_plant_f32 (a plant of its own, c.hold tracked steps per plan); the <RK4, false> code is the
// loop as it always was
// PHYS (with PLANT only: quattro_ilqr_solve_phys_f32 has n_ctrl == 0 and never reaches the MPC code): every row evaluates its
// trajectory's model — nominal rollout, records, terminal pair, line search — on a block whose phys is its row of c.model_phys
// REF (with PLANT only, like PHYS): the cost of horizon step t is taken against the row of c.x_ref_rows that step reads
// (qt_ref_row): the row's private block gets it as x_ref before every stage cost, record and terminal pair (set_ref_row)
// COST (with PLANT only; alone, or with PHYS and REF together, each of which then also runs without its array: trajectory_params,
// rows_given): the private block's q, qf and r are the trajectory's row of c.cost_rows, so every cost evaluated on that block follows
template <bool RK4, bool PLANT, bool PHYS, bool REF, bool COST>
__global__ __launch_bounds__(QT_WAVE) void solve_cartpole_kernel(const CpSolveArgs a) {
  constexpr int MODEL = QUATTRO_MODEL_CARTPOLE, NX = 4;
  __shared__ __attribute__((aligned(16))) float s_stage[4 * cp16::STAGE_FLOATS];
  const SolveLoop& c = a.c;
  const int lane = threadIdx.x;
  const int sub = lane & 15;
  const int b = blockIdx.x * 4 + (lane >> 4);
  const bool have = b < c.B;
  const size_t bb = have ? b : 0;
  const bool force = (c.flags & QUATTRO_SOLVE_FIXED_ITERS) != 0;
  const int N = c.N;
  float* stage = s_stage + (lane >> 4) * cp16::STAGE_FLOATS;
  quattro_model_params own;
  const quattro_model_params& mp = trajectory_params<PHYS, REF, COST>(a.p, c, bb, own);
  const int n_ctrl = c.n_ctrl > 0 ? c.n_ctrl : 1;
  for (int cs = 0; cs < n_ctrl; ++cs) {
    auto ref = [&](int t) __attribute__((always_inline)) {
      if constexpr (REF) {
        if (rows_given<REF, COST>(c)) set_ref_row<NX>(own, plan_ref_rows(c, cs), bb, t);
      }
    };
    wave_step_prologue<NX, PLANT>(c, bb, cs, have && sub == 0,
                           [&] { simulate_body<MODEL, RK4>(mp, c.x0, c.u, N, c.x, c.cost, b, ref); });
    const bool logging = c.log.rec != nullptr && c.n_ctrl == 0;
    for (int it = 0; it < c.max_iter; ++it) {
      const bool act = have && (force || c.active[bb] != 0);
      if (!__any(act)) break;
      int log_it = 0;
      if (logging && act) {      // the record of this iteration: nominal, cost, start stamp (the row's 16 lanes)
        log_it = c.iters[bb];
        log_begin(c.log, b, log_it, c.x + bb * (N + 1) * NX, c.u + bb * N, c.cost[bb], sub, 16);
      }
      sweep16_cartpole_body<RK4, PHYS || REF || COST>(mp, c.x, c.u, N, 0, c.reg, c.K, c.k, c.status, b, act, lane, stage, 0, &a.p, ref,
                                                      COST ? c.cost_rows + bb * QUATTRO_COST_ROW_FLOATS + QUATTRO_MAX_NX : nullptr);
      if (logging && act && sub == 0) log_stamp(c.log, b, log_it, 1, 2);
      wave_handoff();
      linesearch_body<MODEL, RK4, 16>(mp, c.x, c.u, c.K, c.k, c.al, c.n_alpha, c.B, N, c.tol, c.cost, c.alpha_idx, c.active,
                                      c.iters, c.scratch, 16 * b + sub, force, ref);
      wave_handoff();
      if (logging && act)        // gains, accepted step, cost after the iteration, end stamp
        log_end(c.log, b, log_it, c.K + bb * N * NX, c.k + bb * N, c.alpha_idx[bb], c.cost[bb], sub, 16);
    }
    // apply u_0, record, shift the warm start: CartPoleMPC._ilqr_step after optimize() (cartpole_mpc.py:331) and the
    // simulator's step around it
    if (c.n_ctrl > 0)
      wave_mpc_epilogue<NX, 1, 16, PLANT>(c, bb, cs, sub, have,
                                          [&](const float* xo, const float* u0, float* xn) { qt_step<MODEL, RK4>(mp, xo, u0, xn); },
                                          [&](float* xh, const size_t s0) { track_plan<MODEL>(a.p, c, bb, xh, s0); });
  }
}

}  // namespace

int quattro_launch_solve_cartpole(const quattro_model_params& p, const SolveLoop& c, hipStream_t stream) {
  const CpSolveArgs a{p, c};
  const dim3 grid((unsigned)((c.B + 3) / 4));
  if (p.integrator != QUATTRO_INTEGRATOR_EULER && p.integrator != QUATTRO_INTEGRATOR_RK4) return QUATTRO_ERR_UNSUPPORTED;
  const bool rk4 = p.integrator == QUATTRO_INTEGRATOR_RK4;
  // (c.x_ref_rows: the two ref entries alone set it; c.model_phys: they and the two phys entries; c.hold: the plant run and those)
#define QT_LAUNCH(PLANT, PHYS, REF, COST)                                                                                     \
  do {                                                                                                                  \
    if (rk4) hipLaunchKernelGGL((solve_cartpole_kernel<true, PLANT, PHYS, REF, COST>), grid, dim3(QT_WAVE), 0, stream, a);    \
    else hipLaunchKernelGGL((solve_cartpole_kernel<false, PLANT, PHYS, REF, COST>), grid, dim3(QT_WAVE), 0, stream, a);       \
  } while (0)
  // (c.cost_rows: the two cost entries alone set it; weights alone have a kernel of their own, weights with either array share one)
  if (c.cost_rows != nullptr && (c.x_ref_rows != nullptr || c.model_phys != nullptr)) QT_LAUNCH(true, true, true, true);
  else if (c.cost_rows != nullptr) QT_LAUNCH(true, false, false, true);
  else if (c.x_ref_rows != nullptr && c.model_phys != nullptr) QT_LAUNCH(true, true, true, false);
  else if (c.x_ref_rows != nullptr) QT_LAUNCH(true, false, true, false);
  else if (c.model_phys != nullptr) QT_LAUNCH(true, true, false, false);
  else if (c.hold > 0) QT_LAUNCH(true, false, false, false);
  else QT_LAUNCH(false, false, false, false);
#undef QT_LAUNCH
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}
