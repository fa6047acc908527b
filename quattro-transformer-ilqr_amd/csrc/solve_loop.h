// What the three device-resident solve loops share (solve_quad.hip, solve_cartpole.hip, solve_user.hip): the block of loop
// arguments every one of them takes, filled on the host by capi.hip from the C entry's arguments, and the wave-private pieces
// of the control step that the cart-pole and user-model loops run alike.  The quadrotor's two-wave workgroup loop has a lane
// mapping of its own and keeps its prologue and MPC step in solve_quad.hip.
#pragma once
#include "solve_log.h"

// (outside the anonymous namespace: the kernel launchers take it from capi.hip)
struct SolveLoop {
  const float* x0;      // [B][n]  states the rollouts start from (MPC: the controllers' current states, == x_cur)
  float* x;             // [B][N+1][n]  nominal, in/out
  float* u;             // [B][N][m]
  float* K;             // [B][N][m][n]
  float* k;             // [B][N][m]
  double* cost;         // [B]
  int32_t* alpha_idx;   // [B]
  int32_t* active;      // [B]
  int32_t* iters;       // [B]
  int32_t* status;      // [B] (may be NULL)
  float* scratch;       // line-search candidates
  AlphaList al;
  int n_alpha, B, N, max_iter, flags;   // flags: QUATTRO_SOLVE_SIMULATE | QUATTRO_SOLVE_FIXED_ITERS | QUATTRO_SOLVE_RESET
  float reg;
  double tol;
  // receding-horizon mode (n_ctrl > 0)
  int n_ctrl;
  float* x_cur;               // [B][n]  == x0 (writable)
  float* traj_x;              // [B][n_ctrl+1][n]
  float* traj_u;              // [B][n_ctrl][m]
  int32_t* traj_iters;        // [B][n_ctrl]
  const float* disturbance;   // [n_ctrl][B][n] or NULL
  // a plant of its own and gain feedback between solves (quattro_mpc_run_plant_f32; the PLANT instantiations of the kernels).
  // n_ctrl then counts PLANS: each is followed by `hold` tracked plant steps, the trajectory arrays hold n_ctrl * hold steps
  // (traj_iters one entry per plan) and the warm start shifts by `hold`.  hold == 0: the loops above as they always were.
  PlantSpec plant;            // the plant's integrator and physical parameters
  const float* plant_phys;    // [B][8] per-controller physical parameters, or NULL
  int hold, feedback;
  SolveLogDev log;            // per-iteration log ring (rec == nullptr: none); plain solves only (n_ctrl == 0)
  // per-trajectory model parameters (quattro_ilqr_solve_phys_f32, quattro_mpc_run_phys_f32; the PHYS instantiations of the kernels):
  // row b replaces the parameter block's phys wherever the controller's model of trajectory b is evaluated.  NULL: none.
  const float* model_phys;    // [B][8]
  // reference rows (quattro_ilqr_solve_ref_f32, quattro_mpc_run_ref_f32; the REF instantiations of the kernels): row
  // min(s + preview * t, ref_rows - 1) of trajectory b replaces the parameter block's x_ref at horizon step t of the plan that starts
  // at plant step s (qt_ref_row, quattro_device.h).  A plain solve has s = 0 and preview = 1.  NULL: none.
  const float* x_ref_rows;    // [B][ref_rows][n]
  int ref_rows, preview;
  // per-trajectory cost weights (quattro_ilqr_solve_cost_f32, quattro_mpc_run_cost_f32; the COST instantiations of the kernels): row b
  // (q at float 0, qf at float 16, r at float 32: the parameter block's three arrays, back to back) replaces the block's q, qf and r wherever the cost of
  // trajectory b is evaluated, constant over the horizon and over a run.  NULL: none.
  const float* cost_rows;     // [B][QUATTRO_COST_ROW_FLOATS]
};

namespace {

// plant steps a run records (the trajectory arrays' row count)
template <bool PLANT>
__device__ __forceinline__ int traj_steps(const SolveLoop& c) {
  if constexpr (PLANT) return c.n_ctrl * c.hold;
  else return c.n_ctrl;
}

// The parameter block a lane evaluates the model of trajectory bb with.  PHYS: `own`, a copy of the kernel's block whose phys is row
// bb of c.model_phys, taken as values (the cart-pole's four rows of a wave hold four different sets; a user model's wave one);
// otherwise the kernel's block itself, and `own` is never touched.  REF without PHYS: `own` as a plain copy, whose x_ref set_ref_row
// then rewrites step by step.
// COST: `own` with q, qf and r of row bb of c.cost_rows, taken as values like phys.  COST is instantiated alone and with PHYS and REF
// together; in the latter a NULL c.model_phys leaves the copy's phys what the kernel's block holds (a wave-uniform branch around the
// row's loads: values either way, never a pointer into one block or the other), and a NULL c.x_ref_rows its x_ref (rows_given).
template <bool PHYS, bool REF = false, bool COST = false>
__device__ __forceinline__ const quattro_model_params& trajectory_params(const quattro_model_params& p, const SolveLoop& c,
                                                                         const size_t bb, quattro_model_params& own) {
  if constexpr (COST) {
    float w[QUATTRO_COST_ROW_FLOATS];
#pragma unroll
    for (int i = 0; i < QUATTRO_COST_ROW_FLOATS; ++i) w[i] = c.cost_rows[bb * QUATTRO_COST_ROW_FLOATS + i];
    own = p;
    if constexpr (PHYS) {
      if (c.model_phys != nullptr) {
        float ph[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) ph[i] = c.model_phys[bb * 8 + i];
#pragma unroll
        for (int i = 0; i < 8; ++i) own.phys[i] = ph[i];
      }
    }
#pragma unroll
    for (int i = 0; i < QUATTRO_MAX_NX; ++i) {
      own.q[i] = w[i];
      own.qf[i] = w[QUATTRO_MAX_NX + i];
    }
#pragma unroll
    for (int i = 0; i < QUATTRO_MAX_NU; ++i) own.r[i] = w[2 * QUATTRO_MAX_NX + i];
    return own;
  } else if constexpr (PHYS) {
    float ph[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) ph[i] = c.model_phys[bb * 8 + i];
    own = p;
#pragma unroll
    for (int i = 0; i < 8; ++i) own.phys[i] = ph[i];
    return own;
  } else if constexpr (REF) {
    own = p;
    return own;
  } else {
    return p;
  }
}

// REF: whether this launch has reference rows to read.  Without COST the REF kernels run with rows only; the COST kernel that
// carries REF also runs without (wave-uniform).
template <bool REF, bool COST>
__device__ __forceinline__ bool rows_given(const SolveLoop& c) {
  if constexpr (!REF) return false;
  else if constexpr (COST) return c.x_ref_rows != nullptr;
  else return true;
}

// The rows of c.x_ref_rows as plan cs of the loop reads them (cs = 0 in a plain solve, where c.hold is 0 too)
__device__ __forceinline__ RefRows plan_ref_rows(const SolveLoop& c, const int cs) {
  return RefRows{c.x_ref_rows, c.ref_rows, cs * c.hold, c.preview};
}

// REF, for the bodies that evaluate the model on a block of their own (trajectory_params: the cart-pole's rows, a user model's
// wave): x_ref of that block becomes the row of trajectory bb that horizon step t reads.  Called before every evaluation of a
// stage cost, a record or the terminal pair (t = N); NX: the model's state dimension (the rows' length).
template <int NX>
__device__ __forceinline__ void set_ref_row(quattro_model_params& own, const RefRows& rr, const size_t bb, const int t) {
  const float* row = rr.rows + (bb * rr.R + qt_ref_row(rr, t)) * NX;
  float v[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) v[i] = row[i];
#pragma unroll
  for (int i = 0; i < NX; ++i) own.x_ref[i] = v[i];
}

// every store of this wave has completed before its lanes read what other lanes of the wave wrote (the phases of a
// wave-private loop hand trajectories over through global memory)
__device__ __forceinline__ void wave_handoff() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Top of control step cs of a wave-private loop: the lane that leads trajectory bb (lead) records its start state (MPC),
// resets the per-solve state (what a host caller resets before a solve; after the last control step it stays as that solve
// left it) and rolls the nominal out from x0 (simulate(): the model's rollout body, run by that lane alone).
template <int NX, bool PLANT, class Simulate>
__device__ __forceinline__ void wave_step_prologue(const SolveLoop& c, const size_t bb, const int cs, const bool lead,
                                                   Simulate simulate) {
  if ((c.flags & (QUATTRO_SOLVE_SIMULATE | QUATTRO_SOLVE_RESET)) == 0 && c.n_ctrl == 0) return;
  if (lead) {
    if (c.n_ctrl > 0 && cs == 0) {
#pragma unroll
      for (int i = 0; i < NX; ++i) c.traj_x[(bb * (traj_steps<PLANT>(c) + 1)) * NX + i] = c.x0[bb * NX + i];
    }
    if (c.n_ctrl > 0 || (c.flags & QUATTRO_SOLVE_RESET) != 0) {
      c.iters[bb] = 0;
      c.active[bb] = 1;
      c.alpha_idx[bb] = -1;
      if (c.status != nullptr) c.status[bb] = 0;
    }
    if ((c.flags & QUATTRO_SOLVE_SIMULATE) != 0 || c.n_ctrl > 0) simulate();
  }
  wave_handoff();
}

// End of MPC control step cs of a wave-private loop, W lanes per trajectory (l: lane in the group, have: the group has a
// trajectory): apply u_0 to the plant (step(x, u, x_next): the device model itself), add the disturbance, record, and shift the
// warm start u <- (u_1 .. u_{N-1}, u_{N-1}) in passes of a wave's worth of elements.  Every element of a pass is read before
// any is written.
// PLANT (quattro_mpc_run_plant_f32): the lead lane first runs the plan's c.hold tracked steps on the plant (track(x, first step):
// the model's track_body on the nominal and gains this solve left behind, writing the trajectory rows), then the warm start
// shifts by c.hold: u <- (u_h .. u_{N-1}, u_{N-1} x h).  A pass reads rows at or above the ones it writes, and the rows above
// belong to later passes (or to none: row N - 1), so "read before written" holds pass by pass as before.
template <int NX, int NU, int W, bool PLANT, class Step, class Track>
__device__ __forceinline__ void wave_mpc_epilogue(const SolveLoop& c, const size_t bb, const int cs, const int l, const bool have,
                                                  Step step, Track track) {
  constexpr int PER = QT_WAVE / W;                             // elements a lane moves per pass
  float* ub = c.u + bb * c.N * NU;
  const int tot = (c.N - 1) * NU;                              // elements that move
  const bool lead = have && l == 0;
  if constexpr (PLANT) {
    if (lead) {
      float xh[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) xh[i] = c.x_cur[bb * NX + i];
      track(xh, (size_t)cs * c.hold);
#pragma unroll
      for (int i = 0; i < NX; ++i) c.x_cur[bb * NX + i] = xh[i];
      c.traj_iters[bb * c.n_ctrl + cs] = c.iters[bb];
    }
    wave_handoff();                                            // the tracked steps have read their controls before any moves
  }
  for (int base = 0; base < tot || (!PLANT && base == 0); base += W * PER) {    // (at least once: the plant step below rides on the first pass, also when N = 1 and nothing shifts)
    float v[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = base + l + W * q;
      int src = e + NU;
      if constexpr (PLANT) {
        const int row = e / NU + c.hold;                       // row t takes row min(t + h, N - 1)
        src = row < c.N ? e + c.hold * NU : (c.N - 1) * NU + e % NU;
      }
      v[q] = (have && e < tot) ? ub[src] : 0.0f;
    }
    float u0[NU] = {};
    if (!PLANT && base == 0 && lead) {
#pragma unroll
      for (int q = 0; q < NU; ++q) u0[q] = ub[q];
    }
    wave_handoff();                                            // every element of the pass is read before any is written
    if (!PLANT && base == 0 && lead) {
      float xo[NX], xn[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) xo[i] = c.x_cur[bb * NX + i];
      step(xo, u0, xn);
      if (c.disturbance != nullptr) {
#pragma unroll
        for (int i = 0; i < NX; ++i) xn[i] += c.disturbance[((size_t)cs * c.B + bb) * NX + i];
      }
#pragma unroll
      for (int q = 0; q < NU; ++q) c.traj_u[(bb * c.n_ctrl + cs) * NU + q] = u0[q];
      c.traj_iters[bb * c.n_ctrl + cs] = c.iters[bb];
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        c.x_cur[bb * NX + i] = xn[i];
        c.traj_x[(bb * (c.n_ctrl + 1) + cs + 1) * NX + i] = xn[i];
      }
    }
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = base + l + W * q;
      if (have && e < tot) ub[e] = v[q];
    }
  }
  wave_handoff();
}

}  // namespace
