// Device-resident iLQR solve loop and receding-horizon (MPC) loop for a USER-COMPILED model (user_model.h): ONE launch runs,
// for every trajectory, the whole `while` loop of iLQR_TF.optimize (quattro_ilqr_tf/quattro_ilqr_tf.py:428-472) and, in MPC
// mode, the caller's loop around it (the shape of examples/quadrotor/quadrotor_mpc.py:102-124: solve, apply u_0, shift the warm
// start), with no host involvement.  Only compiled into a user model's library (-DQT_USER_MODEL_HEADER=...).
//
// Same idea as solve_quad.hip / solve_cartpole.hip with the generic device bodies: a trajectory owns ONE wavefront (a
// workgroup of its own), trajectories are independent, so a wave leaves its loop as soon as its trajectory stops — no grid-wide
// dependency.  The phases hand their data over through global memory in the program order of that wave:
//   nominal rollout : lane 0                                              (rollout_body.h: simulate_body)
//   linearisation   : LPI lanes per step, 64 / LPI steps at a time        (user_linearize.h: forward-mode duals) -> ROWMAJOR records
//   terminal pair   : lanes 0..n-1                                        (user_linearize.h)
//   sweep           : the 64 lanes   (n <= 12, m <= 4: sweep_tile16_body.h, the MFMA tile recursion without pivoting, and for a
//                                     trajectory it flags QUATTRO_TRAJ_ILLCOND the same records again through sweep_generic_body.h;
//                                     larger problems: sweep_generic_body.h alone — pivoting, the reference's formulas)
//   line search     : lanes 0..5 roll the candidates out, all 64 copy the accepted one   (rollout_body.h: linesearch_body<.., 64>)
// Bit-identical to the host-driven loop of the same library (all of a user library's translation units are compiled with
// -ffp-contract=off so that the shared device functions round alike wherever they are inlined).
#ifndef QT_USER_MODEL_HEADER
#error "solve_user.hip is part of a user model's library"
#endif
#include "rollout_body.h"
#include "solve_loop.h"
#include "sweep_generic_body.h"
#include "sweep_tile16_body.h"
#include "user_linearize.h"

namespace {

// The pivoting re-sweep of a trajectory the tile sweep flagged QUATTRO_TRAJ_ILLCOND, out of line: inlined, it raised the persistent
// kernel's scratch from 100 to 256 B per lane (planar example, Euler); as a call, to 112.
template <int NX, int NU>
__device__ __noinline__ void sweep_generic_repair(const float* rec, const float* VxN, const float* VxxN, int S, float reg, float* Kout,
                                                  float* kout, int32_t* status, const int b, const int lane) {
  sweep_generic_body<NX, NU>(rec, VxN, VxxN, S, reg, Kout, kout, status, b, lane);
}

struct UserSolveArgs {
  quattro_model_params p;
  float* rec;           // [B][N][RowMajorRec stride]
  float* VxN;           // [B][n]
  float* VxxN;          // [B][n][n]
  SolveLoop c;          // x [B][N+1][n], u [B][N][m], K [B][N][m][n], k [B][N][m]
};

// (two waves per SIMD: left to itself the allocator takes 300 registers for the dual-number linearisation next to the tile sweep —
//  one wave per SIMD — and the loop runs 3x slower than with the 42 spilled registers this bound costs)
// PLANT: the loop of quattro_mpc_run_plant_f32 (a plant of its own, c.hold tracked steps per plan); the <RK4, false> code is the
// loop as it always was
// PHYS (with PLANT only: quattro_ilqr_solve_phys_f32 has n_ctrl == 0 and never reaches the MPC code): the wave evaluates its
// trajectory's model — nominal rollout, linearisation, terminal pair, line search — on a block whose phys (the model's free
// parameters P[0..7]) is its row of c.model_phys
// REF (with PLANT only, like PHYS): the cost of horizon step t is taken against the row of c.x_ref_rows that step reads
// (qt_ref_row): the wave's private block gets it as x_ref before every stage cost, record and terminal row (set_ref_row), so the
// model's stage_cost / final_cost see it as p.x_ref, whatever they do with it
// COST (with PLANT only; alone, or with PHYS and REF together, each of which then also runs without its array: trajectory_params,
// rows_given): the private block's q, qf and r are the trajectory's row of c.cost_rows, so every cost evaluated on that block follows
template <bool RK4, bool PLANT, bool PHYS, bool REF, bool COST>
__global__ __launch_bounds__(QT_WAVE, 2) void solve_user_kernel(const UserSolveArgs a) {
  constexpr int MODEL = QUATTRO_MODEL_USER, NX = QT_USER_NX, NU = QT_USER_NU, NZ = NX + NU;
  constexpr int LPI = NZ <= 8 ? 8 : (NZ <= 16 ? 16 : 32), IPP = QT_WAVE / LPI;      // lanes per item, items per pass
  using R = RowMajorRec<NX, NU>;
  // the sweep quattro_model_layout promises for this model, so that this loop and the host-driven one agree bit for bit:
  // ROWMAJOR_TILE (the MFMA tile recursion on the same records, padded inside the kernel) where the problem fits a tile
  constexpr bool TILE = NX <= 12 && NU <= 4 && NX + NU >= 6;
  __shared__ __attribute__((aligned(16))) float s_t[TILE ? 16 * LD : 4];
  __shared__ __attribute__((aligned(16))) float s_vx[64];
  __shared__ __attribute__((aligned(16))) float s_lin[4];
  const SolveLoop& c = a.c;
  const int lane = threadIdx.x;
  const int b = blockIdx.x;                      // (grid = B exactly)
  const size_t bb = b;
  const bool force = (c.flags & QUATTRO_SOLVE_FIXED_ITERS) != 0;
  const int N = c.N;
  float* xb = c.x + bb * (N + 1) * NX;
  float* ub = c.u + bb * N * NU;
  float* recb = a.rec + bb * N * R::STRIDE;
  volatile int32_t* act_flag = c.active + b;     // written by this wave's line search: always re-read from memory
  quattro_model_params own;
  const quattro_model_params& mp = trajectory_params<PHYS, REF, COST>(a.p, c, bb, own);
  const int n_ctrl = c.n_ctrl > 0 ? c.n_ctrl : 1;
  for (int cs = 0; cs < n_ctrl; ++cs) {
    auto ref = [&](int t) __attribute__((always_inline)) {
      if constexpr (REF) {
        if (rows_given<REF, COST>(c)) set_ref_row<NX>(own, plan_ref_rows(c, cs), bb, t);
      }
    };
    wave_step_prologue<NX, PLANT>(c, bb, cs, lane == 0, [&] { simulate_body<MODEL, RK4>(mp, c.x0, c.u, N, c.x, c.cost, b, ref); });
    const bool logging = c.log.rec != nullptr && c.n_ctrl == 0;
    for (int it = 0; it < c.max_iter; ++it) {
      if (!(force || *act_flag != 0)) break;       // wave-uniform: one trajectory per wave
      if (force && lane == 0) *act_flag = 1;       // as the enqueued loop sets it before every forced iteration: afterwards
                                                   // `active` holds the last line search's verdict, not the first stop's
      int log_it = 0;
      if (logging) {             // the record of this iteration: nominal, cost, start stamp
        log_it = *(volatile int32_t*)(c.iters + b);
        log_begin(c.log, b, log_it, xb, ub, *(volatile double*)(c.cost + b), lane, QT_WAVE);
      }
      // linearisation about the nominal: LPI lanes per step
      {
        const int j = lane % LPI;
        for (int t0 = 0; t0 < N; t0 += IPP) {
          const int t = t0 + lane / LPI;
          if (t < N && j < NZ) {
            ref(t);
            user_linearize_item<R, RK4>(mp, xb + (size_t)t * NX, ub + (size_t)t * NU, recb + (size_t)t * R::STRIDE, j);
          }
        }
        ref(N);
        if (lane < NX) user_terminal_row(mp, xb + (size_t)N * NX, lane, a.VxN + bb * NX, a.VxxN + bb * NX * NX);
      }
      wave_handoff();
      if constexpr (TILE) {
        FusedArgs fa;
        fa.B = c.B;
        fa.k_rows = 0;
        fa.rn = NX;
        fa.rm = NU;
        if (sweep_tile16_body<MODE_ROWPAD>(a.rec, a.VxN, a.VxxN, N, c.reg, c.K, c.k, c.status, fa, b, lane, s_t, s_vx, s_lin)) {
          // a pivot needed pivoting (an indefinite Q_uu + reg I): the pivoting sweep on the same records, like
          // sweep_rowpad_user_kernel<true> of the host-driven loop; it rewrites K, k and status[b] (wave-uniform branch)
          wave_handoff();
          sweep_generic_repair<NX, NU>(a.rec, a.VxN, a.VxxN, N, c.reg, c.K, c.k, c.status, b, lane);
        }
      } else {
        sweep_generic_body<NX, NU>(a.rec, a.VxN, a.VxxN, N, c.reg, c.K, c.k, c.status, b, lane);
      }
      if (logging && lane == 0) log_stamp(c.log, b, log_it, 1, 2);
      wave_handoff();
      linesearch_body<MODEL, RK4, 64>(mp, c.x, c.u, c.K, c.k, c.al, c.n_alpha, c.B, N, c.tol, c.cost, c.alpha_idx, c.active,
                                      c.iters, c.scratch, 64 * b + lane, force, ref);
      wave_handoff();
      if (logging)               // gains, accepted step, cost after the iteration, end stamp
        log_end(c.log, b, log_it, c.K + bb * N * NU * NX, c.k + bb * N * NU, *(volatile int32_t*)(c.alpha_idx + b),
                *(volatile double*)(c.cost + b), lane, QT_WAVE);
    }
    if (c.n_ctrl > 0)            // apply u_0 to the plant (the device model itself), record, shift the warm start
      wave_mpc_epilogue<NX, NU, QT_WAVE, PLANT>(c, bb, cs, lane, true,
                                                [&](const float* xo, const float* u0, float* xn) { qt_step<MODEL, RK4>(mp, xo, u0, xn); },
                                                [&](float* xh, const size_t s0) { track_plan<MODEL>(a.p, c, bb, xh, s0); });
  }
}

}  // namespace

// The stand-alone tile sweep of THIS library (layout ROWMAJOR_TILE): the same body, compiled in this translation unit with this
// library's flags (no implicit fma contraction), so that the host-driven loop of a user model rounds exactly like its persistent
// kernel above.  (libquattro_hip.so has its own instance for foreign records, compiled with its flags.)
// REPAIR (the iterations of quattro_ilqr_iterate_f32 / the enqueued solve): a trajectory the tile sweep flags QUATTRO_TRAJ_ILLCOND
// is swept again, in the same launch, by the pivoting generic body on the same records — exactly what the persistent kernel does,
// so that no user-model loop returns gains of an unpivoted elimination that needed pivoting.  Without REPAIR (quattro_riccati_sweep_f32)
// the flag is reported and left to the caller (include/quattro_hip.h).
namespace {
template <bool REPAIR>
__global__ __launch_bounds__(QT_WAVE) void sweep_rowpad_user_kernel(const float* __restrict__ rec, const float* __restrict__ VxN,
                                                                    const float* __restrict__ VxxN, int S, float reg,
                                                                    float* __restrict__ Kout, float* __restrict__ kout,
                                                                    int32_t* __restrict__ status,
                                                                    const int32_t* __restrict__ active, int B, int n, int m) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B || (active != nullptr && active[b] == 0)) return;
  __shared__ __attribute__((aligned(16))) float s_t[16 * LD];
  __shared__ __attribute__((aligned(16))) float s_vx[64];
  __shared__ __attribute__((aligned(16))) float s_lin[4];
  FusedArgs fa;
  fa.B = B;
  fa.k_rows = 0;
  fa.rn = n;
  fa.rm = m;
  const bool illc = sweep_tile16_body<MODE_ROWPAD>(rec, VxN, VxxN, S, reg, Kout, kout, status, fa, b, lane, s_t, s_vx, s_lin);
  if constexpr (REPAIR) {
    if (illc) {                 // (wave-uniform; the launcher checked (n, m) == (QT_USER_NX, QT_USER_NU))
      wave_handoff();
      sweep_generic_body<QT_USER_NX, QT_USER_NU>(rec, VxN, VxxN, S, reg, Kout, kout, status, b, lane);
    }
  }
}
}  // namespace

int quattro_launch_sweep_rowpad_user(const float* rec, const float* VxN, const float* VxxN, int B, int S, int n, int m, float reg,
                                     float* K, float* k, int32_t* status, const int32_t* active, bool repair, hipStream_t stream) {
  if (n < 1 || n > 12 || m < 1 || m > 4) return QUATTRO_ERR_UNSUPPORTED;
  if (repair && (n != QT_USER_NX || m != QT_USER_NU)) return QUATTRO_ERR_UNSUPPORTED;
  if (repair)
    hipLaunchKernelGGL(sweep_rowpad_user_kernel<true>, dim3((unsigned)B), dim3(QT_WAVE), 0, stream, rec, VxN, VxxN, S, reg, K, k,
                       status, active, B, n, m);
  else
    hipLaunchKernelGGL(sweep_rowpad_user_kernel<false>, dim3((unsigned)B), dim3(QT_WAVE), 0, stream, rec, VxN, VxxN, S, reg, K, k,
                       status, active, B, n, m);
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

int quattro_launch_solve_user(const quattro_model_params& p, const SolveLoop& c, float* rec, float* VxN, float* VxxN,
                              hipStream_t stream) {
  const UserSolveArgs a{p, rec, VxN, VxxN, c};
  const dim3 grid((unsigned)c.B);
  if (p.integrator != QUATTRO_INTEGRATOR_EULER && p.integrator != QUATTRO_INTEGRATOR_RK4) return QUATTRO_ERR_UNSUPPORTED;
  const bool rk4 = p.integrator == QUATTRO_INTEGRATOR_RK4;
  // (c.x_ref_rows: the two ref entries alone set it; c.model_phys: they and the two phys entries; c.hold: the plant run and those)
#define QT_LAUNCH(PLANT, PHYS, REF, COST)                                                                                 \
  do {                                                                                                              \
    if (rk4) hipLaunchKernelGGL((solve_user_kernel<true, PLANT, PHYS, REF, COST>), grid, dim3(QT_WAVE), 0, stream, a);    \
    else hipLaunchKernelGGL((solve_user_kernel<false, PLANT, PHYS, REF, COST>), grid, dim3(QT_WAVE), 0, stream, a);       \
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
