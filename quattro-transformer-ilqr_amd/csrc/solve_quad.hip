// Device-resident iLQR solve loop and receding-horizon (MPC) loop for the quadrotor: ONE persistent launch runs, for every
// trajectory, the whole `while` loop of iLQR_TF.optimize (quattro_ilqr_tf/quattro_ilqr_tf.py:428-472) — and, in MPC mode,
// the caller's loop around it (examples/quadrotor/quadrotor_mpc.py:102-124: solve, apply u_0, shift the warm start) — with
// no host involvement between iterations or control steps.
//
// Why it can be one launch: trajectories are independent optimisation problems.  Nothing an iteration of
// trajectory b reads was written for another trajectory, so there is no grid-wide dependency anywhere in a solve: a
// workgroup owns its trajectories from the first rollout to the last accepted step and simply leaves when they are done.
// The multi-launch path (quattro_ilqr_iterate_f32 once per iteration) pays, per iteration, two kernel boundaries, the
// drain of the slowest wave of each kernel, a host call, and — because the host cannot know when the last trajectory has
// converged without asking — either a synchronisation every few iterations or empty launches after convergence.
//
// Mapping (the SAME device code as the stand-alone kernels, sweep_tile16_body.h / rollout_quad_body.h, so every number is
// bit-identical to the multi-launch path): a workgroup = 2 wavefronts = 2 trajectories.
//   sweep phase       : wave w linearises and sweeps trajectory 2 blk + w (one wavefront per trajectory, 16x16 tiles,
//                       exact-fp32 MFMA), K / k go to global memory (they are outputs) and stay in the XCD's L2;
//   workgroup barrier
//   line-search phase : wave 0 runs the fused 6-alpha line search of BOTH trajectories (8 candidate quads = 32 lanes per
//                       trajectory), commits the accepted candidate, updates cost / alpha_idx / iters / active;
//   workgroup barrier ; loop until both trajectories have stopped or max_iter.
// Workgroups drift apart in phase, so a SIMD hosts a mix of MFMA-bound sweeps and VALU-bound rollouts instead of four
// copies of the same phase; a trajectory that needs 29 iterations when the mean is 15 runs its last ones on an almost
// empty chip, at the latency of a lone wave (no contention), and the launch ends when the last workgroup leaves.
// Registers: the line search prefetches its nominal data 2 steps ahead here instead of 4 (the gains were written by this
// workgroup a moment ago and come from L2), which keeps the whole loop inside the sweep's 128-register budget: 4 waves
// per SIMD, i.e. B = 4096 resident at once.
#include "rollout_quad_body.h"
#include "solve_loop.h"
#include "sweep_tile16_body.h"

namespace {

struct SolveArgs {
  FusedArgs fa;         // model parameters + nominal (x [B][N+1][12], u [B][N][4], in/out) as the sweep body takes them: kept
                        // inside the kernel-argument block (a private copy with lane-dependent indexing would live in scratch)
  SolveLoop c;          // c.x == fa.x, c.u == fa.u (writable); K [B][N][4][12], k [B][N][4]
  unsigned long long* stamps; // diagnostics (may be NULL): [workgroup][2 * (n_ctrl + 1) + 2] = (s_memrealtime at the start / after
                              // each control step, iterations the workgroup ran in that step; wave 1's exit stamp and loop
                              // passes in the last two slots); 100 MHz ticks
  int stamp_rows;             // workgroups the stamps buffer has rows for (others do not stamp)
};

// the line-search wave above every phase of the sweeps it shares its SIMD with — other workgroups': it is the one wave of two
// that works in this phase, and its partner waits for it (91.2 -> 85.5 us per iteration at B = 4096; 1 / 2: 86.3 / 87.3)
constexpr int LS_PRIO = 3;

// apply u_0 to the plant (the device model itself), record, shift the warm start, reset the per-solve state: what
// QuadrotorMPC.control_step does after optimize() (quadrotor_mpc.py:121-122) plus the simulator's step around it.
// Run by wave 0: quad q = lane >> 2 < 2 owns trajectory b0 + q for the plant step; the shift is spread over 32 lanes per
// trajectory.
// PLANT (quattro_mpc_run_plant_f32): cs counts plans.  The quad runs the plan's a.hold tracked steps on the plant — quad_track_body
// on the nominal and gains this solve left behind, with the plant's lane constants — and the warm start shifts by a.hold:
// u <- (u_h .. u_{N-1}, u_{N-1} x h).  A pass of the shift reads rows at or above the ones it writes, and the rows above belong to
// later passes (or to none: row N - 1), so "read before written" holds pass by pass as before.
template <bool RK4, bool PLANT>
__device__ __forceinline__ void mpc_advance(const SolveArgs& args, const int b0, const int lane, const int cs) {
  const SolveLoop& a = args.c;
  const int q = lane >> 2, tb = b0 + q;
  const bool live = lane < 8 && tb < a.B;
  const size_t bb = live ? tb : 0;
  const int N = a.N;
  if constexpr (PLANT) {
    const LaneConst L = lane_const_plant(a.plant, a.plant_phys, bb, args.fa.p.dt, lane & 3);
    const NomSrc nom(L, a.x, a.u, a.K, a.k, N, b0, live ? q : 0, 2);
    const size_t n_tot = (size_t)a.n_ctrl * a.hold, s0 = (size_t)cs * a.hold;
    float xh[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) xh[g] = a.x_cur[bb * NX + 3 * g + L.a];
    quad_track_body(L, a.plant.integrator == QUATTRO_INTEGRATOR_RK4, a.feedback != 0, nom, xh, a.hold,
                    a.disturbance != nullptr ? a.disturbance + (s0 * a.B + bb) * NX + L.a : nullptr, (size_t)a.B * NX, live,
                    a.traj_x + (bb * (n_tot + 1) + s0) * NX + L.a, a.traj_u + (bb * n_tot + s0) * NU + L.j);
    if (live) {
      if (L.j < 3) {
#pragma unroll
        for (int g = 0; g < 4; ++g) a.x_cur[bb * NX + 3 * g + L.a] = xh[g];
      }
      if (L.j == 0) a.traj_iters[bb * a.n_ctrl + cs] = a.iters[bb];
    }
  } else {
    const LaneConst L = lane_const(args.fa.p, lane & 3);
    float xo[4], xn[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) xo[g] = a.x_cur[bb * NX + 3 * g + L.a];
    const float u0 = a.u[bb * N * NU + L.j];
    const QuadU U(u0);
    quad_step<RK4>(L, xo, U, xn);
    if (a.disturbance != nullptr) {
#pragma unroll
      for (int g = 0; g < 4; ++g) xn[g] += a.disturbance[((size_t)cs * a.B + bb) * NX + 3 * g + L.a];
    }
    if (live) {
      a.traj_u[(bb * a.n_ctrl + cs) * NU + L.j] = u0;
      if (L.j < 3) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          a.x_cur[bb * NX + 3 * g + L.a] = xn[g];
          a.traj_x[(bb * (a.n_ctrl + 1) + cs + 1) * NX + 3 * g + L.a] = xn[g];
        }
      }
      if (L.j == 0) {
        a.traj_iters[bb * a.n_ctrl + cs] = a.iters[bb];
      }
    }
  }
  // warm start u <- (u_1, ..., u_{N-1}, u_{N-1}): every element is read before any is written (the loads below are
  // complete — their values sit in registers — before the first store issues)
  const int half = lane >> 5, l32 = lane & 31, ts = b0 + half;
  if (ts < a.B) {
    float* ub = a.u + (size_t)ts * N * NU;
    const int tot = (N - 1) * NU;
    constexpr int MAXI = 8;    // 32 lanes x 8 = 256 >= (N - 1) * 4 for N <= 65; longer horizons loop
    for (int base = 0; base < tot; base += 32 * MAXI) {
      float v[MAXI];
#pragma unroll
      for (int i = 0; i < MAXI; ++i) {
        const int e = base + l32 + 32 * i;
        int src = e + NU;
        if constexpr (PLANT) src = e / NU + a.hold < N ? e + a.hold * NU : (N - 1) * NU + e % NU;    // row t takes row min(t + h, N - 1)
        v[i] = e < tot ? ub[src] : 0.0f;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
      for (int i = 0; i < MAXI; ++i) {
        const int e = base + l32 + 32 * i;
        if (e < tot) ub[e] = v[i];
      }
    }
  }
}

// Every phase reads the kernel arguments through its OWN opaque copy of the kernel-argument pointer, taken inside the loop.
// With plain by-value access the compiler treats everything computed from the arguments as loop-invariant: the
// parameter-only quotients (arm / Ix, 1 / mass, ...), base addresses and lane constants of ALL phases are hoisted to the top
// of the kernel and stay alive across the other phases — 115 spilled registers at the 128 that 4 waves per SIMD allow.
// Re-deriving them per phase (scalar loads from the constant kernel-argument segment + ~200 vector instructions) is what a
// stand-alone kernel's prologue does anyway.
typedef const SolveArgs __attribute__((address_space(4))) * KernArgPtr;
__device__ __forceinline__ const SolveArgs& fresh_args(KernArgPtr base) {
  asm volatile("" : "+s"(base));
  return *(const SolveArgs*)base;
}

// Workgroup barrier that hands GLOBAL-memory data from one wave to the other.  __syncthreads() alone is not enough here: for
// a workgroup-scope release on gfx950 (waves of a workgroup share their CU's L1) the compiler emits `s_waitcnt lgkmcnt(0)`
// only — no vmcnt(0) — on the premise that the CU performs its vector-memory operations in order.  Across two WAVES that
// premise does not hold: a store issued by wave 0 just before the barrier (an `active` flag, the last gain rows of a sweep)
// can still be in flight when wave 1's load after the barrier is served, and the two waves then disagree about a
// workgroup-uniform loop condition (measured: a wave that runs on alone for milliseconds after its partner has left the
// kernel).  The explicit wait makes every store of this wave complete (written through to L2) before it arrives.
__device__ __forceinline__ void wg_sync() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();
}

// PLANT: the loop of quattro_mpc_run_plant_f32; the <RK4, false> code is the loop as it always was (quattro_ilqr_solve_f32,
// quattro_mpc_run_f32)
// PHYS (with PLANT only: quattro_ilqr_solve_phys_f32 has n_ctrl == 0 and never reaches mpc_advance): row b of c.model_phys is the
// physical parameters of trajectory b.  The sweep's wave owns its trajectory and reads the row once per phase as wave-uniform
// values (sweep_tile16_body<.., PHYS>); in the nominal rollout and the line search each quad of wave 0 takes the row of the
// trajectory it works on (lane_const_phys).  The plant of mpc_advance is a.plant / a.plant_phys as ever: the entry points
// a.plant_phys at the same rows when the run names no plant of its own.
// REF (with PLANT only, like PHYS): the cost of horizon step t of the plan that starts at plant step cs * c.hold is taken against
// the row of c.x_ref_rows that step reads (qt_ref_row) — nominal rollout, l_x and V_x(N) of the sweep, every line-search candidate.
// Each phase takes the rows from its own fresh copy of the arguments (plan_ref_rows), like everything else it reads.
template <bool RK4, bool PLANT, bool PHYS, bool REF>
__global__ __launch_bounds__(128, 4) void solve_quad_kernel(const SolveArgs) {
  const KernArgPtr kap = (KernArgPtr)__builtin_amdgcn_kernarg_segment_ptr();   // the one by-value argument sits at offset 0
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int b0 = blockIdx.x * 2, b = b0 + wv;

  __shared__ __attribute__((aligned(16))) float s_t_all[2 * 16 * LD];
  __shared__ __attribute__((aligned(16))) float s_vx_all[2 * 64];
  constexpr int SWEEP_MODE = RK4 ? MODE_FUSED_RK4 : MODE_FUSED;
  constexpr int LIN_FLOATS = sweep_lin_floats<SWEEP_MODE>();
  __shared__ __attribute__((aligned(16))) float s_lin_all[2 * LIN_FLOATS];

  const SolveArgs& ka = *(const SolveArgs*)kap;    // loop control only (a handful of scalars)
  const SolveLoop& c = ka.c;
  const bool have = b < c.B;
  const bool force = (c.flags & QUATTRO_SOLVE_FIXED_ITERS) != 0;
  const int n_ctrl = c.n_ctrl > 0 ? c.n_ctrl : 1;
  const bool stamping = ka.stamps != nullptr && (int)blockIdx.x < ka.stamp_rows;
  if (stamping && threadIdx.x == 0) ka.stamps[(size_t)blockIdx.x * (2 * (n_ctrl + 1) + 2)] = __builtin_amdgcn_s_memrealtime();
  const bool logging = c.log.rec != nullptr && c.n_ctrl == 0;
  int total_passes = 0;
  for (int cs = 0; cs < n_ctrl; ++cs) {
    int wg_iters = 0;
    if ((c.flags & (QUATTRO_SOLVE_SIMULATE | QUATTRO_SOLVE_RESET)) != 0 || c.n_ctrl > 0) {
      // nominal rollout + cost from the current state (simulate :127-132, compute_total_cost :138-143): quads 0 and 1 of wave 0
      if (wv == 0) {
        const SolveArgs& args = fresh_args(kap);
        const SolveLoop& a = args.c;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        if ((a.n_ctrl > 0 || (a.flags & QUATTRO_SOLVE_RESET) != 0) && ln < 8 && b0 + (ln >> 2) < a.B) {
          const size_t tb = b0 + (ln >> 2);
          if (a.n_ctrl > 0 && cs == 0 && (ln & 3) < 3) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
              a.traj_x[(tb * (traj_steps<PLANT>(a) + 1)) * NX + 3 * g + (ln & 3)] = a.x0[tb * NX + 3 * g + (ln & 3)];
          }
          if ((ln & 3) == 0) {       // per-solve state of this control step (what a host caller resets before a solve); after
            a.iters[tb] = 0;         // the last control step it stays as that solve left it
            a.active[tb] = 1;
            a.alpha_idx[tb] = -1;
            if (a.status != nullptr) a.status[tb] = 0;
          }
        }
        if ((a.flags & QUATTRO_SOLVE_SIMULATE) != 0 || a.n_ctrl > 0)
          simulate_quad_body<RK4, PHYS, REF>(args.fa.p, a.x0, a.u, a.N, a.x, a.cost, 4 * b0 + ln, ln < 8 && b0 + (ln >> 2) < a.B,
                                             a.model_phys, plan_ref_rows(a, cs));
      }
      wg_sync();
    }
    for (int it = 0; it < c.max_iter; ++it) {
      // both waves read both flags (written by wave 0, complete before the last barrier; read from L2, past the L1): the loop
      // condition is workgroup-uniform
      const bool act0 = force || __hip_atomic_load(c.active + b0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
      const bool act1 = (b0 + 1 < c.B) &&
                        (force || __hip_atomic_load(c.active + b0 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0);
      if (!act0 && !act1) break;
      ++wg_iters;
      ++total_passes;
      const bool mine = have && (wv == 0 ? act0 : act1);
      int log_it = 0;
      if (logging && mine) {     // the record of this iteration: nominal, cost, start stamp (this wave's own trajectory)
        const SolveLoop& a = fresh_args(kap).c;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        log_it = __hip_atomic_load(a.iters + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        log_begin(a.log, b, log_it, a.x + (size_t)b * (a.N + 1) * NX, a.u + (size_t)b * a.N * NU, a.cost[b], ln, 64);
      }
      if (mine) {
        const SolveArgs& args = fresh_args(kap);
        const SolveLoop& a = args.c;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        sweep_tile16_body<SWEEP_MODE, PHYS, REF>(nullptr, nullptr, nullptr, a.N, a.reg, a.K, a.k, a.status, args.fa, b, ln,
                                                 s_t_all + wv * 16 * LD, s_vx_all + wv * 64, s_lin_all + wv * LIN_FLOATS, a.model_phys,
                                                 plan_ref_rows(a, cs));
      }
      if (logging && mine && lane == 0) log_stamp(fresh_args(kap).c.log, b, log_it, 1, 2);
      wg_sync();
      if (wv == 0) {
        const SolveArgs& args = fresh_args(kap);
        const SolveLoop& a = args.c;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        __builtin_amdgcn_s_setprio(LS_PRIO);        // (one constant priority: toggling inside the step, as the stand-alone
                                                    //  line search does, bought nothing here)
        linesearch_quad_body<RK4, 2, false, PHYS, REF, RK4>(args.fa.p, a.x, a.u, a.K, a.k, a.al, a.n_alpha, a.B, a.N, a.tol, a.cost,
                                                       a.alpha_idx, a.active, a.iters, a.scratch, 32 * b0 + ln, force, a.model_phys,
                                                       plan_ref_rows(a, cs));
        __builtin_amdgcn_s_setprio(0);
      }
      wg_sync();
      if (logging && mine) {     // gains, accepted step, cost after the iteration, end stamp
        const SolveLoop& a = fresh_args(kap).c;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int ai = __hip_atomic_load(a.alpha_idx + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        log_end(a.log, b, log_it, a.K + (size_t)b * a.N * NU * NX, a.k + (size_t)b * a.N * NU, ai, a.cost[b], ln, 64);
      }
    }
    if (c.n_ctrl > 0) {
      // BOTH waves must have left the loop — i.e. have read the flags that ended it — before wave 0 raises the flags again
      // for the next control step.  Without this barrier a slower wave 1 reads active = 1, makes one more pass, and the two
      // waves' barriers pair up wrongly from then on (found with the per-wave stamps: wave 1 ran on alone for max_iter
      // passes after wave 0 had left the kernel).
      wg_sync();
      if (wv == 0) {
        const SolveArgs& args = fresh_args(kap);
        int ln = lane;
        asm volatile("" : "+v"(ln));
        mpc_advance<RK4, PLANT>(args, b0, ln, cs);
      }
      wg_sync();
    }
    if (stamping && threadIdx.x == 0) {
      unsigned long long* st = ka.stamps + (size_t)blockIdx.x * (2 * (n_ctrl + 1) + 2);
      st[2 * (cs + 1)] = __builtin_amdgcn_s_memrealtime();
      st[2 * (cs + 1) + 1] = (unsigned long long)wg_iters;
    }
  }
  // slot 1: s_memrealtime at which wave 0 left the kernel; the two extra slots at the end of the row: the same for wave 1 and
  // the total number of loop passes wave 1 made
  if (stamping && lane == 0) {
    unsigned long long* st = ka.stamps + (size_t)blockIdx.x * (2 * (n_ctrl + 1) + 2);
    if (wv == 0) {
      st[1] = __builtin_amdgcn_s_memrealtime();
    } else {
      st[2 * (n_ctrl + 1)] = __builtin_amdgcn_s_memrealtime();
      st[2 * (n_ctrl + 1) + 1] = (unsigned long long)total_passes;
    }
  }
}

}  // namespace

int quattro_launch_solve_quad(const quattro_model_params& p, const SolveLoop& c, float* coef, unsigned long long* stamps,
                              int stamp_rows, hipStream_t stream) {
  if (p.integrator != QUATTRO_INTEGRATOR_EULER && p.integrator != QUATTRO_INTEGRATOR_RK4) return QUATTRO_ERR_UNSUPPORTED;
  if (p.integrator == QUATTRO_INTEGRATOR_RK4 && coef == nullptr) return QUATTRO_ERR_WORKSPACE;
  if (c.cost_rows != nullptr) return QUATTRO_ERR_UNSUPPORTED;      // (no COST instantiation of this kernel: capi.hip refuses first)
  SolveArgs a;
  a.fa = fused_args(p, c.x, c.u, c.B, c.N, 0, coef, 0);     // (coef: the RK4 sweep's coefficient scratch, B * N * 132 floats)
  a.c = c;
  a.stamps = stamps;
  a.stamp_rows = stamp_rows;
  const dim3 grid((unsigned)((c.B + 1) / 2));
  const bool rk4 = p.integrator == QUATTRO_INTEGRATOR_RK4;
  // (c.x_ref_rows: the two ref entries alone set it; c.model_phys: they and the two phys entries; c.hold: the plant run and those)
#define QT_LAUNCH(PLANT, PHYS, REF)                                                                          \
  do {                                                                                                       \
    if (rk4) hipLaunchKernelGGL((solve_quad_kernel<true, PLANT, PHYS, REF>), grid, dim3(128), 0, stream, a); \
    else hipLaunchKernelGGL((solve_quad_kernel<false, PLANT, PHYS, REF>), grid, dim3(128), 0, stream, a);    \
  } while (0)
  if (c.x_ref_rows != nullptr && c.model_phys != nullptr) QT_LAUNCH(true, true, true);
  else if (c.x_ref_rows != nullptr) QT_LAUNCH(true, false, true);
  else if (c.model_phys != nullptr) QT_LAUNCH(true, true, false);
  else if (c.hold > 0) QT_LAUNCH(true, false, false);
  else QT_LAUNCH(false, false, false);
#undef QT_LAUNCH
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}
