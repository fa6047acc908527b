/*
 * quattro_hip.h — C ABI of libquattro_hip.so, the MI355X (gfx950) implementation of the Quattro iLQR
 * hot path.  Plain C: device pointers as `float*`/`int*`, sizes as int, a HIP stream as `void*`.
 *
 * The reference (salemon/quattro-transformer-ilqr) has NO native/FFI boundary: the path lives in the
 * Python class quattro_ilqr_tf/quattro_ilqr_tf.py:50 (iLQR_TF) and in
 * quattro_ilqr_tf/transformer_model.py:85 (TransformerPredictor).  Each entry point below names the
 * reference method whose arithmetic it replaces; the Python host package
 * (quattro-transformer-ilqr_amd/quattro_ilqr_amd) binds them with ctypes and re-exposes the reference's
 * own interface (iLQR_TF.optimize/backward_pass/…, TransformerILQR.predict) on top.  INTEGRATION.md
 * shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - every function returns a status: 0 = QUATTRO_OK, < 0 = argument / launch error (nothing launched);
 *   - all array arguments are DEVICE pointers (fp32 unless stated), row-major, indices [b][t][...], 16-byte aligned
 *     (the kernels move state rows, gain rows and records with 16-byte accesses; any allocator's base pointer is);
 *   - launches are asynchronous on `stream` (a hipStream_t, may be NULL = default stream);
 *   - the library allocates nothing and keeps no global state; scratch comes from the caller
 *     (quattro_*_workspace_bytes);
 *   - per-trajectory numerical trouble is reported in an int32 status word per trajectory
 *     (QUATTRO_TRAJ_*), never by aborting.
 */
#ifndef QUATTRO_HIP_H
#define QUATTRO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QUATTRO_VERSION 100 /* 0.1.0 */

/* status codes */
#define QUATTRO_OK 0
#define QUATTRO_ERR_BAD_ARG (-1)     /* null pointer, negative size, t_start outside [0,N) ...            */
#define QUATTRO_ERR_UNSUPPORTED (-2) /* (n,m)/layout/model/integrator combination without a device kernel */
#define QUATTRO_ERR_LAUNCH (-3)      /* hipGetLastError() after the launch was not hipSuccess             */
#define QUATTRO_ERR_WORKSPACE (-4)   /* workspace too small / misaligned                                  */

/* per-trajectory status bits (int32 status[b]) */
#define QUATTRO_TRAJ_NONFINITE 1 /* a non-finite value appeared in the recursion / rollout            */
#define QUATTRO_TRAJ_SINGULAR 2  /* Q_uu + reg*I had a zero / non-finite pivot (np.linalg.inv would raise) */
#define QUATTRO_TRAJ_ILLCOND 4   /* TILE16 records only: the quadrotor-shaped sweep eliminates Q_uu + reg*I WITHOUT pivoting,
                                  * which assumes a symmetric positive definite block (any convex cost).  A pivot <= 0 or
                                  * <= 1e-6 x the diagonal entry it started from sets this bit: K, k of that trajectory
                                  * may be inaccurate.  The ROWMAJOR path pivots like the reference's LAPACK inverse
                                  * (quattro_ilqr_tf.py:306) and never sets it; re-run flagged trajectories there (the
                                  * iterations and solve loops of a user model's library do it themselves).            */

/* device models: the reference takes Python callables f, L, Lf (quattro_ilqr_tf.py:82-84); a kernel
 * cannot call Python, so the two shipped problems are built in and selected by id.                   */
#define QUATTRO_MODEL_CARTPOLE 1  /* examples/cartpole/cartpole_dynamics.py:32-108 + cartpole_mpc.py:187-269     */
#define QUATTRO_MODEL_QUADROTOR 2 /* examples/quadrotor/quadrotor_dynamics.py:47-198 + quadrotor_mpc.py:40-100  */
/* Any other problem (what the reference's callable arguments allow, quattro_ilqr_tf.py:66-84): written as three function
 * templates over the scalar type (csrc/user_model.h), compiled together with the generic kernels into a library of its own
 * that exports THIS header's ABI (quattro_ilqr_amd.user_model.compile_model does it: hipcc, ~20 s, cached).  In such a
 * library model_id QUATTRO_MODEL_USER selects the compiled-in problem with its (n, m) <= (QUATTRO_MAX_NX, QUATTRO_MAX_NU):
 * exact derivatives by forward-mode differentiation through the whole integrator step (csrc/dual.h) where the reference takes
 * finite differences, ROWMAJOR records, the pivoting generic sweep, one lane per line-search candidate.  libquattro_hip.so
 * itself answers QUATTRO_ERR_UNSUPPORTED for this id.  phys[0..7] are the model's free parameters.                          */
#define QUATTRO_MODEL_USER 3

#define QUATTRO_INTEGRATOR_EULER 0
#define QUATTRO_INTEGRATOR_RK4 1

#define QUATTRO_MAX_NX 16
#define QUATTRO_MAX_NU 8
#define QUATTRO_MAX_ALPHAS 8
/* a row of per-trajectory cost weights (COST ROWS below): q, qf and r back to back */
#define QUATTRO_COST_ROW_FLOATS (2 * QUATTRO_MAX_NX + QUATTRO_MAX_NU)

/* Problem definition handed to the kernels BY VALUE (host struct).  Costs are
 *   L(x,u)  = sum_i q[i] (x_i - x_ref_i)^2 + sum_a r[a] u_a^2 + barrier_alpha * sum_a softplus_beta(-u_a)^2
 *   Lf(x)   = sum_i qf[i] (x_i - x_ref_i)^2
 * which covers both shipped costs (diagonal Q, R, Qf; barrier_alpha = 0 for the cart-pole).
 * phys[]: cart-pole {m_cart, m_pole, length, gravity}; quadrotor {mass, Ix, Iy, Iz, arm, gravity, k_yaw}. */
typedef struct quattro_model_params {
  int32_t model_id;
  int32_t integrator;
  int32_t n; /* state dim   (4 / 12) */
  int32_t m; /* control dim (1 / 4)  */
  float dt;
  float barrier_alpha;
  float barrier_beta;
  float reserved0;
  float phys[8];
  float q[QUATTRO_MAX_NX];
  float qf[QUATTRO_MAX_NX];
  float x_ref[QUATTRO_MAX_NX];
  float r[QUATTRO_MAX_NU];
} quattro_model_params;

/* Derivative-record layouts.  One record per (trajectory b, step t) holds the blocks the sweep consumes
 * — A (n x n), B (n x m), l_xx (n x n), l_ux (m x n), l_uu (m x m), l_x (n), l_u (m) —
 * 2n^2 + 2nm + m^2 + n + m floats (416 for the quadrotor, 46 for the cart-pole), stored contiguously so a
 * wave streams it with full-width coalesced loads.  Record (b,t) starts at float offset
 * (b*N + t) * quattro_record_stride(n,m,layout).
 *   ROWMAJOR: [A | B | l_xx | l_ux | l_uu | l_x | l_u], each block row-major, stride padded to 4 floats.
 *   TILE16  : (n,m) = (12,4) only.  The same 416 floats permuted into the per-lane order of the 16x16
 *             wave tile the quadrotor sweep kernel computes on (see DESIGN.md "tile16 record").        */
#define QUATTRO_LAYOUT_ROWMAJOR 0
#define QUATTRO_LAYOUT_TILE16 1
/*   TILE16C : quadrotor with the Euler integrator only, produced by quattro_linearize_f32 (not by quattro_pack_derivs_f32).
 *             Most of an Euler record is a constant of the problem (identity / dt entries of A, the torque rows of B,
 *             l_xx = 2Q, l_ux = 0): those live once in a HEADER record at the start of the buffer, and each (b,t) record
 *             keeps only the 76 floats that depend on (x_t, u_t).  The buffer is
 *             quattro_record_header(n,m,layout) floats of header followed by B*(N - t_start) records of
 *             quattro_record_stride floats: 304 B per step through HBM instead of 1,664 B, same sweep arithmetic.     */
#define QUATTRO_LAYOUT_TILE16C 2
/*   TILE16R : quadrotor with the RK4 integrator, produced by quattro_linearize_f32.  Ten columns of [A | B] (the angle, body-rate
 *             and control directions) are dense and change every step; the position and velocity directions give constant
 *             columns (unit vectors / e_v + dt e_p through all four stages), which sit in the header record together with
 *             l_xx = 2Q, l_ux = 0 of the built-in cost.  Each (b,t) record keeps those ten columns, l_uu and l_z: 156 floats
 *             = 624 B per step instead of 1,664 B.                                                                        */
#define QUATTRO_LAYOUT_TILE16R 3
/*   ROWMAJOR_TILE : ROWMAJOR records (the same buffer, byte for byte) of a problem with n <= 12, m <= 4, swept by the MFMA
 *             tile kernel instead of the generic one: the kernel zero-pads the problem into its 16 x 16 tile as it loads
 *             (unit pivots for the controls that are not there), so the records stay as small as the problem.  Like every
 *             tile sweep it eliminates WITHOUT pivoting (QUATTRO_TRAJ_ILLCOND): quattro_riccati_sweep_f32 reports the bit
 *             and the caller sweeps flagged trajectories again with layout ROWMAJOR — no repacking needed.  What a
 *             user-compiled model with n <= 12, m <= 4 gets; its quattro_ilqr_iterate_f32, quattro_ilqr_solve_f32 and
 *             quattro_mpc_run_f32 re-sweep flagged trajectories with pivoting themselves, in the same launch.            */
#define QUATTRO_LAYOUT_ROWMAJOR_TILE 4

int quattro_version(void);
const char* quattro_status_string(int status);

/* floats between consecutive records; 0 if the combination is unsupported */
int quattro_record_stride(int n, int m, int layout);
/* floats of header in front of the first record (0 except for TILE16C / TILE16R) */
int quattro_record_header(int n, int m, int layout);
/* the layout the fastest sweep kernel for (n,m) wants when the records come from anywhere (quattro_pack_derivs_f32) */
int quattro_preferred_layout(int n, int m);
/* the layout quattro_linearize_f32 + quattro_riccati_sweep_f32 are fastest with for this model: TILE16C for the
 * Euler quadrotor, TILE16R for the RK4 quadrotor, quattro_preferred_layout(n, m) otherwise; -1 for an unknown model */
int quattro_model_layout(const quattro_model_params* p);

/* Gather separately stored row-major blocks into records (test/utility path; the linearisation kernel writes
 * records directly).  A[B*S][n][n], Bm[B*S][n][m], lx[B*S][n], lu[B*S][m], lxx[B*S][n][n], luu[B*S][m][m],
 * lux[B*S][m][n]  ->  rec[B*S][stride].  Replaces nothing in the reference (pure data movement).        */
int quattro_pack_derivs_f32(const float* A, const float* Bm, const float* lx, const float* lu, const float* lxx,
                            const float* luu, const float* lux, int B, int S, int n, int m, int layout, float* rec,
                            void* stream);

/* The inverse: records (any layout, TILE16C included: rec points at the header) -> separately stored row-major blocks,
 * i.e. the arrays the reference's own methods return: A, B of _compute_dynamics_jacobians (:182-204) and L_x, L_u, L_xx,
 * L_uu, L_ux (= L_xu^T) of _compute_cost_derivatives (:217-275) for every (b, t) of the buffer.                      */
int quattro_unpack_derivs_f32(const float* rec, int B, int S, int n, int m, int layout, float* A, float* Bm, float* lx,
                              float* lu, float* lxx, float* luu, float* lux, void* stream);

/* Riccati-like backward sweep.  Replaces the recursion of iLQR_TF.backward_pass
 * (quattro_ilqr_tf.py:290-317) and, with t_start > 0, iLQR_TF.backward_pass_segment (:336-364).
 *   rec   : records for steps t_start..N-1 of every trajectory, [B][N - t_start][stride]
 *   VxN   : [B][n]    terminal gradient   (reference: _finite_diff_gradient_final, :149)
 *   VxxN  : [B][n][n] terminal Hessian    (reference: _finite_diff_hessian_final,  :163; used as given)
 *   reg   : added to diag(Q_uu) before inversion only (1e-6 in the reference, :304)
 *   K     : [B][N - t_start][m][n], k: [B][N - t_start][m]   (index t - t_start, as :357-359)
 *   status: [B] QUATTRO_TRAJ_* bits (may be NULL)
 *   active: [B] optional mask; trajectories with active[b] == 0 are skipped (outputs untouched); NULL = all */
int quattro_riccati_sweep_f32(const float* rec, const float* VxN, const float* VxxN, int B, int N, int t_start, int n,
                              int m, int layout, float reg, float* K, float* k, int32_t* status,
                              const int32_t* active, void* stream);

/* Linearisation about a nominal trajectory: exact derivatives of the device model, written as records.
 * Replaces _compute_dynamics_jacobians (:182-204), _compute_cost_derivatives (:217-275) for every step
 * t in [t_start, N) and the two _finite_diff_*_final (:149-174) at x_N.
 *   x: [B][N+1][n], u: [B][N][m]  ->  rec [B][N - t_start][stride], VxN [B][n], VxxN [B][n][n]          */
int quattro_linearize_f32(const quattro_model_params* p, const float* x, const float* u, int B, int N, int t_start,
                          int layout, float* rec, float* VxN, float* VxxN, const int32_t* active, void* stream);

/* Linearisation and sweep in ONE launch, no record buffer (every built-in model; `scratch` may be NULL where
 * quattro_linearize_sweep_scratch_bytes is 0, else 16-byte aligned device memory of at least that size):
 *   - the Euler-discretised quadrotor: the sweep's own wave linearises its trajectory ahead of the recursion (17 steps
 *     at a time into LDS); per step 64 B instead of 304 B come from HBM and one launch disappears;
 *   - the RK4-discretised quadrotor: the same, in two stages (stage points -> Jacobian coefficients by one lane per step,
 *     then 4 steps x 16 unit directions per pass through the four stages); 0.9 KB per step of TILE16R records and the
 *     linearisation launch disappear;
 *   - the cart-pole (Euler and RK4): a 16-lane DPP row per trajectory runs the 4 x 4 recursion on records formed ahead of
 *     the chain in LDS — instead of a 64-lane wave per trajectory with seven barriers per step (one launch instead of three).
 * Same K, k as quattro_linearize_f32 (model layout) followed by quattro_riccati_sweep_f32: bit-identical for the quadrotor,
 * to fp32 round-off (<= 2e-6 per step) for the cart-pole.  Replaces
 * _compute_dynamics_jacobians / _compute_cost_derivatives / _finite_diff_*_final + backward_pass(_segment)
 * (quattro_ilqr_tf.py:149-275, :290-317 / :336-364).  QUATTRO_ERR_UNSUPPORTED for other models (quattro_model_fuses_sweep
 * says which): use the two calls above.
 *   x [B][N+1][n], u [B][N][m]  ->  K [B][N - t_start][m][n], k [B][N - t_start][m], status [B] (may be NULL)          */
/* 0: no fused kernel; 1: quattro_linearize_sweep_f32 is this model's fastest backward pass; 2: it works, but
 * quattro_linearize_f32 + quattro_riccati_sweep_f32 through records are faster as stand-alone launches (RK4 quadrotor: 180 us
 * against 58 + 69 us at B = 4096 — the fused form exists for the device-resident loop, which cannot run a second kernel) */
int quattro_model_fuses_sweep(const quattro_model_params* p);
/* device scratch quattro_linearize_sweep_f32 needs for this model and size (0 for all but the RK4 quadrotor, whose wave leaves
 * the coefficients of its four stage Jacobians — 528 B per step — in it between the two stages of its linearisation) */
size_t quattro_linearize_sweep_scratch_bytes(const quattro_model_params* p, int B, int N, int t_start);
int quattro_linearize_sweep_f32(const quattro_model_params* p, const float* x, const float* u, int B, int N, int t_start,
                                float reg, float* K, float* k, int32_t* status, const int32_t* active, void* scratch,
                                size_t scratch_bytes, void* stream);

/* The same launch writing into gain arrays of `k_rows` rows per trajectory (K [B][k_rows][m][n], k [B][k_rows][m]): step t lands
 * at row k_rows - (N - t).  k_rows = 0 or N - t_start: the segment form above (index t - t_start, quattro_ilqr_tf.py:357-359);
 * k_rows = N: the FULL gain stacks, the swept tail written in place at rows t_start .. N - 1 — where the hybrid iteration's
 * line search reads it and where quattro_tf_gains_* (prompt = NULL) reads its prompt from: no segment buffers, no packing and
 * no concatenation (np.concatenate of :515-518) in a hybrid iteration.                                                      */
int quattro_linearize_sweep_rows_f32(const quattro_model_params* p, const float* x, const float* u, int B, int N, int t_start,
                                     float reg, float* K, float* k, int k_rows, int32_t* status, const int32_t* active,
                                     void* scratch, size_t scratch_bytes, void* stream);

/* Open-loop rollout + total cost.  Replaces iLQR_TF.simulate (:127-132) + compute_total_cost (:138-143).
 *   x0 [B][n], u [B][N][m]  ->  x [B][N+1][n], cost [B] (fp64)                                          */
int quattro_simulate_f32(const quattro_model_params* p, const float* x0, const float* u, int B, int N, float* x,
                         double* cost, void* stream);

/* Total cost of given sequences (they need not satisfy the dynamics).  Replaces compute_total_cost (:138-143).
 *   x [B][N+1][n], u [B][N][m]  ->  cost [B] (fp64)                                                        */
int quattro_total_cost_f32(const quattro_model_params* p, const float* x, const float* u, int B, int N, double* cost,
                           void* stream);

/* Closed-loop rollouts for n_alpha step sizes at once.  Replaces iLQR_TF.forward_pass (:377-390) for every
 * alpha of the line search (:440 / :552).
 *   x_nom [B][N+1][n], u_nom [B][N][m], K [B][N][m][n], k [B][N][m], alphas: HOST array of n_alpha floats
 *   -> cost [n_alpha][B] (fp64);  x_new / u_new: optional [n_alpha][B][N+1][n] / [n_alpha][B][N][m] (NULL = costs only) */
int quattro_rollout_f32(const quattro_model_params* p, const float* x_nom, const float* u_nom, const float* K,
                        const float* k, const float* alphas, int n_alpha, int B, int N, float* x_new, float* u_new,
                        double* cost, const int32_t* active, void* stream);

/* Line search + accept, fused.  Replaces the alpha loop of iLQR_TF.optimize (:433-451 / :546-563) and its stop
 * test (:472 / :584): evaluates every alpha, takes the FIRST one (in the given order) whose cost is <= cost[b],
 * and for accepting trajectories overwrites x_nom/u_nom/cost in place with the accepted candidate.
 *   alpha_idx [B] : index of the accepted alpha, -1 if none
 *   active    [B] : in/out; cleared when no alpha was accepted or |cost_old - cost_new| < tol (converged).
 *                   Inactive trajectories are left untouched.
 *   iters     [B] : incremented for every trajectory that was active on entry (may be NULL)
 *   scratch       : device buffer of at least quattro_linesearch_scratch_bytes(n, m, B, N) bytes, 16-byte aligned;
 *                   holds the candidate trajectories between the rollouts and the commit                   */
size_t quattro_linesearch_scratch_bytes(int n, int m, int B, int N);
int quattro_linesearch_f32(const quattro_model_params* p, float* x_nom, float* u_nom, const float* K, const float* k,
                           const float* alphas, int n_alpha, int B, int N, double tol, double* cost,
                           int32_t* alpha_idx, int32_t* active, int32_t* iters, void* scratch, size_t scratch_bytes,
                           void* stream);

/* One whole pure-iLQR iteration for B trajectories: the body of the while-loop of iLQR_TF.optimize (:428-472) —
 * linearise about (x_nom, u_nom), Riccati sweep, 6-alpha line search with accept/commit and the stop test — as three
 * launches on `stream` from ONE host call (the `quattro_ilqr_iterate` fused driver) — two where the model fuses the
 * linearisation into the sweep (quattro_model_fuses_sweep).  Exactly equivalent to
 * quattro_linearize_f32 (t_start = 0, preferred layout) + quattro_riccati_sweep_f32 + quattro_linesearch_f32 on the
 * same buffers.  `workspace` (device, 256-byte aligned, >= quattro_model_workspace_bytes(p, B, N) bytes) holds the
 * derivative records, V_x(N), V_xx(N) and the candidate trajectories; nothing in it needs to survive between calls.
 *   in/out: x_nom [B][N+1][n], u_nom [B][N][m], cost [B] fp64 (cost of the nominal on entry), active [B], iters [B]
 *   out   : K [B][N][m][n], k [B][N][m], alpha_idx [B], status [B] (QUATTRO_TRAJ_* bits, may be NULL)             */
size_t quattro_workspace_bytes(int n, int m, int B, int N);                            /* enough for any model of these dims */
size_t quattro_model_workspace_bytes(const quattro_model_params* p, int B, int N);    /* exact for this model (<= the above) */
int quattro_ilqr_iterate_f32(const quattro_model_params* p, float* x_nom, float* u_nom, int B, int N, float reg,
                             const float* alphas, int n_alpha, double tol, float* K, float* k, double* cost,
                             int32_t* alpha_idx, int32_t* active, int32_t* iters, int32_t* status, void* workspace,
                             size_t workspace_bytes, void* stream);

/* The whole solve, device-resident: the `while` loop of iLQR_TF.optimize (quattro_ilqr_tf.py:428-472) — up to max_iter
 * iterations, every trajectory stopping on its own test (:472: no accepted step, or |cost_old - cost_new| < tol) — from ONE
 * host call with no host involvement in between.  For models with a persistent kernel (quattro_model_has_device_loop
 * != 0) it is ONE launch: the quadrotor (csrc/solve_quad.hip: a workgroup owns two trajectories from the first rollout to their
 * last accepted step and leaves when both have stopped), the cart-pole (csrc/solve_cartpole.hip: a 16-lane row per trajectory),
 * both integrators, and — in a user model's library — the compiled-in problem (csrc/solve_user.hip: one wave per trajectory
 * through the generic device bodies).  quattro_model_has_device_loop returns 1 where that launch is also the fastest form and 2
 * where it exists but enqueued iterations are faster (user models: the host mirror then enqueues unless asked otherwise); for
 * models without one (0) the same loop is enqueued as max_iter iterations of quattro_ilqr_iterate_f32, which skip stopped
 * trajectories.  Results are bit-identical to calling quattro_simulate_f32 once
 * and quattro_ilqr_iterate_f32 until every `active` flag is down.
 *   flags: QUATTRO_SOLVE_SIMULATE    roll the nominal out from x0 [B][n] first (x_nom, cost are outputs); without it x_nom and
 *                                    cost must hold the nominal rollout of u_nom and its cost (as after quattro_simulate_f32)
 *          QUATTRO_SOLVE_FIXED_ITERS ignore the stop flags: exactly max_iter iterations for every trajectory (benchmarking)
 *   in/out: u_nom [B][N][m]; active [B] (1 = solve this trajectory), iters [B] (incremented per iteration), as
 *           quattro_ilqr_iterate_f32;   out: x_nom, K, k, cost, alpha_idx, status (may be NULL)
 *   workspace: >= quattro_model_workspace_bytes(p, B, N), 256-byte aligned                                           */
#define QUATTRO_SOLVE_SIMULATE 1
#define QUATTRO_SOLVE_FIXED_ITERS 2
/*          QUATTRO_SOLVE_RESET       the call itself sets the per-solve state first (active = 1, iters = 0, alpha_idx = -1,
 *                                    status = 0) — what a caller otherwise does with four fills before a solve              */
#define QUATTRO_SOLVE_RESET 4
/*          QUATTRO_SOLVE_ENQUEUE     never the persistent kernel: max_iter enqueued iterations of quattro_ilqr_iterate_f32
 *                                    (what models with quattro_model_has_device_loop == 0 get anyway); without this flag a
 *                                    model whose persistent kernel exists but is slower (== 2) runs the persistent kernel
 *                                    only when QUATTRO_SOLVE_PERSISTENT is set                                              */
#define QUATTRO_SOLVE_ENQUEUE 8
#define QUATTRO_SOLVE_PERSISTENT 16
int quattro_model_has_device_loop(const quattro_model_params* p);
int quattro_ilqr_solve_f32(const quattro_model_params* p, const float* x0, float* x_nom, float* u_nom, int B, int N,
                           float reg, const float* alphas, int n_alpha, double tol, int max_iter, int flags, float* K,
                           float* k, double* cost, int32_t* alpha_idx, int32_t* active, int32_t* iters, int32_t* status,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Per-iteration log of a solve, written by the device: what iLQR_TF.optimize appends to self.logs every iteration
 * (quattro_ilqr_tf.py:453-466 pure / :565-578 hybrid: x_seq, u_seq, current_cost, k_seq, K_seq, alpha, new_cost, found_update;
 * new_x_seq / new_u_seq of iteration i are x_seq / u_seq of iteration i + 1 or the solve's result) and what its measure_time
 * decorators append to backward_pass_time / inference_time / forward_pass_time (:16-42) — so that a LOGGED solve is still one
 * launch and one download instead of a host round trip per iteration.
 *   records : device memory, B x capacity records of quattro_solve_log_record_bytes(n, m, N, flags) bytes, 16-byte aligned,
 *             zero-filled once by the caller; iteration i (0-based) of trajectory b is record b * capacity + (i % capacity)
 *   flags   : QUATTRO_LOG_TRAJ  (x_seq, u_seq entering the iteration), QUATTRO_LOG_GAINS (K, k of the iteration); the 64-byte
 *             header is always written:
 *               uint64 stamp[4]  s_memrealtime ticks (100 MHz): iteration begins / backward pass done / gains complete (equal to
 *                                the second in pure mode; after the predictor in hybrid mode) / line search done
 *               double cost_pre, cost_new   cost of the nominal entering the iteration / after it (unchanged if no step accepted)
 *               int32  alpha_idx            accepted step (index into `alphas`), -1 = none (found_update false)
 *               int32  iteration, 2 x int32 padding
 *   field offsets inside a record: quattro_solve_log_offset(n, m, N, flags, QUATTRO_LOG_FIELD_*)  (0 for a part the flags exclude) */
#define QUATTRO_LOG_TRAJ 1
#define QUATTRO_LOG_GAINS 2
#define QUATTRO_LOG_FIELD_X 0
#define QUATTRO_LOG_FIELD_U 1
#define QUATTRO_LOG_FIELD_K 2
#define QUATTRO_LOG_FIELD_KFF 3 /* k, the feed-forward term */
typedef struct quattro_solve_log {
  void* records;
  int32_t capacity;
  int32_t flags;
} quattro_solve_log;
size_t quattro_solve_log_record_bytes(int n, int m, int N, int flags);
size_t quattro_solve_log_offset(int n, int m, int N, int flags, int field);

/* quattro_ilqr_solve_f32 with a log (NULL = none: exactly quattro_ilqr_solve_f32).  The persistent kernels fill the records
 * between the phases of their loop; for models solved by enqueued iterations the record kernel below runs between the launches. */
int quattro_ilqr_solve_logged_f32(const quattro_model_params* p, const float* x0, float* x_nom, float* u_nom, int B, int N,
                                  float reg, const float* alphas, int n_alpha, double tol, int max_iter, int flags, float* K,
                                  float* k, double* cost, int32_t* alpha_idx, int32_t* active, int32_t* iters, int32_t* status,
                                  void* workspace, size_t workspace_bytes, const quattro_solve_log* log, void* stream);

/* The same records for a loop the CALLER enqueues kernel by kernel (hybrid iterations: sweep of the tail, predictor, line
 * search): one small launch per phase, trajectories selected on the device from `active` / `iters`, no host involvement.
 *   QUATTRO_LOG_PHASE_BEGIN          before the backward pass: header (stamp 0, cost_pre, iteration = iters[b]) + x, u for every
 *                                    trajectory with active[b] != 0 (or every one with `force`)
 *   QUATTRO_LOG_PHASE_BACKWARD_DONE  stamps 1 and 2;  QUATTRO_LOG_PHASE_GAINS_DONE  stamp 2 (after the predictor)
 *   QUATTRO_LOG_PHASE_END            after quattro_linesearch_f32 (which has incremented iters[b]): K, k, alpha_idx, cost_new,
 *                                    stamp 3 for the trajectories whose record iters[b] - 1 is pending                       */
#define QUATTRO_LOG_PHASE_BEGIN 0
#define QUATTRO_LOG_PHASE_BACKWARD_DONE 1
#define QUATTRO_LOG_PHASE_GAINS_DONE 2
#define QUATTRO_LOG_PHASE_END 3
int quattro_solve_log_record_f32(const quattro_solve_log* log, int phase, const float* x_nom, const float* u_nom,
                                 const float* K, const float* k, const double* cost, const int32_t* alpha_idx,
                                 const int32_t* active, const int32_t* iters, int B, int N, int n, int m, int force,
                                 void* stream);

/* Receding-horizon loop, device-resident: B controllers advance n_steps control steps in ONE launch (models with
 * quattro_model_has_device_loop; QUATTRO_ERR_UNSUPPORTED otherwise).  Per control step and controller, what
 * QuadrotorMPC.control_step (examples/quadrotor/quadrotor_mpc.py:102-124) and the simulator's loop around it do: solve from
 * the current state with the warm start (the loop above: nominal rollout, iterations until the stop test or max_iter), apply
 * u_0 to the plant — the device model itself; the reference's plant is MuJoCo, out of scope — plus an optional additive state
 * disturbance, shift the warm start (u_1 .. u_{N-1}, u_{N-1}), continue.  A controller never waits for another one.
 *   in/out: x_cur [B][n] current states (advanced n_steps times), u_nom [B][N][m] warm start (shifted result on return)
 *   out   : traj_x [B][n_steps+1][n] (traj_x[:,0] = the initial x_cur), traj_u [B][n_steps][m] applied controls,
 *           traj_iters [B][n_steps] iLQR iterations per control step; x_nom, K, k, cost, alpha_idx, status: of the LAST solve
 *   disturbance [n_steps][B][n] or NULL; active / iters [B]: scratch state of the loop (any contents on entry)            */
int quattro_mpc_run_f32(const quattro_model_params* p, float* x_cur, float* x_nom, float* u_nom, int B, int N, float reg,
                        const float* alphas, int n_alpha, double tol, int max_iter, int n_steps, float* traj_x, float* traj_u,
                        int32_t* traj_iters, const float* disturbance, float* K, float* k, double* cost, int32_t* alpha_idx,
                        int32_t* active, int32_t* iters, int32_t* status, void* workspace, size_t workspace_bytes,
                        void* stream);

/* The closed loop with a PLANT OF ITS OWN and gain feedback between solves.  A real controller replans slowly and, between
 * plans, runs u = u_nom[j] + K[j] (x - x_nom[j]) at the plant rate; and the plant is never exactly the model it plans with.
 *
 * quattro_track_f32: n_steps <= N tracked plant steps from x0 [B][n] along rows 0 .. n_steps-1 of a nominal (x_nom [B][N+1][n],
 * u_nom [B][N][m]) and its gains K [B][N][m][n] (required also without feedback).  For j = 0 .. n_steps-1:
 *     u_app = u_nom[j] + (feedback ? K[j] (x - x_nom[j]) : 0),   x <- f_plant(x, u_app) + disturbance[j][b]
 *   plant       : the plant's parameters, NULL = p.  Its model_id, n, m and dt must equal p's (QUATTRO_ERR_BAD_ARG otherwise); its
 *                 integrator and phys define f_plant; its cost fields are ignored.
 *   plant_phys  : [B][8] device array or NULL: row b replaces plant->phys for controller b (a user model's free parameters
 *                 likewise: the study of B controllers against B different plants)
 *   disturbance : [n_steps][B][n] or NULL
 *   out         : x_out [B][n_steps+1][n] (row 0 = x0), u_out [B][n_steps][m] applied controls
 *
 * quattro_mpc_run_plant_f32: quattro_mpc_run_f32 (its arguments, in its order) with such a plant and a hold count.  n_steps PLANT
 * steps; for plan c = 0 .. n_steps/hold - 1: solve from x_cur with the warm start exactly as quattro_mpc_run_f32 does (x_nom,
 * u_nom, K are what that solve leaves behind, K from its last backward pass), run `hold` tracked steps as above (the device
 * function of quattro_track_f32: bit-identical), shift the warm start by hold (u_hold .. u_{N-1}, u_{N-1} x hold), and
 * traj_iters[b][c] = iterations of the solve.  traj_x / traj_u as in quattro_mpc_run_f32, traj_iters [B][n_steps/hold],
 * disturbance [n_steps][B][n] or NULL.  With hold = 1 the feedback term is exactly zero (x_cur == x_nom[0]).
 * QUATTRO_ERR_BAD_ARG, nothing launched: hold outside 1..N, n_steps % hold != 0, a plant whose model_id, n, m or dt differ from
 * p's, feedback with max_iter < 1.  quattro_mpc_run_f32 itself keeps its own kernels and results.                               */
int quattro_track_f32(const quattro_model_params* p, const quattro_model_params* plant, const float* plant_phys, const float* x0,
                      const float* x_nom, const float* u_nom, const float* K, int feedback, int B, int N, int n_steps,
                      const float* disturbance, float* x_out, float* u_out, void* stream);
int quattro_mpc_run_plant_f32(const quattro_model_params* p, float* x_cur, float* x_nom, float* u_nom, int B, int N, float reg,
                              const float* alphas, int n_alpha, double tol, int max_iter, int n_steps, float* traj_x,
                              float* traj_u, int32_t* traj_iters, const float* disturbance, float* K, float* k, double* cost,
                              int32_t* alpha_idx, int32_t* active, int32_t* iters, int32_t* status, void* workspace,
                              size_t workspace_bytes, const quattro_model_params* plant, const float* plant_phys, int hold,
                              int feedback, void* stream);

/* PER-TRAJECTORY MODEL PARAMETERS.  A batch otherwise shares one quattro_model_params, so its trajectories can differ in x0 and
 * warm start only.  model_phys [B][8] (device, fp32) lifts that for the physical parameters: row b replaces p->phys for trajectory
 * (controller) b wherever the controller's model is evaluated — nominal rollout, linearisation, terminal pair, sweep, line-search
 * rollouts and, in the closed loop, the default plant.  For a user-compiled model the row holds its eight free parameters
 * P[0..7].  p->phys is ignored; every other field of p (dt, integrator, cost, barrier) stays shared.  Rows are used as given,
 * with no host validation of their values: a non-physical row shows up as QUATTRO_TRAJ_NONFINITE / QUATTRO_TRAJ_SINGULAR for that
 * trajectory alone.  Results are those of B separate calls with B = 1 and p->phys = row b, bit for bit.
 *
 * quattro_ilqr_solve_phys_f32: the arguments of quattro_ilqr_solve_logged_f32 in their order (the log ring works as there), then
 * model_phys.  quattro_mpc_run_phys_f32: the arguments of quattro_mpc_run_plant_f32 in their order up to `feedback`, then
 * model_phys; the plant of controller b is plant_phys[b] if that array is given, else plant->phys if a plant is given, else
 * model_phys[b] (the default plant is the controller's own model); its integrator is the plant's, else p's.
 *   model_phys == NULL : exactly the entry each extends (the same call, the same kernels, the same results).
 *   model_phys != NULL : always the model's persistent kernel (csrc/solve_*.hip, their PHYS instantiations), whether or not that
 *                        is the model's fastest form.  Before any launch: QUATTRO_ERR_UNSUPPORTED for a model without one
 *                        (quattro_model_has_device_loop(p) == 0), QUATTRO_ERR_BAD_ARG for QUATTRO_SOLVE_ENQUEUE together with
 *                        model_phys; every other argument is checked as by the entry each extends.
 * The stand-alone entries (quattro_simulate_f32, quattro_linearize*_f32, quattro_rollout_f32, quattro_linesearch_f32,
 * quattro_ilqr_iterate_f32, quattro_track_f32) and the other fields of p (barrier, dt, integrator) have no per-trajectory form
 * (x_ref has one of its own: REFERENCE ROWS below; q, qf and r theirs, for the cart-pole and user models: COST ROWS below). */
int quattro_ilqr_solve_phys_f32(const quattro_model_params* p, const float* x0, float* x_nom, float* u_nom, int B, int N,
                                float reg, const float* alphas, int n_alpha, double tol, int max_iter, int flags, float* K,
                                float* k, double* cost, int32_t* alpha_idx, int32_t* active, int32_t* iters, int32_t* status,
                                void* workspace, size_t workspace_bytes, const quattro_solve_log* log, const float* model_phys,
                                void* stream);
int quattro_mpc_run_phys_f32(const quattro_model_params* p, float* x_cur, float* x_nom, float* u_nom, int B, int N, float reg,
                             const float* alphas, int n_alpha, double tol, int max_iter, int n_steps, float* traj_x,
                             float* traj_u, int32_t* traj_iters, const float* disturbance, float* K, float* k, double* cost,
                             int32_t* alpha_idx, int32_t* active, int32_t* iters, int32_t* status, void* workspace,
                             size_t workspace_bytes, const quattro_model_params* plant, const float* plant_phys, int hold,
                             int feedback, const float* model_phys, void* stream);

/* REFERENCE ROWS: per-trajectory, per-step state targets.  The cost is otherwise taken against the one p->x_ref of the batch, constant
 * over the horizon and over a closed-loop run.  x_ref_rows [B][ref_rows][n] (device, fp32, 16-byte aligned, ref_rows >= 1) lifts that:
 * for trajectory (controller) b a row of it replaces p->x_ref wherever the cost is evaluated — stage cost and total cost of the
 * nominal rollout and of every line-search rollout, l_x of the linearisation, and the terminal gradient V_x(N).  l_xx, V_xx(N), q,
 * qf, r, the barrier, dt and the integrator stay shared; p->x_ref is ignored.  A user-compiled model's stage_cost / final_cost see
 * the row as p.x_ref.  Which row, with R = ref_rows:
 *   plain solve : horizon step t in [0, N] (t = N: the terminal cost) reads row min(t, R - 1);
 *   closed loop : plan c starts at plant step s = c * hold; horizon step t of that plan reads row min(s + preview * t, R - 1),
 *                 preview in {0, 1}.
 * Running past the last row holds the last row.  R = 1: every trajectory its own constant goal.  preview = 0, R = n_steps: a
 * set-point schedule as the reference's simulator drives one (examples/quadrotor/quadrotor_sim.py:135-145 moves mpc_controller.x_ref
 * between control steps: known at replan time only, constant inside a solve).  preview = 1, R >= n_steps + N + 1: tracking along a
 * sliding window of a path — nothing is shifted or copied, only the offset moves.  The tracked steps between solves (hold,
 * feedback) follow x_nom, u_nom and K as ever; they have no cost and read no rows.
 *
 * quattro_ilqr_solve_ref_f32: the arguments of quattro_ilqr_solve_phys_f32 in their order (log ring and model_phys as there), then
 * x_ref_rows, ref_rows.  quattro_mpc_run_ref_f32: the arguments of quattro_mpc_run_phys_f32 in their order up to model_phys, then
 * x_ref_rows, ref_rows, preview.  Rows work with and without model_phys, with and without a plant.
 *   x_ref_rows == NULL : exactly the entry each extends (the same call, the same kernels, the same results); ref_rows and preview
 *                        are not looked at.
 *   x_ref_rows != NULL : always the model's persistent kernel (csrc/solve_*.hip, their REF instantiations), as with model_phys.
 *                        Before any launch: QUATTRO_ERR_UNSUPPORTED for a model without one, QUATTRO_ERR_BAD_ARG for ref_rows < 1 or
 *                        > 2^20 (the kernels address the rows with 32-bit byte offsets), preview outside {0, 1}, or
 *                        QUATTRO_SOLVE_ENQUEUE together with rows; every other argument is checked as by the entry each extends.
 * The library still allocates nothing and quattro_model_workspace_bytes keeps its values.  The stand-alone entries
 * (quattro_simulate_f32, quattro_linearize*_f32, quattro_rollout_f32, quattro_linesearch_f32, quattro_ilqr_iterate_f32,
 * quattro_track_f32) have no row form.  The cost weights have a per-trajectory form of their own: COST ROWS below. */
int quattro_ilqr_solve_ref_f32(const quattro_model_params* p, const float* x0, float* x_nom, float* u_nom, int B, int N,
                               float reg, const float* alphas, int n_alpha, double tol, int max_iter, int flags, float* K,
                               float* k, double* cost, int32_t* alpha_idx, int32_t* active, int32_t* iters, int32_t* status,
                               void* workspace, size_t workspace_bytes, const quattro_solve_log* log, const float* model_phys,
                               const float* x_ref_rows, int ref_rows, void* stream);
int quattro_mpc_run_ref_f32(const quattro_model_params* p, float* x_cur, float* x_nom, float* u_nom, int B, int N, float reg,
                            const float* alphas, int n_alpha, double tol, int max_iter, int n_steps, float* traj_x,
                            float* traj_u, int32_t* traj_iters, const float* disturbance, float* K, float* k, double* cost,
                            int32_t* alpha_idx, int32_t* active, int32_t* iters, int32_t* status, void* workspace,
                            size_t workspace_bytes, const quattro_model_params* plant, const float* plant_phys, int hold,
                            int feedback, const float* model_phys, const float* x_ref_rows, int ref_rows, int preview,
                            void* stream);

/* COST ROWS: per-trajectory cost weights.  The weights q, qf, r are otherwise the one set of p for the whole batch.  cost_rows
 * [B][QUATTRO_COST_ROW_FLOATS] (device, fp32, 16-byte aligned; 40 floats a row: q at float 0, qf at float 16, r at float 32 -- p's three
 * arrays back to back; entries beyond n / m are ignored) lifts that: row b replaces p->q, p->qf and p->r for trajectory (controller)
 * b wherever the cost is evaluated -- stage cost and total cost of the nominal rollout and of every line-search rollout, l_x, l_xx
 * (= 2Q), l_u and l_uu (2R plus the barrier's second derivative) of the linearisation, V_x(N) and V_xx(N) (= 2Qf).  barrier_alpha and
 * barrier_beta, x_ref (unless reference rows are given), dt, the integrator and phys (unless model_phys is given) stay shared; p->q,
 * p->qf and p->r are ignored.  The weights are constant over the horizon and over a closed-loop run; the tracked steps between
 * solves (hold, feedback) have no cost and read no row.  A user-compiled model's stage_cost / final_cost see the row as p.q, p.qf,
 * p.r, so default_stage_cost / default_final_cost follow it.  Rows are used as given: no value is validated, and a row that makes
 * Q_uu singular or ill-conditioned shows in that trajectory's status bits alone.  The results are those of B calls with B = 1 and
 * p->q, qf, r = row b, bit for bit.
 *
 * quattro_ilqr_solve_cost_f32: the arguments of quattro_ilqr_solve_ref_f32 in their order up to ref_rows, then cost_rows.
 * quattro_mpc_run_cost_f32: the arguments of quattro_mpc_run_ref_f32 in their order up to preview, then cost_rows.  The log ring,
 * model_phys, x_ref_rows, plant, plant_phys, hold and feedback all work together with cost_rows.
 *   cost_rows == NULL : exactly the entry each extends (the same call, the same kernels, the same results).
 *   cost_rows != NULL : always the model's persistent kernel (csrc/solve_cartpole.hip, csrc/solve_user.hip, their COST
 *                       instantiations: one for weights alone, one that also takes model_phys and x_ref_rows, either or both).
 *                       Before any launch: QUATTRO_ERR_UNSUPPORTED for a model without such a kernel -- which includes
 *                       QUATTRO_MODEL_QUADROTOR, whose persistent kernel has no COST instantiation yet --, QUATTRO_ERR_BAD_ARG
 *                       for QUATTRO_SOLVE_ENQUEUE together with rows; every other argument is checked as by the entry each
 *                       extends.
 * The library still allocates nothing and quattro_model_workspace_bytes keeps its values.  The stand-alone entries
 * (quattro_simulate_f32, quattro_linearize*_f32, quattro_rollout_f32, quattro_linesearch_f32, quattro_ilqr_iterate_f32,
 * quattro_track_f32, quattro_total_cost_f32) have no row form; per-step weights, per-trajectory barrier parameters, dt and
 * integrator have none either. */
int quattro_ilqr_solve_cost_f32(const quattro_model_params* p, const float* x0, float* x_nom, float* u_nom, int B, int N,
                                float reg, const float* alphas, int n_alpha, double tol, int max_iter, int flags, float* K,
                                float* k, double* cost, int32_t* alpha_idx, int32_t* active, int32_t* iters, int32_t* status,
                                void* workspace, size_t workspace_bytes, const quattro_solve_log* log, const float* model_phys,
                                const float* x_ref_rows, int ref_rows, const float* cost_rows, void* stream);
int quattro_mpc_run_cost_f32(const quattro_model_params* p, float* x_cur, float* x_nom, float* u_nom, int B, int N, float reg,
                             const float* alphas, int n_alpha, double tol, int max_iter, int n_steps, float* traj_x,
                             float* traj_u, int32_t* traj_iters, const float* disturbance, float* K, float* k, double* cost,
                             int32_t* alpha_idx, int32_t* active, int32_t* iters, int32_t* status, void* workspace,
                             size_t workspace_bytes, const quattro_model_params* plant, const float* plant_phys, int hold,
                             int feedback, const float* model_phys, const float* x_ref_rows, int ref_rows, int preview,
                             const float* cost_rows, void* stream);

/* SCORING: per-step costs and their fp64 total of given sequences, under per-trajectory targets, weights and parameters.  The last
 * stage of a tuning or fleet study: a closed-loop run made with reference rows, cost rows or model_phys (the entries above) is scored
 * on the device against what it was asked to follow, under ONE evaluation cost or under each controller's own.  Replaces
 * compute_total_cost (quattro_ilqr_tf.py:138-143) step by step: the reference sums L over the sequence and adds Lf; this entry returns
 * every term of that sum and the sum, with the terminal term optional (Lf belongs to a horizon, not to a run of plant steps).
 *   x [B][S+1][n], u [B][S][m] : any sequences; they need not satisfy the dynamics
 *   model_phys [B][8], x_ref_rows [B][ref_rows][n], cost_rows [B][QUATTRO_COST_ROW_FLOATS] : the arrays of the *_phys / *_ref / *_cost
 *                       entries, the same layouts, 16-byte aligned; each may be NULL on its own (p's values then).  phys matters only
 *                       to a user model whose cost reads P: the built-in costs do not read it, and the rows are accepted without effect
 *   step s < S        : stage[b][s] = L(x_s, u_s) with q, r of row b of cost_rows, phys of row b of model_phys and x_ref = row
 *                       min((s / ref_hold) * ref_hold, ref_rows - 1) of trajectory b's reference rows (integer division).  ref_hold = 1
 *                       is "row s": what a closed loop with preview = 1 was planned against at plant step s.  ref_hold = h is the
 *                       set-point schedule of preview = 0 with a plan every h plant steps.  Past the last row the last row holds (the
 *                       row rule of the REFERENCE ROWS, stated for plant steps)
 *   slot S            : with QUATTRO_SCORE_TERMINAL in flags, stage[b][S] = Lf(x_S) with qf of the row and the reference row of the
 *                       same rule at s = S; without it +0.0f
 *   total [b] (fp64)  : sum of (double)stage[b][s] for s = 0 .. S in that order -- the accumulation of quattro_total_cost_f32, so that
 *                       without rows and with the flag total equals its cost bit for bit.  Without the flag slot S adds nothing
 *   stage [B][S+1]    : may be NULL (totals only); total may not
 * One wave per trajectory evaluates 64 steps at a time (quattro_total_cost_f32 is one lane per trajectory, serial over steps: right
 * for a horizon of 50, wrong for a run of thousands of plant steps); the total is accumulated in step order whatever the mapping.
 * Nothing is allocated and no workspace is taken.  Every model takes every kind of row here, the built-in quadrotor's cost rows
 * included (scoring needs the model's stage and final cost only, not its persistent kernel).  Before any launch: the model check
 * of quattro_total_cost_f32 first; then QUATTRO_ERR_BAD_ARG for a NULL x, u or total, B <= 0, S <= 0, unknown bits in flags,
 * reference rows with ref_rows < 1 or ref_hold < 1 (neither is looked at without rows), or a row array that is not 16-byte aligned. */
#define QUATTRO_SCORE_TERMINAL 1
int quattro_score_f32(const quattro_model_params* p, const float* x, const float* u, int B, int S, const float* model_phys,
                      const float* x_ref_rows, int ref_rows, int ref_hold, const float* cost_rows, int flags, float* stage,
                      double* total, void* stream);

/* COST GRADIENT: dJ/du and dJ/dx0 of the trajectory cost J(x0, u) = sum_t L(x_t, u_t) + Lf(x_N) with x_{t+1} = f(x_t, u_t), by the
 * adjoint sweep.  Differentiates iLQR_TF.simulate (quattro_ilqr_tf.py:127-132) composed with compute_total_cost (:138-143); the
 * reference has no counterpart (it never forms the gradient of the cost it minimises: a first-order optimality measure for a solve,
 * a gradient method over the controls, or a loss through the device model all start here).
 *   x [B][N+1][n], u [B][N][m] : x is meant to be the rollout of u (quattro_simulate_f32); as for quattro_linearize_f32 this is
 *                       not checked, and for other sequences the outputs are the recursion below about the given points
 *   lambda_N = Lf_x(x_N);  for t = N-1 .. 0:  g_t = L_u(x_t, u_t) + B_t^T lambda_{t+1},  lambda_t = L_x(x_t, u_t) + A_t^T lambda_{t+1}
 *                       with [A_t | B_t] the derivative of the whole integrator step (Euler or RK4, p->integrator) at (x_t, u_t)
 *   grad_u [B][N][m]  = g          grad_x0 [B][n] = lambda_0 (may be NULL)          costate [B][N+1][n] = lambda (may be NULL)
 *                       all fp32, the recursion runs in fp32; grad_x0[b] and costate[b][0] are the same value, bit for bit
 *   model_phys [B][8], x_ref_rows [B][ref_rows][n], cost_rows [B][QUATTRO_COST_ROW_FLOATS] : the arrays of the *_phys / *_ref / *_cost
 *                       entries, the same layouts, 16-byte aligned; each may be NULL on its own (p's values then).  model_phys
 *                       reaches the dynamics as well as a user model's cost.  Horizon step t takes its cost against row
 *                       min(t, ref_rows - 1) of trajectory b's reference rows and the terminal term against the row of t = N: the
 *                       solves' row rule for a plan that starts at step 0.  Every model takes every kind of row, the built-in
 *                       quadrotor's cost rows included (as for scoring, the model's step and cost are all that is needed)
 * A group of 8, 16 or 32 adjacent lanes (by n + m; 16 for both built-in models) owns one trajectory and lane j direction j of
 * z = (x, u): column j of [A_t | B_t] and entry j of l_z are formed off the serial chain for QUATTRO_GRAD_BLOCK steps at a time and
 * staged in LDS; the chain is one n-term dot product per lane and step plus the exchange of lambda inside the group
 * (csrc/cost_gradient.hip).  The barrier part of L_u is evaluated with a softplus accurate relative to itself, so it is not the l_u of
 * quattro_linearize_f32's records bit for bit (they differ by up to about 1e-6 relative where the barrier is inactive).
 * Nothing is allocated and no workspace is taken.  The results of trajectory b are those of a call with
 * B = 1 and p's fields set to row b, bit for bit.  Before any launch: the model check of quattro_total_cost_f32 first; then
 * QUATTRO_ERR_BAD_ARG for a NULL x, u or grad_u, B <= 0, N <= 0, reference rows with ref_rows < 1 (not looked at without rows), or a
 * row array that is not 16-byte aligned. */
#define QUATTRO_GRAD_BLOCK 3
int quattro_cost_gradient_f32(const quattro_model_params* p, const float* x, const float* u, int B, int N,
                              const float* model_phys, const float* x_ref_rows, int ref_rows, const float* cost_rows,
                              float* grad_u, float* grad_x0, float* costate, void* stream);

/* COST GRADIENT WITH RESPECT TO THE ROWS: dJ/d(model_phys), dJ/d(cost_rows) and dJ/d(x_ref_rows) of the same trajectory cost, per
 * trajectory, for the built-in cart-pole and quadrotor (Euler and RK4).  What system identification (fit each vehicle's mass or
 * inertia to a logged trajectory), weight tuning and set-point optimisation descend along.  The serial work is the costate of
 * quattro_cost_gradient_f32; given it, every (trajectory, step) item stands alone.  The reference has no counterpart (its model
 * parameters, weights and targets live inside the Python callables it is handed).
 *   x [B][N+1][n], u [B][N][m] : as for quattro_cost_gradient_f32 (x is meant to be the rollout of u under the same rows; not checked)
 *   costate [B][N+1][n] : fp32, the `costate` output of quattro_cost_gradient_f32 under the same rows; may be NULL when grad_phys is
 *   model_phys [B][8], x_ref_rows [B][ref_rows][n], cost_rows [B][QUATTRO_COST_ROW_FLOATS] : exactly as quattro_cost_gradient_f32 takes
 *                       them, each may be NULL on its own (p's values then)
 * Outputs, all fp64, each may be NULL on its own, at least one must be given:
 *   grad_phys [B][8]  : entry k < NP (4: cart-pole, 7: quadrotor) = sum_{t=0}^{N-1} sum_i lambda_{t+1,i} d f_i / d theta_k (x_t, u_t),
 *                       f the whole integrator step (p->integrator, zero-order-hold u) at trajectory b's own phys; entries
 *                       k >= NP are +0.0
 *   grad_cost_rows [B][QUATTRO_COST_ROW_FLOATS], in the layout of a cost row:
 *                       q_i  at float 0  : sum_{t<N} (x_{t,i} - ref_{t,i})^2
 *                       qf_i at float 16 : (x_{N,i} - ref_{N,i})^2
 *                       r_a  at float 32 : sum_{t<N} u_{t,a}^2           and +0.0 beyond n / m
 *   grad_ref_rows [B][R][n], R = ref_rows, or R = 1 when x_ref_rows is NULL (the gradient with respect to a per-trajectory copy
 *                       of p->x_ref): row rho = sum_{t<N, min(t,R-1)=rho} -2 q_i (x_{t,i} - ref_{rho,i}), plus the terminal term
 *                       -2 qf_i (x_{N,i} - ref_{rho,i}) in the row with min(N, R-1) = rho: the row rule of
 *                       quattro_cost_gradient_f32.  Rows past the horizon are +0.0
 * Not differentiated: dt, the barrier (it has no weight in a row and contributes nothing to grad_cost_rows), anything of a user
 * model.  d f / d theta comes from forward-mode duals through a scalar-generic statement of the two rates and the integrator
 * (csrc/models_generic.h): its derivative part is used, its value part is not the rollouts' bits.
 * One wave per trajectory, a step per lane, 64 steps a pass (csrc/cost_param_gradient.hip).  Per-step terms are fp32 (the
 * cart-pole's are formed in fp64 and rounded once: its d f / d length cancels where the pole balances under the force, and fp32
 * sines and products lose the bound there), every sum is
 * fp64 and runs over t = 0 .. N in that order whatever B or the launch geometry: no atomics, nothing allocated, no workspace.  An
 * entry with no non-zero term is +0.0.  The results of trajectory b are those of a call with B = 1 and p's fields set to row b, bit
 * for bit, and an output does not depend on which other outputs are asked for.
 * Before any launch: the model check of quattro_total_cost_f32 first; QUATTRO_ERR_UNSUPPORTED for QUATTRO_MODEL_USER (a user-model
 * library exports the entry and answers this); then QUATTRO_ERR_BAD_ARG for a NULL x or u, all three outputs NULL, grad_phys without
 * costate, B <= 0, N <= 0, reference rows with ref_rows < 1 (not looked at without rows), or a row array that is not 16-byte
 * aligned. */
int quattro_cost_param_gradient_f32(const quattro_model_params* p, const float* x, const float* u, int B, int N,
                                    const float* costate, const float* model_phys, const float* x_ref_rows, int ref_rows,
                                    const float* cost_rows, double* grad_phys, double* grad_cost_rows, double* grad_ref_rows,
                                    void* stream);

/* GRADIENT OF THE TRACKED CLOSED-LOOP COST: dJ/dK, dJ/du_nom, dJ/dx_nom, dJ/dx0 and the closed-loop costate of n_steps <= N steps of
 * quattro_track_f32 composed with quattro_score_f32 at ref_hold = 1,
 *   u_t = u_nom_t + K_t (x_t - x_nom_t)   (K == NULL: feedback off, u_t = u_nom_t),   x_{t+1} = f_plant(x_t, u_t) + d_t,
 *   J = sum_{t < n_steps} L(x_t, u_t) + [QUATTRO_SCORE_TERMINAL] Lf(x_{n_steps}).
 * The law differentiated is iLQR_TF.forward_pass (quattro_ilqr_tf.py:377-390) with k = 0 and alpha = 1 (a feed-forward k or a step
 * size alpha is an expression in front of u_nom and K, whose chain rule is the caller's); the reference has no counterpart (it never
 * differentiates its forward pass).  What tuning the gains or the nominal, training a gain predictor on the cost its gains produce,
 * and fitting a plant to a logged closed-loop run descend along.
 *   x [B][n_steps+1][n], u [B][n_steps][m] : the outputs of quattro_track_f32 (the realised run; not checked)
 *   x_nom [B][N+1][n], K [B][N][m][n] : the arrays that call was given; only rows < n_steps are read.  K == NULL: feedback off, x_nom is
 *                       then not read, and grad_K and grad_x_nom must be NULL
 *   p                 : the cost fields, and the integrator and phys the PLANT steps with (the host composes it)
 *   model_phys [B][8] : per-trajectory plant rows (a user model's cost bodies see the same row); x_ref_rows [B][ref_rows][n], cost_rows
 *                       [B][QUATTRO_COST_ROW_FLOATS] : exactly as quattro_cost_gradient_f32 takes them.  Step t is costed against row
 *                       min(t, ref_rows - 1), the terminal term against the row of t = n_steps
 *   flags             : QUATTRO_SCORE_TERMINAL or 0
 *   lambda_S = terminal ? Lf_x(x_S) : 0;  for t = S-1 .. 0:  g_t = L_u + B_t^T lambda_{t+1},  lambda_t = L_x + A_t^T lambda_{t+1} + K_t^T g_t
 *                       with [A_t | B_t] the derivative of the plant's whole integrator step at (x_t, u_t), S = n_steps
 *   grad_u_nom [B][N][m] = g_t          grad_K [B][N][m][n] = g_t (x_t - x_nom_t)^T          grad_x_nom [B][N+1][n] = -K_t^T g_t
 *                       the inputs' shapes; rows the tracked steps did not read (t >= n_steps) are written as +0.0
 *   grad_x0 [B][n] = lambda_0           costate [B][n_steps+1][n] = lambda;  costate[b][t+1] is dJ/dd_t, and the multiplier
 *                       quattro_cost_param_gradient_f32 takes (N = n_steps, the realised x, u) for the plant-parameter, weight and
 *                       target gradients of the tracked cost.  All fp32; any output but grad_u_nom may be NULL
 * The mapping of quattro_cost_gradient_f32 (csrc/track_gradient.hip).  The feedback is folded into what is staged off the chain: state
 * lane j pushes the direction (e_j, K_t[:, j]) through the step (column j of A_t + B_t K_t, one tangent) and stages it with
 * l_x[j] + K_t[:, j]^T l_u, so the chain stays one n-term dot product per lane and ONE exchange of lambda per step; grad_K and
 * grad_x_nom are formed after each block of QUATTRO_GRAD_BLOCK steps from the g_t parked in LDS (one fp32 subtraction and one product
 * per entry of grad_K).  No atomics, nothing allocated, no workspace; the results of trajectory b are those of a call with B = 1 and
 * p's fields set to row b, bit for bit, and an output does not depend on which others are asked for.
 * Before any launch: the model check of quattro_total_cost_f32 first; then QUATTRO_ERR_BAD_ARG for a NULL x, u or grad_u_nom, B, N or
 * n_steps <= 0, n_steps > N, K without x_nom, grad_K or grad_x_nom without K, reference rows with ref_rows < 1, a row array that is not
 * 16-byte aligned, or unknown bits in flags. */
int quattro_track_gradient_f32(const quattro_model_params* p, const float* x, const float* u, int B, int N, int n_steps,
                               const float* x_nom, const float* K, const float* model_phys, const float* x_ref_rows, int ref_rows,
                               const float* cost_rows, int flags, float* grad_u_nom, float* grad_K, float* grad_x_nom,
                               float* grad_x0, float* costate, void* stream);

/* CLOSED-LOOP COVARIANCE: how far a tracked run spreads under noise, to first order.  About the realised run of n_steps <= N steps of
 * quattro_track_f32, with A_t, B_t the plant's step Jacobians at (x_t, u_t) and S = n_steps,
 *   Acl_t = A_t + B_t K_t   (K == NULL: Acl_t = A_t, the open loop)
 *   Sigma_0 = cov0[b] (NULL: 0),   Sigma_{t+1} = Acl_t Sigma_t Acl_t^T + W[b]   (W = noise, NULL: 0: the covariance of
 *                       quattro_track_f32's additive disturbance d_t, which enters after the plant step)
 *   var_u_t = diag(K_t Sigma_t K_t^T)   (t < S; K == NULL: 0)
 *   excess  = sum_{t<S} [ sum_i q_i Sigma_t[i][i] + 1/2 sum_a l_uu,t[a][a] var_u_t[a] ] + [QUATTRO_SCORE_TERMINAL] sum_i qf_i Sigma_S[i][i]
 * excess is the second-order estimate of E[J] - J(realised run) under quattro_score_f32's cost (the built-in models' stage Hessian is
 * diagonal with l_ux = 0; l_uu is 2 r_a plus the barrier's second derivative at u_t; targets do not enter).  The reference has no
 * counterpart.
 *   x [B][n_steps+1][n], u [B][n_steps][m] : the outputs of quattro_track_f32 (the realised run; not checked)
 *   K [B][N][m][n]    : the gains that call was given; only rows < n_steps are read.  The nominal is not an argument: nothing reads it
 *   p                 : the cost fields (q, qf, r, barrier), and the integrator and phys the PLANT steps with (the host composes it)
 *   plant_phys [B][8], cost_rows [B][QUATTRO_COST_ROW_FLOATS] : exactly as quattro_track_gradient_f32 takes them (the built-in
 *                       quadrotor's weights too, as in quattro_score_f32)
 *   cov0, noise [B][n][n] : symmetric positive semi-definite; neither is checked, and the recursion READS Sigma AS SYMMETRIC
 *   cov [B][n_steps+1][n][n] = Sigma_t,  var [B][n_steps+1][n] = its diagonal (the same bits),  var_u [B][N][m] (rows t >= n_steps are
 *                       written as +0.0), all fp32;  excess [B] fp64: each step's term is an fp64 sum of fp64 products of the fp32
 *                       entries, and the terms are added in step order.  Any output may be NULL and is then not written; at least one
 * The built-in models only: a user-model library exports the symbol and answers QUATTRO_ERR_UNSUPPORTED for its model.  Per block of
 * four steps (csrc/track_covariance.hip): the columns of Acl_t are formed off the serial chain (the tangent of
 * quattro_track_gradient_f32) and staged in LDS; the chain holds the two products per step -- for the quadrotor 4 + 4
 * v_mfma_f32_16x16x4_f32 on a 16 x 16 tile with Sigma in the C/D layout, which serves as both operands without a transposition; the
 * outputs are formed from the parked Sigma_t after the block.  The device's Sigma is symmetric to round-off only.  No atomics, nothing
 * allocated, no workspace; the results of trajectory b are those of a call with B = 1, bit for bit, and an output does not depend on
 * which others are asked for.
 * Before any launch: the model check of quattro_total_cost_f32 first (QUATTRO_ERR_UNSUPPORTED for a user model); then
 * QUATTRO_ERR_BAD_ARG for a NULL x or u, B, N or n_steps <= 0, n_steps > N, no output at all, a row array that is not 16-byte aligned,
 * or unknown bits in flags. */
int quattro_track_covariance_f32(const quattro_model_params* p, const float* x, const float* u, int B, int N, int n_steps,
                                 const float* K, const float* plant_phys, const float* cost_rows, const float* cov0,
                                 const float* noise, int flags, float* cov, float* var, float* var_u, double* excess, void* stream);

/* OUTPUT FEEDBACK: n_steps <= N steps of quattro_track_f32's gain law acting on the ESTIMATE of an extended Kalman filter that runs in
 * the same launch, behind a sensor that measures p_y of the n states.  Per trajectory b, f_plant the plant's step (the integrator and
 * phys of `plant`, or row b of plant_phys), f_model the estimator's (the integrator and phys of p, or row b of model_phys), obs the
 * observed indices:
 *   x_0 = x0[b],  xh = xhat0[b] (NULL: x0[b]),  P = cov0[b] (NULL: 0);  for t = 0 .. n_steps - 1:
 *   measure   y_i = x_t[obs_i] + v_t[b][i]                                   (meas_noise NULL: v = 0)
 *   update    for i = 0 .. p_y - 1 in order, j = obs_i:  g = P[:, j],  s = P[j][j] + R[b][i],  e = y_i - xh[j],
 *             nis_t += e^2 / s,  xh += g e / s,  P -= g g^T / s
 *   control   u_t = u_nom_t + K_t (xh - x_nom_t)                             (xh AFTER the update)
 *   plant     x_{t+1} = f_plant(x_t, u_t) + d_t[b]                           (disturbance NULL: 0)
 *   predict   A = df_model/dx at (xh, u_t),  xh <- f_model(xh, u_t),  P <- A P A^T + W[b]      (noise NULL: W = 0)
 * The sensor is a selection of state components with independent noise (R diagonal, > 0), for which the scalar updates in sequence
 * are exactly the batch Kalman update.  The reference has no counterpart.
 *   x0 [B][n], x_nom [B][N+1][n], u_nom [B][N][m], K [B][N][m][n] : as quattro_track_f32 takes them
 *   observed [p_y]     : HOST array of state indices, ascending and distinct, 1 <= p_y <= n, shared by the batch
 *   meas_var           : R, device array [p_y] (meas_var_rows == 0) or [B][p_y] (meas_var_rows == 1); > 0 is the caller's business
 *   xhat0 [B][n], cov0 [B][n][n], noise [B][n][n] : optional; P IS READ AS SYMMETRIC, positive semi-definite is not checked
 *   meas_noise [n_steps][B][p_y], disturbance [n_steps][B][n] : optional realised noises
 *   plant (NULL: p), plant_phys [B][8], model_phys [B][8] : as quattro_track_f32 and quattro_track_gradient_f32 take them
 *   x [B][n_steps+1][n], u [B][n_steps][m] : required.  Optional, NULL is not written: xhat [B][n_steps+1][n] (row t < n_steps the
 *                        updated estimate the control of step t used, row n_steps the last prediction), var [B][n_steps+1][n] the
 *                        diagonal of the same P (the same bits as cov's), cov [B][n_steps+1][n][n], nis [B][n_steps] the normalised
 *                        innovation squared.  All fp32; cov is symmetric to round-off only
 * One kernel (csrc/track_estimate.hip): the lane mapping of quattro_track_covariance_f32 with the Jacobian on the serial chain.  The
 * plant's step and the estimator's base step are one statement of the dynamics: with xhat0 NULL, no meas_noise and the plant equal to
 * the model, xhat equals x bit for bit and nis is +0.0.  No atomics, nothing allocated, no workspace; the results of trajectory b are
 * those of a call with B = 1, bit for bit, and an output does not depend on which others are asked for.
 * The built-in models only: a user-model library exports the symbol and answers QUATTRO_ERR_UNSUPPORTED for its model.
 * Before any launch: the model check of quattro_total_cost_f32 first (QUATTRO_ERR_UNSUPPORTED for a user model); then
 * QUATTRO_ERR_BAD_ARG for a NULL x0, x_nom, u_nom, K, observed, meas_var, x or u, B, N or n_steps <= 0, n_steps > N, p_y outside 1 .. n,
 * meas_var_rows other than 0 or 1, an index out of range, repeated or not ascending, a row array (plant_phys, model_phys) that is not
 * 16-byte aligned, or a plant that is not the same problem (quattro_track_f32's check). */
int quattro_track_estimate_f32(const quattro_model_params* p, const quattro_model_params* plant, const float* x0, const float* x_nom,
                               const float* u_nom, const float* K, int B, int N, int n_steps, const int32_t* observed, int p_y,
                               const float* meas_var, int meas_var_rows, const float* xhat0, const float* cov0, const float* noise,
                               const float* meas_noise, const float* disturbance, const float* plant_phys, const float* model_phys,
                               float* x, float* u, float* xhat, float* var, float* cov, float* nis, void* stream);

/* A LOGGED RUN filtered and smoothed: the extended Kalman filter of quattro_track_estimate_f32 over sensor readings and controls that
 * are INPUTS (nothing here steps a plant or forms a control), its log-likelihood, and the fixed-interval smoother.  Per trajectory b,
 * f the model's step (the integrator and phys of p, or row b of model_phys), obs the observed indices, S = n_steps the number of
 * logged controls; a NaN in y is "no reading of that sensor at that step":
 *   filter    xh = xhat0[b],  P = cov0[b] (NULL: 0);  for t = 0 .. S:
 *     update  for i = 0 .. p_y - 1 in order, j = obs_i, only where y_t[i] is not NaN:  g = P[:, j],  s = P[j][j] + R[b][i],
 *             e = y_t[i] - xh[j],  innov[t][i] = e,  innov_var[t][i] = s,  nis_t += e^2 / s,  xh += g e / s,  P -= g g^T / s
 *             (a missing reading: innov = innov_var = NaN, xh and P untouched bit for bit, nothing added to nis_t)
 *     record  xhat[t] = xh,  cov[t] = P,  var[t] = diag P                     (the posterior of step t)
 *     predict (t < S)  A_t = df/dx at (xh, u_t),  xh <- f(xh, u_t),  P <- A_t P A_t^T + W[b]      (noise NULL: W = 0)
 *   loglik[b] = -1/2 sum_t sum_i (ln(2 pi s) + e^2 / s) over the readings that exist: an fp64 sum, in step order and then sensor order,
 *             of fp64 terms formed from the fp32 e and s that are returned
 *   smoother  modified Bryson-Frazier in the posterior form, r [n] and Lambda [n][n] zero after the last step;  for t = S .. 0:
 *     xs[t] = xhat[t] + cov[t] r,   cov_s[t] = cov[t] - cov[t] Lambda cov[t],   var_s[t] = its diagonal (the same bits)
 *     for i = p_y - 1 .. 0 (REVERSE order), the readings that exist, with that update's g, s, e and k = g / s:
 *             q = Lambda k,  c = k^T q,  rj = r[j] + e / s - k^T r,  Lambda[j][:] -= q^T,  Lambda[:, j] -= q,  Lambda[j][j] += c + 1 / s,
 *             r[j] = rj
 *     (t > 0) r <- A_{t-1}^T r,  Lambda <- A_{t-1}^T Lambda A_{t-1}
 * In exact arithmetic the smoother is the extended Rauch-Tung-Striebel smoother about the filter's own linearisation points; it needs
 * no matrix inverse.  The update's statements and their order are quattro_track_estimate_f32's.  The reference has no counterpart.
 *   y                  : the readings, [n_steps+1][p_y] for one log shared by the batch (y_rows == 0) or [B][n_steps+1][p_y] (y_rows == 1)
 *   u                  : the applied controls, [n_steps][m] (u_rows == 0) or [B][n_steps][m] (u_rows == 1)
 *   observed, p_y, meas_var, meas_var_rows, cov0, noise, model_phys : as quattro_track_estimate_f32 takes them; P IS READ AS SYMMETRIC
 *   xhat0 [B][n]       : required (a log has no true state to default to)
 *   workspace          : device memory, 16-byte aligned, at least quattro_estimate_log_workspace_bytes(p, B, n_steps, p_y, smooth) bytes,
 *                        smooth != 0 where any of xs, var_s, cov_s is asked for; nothing beyond that many bytes is touched
 *   Outputs, all optional (NULL is not written), at least one: xhat, var [B][n_steps+1][n], cov [B][n_steps+1][n][n], innov,
 *                        innov_var [B][n_steps+1][p_y], nis [B][n_steps+1], xs, var_s [B][n_steps+1][n], cov_s [B][n_steps+1][n][n],
 *                        all fp32; loglik [B] fp64.  The covariances are symmetric to round-off only
 * Two kernels on the one stream (csrc/estimate_log.hip): the forward pass is quattro_track_estimate_f32's chain without the plant,
 * leaving per update k, e / s and 1 / s in the workspace; the backward pass, launched only where xs, var_s or cov_s is asked for,
 * recomputes the A_t in blocks off its serial chain.  No atomics, nothing allocated; the results of trajectory b are those of a call
 * with B = 1, bit for bit, an output does not depend on which others are asked for, and the filter's do not depend on the smoother.
 * The built-in models only: a user-model library exports both symbols and answers QUATTRO_ERR_UNSUPPORTED (the query: 0) for its model.
 * Before any launch: the model check of quattro_total_cost_f32 first (QUATTRO_ERR_UNSUPPORTED for a user model); then
 * QUATTRO_ERR_BAD_ARG for a NULL y, u, observed, meas_var or xhat0, B or n_steps <= 0, p_y outside 1 .. n, y_rows, u_rows or
 * meas_var_rows other than 0 or 1, an index out of range, repeated or not ascending, no output at all, model_phys -- or, with the
 * smoother, u or xhat -- not 16-byte aligned; then QUATTRO_ERR_WORKSPACE for a NULL, misaligned or short workspace.  The query answers
 * 0 for what the entry would refuse. */
size_t quattro_estimate_log_workspace_bytes(const quattro_model_params* p, int B, int n_steps, int p_y, int smooth);
int quattro_estimate_log_f32(const quattro_model_params* p, const float* y, int y_rows, const float* u, int u_rows, int B, int n_steps,
                             const int32_t* observed, int p_y, const float* meas_var, int meas_var_rows, const float* xhat0,
                             const float* cov0, const float* noise, const float* model_phys, void* workspace, size_t workspace_bytes,
                             float* xhat, float* var, float* cov, float* innov, float* innov_var, float* nis, double* loglik,
                             float* xs, float* var_s, float* cov_s, void* stream);

/* Transformer gain predictor: weights of the reference's TransformerPredictor (quattro_ilqr_tf/transformer_model.py:85-138)
 * as DEVICE pointers, plus the DataNormalizer vectors (:15-50).  Matrices are PyTorch Linear layout [out][in];
 * the `w_*` matrices are 16-bit (raw uint16 bit patterns: bf16, or IEEE half when `precision` says so), everything else
 * fp32.
 *   precision            : QUATTRO_TF_PRECISION_BF16 (the *_bf16 entry points) or QUATTRO_TF_PRECISION_F16 (the *_f16 entry
 *                          points: the same kernel with fp16 MFMA operands — what the shipped checkpoints store and what
 *                          the reference's own predict() computes in, transformer_ilqr.py:317-319; fp32 accumulation,
 *                          LayerNorm, softmax and residual stream either way)
 *   tok_bias             : unused (kept for layout compatibility; see tok_bias_t below)
 *   w_out    [64][d]     : output_linear.weight zero-padded to 64 rows
 * Supported shape family: d_model = 128, n_head = 4, d_ff % 64 == 0 (64 .. 1024), L <= 128, c_dim <= 64 (both shipped models). */
#define QUATTRO_TF_MAX_LAYERS 8
#define QUATTRO_TF_PRECISION_BF16 0
#define QUATTRO_TF_PRECISION_F16 1
typedef struct quattro_tf_weights {
  int32_t n_x, c_dim, d_model, n_head, d_ff, n_layers, n_state_tok, prompt_len, target_len, precision;
  const float *x_mean, *x_std, *u_mean, *u_std;
  const uint16_t* w_state; /* state_embed.weight as bf16 [d][16], columns >= n_x zero (one MFMA k-step) */
  const float *state_b, *ctrl_w, *ctrl_b;
  const float* tok_bias;
  const uint16_t* w_qkv[QUATTRO_TF_MAX_LAYERS]; /* in_proj_weight [3d][d] */
  const float* b_qkv[QUATTRO_TF_MAX_LAYERS];
  const uint16_t* w_o[QUATTRO_TF_MAX_LAYERS];   /* out_proj.weight [d][d] */
  const float* b_o[QUATTRO_TF_MAX_LAYERS];
  const uint16_t* w_1[QUATTRO_TF_MAX_LAYERS];   /* linear1.weight [ff][d] */
  const float* b_1[QUATTRO_TF_MAX_LAYERS];
  const uint16_t* w_2[QUATTRO_TF_MAX_LAYERS];   /* linear2.weight [d][ff] */
  const float* b_2[QUATTRO_TF_MAX_LAYERS];
  const float* ln1_g[QUATTRO_TF_MAX_LAYERS];
  const float* ln1_b[QUATTRO_TF_MAX_LAYERS];
  const float* ln2_g[QUATTRO_TF_MAX_LAYERS];
  const float* ln2_b[QUATTRO_TF_MAX_LAYERS];
  const uint16_t* w_out;
  const float* b_out;
  /* What the kernel actually reads (built from the arrays above, which stay in the reference's own layout):
   *   tok_bias_t [d][128] : tok_bias transposed and zero-padded to 128 tokens, with the embedding bias of the token's kind
   *                         folded in (state_b on state tokens, ctrl_b on prompt tokens); depends on n_state_tok
   *   w_stream            : every weight matrix as 1-KB MFMA fragments in the order the kernel consumes them
   *                         (quattro_tf_stream_elems bf16 elements, written by quattro_tf_pack_stream_bf16)
   *   p_stream            : biases / LayerNorm vectors / output de-normalisation per layer (quattro_tf_param_floats)      */
  const float* tok_bias_t;
  const uint16_t* w_stream;
  const float* p_stream;
} quattro_tf_weights;

/* Sizes of the two streams for the shape in `w` (0 = unsupported shape), and the packing itself: reads the PyTorch-layout
 * device arrays named in `w` (w_state, ctrl_w, w_qkv .. w_out, every bias / LayerNorm / normaliser vector) and writes
 * w_stream / p_stream (device buffers of the caller).  Run once per set of weights; pure data movement.               */
size_t quattro_tf_stream_elems(const quattro_tf_weights* w);
size_t quattro_tf_param_floats(const quattro_tf_weights* w);
int quattro_tf_pack_stream_bf16(const quattro_tf_weights* w, uint16_t* w_stream, float* p_stream, void* stream);

/* Batched predictor forward, bf16 MFMA with fp32 accumulation, one launch for the whole model (reads tok_bias_t, w_stream,
 * p_stream and the normaliser vectors x_mean — which a caller may point at a shifted mean — only).  Replaces
 * TransformerILQR.predict (quattro_ilqr_tf/transformer_ilqr.py:311-325: normalise, forward, de-normalise) around
 * TransformerPredictor.forward (transformer_model.py:122-138, PositionalEncoding :77-80) for B sequences at once.
 *   x_err  [B][n_state_tok][n_x] : x_seq - x_ref + state_offset (raw, un-normalised)
 *   prompt [B][P][c]             : [k | K.flat] rows of the swept tail (raw)
 *   pred   [B][T][c]             : de-normalised prediction                                                   */
int quattro_tf_forward_bf16(const quattro_tf_weights* w, const float* x_err, const float* prompt, int B, float* pred,
                            void* stream);

/* The same forward with the prediction written straight into gain stacks: row t of the (T, c) prediction viewed as
 * (m, 1 + n) is k_t (column 0) and K_t (the rest), exactly the unpacking of iLQR_TF.optimize (quattro_ilqr_tf.py:510-514
 * / :536-540); c_dim must equal m (1 + n).  Rows t >= N of a prediction longer than the horizon are dropped (the
 * reference's forward_pass never reads them).  Replaces predict + reshape + slicing + the np.concatenate head of
 * :515-518 for a batch.
 *   K [B][N][m][n], k [B][N][m] : rows t < min(T, N) are overwritten, the swept tail rows are the caller's
 *   active [B] (may be NULL)    : trajectories with active[b] == 0 are skipped entirely
 *   prompt == NULL              : the P prompt rows [k | K.flat] (quattro_ilqr_tf.py:498-502) are read from rows N - P .. N - 1
 *                                 of K, k themselves — the tail quattro_linearize_sweep_rows_f32 (k_rows = N) has just swept;
 *                                 requires T + P <= N (the kernel must not write the rows it reads)                          */
int quattro_tf_gains_bf16(const quattro_tf_weights* w, const float* x_err, const float* prompt, int B, int N, int n,
                          int m, float* K, float* k, const int32_t* active, void* stream);

/* The three entry points above with fp16 MFMA operands (w->precision == QUATTRO_TF_PRECISION_F16, `w_*` and w_stream
 * holding IEEE half bit patterns); same arguments, same kernel source (second instantiation: 238 instead of 196
 * registers, measured ~5 % slower at B = 4096; 12x closer to the reference module's fp32 output on the shipped
 * checkpoints).  Each family rejects a weight set of the other precision with QUATTRO_ERR_BAD_ARG.                                                                          */
int quattro_tf_pack_stream_f16(const quattro_tf_weights* w, uint16_t* w_stream, float* p_stream, void* stream);
int quattro_tf_forward_f16(const quattro_tf_weights* w, const float* x_err, const float* prompt, int B, float* pred,
                           void* stream);
int quattro_tf_gains_f16(const quattro_tf_weights* w, const float* x_err, const float* prompt, int B, int N, int n, int m,
                         float* K, float* k, const int32_t* active, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training of the gain predictor, fp32, hand-written forward + backward + Adam.
 * Replaces the body of the mini-batch loop of TransformerILQR.fit (quattro_ilqr_tf/transformer_ilqr.py:150-172:
 * model(x, u_prompt) -> nn.MSELoss -> loss.backward() -> Adam.step()) around TransformerPredictor
 * (transformer_model.py:85-138).  Parameters, gradients and Adam moments are ONE flat fp32 device array each, in the
 * order of quattro_tf_train_param_offset (every block 16-byte aligned; padding floats stay zero); each block has the
 * reference module's own shape and layout (PyTorch [out][in] matrices), so a state dict is a set of slices of it.
 * Shapes: head dimension d_model / nhead <= 32 (the reference's default constructor is 64 / 8), d_model <= 512,
 * L = n_state_tok + prompt_len + target_len <= 128; anything else returns QUATTRO_ERR_UNSUPPORTED.                                                   */
typedef struct quattro_tf_train_desc {
  int32_t state_dim, control_dim, d_model, nhead, n_layers, d_ff;
  int32_t n_state_tok, prompt_len, target_len; /* tokens: N+1 states, P prompt rows, T learnable target rows */
  float dropout;                               /* transformer_model.py:97 (applied only when `training` != 0) */
} quattro_tf_train_desc;

/* blocks of the flat parameter array (reference state_dict name in the comment); the last twelve are per layer */
#define QUATTRO_TF_P_TARGET 0   /* target_embedding [T][d]                    */
#define QUATTRO_TF_P_STATE_W 1  /* state_embed.weight [d][n]                  */
#define QUATTRO_TF_P_STATE_B 2  /* state_embed.bias [d]                       */
#define QUATTRO_TF_P_CTRL_W 3   /* control_embed.weight [d][c]                */
#define QUATTRO_TF_P_CTRL_B 4   /* control_embed.bias [d]                     */
#define QUATTRO_TF_P_OUT_W 5    /* output_linear.weight [c][d]                */
#define QUATTRO_TF_P_OUT_B 6    /* output_linear.bias [c]                     */
#define QUATTRO_TF_P_QKV_W 7    /* layers.l.self_attn.in_proj_weight [3d][d]  */
#define QUATTRO_TF_P_QKV_B 8    /* layers.l.self_attn.in_proj_bias [3d]       */
#define QUATTRO_TF_P_O_W 9      /* layers.l.self_attn.out_proj.weight [d][d]  */
#define QUATTRO_TF_P_O_B 10     /* layers.l.self_attn.out_proj.bias [d]       */
#define QUATTRO_TF_P_FF1_W 11   /* layers.l.linear1.weight [ff][d]            */
#define QUATTRO_TF_P_FF1_B 12   /* layers.l.linear1.bias [ff]                 */
#define QUATTRO_TF_P_FF2_W 13   /* layers.l.linear2.weight [d][ff]            */
#define QUATTRO_TF_P_FF2_B 14   /* layers.l.linear2.bias [d]                  */
#define QUATTRO_TF_P_LN1_G 15   /* layers.l.norm1.weight [d]                  */
#define QUATTRO_TF_P_LN1_B 16   /* layers.l.norm1.bias [d]                    */
#define QUATTRO_TF_P_LN2_G 17   /* layers.l.norm2.weight [d]                  */
#define QUATTRO_TF_P_LN2_B 18   /* layers.l.norm2.bias [d]                    */
#define QUATTRO_TF_P_COUNT 19

/* floats in the flat array (0 = unsupported shape); float offset of a block (-1 = no such block) */
size_t quattro_tf_train_param_count(const quattro_tf_train_desc* desc);
long quattro_tf_train_param_offset(const quattro_tf_train_desc* desc, int which, int layer);
/* bytes of caller-provided scratch for a mini-batch of `batch` sequences (saved activations + gradient temporaries) */
size_t quattro_tf_train_workspace_bytes(const quattro_tf_train_desc* desc, int batch);

/* Forward (+ loss) (+ backward) of one mini-batch.
 *   x_norm [B][n_state_tok][n], prompt_norm [B][P][c], target_norm [B][T][c] : normalised inputs / targets
 *     (DataNormalizer, transformer_model.py:37-50; the slices of transformer_ilqr.py:112-118)
 *   pe [L][d]            : rows of the sinusoidal table pos_encoder.pe (a buffer of the module, not a parameter)
 *   training             : != 0 applies dropout (masks = hash of dropout_seed, site and element index)
 *   loss (may be NULL)   : device scalar, mean squared error over B*T*c
 *   pred_out (may be NULL) : [B][T][c] normalised prediction
 *   grads (may be NULL)  : flat gradient array, overwritten; NULL = forward (+ loss) only (evaluation on the test set,
 *                          transformer_ilqr.py:177-184)
 *   workspace            : 256-byte aligned, >= quattro_tf_train_workspace_bytes                                     */
int quattro_tf_train_step_f32(const quattro_tf_train_desc* desc, const float* params, float* grads, void* workspace,
                              size_t workspace_bytes, const float* x_norm, const float* prompt_norm,
                              const float* target_norm, const float* pe, int batch, uint64_t dropout_seed, int training,
                              float* loss, float* pred_out, void* stream);

/* The backward half of quattro_tf_train_step_f32 on its own, started from a gradient the caller supplies: the gradient of ANY scalar
 * with respect to the normalised prediction, not only the MSE's.  It is the backward of the mini-batch whose forward last filled
 * this workspace, i.e. of quattro_tf_train_step_f32(desc, params, grads = NULL, workspace, ..., pred_out != NULL, ...) with the same
 * desc, params, x_norm, prompt_norm, batch, dropout_seed and training flag (the dropout masks are recomputed from the seed; the saved
 * activations are read from the workspace, which nothing may have written in between).
 *   d_pred [B][T][c]     : d(scalar) / d(pred_out)
 *   grads                : flat gradient array, overwritten, as the step overwrites it
 * The step itself is forward half, MSE kernel, this backward half on its own d_pred buffer: the same launches in the same order.
 * Return codes as the step's: QUATTRO_ERR_BAD_ARG (a NULL pointer, batch <= 0), QUATTRO_ERR_UNSUPPORTED (shape),
 * QUATTRO_ERR_WORKSPACE, QUATTRO_ERR_LAUNCH.                                                                             */
int quattro_tf_train_backward_f32(const quattro_tf_train_desc* desc, const float* params, float* grads, void* workspace,
                                  size_t workspace_bytes, const float* x_norm, const float* prompt_norm, const float* d_pred,
                                  int batch, uint64_t dropout_seed, int training, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Task loss of the gain predictor: between its output tokens and the gain stacks of a tracked run (csrc/tf_gain_loss.hip).
 * A training step on the closed-loop cost of the predicted gains is: quattro_tf_train_step_f32 (grads = NULL, pred_out),
 * quattro_tf_gains_unpack_f32, quattro_track_f32 (K_out, u_ff), quattro_score_f32, quattro_track_gradient_f32 (grad_K, grad_u_nom),
 * quattro_tf_gains_pack_grad_f32, quattro_tf_train_backward_f32.
 * Token layout, c = m (1 + n): element i (1 + n) is the feed-forward k_i, element i (1 + n) + 1 + j the gain K_ij -- the data set's
 * layout (what quattro_tf_gains_* unpack), NOT the solver's prompt layout [k | K.flat].  Tn = min(T, N).
 * Every fp32 value below is formed by the single rounded operations written, in that order, never contracted to an FMA.
 *
 * unpack:   raw = pred_norm * u_std[e] + u_mean[e]                       (product, then sum)
 *           K_out[b][t] = t < Tn ? raw gains of token t : K_log[b][t]
 *           u_ff[b][t]  = u_nom[b][t] + alpha * (t < Tn ? raw k of token t : k_log[b][t])      (product, then sum)
 *   pred_norm [B][T][c]; u_mean, u_std [c]; K_log, K_out [B][N][m][n]; k_log, u_nom, u_ff [B][N][m].  Outputs must not alias inputs.
 *
 * pack_grad: with f_b = (float)((double)task_weight * (scale ? scale[b] : 1) / B), for rows t < Tn
 *           d_pred[b][t][i (1 + n)]         = ((grad_u_nom[b][t][i] * alpha) * f_b) * u_std[e]
 *           d_pred[b][t][i (1 + n) + 1 + j] = (grad_K[b][t][i][j] * f_b) * u_std[e]
 *           rows Tn <= t < T are +0.0 (predicted rows that no step uses); with mse_weight != 0 every row additionally receives
 *           mse_weight * ((2 * (pred_norm - target_norm)) * (1.0f / (float)(B T c)))             (the MSE kernel's gradient)
 *           terms[b] = ((double)task_weight * scale[b] * cost[b]) / B + mse_weight * (sum over the block of (pred - target)^2, fp64) / (B T c)
 *           loss = terms[0] + terms[1] + ... + terms[B - 1], fp64, in that order (one lane: no atomics, the same on every run)
 *   A trajectory whose cost, factor f_b or any element of grad_K[b], grad_u_nom[b] is not finite is left out: diverged[b] = 1, its
 *   whole block of d_pred is +0.0 and terms[b] = 0; this is decided by a vote of the one wave that owns the trajectory before it
 *   writes anything.  Otherwise diverged[b] = 0.
 *   grad_K [B][N][m][n], grad_u_nom [B][N][m] : what quattro_track_gradient_f32 wrote;  cost [B] fp64 : quattro_score_f32's totals
 *   scale [B] or NULL (= 1); pred_norm, target_norm [B][T][c] : read only with mse_weight != 0 (QUATTRO_ERR_BAD_ARG if then NULL)
 *   d_pred [B][T][c], diverged [B], terms [B] fp64, loss [1] fp64 : outputs
 * Both: QUATTRO_ERR_BAD_ARG for a NULL pointer (other than the optional ones) or B, T, N, n, m <= 0.                    */
int quattro_tf_gains_unpack_f32(const float* pred_norm, const float* u_mean, const float* u_std, const float* K_log,
                                const float* k_log, const float* u_nom, float alpha, int B, int T, int N, int n, int m,
                                float* K_out, float* u_ff, void* stream);
int quattro_tf_gains_pack_grad_f32(const float* grad_K, const float* grad_u_nom, const double* cost, const float* scale,
                                   const float* u_std, float alpha, float task_weight, const float* pred_norm,
                                   const float* target_norm, float mse_weight, int B, int T, int N, int n, int m, float* d_pred,
                                   int32_t* diverged, double* terms, double* loss, void* stream);

/* torch.optim.Adam with its defaults as the reference uses it (transformer_ilqr.py:140; no weight decay, bias-corrected
 * moments), over the flat arrays; `step` counts from 1.                                                               */
int quattro_tf_adam_f32(float* params, const float* grads, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                        float eps, int step, void* stream);

/* Test hook: the dropout factors (0 or 1 / (1 - p)) the training step applies at `site` (0: positions; 1 + 4 l + k for
 * layer l: k = 0 attention weights [B][H][L][L], 1 out-projection [B L][d], 2 feed-forward hidden [B L][ff],
 * 3 feed-forward output [B L][d]) for elements 0 .. n-1.                                                              */
int quattro_tf_train_dropout_mask_f32(uint64_t dropout_seed, float p, int site, size_t n, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QUATTRO_HIP_H */
