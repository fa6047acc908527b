// Gradient of the tracked closed-loop cost (quattro_track_gradient_f32): S = n_steps <= N steps of quattro_track_f32 composed with
// quattro_score_f32 at ref_hold = 1,
//   u_t = u_nom_t + K_t (x_t - x_nom_t),   x_{t+1} = f_plant(x_t, u_t) + d_t,   J = sum_{t<S} L(x_t, u_t) + [terminal] Lf(x_S)
// about the realised (x, u):
//   lambda_S = terminal ? Lf_x(x_S) : 0;   t = S-1 .. 0:   g_t = L_u + B_t^T lambda_{t+1},   lambda_t = L_x + A_t^T lambda_{t+1} + K_t^T g_t
//   dJ/du_nom_t = g_t,  dJ/dK_t = g_t (x_t - x_nom_t)^T,  dJ/dx_nom_t = -K_t^T g_t,  dJ/dx0 = lambda_0,  dJ/dd_t = lambda_{t+1}
// The law differentiated is the reference's forward_pass (quattro_ilqr_tf/quattro_ilqr_tf.py:377-390) with k = 0, alpha = 1; the
// reference has no counterpart (it never differentiates its forward pass).
//
// The mapping is cost_gradient_kernel's (cost_gradient.hip): a group of LPI adjacent lanes owns one trajectory, lane j direction j of
// z = (x, u); columns and l_z entries are formed off the chain for QUATTRO_GRAD_BLOCK steps at a time and staged in LDS.  The
// feedback is folded into what is STAGED, so the chain does not change:
//   lambda_t = (l_x + K^T l_u) + (A + B K)^T lambda_{t+1}      -- K^T g_t spelled out
//   state lane j   : pushes the direction (e_j, K_t[:, j]) through the step -- ONE tangent, as before -- which is column j of
//                    A_t + B_t K_t, and stages it with l_x[j] + K_t[:, j]^T l_u
//   control lane a : column a of B_t and l_u[a], as before
//   on the chain   : per step one n-term fmaf chain per lane and ONE exchange of lambda inside the group.  g_t is what the control
//                    lanes' chains produce; K_t^T g_t is never formed there, so no second exchange is needed.  The control lanes
//                    park g_t in LDS (a write nobody waits for)
//   after a block  : state lane j reads the block's g_t back and writes g_a (x_{t,j} - x_nom_{t,j}) and -sum_a K_t[a][j] g_a
// K == NULL: the state lanes' control seed is zero and the kernel is the open-loop adjoint sweep.
// Rows as cost_gradient_kernel takes them (a private block of VALUES behind wave-uniform branches).  No atomics, no global workspace,
// nothing allocated; a trajectory's results do not depend on B or on its place in the batch.
#include "grad_device.h"

namespace {

constexpr int GRAD_BLOCK = QUATTRO_GRAD_BLOCK;

template <int MODEL, bool RK4, int LPI>
__global__ __launch_bounds__(QT_WAVE) void track_gradient_kernel(
    const quattro_model_params p, const float* __restrict__ x, const float* __restrict__ u, const int B, const int N, const int S,
    const float* __restrict__ x_nom, const float* __restrict__ K, const float* __restrict__ model_phys,
    const float* __restrict__ x_ref_rows, const int ref_rows, const float* __restrict__ cost_rows, const int terminal,
    float* __restrict__ grad_u_nom, float* __restrict__ grad_K, float* __restrict__ grad_x_nom, float* __restrict__ grad_x0,
    float* __restrict__ costate) {
  constexpr int NX = ModelDims<MODEL>::NX, NU = ModelDims<MODEL>::NU, NZ = NX + NU;
  constexpr int ROW = NX + 1;                                  // staged per step and lane: the column and the l_z entry
  static_assert(NZ <= LPI && QT_WAVE % LPI == 0, "one lane per direction of z");
  __shared__ float s_stage[GRAD_BLOCK * ROW * QT_WAVE];
  __shared__ float s_lam[QT_WAVE];
  __shared__ float s_g[GRAD_BLOCK * QT_WAVE];                  // g_t of the block's steps: [slot][group's lanes][control]
  const int lane = threadIdx.x;
  const int grp = lane / LPI, j = lane % LPI;
  constexpr int SPP = LPI / NZ;                                // steps a group linearises per pass (cost_gradient_kernel)
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
  const float* xb = x + bb * (size_t)(S + 1) * NX;             // the realised run: S + 1 states, S controls
  const float* ub = u + bb * (size_t)S * NU;
  const float* Kb = K != nullptr ? K + bb * (size_t)N * NU * NX : nullptr;      // what the run was given: N rows
  const float* xnb = K != nullptr ? x_nom + bb * (size_t)(N + 1) * NX : nullptr;
  // the reference of step t (t = S: the terminal term): row min(t, ref_rows - 1), quattro_score_f32's rule at ref_hold = 1
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
  float lam[NX];
  // (one wave per workgroup: its LDS operations complete in program order, cost_gradient_kernel's note)
  auto exchange = [&](float v) __attribute__((always_inline)) {
    if (j < NX) s_lam[grp * LPI + j] = v;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NX; ++i) lam[i] = s_lam[grp * LPI + i];
  };

  // rows the tracked steps did not read: +0.0
  if (live) {
    float* z = grad_u_nom + (bb * (size_t)N + (size_t)S) * NU;
    for (int i = j; i < (N - S) * NU; i += LPI) z[i] = 0.0f;
    if (grad_K != nullptr) {
      z = grad_K + (bb * (size_t)N + (size_t)S) * NU * NX;
      for (int i = j; i < (N - S) * NU * NX; i += LPI) z[i] = 0.0f;
    }
    if (grad_x_nom != nullptr) {
      z = grad_x_nom + (bb * (size_t)(N + 1) + (size_t)S) * NX;
      for (int i = j; i < (N + 1 - S) * NX; i += LPI) z[i] = 0.0f;
    }
  }

  float v;
  {
    float xS[NX];
    load_vec<NX>(xb + (size_t)S * NX, xS);
    set_ref(S);
    v = grad_terminal_entry<MODEL>(own, xS, j);
    v = terminal != 0 ? v : 0.0f;
    if (live && j < NX && costate != nullptr) costate[(bb * (size_t)(S + 1) + (size_t)S) * NX + j] = v;
    exchange(v);
  }
  for (int t_hi = S; t_hi > 0; t_hi -= GRAD_BLOCK) {
    const int cnt = t_hi < GRAD_BLOCK ? t_hi : GRAD_BLOCK;     // steps t_hi - 1 .. t_hi - cnt, slot s holds step t_hi - 1 - s
#pragma unroll 1
    for (int s0 = 0; s0 < cnt; s0 += SPP) {
      const int s = s0 + sub;
      const bool mine = sub < SPP && s < cnt;                  // lanes without a step of their own redo step s0 and store nothing
      const int t = t_hi - 1 - (mine ? s : s0);
      float xs[NX], us[NU], du[NU], col[NX];
      load_vec<NX>(xb + (size_t)t * NX, xs);
      load_vec<NU>(ub + (size_t)t * NU, us);
      // the lane's control seed: a control lane's own unit vector; a state lane's column of K_t (zero with the feedback off)
#pragma unroll
      for (int a = 0; a < NU; ++a) du[a] = (NX + a == dir) ? 1.0f : 0.0f;
      if (Kb != nullptr && dir < NX) {
        const float* kc = Kb + (size_t)t * NU * NX + dir;
#pragma unroll
        for (int a = 0; a < NU; ++a) du[a] = kc[a * NX];
      }
      set_ref(t);
      const float lz = track_item<MODEL, RK4>(own, xs, us, dir, du, col);
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
      if (j >= NX && j < NZ) s_g[s * QT_WAVE + grp * LPI + (j - NX)] = v;      // parked for the block's products below
      if (live) {
        if (j >= NX && j < NZ) grad_u_nom[(bb * (size_t)N + (size_t)t) * NU + (j - NX)] = v;
        if (j < NX && costate != nullptr) costate[(bb * (size_t)(S + 1) + (size_t)t) * NX + j] = v;
      }
      exchange(v);
      if (s + 1 < cnt) {
#pragma unroll
        for (int i = 0; i < NX; ++i) col[i] = coln[i];
        lz = lzn;
      }
    }
    __syncthreads();                                           // the stage is rewritten by the next block of steps; s_g is complete
    // off the chain: dJ/dK_t = g_t (x_t - x_nom_t)^T and dJ/dx_nom_t = -K_t^T g_t of the block's steps, entry j by state lane j
    if (Kb != nullptr && (grad_K != nullptr || grad_x_nom != nullptr) && live && j < NX) {
      for (int s = 0; s < cnt; ++s) {
        const int t = t_hi - 1 - s;
        float g[NU];
#pragma unroll
        for (int a = 0; a < NU; ++a) g[a] = s_g[s * QT_WAVE + grp * LPI + a];
        if (grad_K != nullptr) {
          const float e = xb[(size_t)t * NX + j] - xnb[(size_t)t * NX + j];
          float* gk = grad_K + (bb * (size_t)N + (size_t)t) * NU * NX + j;
#pragma unroll
          for (int a = 0; a < NU; ++a) gk[a * NX] = g[a] * e;
        }
        if (grad_x_nom != nullptr) {
          const float* kc = Kb + (size_t)t * NU * NX + j;
          float acc = 0.0f;
#pragma unroll
          for (int a = 0; a < NU; ++a) acc = fmaf(kc[a * NX], g[a], acc);
          grad_x_nom[(bb * (size_t)(N + 1) + (size_t)t) * NX + j] = -acc;
        }
      }
    }
    __syncthreads();                                           // s_g is rewritten by the next block's chain
  }
  if (live && j < NX && grad_x0 != nullptr) grad_x0[bb * NX + j] = v;     // lambda_0: the value costate[b][0] was given
}

template <int MODEL, int LPI>
int launch_track_gradient(const quattro_model_params& p, const float* x, const float* u, int B, int N, int S, const float* x_nom,
                          const float* K, const float* model_phys, const float* x_ref_rows, int ref_rows, const float* cost_rows,
                          int terminal, float* grad_u_nom, float* grad_K, float* grad_x_nom, float* grad_x0, float* costate,
                          hipStream_t stream) {
  constexpr int PER = QT_WAVE / LPI;
  const dim3 grid((unsigned)((B + PER - 1) / PER)), block(QT_WAVE);
  if (p.integrator == QUATTRO_INTEGRATOR_EULER)
    hipLaunchKernelGGL((track_gradient_kernel<MODEL, false, LPI>), grid, block, 0, stream, p, x, u, B, N, S, x_nom, K, model_phys,
                       x_ref_rows, ref_rows, cost_rows, terminal, grad_u_nom, grad_K, grad_x_nom, grad_x0, costate);
  else if (p.integrator == QUATTRO_INTEGRATOR_RK4)
    hipLaunchKernelGGL((track_gradient_kernel<MODEL, true, LPI>), grid, block, 0, stream, p, x, u, B, N, S, x_nom, K, model_phys,
                       x_ref_rows, ref_rows, cost_rows, terminal, grad_u_nom, grad_K, grad_x_nom, grad_x0, costate);
  else
    return QUATTRO_ERR_UNSUPPORTED;
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

}  // namespace

int quattro_launch_track_gradient(const quattro_model_params& p, const float* x, const float* u, int B, int N, int S,
                                  const float* x_nom, const float* K, const float* model_phys, const float* x_ref_rows, int ref_rows,
                                  const float* cost_rows, int terminal, float* grad_u_nom, float* grad_K, float* grad_x_nom,
                                  float* grad_x0, float* costate, hipStream_t stream) {
  if (p.model_id == QUATTRO_MODEL_CARTPOLE)
    return launch_track_gradient<QUATTRO_MODEL_CARTPOLE, 16>(p, x, u, B, N, S, x_nom, K, model_phys, x_ref_rows, ref_rows, cost_rows,
                                                             terminal, grad_u_nom, grad_K, grad_x_nom, grad_x0, costate, stream);
  if (p.model_id == QUATTRO_MODEL_QUADROTOR)
    return launch_track_gradient<QUATTRO_MODEL_QUADROTOR, 16>(p, x, u, B, N, S, x_nom, K, model_phys, x_ref_rows, ref_rows, cost_rows,
                                                              terminal, grad_u_nom, grad_K, grad_x_nom, grad_x0, costate, stream);
#ifdef QT_USER_MODEL_HEADER
  if (p.model_id == QUATTRO_MODEL_USER) {
    constexpr int NZ = QT_USER_NX + QT_USER_NU, LPI = NZ <= 8 ? 8 : (NZ <= 16 ? 16 : 32);
    return launch_track_gradient<QUATTRO_MODEL_USER, LPI>(p, x, u, B, N, S, x_nom, K, model_phys, x_ref_rows, ref_rows, cost_rows,
                                                          terminal, grad_u_nom, grad_K, grad_x_nom, grad_x0, costate, stream);
  }
#endif
  return QUATTRO_ERR_UNSUPPORTED;
}
