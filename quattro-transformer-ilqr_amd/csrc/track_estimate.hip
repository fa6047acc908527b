// Output feedback inside a tracked closed-loop run (quattro_track_estimate_f32): S steps of the gain law acting on the estimate of an
// extended Kalman filter that runs in the same launch.  Per trajectory, obs the p_y observed state indices (ascending, distinct):
//   x_0 = x0,  xh = xhat0 (NULL: x0),  P = cov0 (NULL: 0)
//   measure   y_i = x_t[obs_i] + v_t[i]
//   update    for i in order, j = obs_i:  g = P[:, j],  s = P[j][j] + R_i,  e = y_i - xh[j],  nis_t += e^2 / s,  xh += g e / s,
//             P -= g g^T / s                                 (a selection sensor with diagonal R: exactly the batch update)
//   control   u_t = u_nom_t + K_t (xh - x_nom_t)            (xh AFTER the update)
//   plant     x_{t+1} = f_plant(x_t, u_t) + d_t
//   predict   A = df_model/dx at (xh, u_t),  xh <- f_model(xh, u_t),  P <- A P A^T + W
// The reference has no counterpart.
//
// Mapping: track_covariance.hip's.  A trajectory owns 4 NP lanes, NP the padded state dimension: the quadrotor a whole wave with P in
// the C/D layout of v_mfma_f32_16x16x4_f32 (lane (g, c), register v: P[4 g + v][c], the padding held at zero), the cart-pole a group
// of 16 lanes with lane (i, c) holding P[i][c], four trajectories a wave.  Besides P a lane keeps x_t[c] and xh[c] of its column.
// Everything is on the serial chain here, because the estimator linearises at its own estimate:
//   update    j is wave-uniform.  The row g^T = P[j][:] (P is read as symmetric) is register j % 4 of lane row j / 4, the column
//             g = P[:, j] is lane c = j of every lane row: both come by ds_bpermute (__shfl), one per register of P plus three for
//             P[j][j], x_t[j] and xh[j].  Chosen over parking the column in LDS because a bpermute is one LDS-crossbar trip with no
//             store to wait for, and the update never needs more than these lanes' registers; DPP row broadcasts cannot take a
//             run-time source lane.  Per observed state: 1 / s once, then xh[c] += g[c] (e / s), P[i][c] -= g[i] (g[c] / s).
//   control   xh, x_nom_t, u_nom_t and K_t go through LDS (K_t, x_nom_t, u_nom_t loaded one step ahead, one float a lane) and every
//             lane forms u_t with the fmaf chain of track_body (rollout_body.h): no lane waits for another's u.
//   steps     lane c < n: column c of A (track_item with a zero control seed, grad_device.h), staged as the tile's row-major operand;
//             lane n: the plant's step; lane n + 1: the estimator's base step.  Where the two integrators agree these two lanes run ONE
//             qt_step on lane-selected parameters and states, so a perfectly informed estimator (xh = x, the same parameters) stays
//             bit-identical to the plant: every innovation is then an exact zero.
//   predict   quadrotor: U = P A^T and P' = A U + W, 4 + 4 MFMAs with the one staged operand (track_covariance.hip's note); the
//             cart-pole forms the products with fmaf over LDS broadcasts.
// Outputs leave from the registers that hold them (no parking): x, xh from the column lanes of lane row 0, var / cov from the tile.
// Rows (model_phys, plant_phys, meas_var) enter as VALUES behind wave-uniform branches.  No atomics, no global workspace, nothing
// allocated; a trajectory's results do not depend on B or on its place in the batch; groups past the batch store nothing.
// One wave per workgroup: its LDS operations complete in program order; __syncthreads() is the compiler's fence and one s_barrier.
#include "grad_device.h"

namespace {

typedef float est_f32x4 __attribute__((ext_vector_type(4)));

struct EstArgs {
  const float *x0, *x_nom, *u_nom, *K, *meas_var, *xhat0, *cov0, *noise, *meas_noise, *disturbance, *plant_phys, *model_phys;
  float *x, *u, *xhat, *var, *cov, *nis;
  int B, N, S, p_y, meas_var_rows;
  int obs[QUATTRO_MAX_NX];
  float plant_phys0[8];
};

template <int MODEL, bool RK4_PLANT, bool RK4_MODEL>
__global__ __launch_bounds__(QT_WAVE) void track_estimate_kernel(const quattro_model_params p, const EstArgs a) {
  constexpr int NX = ModelDims<MODEL>::NX, NU = ModelDims<MODEL>::NU;
  constexpr bool TILE16 = NX > 4;
  constexpr int NP = TILE16 ? 16 : 4;                          // padded state dimension
  constexpr int LD = TILE16 ? 20 : 4;                          // row stride of the staged tile (track_covariance.hip)
  constexpr int TILE = NP * LD, LPT = 4 * NP, PER = QT_WAVE / LPT;
  constexpr int VX = 0, VXH = NP, VXN = 2 * NP, VUN = 3 * NP, VK = 3 * NP + 4, VEC = VK + NU * NX;     // the group's vectors in LDS
  static_assert(NX + 2 <= LPT && NU <= 4 && NU * NX <= LPT && VEC % 4 == 0 && NX % 4 == 0, "a lane per direction, step and gain entry");
  __shared__ __attribute__((aligned(16))) float s_a[PER * TILE];                 // A, row-major, the padding zero
  __shared__ __attribute__((aligned(16))) float s_v[PER * VEC];
  __shared__ __attribute__((aligned(16))) float s_p[TILE16 ? 4 : PER * TILE];    // the cart-pole's P and U = P A^T
  __shared__ __attribute__((aligned(16))) float s_u[TILE16 ? 4 : PER * TILE];
  const int lane = threadIdx.x;
  const int grp = lane / LPT, r = lane % LPT;
  const int sub = r / NP, dir = r % NP;                        // tile row group (or row) and column
  const long long braw = (long long)blockIdx.x * PER + grp;
  const bool live = braw < a.B;                                // groups past the batch recompute trajectory B - 1 and store nothing
  const size_t bb = live ? (size_t)braw : (size_t)(a.B - 1);
  const int B = a.B, N = a.N, S = a.S, p_y = a.p_y;
  const bool col_lane = sub == 0 && dir < NX;                  // the lane that keeps x[dir] and xh[dir] for the outputs

  float phm[8], php[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    phm[i] = p.phys[i];
    php[i] = a.plant_phys0[i];
  }
  if (a.model_phys != nullptr) {
#pragma unroll
    for (int i = 0; i < 8; ++i) phm[i] = a.model_phys[bb * 8 + i];
  }
  if (a.plant_phys != nullptr) {
#pragma unroll
    for (int i = 0; i < 8; ++i) php[i] = a.plant_phys[bb * 8 + i];
  }
  quattro_model_params pm = p;
#pragma unroll
  for (int i = 0; i < 8; ++i) pm.phys[i] = phm[i];

  float* const ag = s_a + grp * TILE;
  float* const vg = s_v + grp * VEC;
  for (int i = r; i < TILE; i += LPT) ag[i] = 0.0f;            // the padding of A: staged once, never written again

  const float* xnb = a.x_nom + bb * (size_t)(N + 1) * NX;
  const float* unb = a.u_nom + bb * (size_t)N * NU;
  const float* Kb = a.K + bb * (size_t)N * NU * NX;
  float* xo = a.x + bb * (size_t)(S + 1) * NX;
  float* xho = a.xhat != nullptr ? a.xhat + bb * (size_t)(S + 1) * NX : nullptr;

  // entry (i, j) of a [B][n][n] input, zero in the padding and for a NULL input
  auto entry = [&](const float* m, int i, int j) __attribute__((always_inline)) {
    return (m != nullptr && i < NX && j < NX) ? m[bb * (size_t)(NX * NX) + (size_t)(i * NX + j)] : 0.0f;
  };
  // TILE16: P[v] = P[4 sub + v][dir], wn[v] the same entries of W; else P[0] = P[sub][dir]
  est_f32x4 P = {0.0f, 0.0f, 0.0f, 0.0f}, wn = {0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (TILE16) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      P[v] = entry(a.cov0, 4 * sub + v, dir);
      wn[v] = entry(a.noise, 4 * sub + v, dir);
    }
  } else {
    P[0] = entry(a.cov0, sub, dir);
    wn[0] = entry(a.noise, sub, dir);
  }
  // var / cov of row t from the registers that hold them
  auto store_P = [&](int t) __attribute__((always_inline)) {
    if (!live || dir >= NX) return;
    const size_t row = bb * (size_t)(S + 1) + (size_t)t;
#pragma unroll
    for (int v = 0; v < (TILE16 ? 4 : 1); ++v) {
      const int i = TILE16 ? 4 * sub + v : sub;
      if (i < NX) {
        if (a.cov != nullptr) a.cov[(row * NX + (size_t)i) * NX + dir] = P[v];
        if (a.var != nullptr && i == dir) a.var[row * NX + dir] = P[v];
      }
    }
  };

  const int dc = dir < NX ? dir : 0;
  float xl = dir < NX ? a.x0[bb * NX + dc] : 0.0f;             // x_t[dir]
  float xhl = xl;                                              // xh[dir]
  if (a.xhat0 != nullptr) xhl = dir < NX ? a.xhat0[bb * NX + dc] : 0.0f;
  if (live && col_lane) xo[dir] = xl;
  if (sub == 0) vg[VX + dir] = xl;
  // a lane's share of what the steps read: R_i (once), and of step t: v_t[i], d_t[dir], K_t, x_nom_t, u_nom_t, one step ahead
  const int oi = r < p_y ? r : 0;
  const float rreg = a.meas_var[(a.meas_var_rows != 0 ? bb * (size_t)p_y : (size_t)0) + oi];
  float vreg = 0.0f, dreg = 0.0f, kreg, xnreg, unreg;
  auto fetch = [&](int t) __attribute__((always_inline)) {
    if (a.meas_noise != nullptr) vreg = a.meas_noise[((size_t)t * B + bb) * p_y + oi];
    if (a.disturbance != nullptr) dreg = a.disturbance[((size_t)t * B + bb) * NX + dc];
    kreg = Kb[(size_t)t * NU * NX + (r < NU * NX ? r : 0)];
    xnreg = xnb[(size_t)t * NX + dc];
    unreg = unb[(size_t)t * NU + (r < NU ? r : 0)];
  };
  fetch(0);

#pragma unroll 1
  for (int t = 0; t < S; ++t) {
    // ---- measure and update, one observed state after the other
    float nis = 0.0f;
#pragma unroll 1
    for (int i = 0; i < p_y; ++i) {
      const int j = a.obs[i];
      const float Ri = __shfl(rreg, i, LPT);
      float y = __shfl(xl, j, LPT);
      if (a.meas_noise != nullptr) y += __shfl(vreg, i, LPT);
      const float xhj = __shfl(xhl, j, LPT);
      float grow, pjj;
      est_f32x4 gcol = {0.0f, 0.0f, 0.0f, 0.0f};
      if constexpr (TILE16) {
        const int jv = j & 3, jr = (j >> 2) * 16;
        const float sel = jv == 0 ? P[0] : (jv == 1 ? P[1] : (jv == 2 ? P[2] : P[3]));
        grow = __shfl(sel, jr + dir, QT_WAVE);                 // P[j][dir]
        pjj = __shfl(sel, jr + j, QT_WAVE);
#pragma unroll
        for (int v = 0; v < 4; ++v) gcol[v] = __shfl(P[v], sub * 16 + j, QT_WAVE);      // P[4 sub + v][j]
      } else {
        grow = __shfl(P[0], j * 4 + dir, LPT);
        pjj = __shfl(P[0], j * 4 + j, LPT);
        gcol[0] = __shfl(P[0], sub * 4 + j, LPT);
      }
      const float inv = 1.0f / (pjj + Ri);
      const float e = y - xhj;
      const float w = e * inv;
      nis += e * w;
      xhl += grow * w;
      const float h = grow * inv;
#pragma unroll
      for (int v = 0; v < (TILE16 ? 4 : 1); ++v) P[v] -= gcol[v] * h;
    }
    // ---- the outputs of row t, and what the control reads
    if (live) {
      if (col_lane && xho != nullptr) xho[(size_t)t * NX + dir] = xhl;
      if (r == 0 && a.nis != nullptr) a.nis[bb * (size_t)S + t] = nis;
    }
    store_P(t);
    if (sub == 0) {
      vg[VXH + dir] = xhl;
      vg[VXN + dir] = xnreg;
    }
    if (r < NU) vg[VUN + r] = unreg;
    if (r < NU * NX) vg[VK + r] = kreg;
    __syncthreads();
    const float dnow = dreg;
    fetch(t + 1 < S ? t + 1 : t);
    // ---- control: every lane, the fmaf chain of track_body
    float xh[NX], us[NU];
    {
      float xn[NX];
      load_vec<NX>(vg + VXH, xh);
      load_vec<NX>(vg + VXN, xn);
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        float Kc[NX];
        load_vec<NX>(vg + VK + c * NX, Kc);
        float uc = vg[VUN + c];
#pragma unroll
        for (int i = 0; i < NX; ++i) uc = fmaf(Kc[i], xh[i] - xn[i], uc);
        us[c] = uc;
        if (live && r == c) a.u[(bb * (size_t)S + (size_t)t) * NU + c] = uc;
      }
    }
    // ---- column dir of A at (xh, u_t); the plant's step and the estimator's base step
    if (r < NX) {
      float du[NU], col[NX];
#pragma unroll
      for (int c = 0; c < NU; ++c) du[c] = 0.0f;
      track_item<MODEL, RK4_MODEL>(pm, xh, us, dir, du, col);
#pragma unroll
      for (int i = 0; i < NX; ++i) ag[i * LD + dir] = col[i];
    }
    if constexpr (RK4_PLANT == RK4_MODEL) {
      if (r == NX || r == NX + 1) {
        const bool plant = r == NX;
        quattro_model_params ps = p;
        float xin[NX], xnext[NX];
        load_vec<NX>(vg + VX, xin);
#pragma unroll
        for (int i = 0; i < 8; ++i) ps.phys[i] = plant ? php[i] : phm[i];
#pragma unroll
        for (int i = 0; i < NX; ++i) xin[i] = plant ? xin[i] : xh[i];
        qt_step<MODEL, RK4_MODEL>(ps, xin, us, xnext);
        store_vec<NX>(vg + (plant ? VX : VXH), xnext);
      }
    } else {
      if (r == NX) {
        quattro_model_params ps = p;
        float xin[NX], xnext[NX];
        load_vec<NX>(vg + VX, xin);
#pragma unroll
        for (int i = 0; i < 8; ++i) ps.phys[i] = php[i];
        qt_step<MODEL, RK4_PLANT>(ps, xin, us, xnext);
        store_vec<NX>(vg + VX, xnext);
      }
      if (r == NX + 1) {
        float xnext[NX];
        qt_step<MODEL, RK4_MODEL>(pm, xh, us, xnext);
        store_vec<NX>(vg + VXH, xnext);
      }
    }
    __syncthreads();
    // ---- predict: P <- A P A^T + W
    if constexpr (TILE16) {
      // lane (g, c) = (sub, dir): A[c][4 g .. 4 g + 3], the k-slices of A^T as a B operand and of A as an A operand
      const est_f32x4 av = *reinterpret_cast<const est_f32x4*>(ag + dir * LD + 4 * sub);
      est_f32x4 U = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int v = 0; v < 4; ++v) U = __builtin_amdgcn_mfma_f32_16x16x4f32(P[v], av[v], U, 0, 0, 0);       // U = P A^T
      est_f32x4 pn = wn;
#pragma unroll
      for (int v = 0; v < 4; ++v) pn = __builtin_amdgcn_mfma_f32_16x16x4f32(av[v], U[v], pn, 0, 0, 0);     // P' = A U + W
      P = pn;
    } else {
      // lane (i, c) = (sub, dir): U[i][c] = sum_k P[i][k] A[c][k], P'[i][c] = W[i][c] + sum_k A[i][k] U[k][c]
      float* pg = s_p + grp * TILE;
      float* ug = s_u + grp * TILE;
      const est_f32x4 ac = *reinterpret_cast<const est_f32x4*>(ag + dir * LD);
      const est_f32x4 ai = *reinterpret_cast<const est_f32x4*>(ag + sub * LD);
      pg[sub * LD + dir] = P[0];
      __syncthreads();
      const est_f32x4 row = *reinterpret_cast<const est_f32x4*>(pg + sub * LD);
      float uv = row[0] * ac[0];
#pragma unroll
      for (int k = 1; k < 4; ++k) uv = fmaf(row[k], ac[k], uv);
      ug[sub * LD + dir] = uv;
      __syncthreads();
      float pn = wn[0];
#pragma unroll
      for (int k = 0; k < 4; ++k) pn = fmaf(ai[k], ug[k * LD + dir], pn);
      P[0] = pn;
    }
    // ---- the lane's entries of x_{t+1} (the disturbance enters after the plant's step) and of the predicted xh
    xhl = dir < NX ? vg[VXH + dc] : 0.0f;
    xl = dir < NX ? vg[VX + dc] : 0.0f;
    if (a.disturbance != nullptr) xl += dnow;
    if (sub == 0) vg[VX + dir] = xl;
    if (live && col_lane) xo[(size_t)(t + 1) * NX + dir] = xl;
  }
  // row S: the last prediction
  if (live && col_lane && xho != nullptr) xho[(size_t)S * NX + dir] = xhl;
  store_P(S);
}

template <int MODEL>
int launch_track_estimate(const quattro_model_params& p, int plant_integrator, const EstArgs& a, hipStream_t stream) {
  constexpr int PER = ModelDims<MODEL>::NX > 4 ? 1 : 4;
  const dim3 grid((unsigned)((a.B + PER - 1) / PER)), block(QT_WAVE);
  const bool rm = p.integrator == QUATTRO_INTEGRATOR_RK4, rp = plant_integrator == QUATTRO_INTEGRATOR_RK4;
  if ((!rm && p.integrator != QUATTRO_INTEGRATOR_EULER) || (!rp && plant_integrator != QUATTRO_INTEGRATOR_EULER))
    return QUATTRO_ERR_UNSUPPORTED;
  if (rp && rm) hipLaunchKernelGGL((track_estimate_kernel<MODEL, true, true>), grid, block, 0, stream, p, a);
  else if (rp) hipLaunchKernelGGL((track_estimate_kernel<MODEL, true, false>), grid, block, 0, stream, p, a);
  else if (rm) hipLaunchKernelGGL((track_estimate_kernel<MODEL, false, true>), grid, block, 0, stream, p, a);
  else hipLaunchKernelGGL((track_estimate_kernel<MODEL, false, false>), grid, block, 0, stream, p, a);
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

}  // namespace

// observed: HOST array of p_y indices (checked by the caller); everything else as quattro_track_estimate_f32 takes it
int quattro_launch_track_estimate(const quattro_model_params& p, const PlantSpec& plant, const float* x0, const float* x_nom,
                                  const float* u_nom, const float* K, int B, int N, int S, const int32_t* observed, int p_y,
                                  const float* meas_var, int meas_var_rows, const float* xhat0, const float* cov0, const float* noise,
                                  const float* meas_noise, const float* disturbance, const float* plant_phys, const float* model_phys,
                                  float* x, float* u, float* xhat, float* var, float* cov, float* nis, hipStream_t stream) {
  EstArgs a;
  a.x0 = x0; a.x_nom = x_nom; a.u_nom = u_nom; a.K = K; a.meas_var = meas_var; a.xhat0 = xhat0; a.cov0 = cov0; a.noise = noise;
  a.meas_noise = meas_noise; a.disturbance = disturbance; a.plant_phys = plant_phys; a.model_phys = model_phys;
  a.x = x; a.u = u; a.xhat = xhat; a.var = var; a.cov = cov; a.nis = nis;
  a.B = B; a.N = N; a.S = S; a.p_y = p_y; a.meas_var_rows = meas_var_rows;
  for (int i = 0; i < QUATTRO_MAX_NX; ++i) a.obs[i] = i < p_y ? observed[i] : 0;
  for (int i = 0; i < 8; ++i) a.plant_phys0[i] = plant.phys[i];
  if (p.model_id == QUATTRO_MODEL_CARTPOLE) return launch_track_estimate<QUATTRO_MODEL_CARTPOLE>(p, plant.integrator, a, stream);
  if (p.model_id == QUATTRO_MODEL_QUADROTOR) return launch_track_estimate<QUATTRO_MODEL_QUADROTOR>(p, plant.integrator, a, stream);
  return QUATTRO_ERR_UNSUPPORTED;
}
