// The extended Kalman filter and the fixed-interval smoother over a LOGGED run (quattro_estimate_log_f32): the sensor readings y
// (S + 1 rows, a NaN = no reading) and the applied controls u (S rows) are inputs; nothing here steps a plant or forms a control.
// Per trajectory, obs the p_y observed state indices (ascending, distinct):
//   filter    xh = xhat0, P = cov0 (NULL: 0);  for t = 0 .. S:
//               update   for i in order, j = obs_i, only where y_t[i] is a number:  g = P[:, j],  s = P[j][j] + R_i,  e = y_t[i] - xh[j],
//                        nis_t += e^2 / s,  xh += g e / s,  P -= g g^T / s             (track_estimate.hip's statements, bit for bit)
//               record   xhat[t], cov[t], var[t]: the posterior of step t
//               predict  (t < S)  A_t = df/dx at (xh, u_t),  xh <- f(xh, u_t),  P <- A_t P A_t^T + W
//   loglik    -1/2 sum_t sum_i (ln(2 pi s) + e^2 / s) over the readings that exist, in fp64, in step order and then sensor order
//   smoother  modified Bryson-Frazier, posterior form; r (n) and Lambda (n x n) zero after the last step;  for t = S .. 0:
//               xs[t] = xhat[t] + cov[t] r,   cov_s[t] = cov[t] - cov[t] Lambda cov[t]
//               for i in REVERSE order, the readings that exist, k = g / s of that update:  q = Lambda k,  c = k^T q,
//                        rj = r[j] + e / s - k^T r,  Lambda[j][:] -= q^T,  Lambda[:, j] -= q,  Lambda[j][j] += c + 1 / s,  r[j] = rj
//               (t > 0)  r <- A_{t-1}^T r,  Lambda <- A_{t-1}^T Lambda A_{t-1}
// The reference has no counterpart.
//
// Mapping: track_estimate.hip's.  A trajectory owns 4 NP lanes: the quadrotor a wave with the matrix (P forward, Lambda backward) in the
// C/D layout of v_mfma_f32_16x16x4_f32 (lane (g, c), register v: M[4 g + v][c], the padding held at zero), the cart-pole a group of 16
// lanes with lane (i, c) holding M[i][c], four trajectories a wave.
//   forward   track_estimate_kernel without the plant lane, the gain law and the noise inputs: u_t and y_t are fetched one step ahead,
//             one float a lane.  A missing reading selects the OLD value of nis, xh and every register of P (v_cndmask, no branch:
//             cart-pole groups of one wave differ in what is missing), so the update is an exact no-op whatever P holds.  (Selecting
//             e = 0 and 1 / s = 0 instead would also keep the bits of a finite P and xh except a -0.0, which x + 0.0 turns into +0.0,
//             but 0 x inf = NaN would spread from a non-finite P.)  Per update the smoother's record -- k (NP floats), e / s, 1 / s,
//             all zero for a missing reading -- goes to the workspace, and so does the posterior where xhat / cov are not outputs.
//   loglik    off the chain: after the last step the same wave reads the stored e and s back (one release / acquire fence), one fp64
//             log per reading and lane, LPT readings a pass through LDS, lane 0 of the group adding them in order.  No atomics.
//   backward  A_{t-1} is not on the chain: the linearisation points (xhat[t], u_t) are all known, so blocks of four steps are
//             recomputed with every lane busy (lane (sub, dir): column dir of A of the block's step sub, track_item on the forward
//             pass's inputs: the forward pass's bits) and staged TRANSPOSED, column c of A contiguous: the lane's 16-byte read
//             A[4 g .. 4 g + 3][c] is then the k-slice of A as a B operand (U = Lambda A) and of A^T as an A operand
//             (Lambda' = A^T U): 4 + 4 MFMAs on one 16-byte LDS read a lane and step, and it serves r <- A^T r as well.
//             q = Lambda k: each lane sums its 4 rows (Lambda read as symmetric), the row groups are added by two ds_bpermute
//             butterflies (__shfl_xor over NP and 2 NP lanes); q, and r, also live in LDS for the lanes that need them by row.
//             The outputs cov[t] Lambda cov[t] (4 + 4 more MFMAs) and cov[t] r hang off the chain: nothing later reads them.  The
//             records and cov[t] are loaded one update / one step ahead.
// Rows (model_phys, meas_var) enter as VALUES behind wave-uniform branches.  No atomics, nothing allocated; a trajectory's results do
// not depend on B or on its place in the batch; groups past the batch store nothing.
// One wave per workgroup: its LDS operations complete in program order; __syncthreads() is the compiler's fence and one s_barrier.
#include "grad_device.h"

namespace {

typedef float log_f32x4 __attribute__((ext_vector_type(4)));
constexpr int LOG_BLOCK = 4;                                   // steps whose A the backward pass stages at a time

struct LogArgs {
  const float *y, *u, *meas_var, *xhat0, *cov0, *noise, *model_phys;
  float *xhat, *var, *cov, *innov, *innov_var, *nis;
  double* loglik;
  float *rec;                                                  // workspace: the smoother's records (NULL: not kept)
  float *led_e, *led_s;                                        // e and s of every reading: innov / innov_var, or the workspace
  float *post_x, *post_p;                                      // the posterior the backward pass reads: xhat / cov, or the workspace
  float *xs, *var_s, *cov_s;
  int B, S, p_y, y_rows, u_rows, meas_var_rows;
  int obs[QUATTRO_MAX_NX];
};

template <int MODEL>
struct LogDims {
  static constexpr int NX = ModelDims<MODEL>::NX, NU = ModelDims<MODEL>::NU;
  static constexpr bool TILE16 = NX > 4;
  static constexpr int NP = TILE16 ? 16 : 4;                   // padded state dimension
  static constexpr int LD = TILE16 ? 20 : 4;                   // row stride of a staged tile (track_covariance.hip)
  static constexpr int TILE = NP * LD, LPT = 4 * NP, PER = QT_WAVE / LPT;
  static constexpr int RV = TILE16 ? 4 : 1;                    // rows of the matrix a lane holds
  static constexpr int REC = NP + 4;                           // a record: k[NP], e / s, 1 / s, two floats of padding
};

template <int MODEL, bool RK4>
__global__ __launch_bounds__(QT_WAVE) void estimate_log_forward_kernel(const quattro_model_params p, const LogArgs a) {
  using D = LogDims<MODEL>;
  constexpr int NX = D::NX, NU = D::NU, NP = D::NP, LD = D::LD, TILE = D::TILE, LPT = D::LPT, PER = D::PER, RV = D::RV, REC = D::REC;
  constexpr bool TILE16 = D::TILE16;
  constexpr int VXH = 0, VU = NP, VEC = NP + 4;                // the group's vectors in LDS
  static_assert(NX + 1 <= LPT && NU <= 4 && NP + 2 <= LPT && NX % 4 == 0, "a lane per direction, the step and the record's scalars");
  __shared__ __attribute__((aligned(16))) float s_a[PER * TILE];                 // A, row-major, the padding zero
  __shared__ __attribute__((aligned(16))) float s_v[PER * VEC];
  __shared__ __attribute__((aligned(16))) float s_p[TILE16 ? 4 : PER * TILE];    // the cart-pole's P and U = P A^T
  __shared__ __attribute__((aligned(16))) float s_u[TILE16 ? 4 : PER * TILE];
  __shared__ double s_ll[QT_WAVE];
  const int lane = threadIdx.x;
  const int grp = lane / LPT, r = lane % LPT;
  const int sub = r / NP, dir = r % NP;                        // tile row group (or row) and column
  const long long braw = (long long)blockIdx.x * PER + grp;
  const bool live = braw < a.B;                                // groups past the batch recompute trajectory B - 1 and store nothing
  const size_t bb = live ? (size_t)braw : (size_t)(a.B - 1);
  const int S = a.S, p_y = a.p_y;
  const bool col_lane = sub == 0 && dir < NX;

  quattro_model_params pm = p;
  if (a.model_phys != nullptr) {
    float ph[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) ph[i] = a.model_phys[bb * 8 + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) pm.phys[i] = ph[i];
  }
  float* const ag = s_a + grp * TILE;
  float* const vg = s_v + grp * VEC;
  for (int i = r; i < TILE; i += LPT) ag[i] = 0.0f;            // the padding of A: staged once, never written again

  const size_t rows = bb * (size_t)(S + 1);
  auto entry = [&](const float* m, int i, int j) __attribute__((always_inline)) {
    return (m != nullptr && i < NX && j < NX) ? m[bb * (size_t)(NX * NX) + (size_t)(i * NX + j)] : 0.0f;
  };
  log_f32x4 P = {0.0f, 0.0f, 0.0f, 0.0f}, wn = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int v = 0; v < RV; ++v) {
    P[v] = entry(a.cov0, RV * sub + v, dir);
    wn[v] = entry(a.noise, RV * sub + v, dir);
  }
  auto store_P = [&](int t) __attribute__((always_inline)) {
    if (!live || dir >= NX) return;
    const size_t row = rows + (size_t)t;
#pragma unroll
    for (int v = 0; v < RV; ++v) {
      const int i = RV * sub + v;
      if (i < NX) {
        if (a.post_p != nullptr) a.post_p[(row * NX + (size_t)i) * NX + dir] = P[v];
        if (a.var != nullptr && i == dir) a.var[row * NX + dir] = P[v];
      }
    }
  };

  const int dc = dir < NX ? dir : 0;
  float xhl = dir < NX ? a.xhat0[bb * NX + dc] : 0.0f;         // xh[dir]
  const int oi = r < p_y ? r : 0;
  const float rreg = a.meas_var[(a.meas_var_rows != 0 ? bb * (size_t)p_y : (size_t)0) + oi];
  const float* yb = a.y + (a.y_rows != 0 ? rows * (size_t)p_y : (size_t)0);
  const float* ub = a.u + (a.u_rows != 0 ? bb * (size_t)S * NU : (size_t)0);
  float yreg, ureg;
  auto fetch = [&](int t) __attribute__((always_inline)) {     // a lane's share of step t: y_t[i] and u_t[a] (row S: the last control again)
    yreg = yb[(size_t)t * p_y + oi];
    ureg = ub[(size_t)(t < S ? t : S - 1) * NU + (r < NU ? r : 0)];
  };
  fetch(0);
  const float qnan = __builtin_nanf("");

#pragma unroll 1
  for (int t = 0; t <= S; ++t) {
    // ---- update, one observed state after the other
    float nis = 0.0f;
#pragma unroll 1
    for (int i = 0; i < p_y; ++i) {
      const int j = a.obs[i];
      const float Ri = __shfl(rreg, i, LPT);
      const float y = __shfl(yreg, i, LPT);
      const float xhj = __shfl(xhl, j, LPT);
      float grow, pjj;
      log_f32x4 gcol = {0.0f, 0.0f, 0.0f, 0.0f};
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
      const bool ok = y == y;                                  // a NaN: no reading
      const float s = pjj + Ri;
      const float inv = 1.0f / s;
      const float e = y - xhj;
      const float w = e * inv;
      nis = ok ? nis + e * w : nis;
      xhl = ok ? xhl + grow * w : xhl;
      const float h = grow * inv;
#pragma unroll
      for (int v = 0; v < RV; ++v) P[v] = ok ? P[v] - gcol[v] * h : P[v];
      if (live) {
        const size_t at = (rows + (size_t)t) * p_y + (size_t)i;
        if (r == i && a.led_e != nullptr) {
          a.led_e[at] = ok ? e : qnan;
          a.led_s[at] = ok ? s : qnan;
        }
        if (a.rec != nullptr) {
          float* rc = a.rec + at * REC;
          if (sub == 0) rc[dir] = ok ? h : 0.0f;               // k[dir] = P[j][dir] / s (zero in the padding)
          if (r == NP) rc[NP] = ok ? w : 0.0f;
          if (r == NP + 1) rc[NP + 1] = ok ? inv : 0.0f;
        }
      }
    }
    // ---- the posterior of row t
    if (live) {
      if (col_lane && a.post_x != nullptr) a.post_x[(rows + (size_t)t) * NX + dir] = xhl;
      if (r == 0 && a.nis != nullptr) a.nis[rows + (size_t)t] = nis;
    }
    store_P(t);
    if (t == S) break;
    if (sub == 0) vg[VXH + dir] = xhl;
    if (r < NU) vg[VU + r] = ureg;
    __syncthreads();
    fetch(t + 1);
    float xh[NX], us[NU];
    load_vec<NX>(vg + VXH, xh);
#pragma unroll
    for (int c = 0; c < NU; ++c) us[c] = vg[VU + c];
    // ---- column dir of A at (xh, u_t); the base step
    if (r < NX) {
      float du[NU], col[NX];
#pragma unroll
      for (int c = 0; c < NU; ++c) du[c] = 0.0f;
      track_item<MODEL, RK4>(pm, xh, us, dir, du, col);
#pragma unroll
      for (int i = 0; i < NX; ++i) ag[i * LD + dir] = col[i];
    }
    if (r == NX) {
      float xnext[NX];
      qt_step<MODEL, RK4>(pm, xh, us, xnext);
      store_vec<NX>(vg + VXH, xnext);
    }
    __syncthreads();
    // ---- predict: P <- A P A^T + W (track_estimate.hip's products)
    if constexpr (TILE16) {
      const log_f32x4 av = *reinterpret_cast<const log_f32x4*>(ag + dir * LD + 4 * sub);
      log_f32x4 U = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int v = 0; v < 4; ++v) U = __builtin_amdgcn_mfma_f32_16x16x4f32(P[v], av[v], U, 0, 0, 0);       // U = P A^T
      log_f32x4 pn = wn;
#pragma unroll
      for (int v = 0; v < 4; ++v) pn = __builtin_amdgcn_mfma_f32_16x16x4f32(av[v], U[v], pn, 0, 0, 0);     // P' = A U + W
      P = pn;
    } else {
      float* pg = s_p + grp * TILE;
      float* ug = s_u + grp * TILE;
      const log_f32x4 ac = *reinterpret_cast<const log_f32x4*>(ag + dir * LD);
      const log_f32x4 ai = *reinterpret_cast<const log_f32x4*>(ag + sub * LD);
      pg[sub * LD + dir] = P[0];
      __syncthreads();
      const log_f32x4 row = *reinterpret_cast<const log_f32x4*>(pg + sub * LD);
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
    xhl = dir < NX ? vg[VXH + dc] : 0.0f;
  }

  // ---- loglik: the readings' e and s read back, LPT of them a pass, added in order by lane 0 of the group
  if (a.loglik != nullptr) {
    __threadfence();
    __syncthreads();
    const int total = (S + 1) * p_y;
    const float* eb = a.led_e + rows * (size_t)p_y;
    const float* sb = a.led_s + rows * (size_t)p_y;
    double acc = 0.0;
#pragma unroll 1
    for (int base = 0; base < total; base += LPT) {
      const int idx = base + r;
      double term = 0.0;
      if (idx < total) {
        const double e = (double)eb[idx], s = (double)sb[idx];
        if (s == s) term = log(6.283185307179586 * s) + e * e / s;
      }
      s_ll[lane] = term;
      __syncthreads();
      if (r == 0) {
        const int cnt = total - base < LPT ? total - base : LPT;
        for (int k = 0; k < cnt; ++k) acc += s_ll[grp * LPT + k];
      }
      __syncthreads();
    }
    if (live && r == 0) a.loglik[bb] = 0.0 - 0.5 * acc;
  }
}

template <int MODEL, bool RK4>
__global__ __launch_bounds__(QT_WAVE) void estimate_log_backward_kernel(const quattro_model_params p, const LogArgs a) {
  using D = LogDims<MODEL>;
  constexpr int NX = D::NX, NU = D::NU, NP = D::NP, LD = D::LD, TILE = D::TILE, LPT = D::LPT, PER = D::PER, RV = D::RV, REC = D::REC;
  constexpr bool TILE16 = D::TILE16;
  static_assert(LOG_BLOCK * NP == LPT, "a lane per direction of each step of the block");
  __shared__ __attribute__((aligned(16))) float s_at[PER * LOG_BLOCK * TILE];    // A^T of the block's steps: [c][i] = A[i][c], padding zero
  __shared__ __attribute__((aligned(16))) float s_r[PER * NP];
  __shared__ __attribute__((aligned(16))) float s_q[PER * NP];
  __shared__ __attribute__((aligned(16))) float s_l[TILE16 ? 4 : PER * TILE];    // the cart-pole's operands
  __shared__ __attribute__((aligned(16))) float s_c[TILE16 ? 4 : PER * TILE];
  __shared__ __attribute__((aligned(16))) float s_m[TILE16 ? 4 : PER * TILE];
  const int lane = threadIdx.x;
  const int grp = lane / LPT, r = lane % LPT;
  const int sub = r / NP, dir = r % NP;
  const long long braw = (long long)blockIdx.x * PER + grp;
  const bool live = braw < a.B;
  const size_t bb = live ? (size_t)braw : (size_t)(a.B - 1);
  const int S = a.S, p_y = a.p_y;

  quattro_model_params pm = p;
  if (a.model_phys != nullptr) {
    float ph[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) ph[i] = a.model_phys[bb * 8 + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) pm.phys[i] = ph[i];
  }
  float* const atg = s_at + grp * LOG_BLOCK * TILE;
  float* const rg = s_r + grp * NP;
  float* const qg = s_q + grp * NP;
  for (int i = r; i < LOG_BLOCK * TILE; i += LPT) atg[i] = 0.0f;
  if (r < NP) rg[r] = 0.0f;
  __syncthreads();

  const size_t rows = bb * (size_t)(S + 1);
  const float* ub = a.u + (a.u_rows != 0 ? bb * (size_t)S * NU : (size_t)0);
  const float* recb = a.rec + rows * (size_t)p_y * REC;
  const int dc = dir < NX ? dir : 0;
  // a lane's entries of cov[t], zero in the padding
  auto load_cov = [&](int t) __attribute__((always_inline)) {
    log_f32x4 c = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int v = 0; v < RV; ++v) {
      const int i = RV * sub + v;
      if (i < NX && dir < NX) c[v] = a.post_p[((rows + (size_t)t) * NX + (size_t)i) * NX + dir];
    }
    return c;
  };
  // a vector of the group in LDS by the lane's rows
  auto by_row = [&](const float* vec) __attribute__((always_inline)) {
    log_f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (TILE16) o = *reinterpret_cast<const log_f32x4*>(vec + 4 * sub);
    else o[0] = vec[sub];
    return o;
  };
  // sum_v m[v] x[v] over the lane's rows, then over the row groups: every lane of column dir gets sum_i M[i][dir] x[i]
  auto col_dot = [&](const log_f32x4 m, const log_f32x4 x) __attribute__((always_inline)) {
    float s = m[0] * x[0];
#pragma unroll
    for (int v = 1; v < RV; ++v) s = fmaf(m[v], x[v], s);
    s += __shfl_xor(s, NP, QT_WAVE);
    s += __shfl_xor(s, 2 * NP, QT_WAVE);
    return s;
  };
  // the record of update f = t p_y + i
  log_f32x4 k4n;
  float wnx, invn;
  auto fetch_rec = [&](int f) __attribute__((always_inline)) {
    const float* rc = recb + (size_t)(f > 0 ? f : 0) * REC;
    if constexpr (TILE16) k4n = *reinterpret_cast<const log_f32x4*>(rc + 4 * sub);
    else k4n = log_f32x4{rc[sub], 0.0f, 0.0f, 0.0f};
    wnx = rc[NP];
    invn = rc[NP + 1];
  };

  log_f32x4 L = {0.0f, 0.0f, 0.0f, 0.0f};                      // Lambda
  int f = (S + 1) * p_y - 1;
  fetch_rec(f);
  log_f32x4 Cn = load_cov(S);
  float xhn = a.post_x[(rows + (size_t)S) * NX + dc];

#pragma unroll 1
  for (int t = S; t >= 0; --t) {
    const log_f32x4 C = Cn;
    const float xht = xhn;
    if (t > 0) {
      Cn = load_cov(t - 1);
      xhn = a.post_x[(rows + (size_t)(t - 1)) * NX + dc];
    }
    // ---- the outputs of row t (nothing later reads them)
    {
      const float cr = col_dot(C, by_row(rg));                 // (cov[t] r)[dir], cov read as symmetric
      if (live && sub == 0 && dir < NX && a.xs != nullptr) a.xs[(rows + (size_t)t) * NX + dir] = xht + cr;
    }
    if (a.cov_s != nullptr || a.var_s != nullptr) {
      log_f32x4 T = {0.0f, 0.0f, 0.0f, 0.0f};
      if constexpr (TILE16) {
        log_f32x4 M = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int v = 0; v < 4; ++v) M = __builtin_amdgcn_mfma_f32_16x16x4f32(L[v], C[v], M, 0, 0, 0);      // M = Lambda cov
#pragma unroll
        for (int v = 0; v < 4; ++v) T = __builtin_amdgcn_mfma_f32_16x16x4f32(C[v], M[v], T, 0, 0, 0);      // T = cov M
      } else {
        float* lg = s_l + grp * TILE;
        float* cg = s_c + grp * TILE;
        float* mg = s_m + grp * TILE;
        lg[sub * LD + dir] = L[0];
        cg[sub * LD + dir] = C[0];
        __syncthreads();
        const log_f32x4 lrow = *reinterpret_cast<const log_f32x4*>(lg + sub * LD);
        const log_f32x4 crow = *reinterpret_cast<const log_f32x4*>(cg + sub * LD);
        float mv = lrow[0] * cg[dir];
#pragma unroll
        for (int k = 1; k < 4; ++k) mv = fmaf(lrow[k], cg[k * LD + dir], mv);
        mg[sub * LD + dir] = mv;
        __syncthreads();
        float tv = crow[0] * mg[dir];
#pragma unroll
        for (int k = 1; k < 4; ++k) tv = fmaf(crow[k], mg[k * LD + dir], tv);
        T[0] = tv;
      }
      if (live && dir < NX) {
        const size_t row = rows + (size_t)t;
#pragma unroll
        for (int v = 0; v < RV; ++v) {
          const int i = RV * sub + v;
          const float o = C[v] - T[v];
          if (i < NX) {
            if (a.cov_s != nullptr) a.cov_s[(row * NX + (size_t)i) * NX + dir] = o;
            if (a.var_s != nullptr && i == dir) a.var_s[row * NX + dir] = o;
          }
        }
      }
    }
    // ---- the updates of row t, last first
#pragma unroll 1
    for (int i = p_y - 1; i >= 0; --i) {
      const int j = a.obs[i];
      const log_f32x4 k4 = k4n;
      const float w = wnx, inv = invn;
      --f;
      fetch_rec(f);
      const bool ok = inv != 0.0f;                             // a missing reading's record is all zeros
      const float qd = col_dot(L, k4);                         // q[dir] = sum_i Lambda[i][dir] k[i]
      if (sub == 0) qg[dir] = qd;
      __syncthreads();
      const log_f32x4 q4 = by_row(qg), r4 = by_row(rg);
      const float rj_old = rg[j];
      const log_f32x4 ones = {1.0f, 1.0f, 1.0f, 1.0f};
      // c = k^T q and k^T r: the lane's rows, then the row groups (the column sum of a matrix whose every column is the same)
      log_f32x4 kq, kr4;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        kq[v] = k4[v] * q4[v];
        kr4[v] = k4[v] * r4[v];
      }
      const float c = col_dot(kq, ones);
      const float kr = col_dot(kr4, ones);
      const float rj = (rj_old + w) - kr;
      const float dd = c + inv;
#pragma unroll
      for (int v = 0; v < RV; ++v) {
        const int row = RV * sub + v;
        float nl = L[v];
        nl = row == j ? nl - qd : nl;
        nl = dir == j ? nl - q4[v] : nl;
        nl = (row == j && dir == j) ? nl + dd : nl;
        L[v] = ok ? nl : L[v];
      }
      __syncthreads();
      if (ok && sub == 0 && dir == j) rg[j] = rj;
      __syncthreads();
    }
    if (t == 0) break;
    // ---- A_{t-1}: a block of steps at a time, off the chain
    const int ai = t - 1;
    const int slot = (S - 1 - ai) % LOG_BLOCK;
    if (slot == 0) {
      const int step = ai - sub;
      const bool mine = step >= 0 && dir < NX;                 // lanes without a step or a direction redo one and store nothing
      const int st = step >= 0 ? step : 0;
      float xl[NX], us[NU], du[NU], col[NX];
      load_vec<NX>(a.post_x + (rows + (size_t)st) * NX, xl);
      load_vec<NU>(ub + (size_t)st * NU, us);
#pragma unroll
      for (int c = 0; c < NU; ++c) du[c] = 0.0f;
      track_item<MODEL, RK4>(pm, xl, us, dc, du, col);
      if (mine) store_vec<NX>(atg + sub * TILE + dir * LD, col);
      __syncthreads();
    }
    const float* at = atg + slot * TILE;
    const log_f32x4 av = by_row(at + dir * LD);                // A[rows of the lane][dir]
    // ---- r <- A^T r
    {
      const float rn = col_dot(av, by_row(rg));
      __syncthreads();
      if (sub == 0) rg[dir] = rn;
      __syncthreads();
    }
    // ---- Lambda <- A^T Lambda A
    if constexpr (TILE16) {
      log_f32x4 U = {0.0f, 0.0f, 0.0f, 0.0f}, Ln = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int v = 0; v < 4; ++v) U = __builtin_amdgcn_mfma_f32_16x16x4f32(L[v], av[v], U, 0, 0, 0);       // U = Lambda A
#pragma unroll
      for (int v = 0; v < 4; ++v) Ln = __builtin_amdgcn_mfma_f32_16x16x4f32(av[v], U[v], Ln, 0, 0, 0);     // Lambda' = A^T U
      L = Ln;
    } else {
      float* lg = s_l + grp * TILE;
      float* mg = s_m + grp * TILE;
      lg[sub * LD + dir] = L[0];
      __syncthreads();
      const log_f32x4 lrow = *reinterpret_cast<const log_f32x4*>(lg + sub * LD);
      const log_f32x4 acol = *reinterpret_cast<const log_f32x4*>(at + dir * LD);          // A[:, dir]
      const log_f32x4 arow = *reinterpret_cast<const log_f32x4*>(at + sub * LD);          // A[:, sub]
      float uv = lrow[0] * acol[0];
#pragma unroll
      for (int k = 1; k < 4; ++k) uv = fmaf(lrow[k], acol[k], uv);
      mg[sub * LD + dir] = uv;                                                             // U = Lambda A
      __syncthreads();
      float ln = arow[0] * mg[dir];
#pragma unroll
      for (int k = 1; k < 4; ++k) ln = fmaf(arow[k], mg[k * LD + dir], ln);
      L[0] = ln;
    }
  }
}

template <int MODEL>
int launch_estimate_log(const quattro_model_params& p, const LogArgs& a, bool smooth, hipStream_t stream) {
  constexpr int PER = LogDims<MODEL>::PER;
  const dim3 grid((unsigned)((a.B + PER - 1) / PER)), block(QT_WAVE);
  const bool rk4 = p.integrator == QUATTRO_INTEGRATOR_RK4;
  if (!rk4 && p.integrator != QUATTRO_INTEGRATOR_EULER) return QUATTRO_ERR_UNSUPPORTED;
  if (rk4) hipLaunchKernelGGL((estimate_log_forward_kernel<MODEL, true>), grid, block, 0, stream, p, a);
  else hipLaunchKernelGGL((estimate_log_forward_kernel<MODEL, false>), grid, block, 0, stream, p, a);
  if (hipGetLastError() != hipSuccess) return QUATTRO_ERR_LAUNCH;
  if (smooth) {
    if (rk4) hipLaunchKernelGGL((estimate_log_backward_kernel<MODEL, true>), grid, block, 0, stream, p, a);
    else hipLaunchKernelGGL((estimate_log_backward_kernel<MODEL, false>), grid, block, 0, stream, p, a);
  }
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

}  // namespace

// observed: HOST array of p_y indices (checked by the caller).  ws: the workspace's four regions (records, e / s ledger, posterior
// xhat, posterior cov), any of them NULL where the caller found it is not needed; everything else as quattro_estimate_log_f32 takes it
int quattro_launch_estimate_log(const quattro_model_params& p, const float* y, int y_rows, const float* u, int u_rows, int B, int S,
                                const int32_t* observed, int p_y, const float* meas_var, int meas_var_rows, const float* xhat0,
                                const float* cov0, const float* noise, const float* model_phys, float* const ws[4], float* xhat,
                                float* var, float* cov, float* innov, float* innov_var, float* nis, double* loglik, float* xs,
                                float* var_s, float* cov_s, hipStream_t stream) {
  const bool smooth = xs != nullptr || var_s != nullptr || cov_s != nullptr;
  LogArgs a;
  a.y = y; a.u = u; a.meas_var = meas_var; a.xhat0 = xhat0; a.cov0 = cov0; a.noise = noise; a.model_phys = model_phys;
  a.xhat = xhat; a.var = var; a.cov = cov; a.innov = innov; a.innov_var = innov_var; a.nis = nis; a.loglik = loglik;
  a.rec = smooth ? ws[0] : nullptr;
  // e and s: where they are returned, else (for loglik, or as the other's companion) the workspace
  a.led_e = innov != nullptr ? innov : ((loglik != nullptr || innov_var != nullptr) ? ws[1] : nullptr);
  a.led_s = innov_var != nullptr ? innov_var : ((loglik != nullptr || innov != nullptr) ? ws[1] + (size_t)B * (S + 1) * p_y : nullptr);
  a.post_x = xhat != nullptr ? xhat : (smooth ? ws[2] : nullptr);
  a.post_p = cov != nullptr ? cov : (smooth ? ws[3] : nullptr);
  a.xs = xs; a.var_s = var_s; a.cov_s = cov_s;
  a.B = B; a.S = S; a.p_y = p_y; a.y_rows = y_rows; a.u_rows = u_rows; a.meas_var_rows = meas_var_rows;
  for (int i = 0; i < QUATTRO_MAX_NX; ++i) a.obs[i] = i < p_y ? observed[i] : 0;
  if (p.model_id == QUATTRO_MODEL_CARTPOLE) return launch_estimate_log<QUATTRO_MODEL_CARTPOLE>(p, a, smooth, stream);
  if (p.model_id == QUATTRO_MODEL_QUADROTOR) return launch_estimate_log<QUATTRO_MODEL_QUADROTOR>(p, a, smooth, stream);
  return QUATTRO_ERR_UNSUPPORTED;
}
