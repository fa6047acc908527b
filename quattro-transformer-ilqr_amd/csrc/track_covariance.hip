// First-order covariance of a tracked closed-loop run (quattro_track_covariance_f32): about the realised x (B, S+1, n), u (B, S, m)
// of quattro_track_f32 under the gains K,
//   Acl_t = A_t + B_t K_t,   Sigma_0 = cov0,   Sigma_{t+1} = Acl_t Sigma_t Acl_t^T + W,   var_u_t = diag(K_t Sigma_t K_t^T)
//   excess = sum_{t<S} [ sum_i q_i Sigma_t[i][i] + 1/2 sum_a l_uu,t[a][a] var_u_t[a] ] + [terminal] sum_i qf_i Sigma_S[i][i]
// (A_t, B_t the plant's step Jacobians at (x_t, u_t); l_uu the luu of qt_control_cost_derivs; the built-in costs have a diagonal
// stage Hessian and l_ux = 0).  K == NULL: Acl_t = A_t and var_u = 0.  The reference has no counterpart.
//
// Mapping.  A trajectory owns 4 NP lanes, NP the padded state dimension: the quadrotor (n = 12, NP = 16) a whole wave, the cart-pole
// (n = 4, NP = 4) a group of 16 lanes, four trajectories a wave.  A block of COV_BLOCK = 4 steps goes through three phases:
//   off the chain  : lane (sub, dir) pushes the direction (e_dir, K_t[:, dir]) through step t_lo + sub (track_item, grad_device.h):
//                    column dir of Acl_t, staged in LDS as the tile row-major, rows and columns n .. NP - 1 staged as zeros
//   on the chain   : the two products of a step.  The quadrotor holds Sigma in the C/D layout of v_mfma_f32_16x16x4_f32 (lane
//                    (g, j), register v: Sigma[4 g + v][j]).  Register v is the k-slice {4 g' + v} of a B operand as it stands and,
//                    Sigma being symmetric, of an A operand too; so U = Sigma Acl^T (A = Sigma, B = Acl^T) and Sigma' = Acl U + W
//                    (A = Acl, B = U, W preloaded as the accumulator) are 4 + 4 MFMAs with ONE staged operand: lane (g, j) reads
//                    Acl[j][4 g .. 4 g + 3], one 16-byte LDS read, which serves both products.  Nothing is transposed and nothing is
//                    masked: the padding is zero because zeros were staged.  The cart-pole's lane (i, j) holds Sigma[i][j] and forms
//                    the products with fmaf over two LDS broadcasts.  Every Sigma_t is parked in LDS, a write nobody waits for
//   after the block: lane (sub, row) reads row `row` of the parked Sigma_{t_lo + sub}: stores it (cov), its diagonal entry (var),
//                    K_t[a][row] (Sigma_t K_t[a]^T)[row] summed over the rows by a butterfly inside the NP lanes (var_u); lane row 0
//                    forms the step's term of `excess` in fp64, and lane 0 adds the block's terms in step order
// Rows as track_gradient_kernel takes them (a private block of VALUES behind wave-uniform branches).  No atomics, no global workspace,
// nothing allocated; a trajectory's results do not depend on B or on its place in the batch; groups past the batch store nothing.
#include "grad_device.h"

namespace {

typedef float cov_f32x4 __attribute__((ext_vector_type(4)));
constexpr int COV_BLOCK = 4;

template <int MODEL, bool RK4>
__global__ __launch_bounds__(QT_WAVE) void track_covariance_kernel(
    const quattro_model_params p, const float* __restrict__ x, const float* __restrict__ u, const int B, const int N, const int S,
    const float* __restrict__ K, const float* __restrict__ plant_phys, const float* __restrict__ cost_rows,
    const float* __restrict__ cov0, const float* __restrict__ noise, const int terminal, float* __restrict__ cov,
    float* __restrict__ var, float* __restrict__ var_u, double* __restrict__ excess) {
  constexpr int NX = ModelDims<MODEL>::NX, NU = ModelDims<MODEL>::NU;
  constexpr bool TILE16 = NX > 4;
  constexpr int NP = TILE16 ? 16 : 4;                          // padded state dimension
  constexpr int LD = TILE16 ? 20 : 4;                          // row stride of a staged tile (20: 16-byte reads of 16 rows, no bank shared)
  constexpr int TILE = NP * LD, LPT = 4 * NP, PER = QT_WAVE / LPT, SLOTS = COV_BLOCK + 1;
  static_assert(NX <= NP && NU <= NP && COV_BLOCK * NP == LPT, "a lane per direction of each step of the block");
  __shared__ __attribute__((aligned(16))) float s_acl[PER * COV_BLOCK * TILE];
  __shared__ __attribute__((aligned(16))) float s_sig[PER * SLOTS * TILE];      // Sigma of the block's steps (and Sigma_S after the last)
  __shared__ __attribute__((aligned(16))) float s_u[TILE16 ? 4 : PER * TILE];   // the cart-pole's U = Sigma Acl^T
  __shared__ double s_e[PER * SLOTS];
  const int lane = threadIdx.x;
  const int grp = lane / LPT, r = lane % LPT;
  const int sub = r / NP, dir = r % NP;                        // on the chain: tile row group (or row) and column
  const long long braw = (long long)blockIdx.x * PER + grp;
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
  if (plant_phys != nullptr) {
    float ph[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) ph[i] = plant_phys[bb * 8 + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) own.phys[i] = ph[i];
  }
  const float* xb = x + bb * (size_t)(S + 1) * NX;             // the realised run: S + 1 states, S controls
  const float* ub = u + bb * (size_t)S * NU;
  const float* Kb = K != nullptr ? K + bb * (size_t)N * NU * NX : nullptr;      // what the run was given: N rows
  float* const acl_g = s_acl + grp * COV_BLOCK * TILE;
  float* const sig_g = s_sig + grp * SLOTS * TILE;

  // rows the tracked steps did not read: +0.0
  if (live && var_u != nullptr) {
    float* z = var_u + (bb * (size_t)N + (size_t)S) * NU;
    for (int i = r; i < (N - S) * NU; i += LPT) z[i] = 0.0f;
  }

  // entry (i, j) of a [B][n][n] input, zero in the padding and for a NULL input
  auto entry = [&](const float* m, int i, int j) __attribute__((always_inline)) {
    return (m != nullptr && i < NX && j < NX) ? m[bb * (size_t)(NX * NX) + (size_t)(i * NX + j)] : 0.0f;
  };
  // the chain's state.  TILE16: sig[v] = Sigma[4 sub + v][dir], wn[v] the same entries of W; else sig[0] = Sigma[sub][dir]
  cov_f32x4 sig = {0.0f, 0.0f, 0.0f, 0.0f}, wn = {0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (TILE16) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      sig[v] = entry(cov0, 4 * sub + v, dir);
      wn[v] = entry(noise, 4 * sub + v, dir);
    }
  } else {
    sig[0] = entry(cov0, sub, dir);
    wn[0] = entry(noise, sub, dir);
  }
  auto park = [&](int slot) __attribute__((always_inline)) {
    float* sp = sig_g + slot * TILE;
    if constexpr (TILE16) {
#pragma unroll
      for (int v = 0; v < 4; ++v) sp[(4 * sub + v) * LD + dir] = sig[v];
    } else {
      sp[sub * LD + dir] = sig[0];
    }
  };

  double acc = 0.0;
  for (int t_lo = 0; t_lo < S; t_lo += COV_BLOCK) {
    const int cnt = S - t_lo < COV_BLOCK ? S - t_lo : COV_BLOCK;           // steps t_lo .. t_lo + cnt - 1, slot s holds step t_lo + s
    const bool last = t_lo + cnt == S;
    // ---- off the chain: the columns of Acl of the block's steps
    {
      const bool mine = sub < cnt;                             // lanes without a step of their own redo step t_lo and store nothing
      const int t = t_lo + (mine ? sub : 0);
      const bool pad = dir >= NX;                              // lanes of the padding redo direction 0 and stage zeros
      const int d = pad ? 0 : dir;
      float xs[NX], us[NU], du[NU], col[NX];
      load_vec<NX>(xb + (size_t)t * NX, xs);
      load_vec<NU>(ub + (size_t)t * NU, us);
      // the lane's control seed: its column of K_t (zero with the feedback off)
#pragma unroll
      for (int a = 0; a < NU; ++a) du[a] = 0.0f;
      if (Kb != nullptr) {
        const float* kc = Kb + (size_t)t * NU * NX + d;
#pragma unroll
        for (int a = 0; a < NU; ++a) du[a] = kc[a * NX];
      }
      track_item<MODEL, RK4>(own, xs, us, d, du, col);
      if (mine) {
        float* st = acl_g + sub * TILE + dir;
#pragma unroll
        for (int i = 0; i < NP; ++i) st[i * LD] = (i < NX && !pad) ? col[i < NX ? i : 0] : 0.0f;
      }
    }
    __syncthreads();
    // ---- on the chain
    if constexpr (TILE16) {
      // lane (g, j) = (sub, dir): Acl[j][4 g .. 4 g + 3], the k-slices of Acl^T as a B operand and of Acl as an A operand
      cov_f32x4 a = *reinterpret_cast<const cov_f32x4*>(acl_g + dir * LD + 4 * sub);
#pragma unroll 1
      for (int s = 0; s < cnt; ++s) {
        cov_f32x4 an = a;
        if (s + 1 < cnt) an = *reinterpret_cast<const cov_f32x4*>(acl_g + (s + 1) * TILE + dir * LD + 4 * sub);
        park(s);
        cov_f32x4 U = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int v = 0; v < 4; ++v) U = __builtin_amdgcn_mfma_f32_16x16x4f32(sig[v], a[v], U, 0, 0, 0);      // U = Sigma Acl^T
        cov_f32x4 sn = wn;
#pragma unroll
        for (int v = 0; v < 4; ++v) sn = __builtin_amdgcn_mfma_f32_16x16x4f32(a[v], U[v], sn, 0, 0, 0);      // Sigma' = Acl U + W
        sig = sn;
        a = an;
      }
    } else {
      // lane (i, j) = (sub, dir): U[i][j] = sum_k Sigma[i][k] Acl[j][k], Sigma'[i][j] = W[i][j] + sum_k Acl[i][k] U[k][j]
      // (one wave per workgroup: its LDS operations complete in program order, cost_gradient_kernel's note)
      float* ug = s_u + grp * TILE;
#pragma unroll 1
      for (int s = 0; s < cnt; ++s) {
        const cov_f32x4 aj = *reinterpret_cast<const cov_f32x4*>(acl_g + s * TILE + dir * LD);
        const cov_f32x4 ai = *reinterpret_cast<const cov_f32x4*>(acl_g + s * TILE + sub * LD);
        park(s);
        __syncthreads();
        const cov_f32x4 row = *reinterpret_cast<const cov_f32x4*>(sig_g + s * TILE + sub * LD);
        float uv = row[0] * aj[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) uv = fmaf(row[k], aj[k], uv);
        ug[sub * LD + dir] = uv;
        __syncthreads();
        float sn = wn[0];
#pragma unroll
        for (int k = 0; k < 4; ++k) sn = fmaf(ai[k], ug[k * LD + dir], sn);
        sig[0] = sn;
      }
    }
    if (last) park(cnt);                                       // Sigma_S: var, cov and the terminal term
    __syncthreads();
    // ---- after the block: the outputs of the parked Sigma_t, lane (sub, row) row `row` of slot s0 + sub
    const int nslots = cnt + (last ? 1 : 0);
    const int row = dir;
#pragma unroll 1
    for (int s0 = 0; s0 < nslots; s0 += COV_BLOCK) {
      const bool mine = s0 + sub < nslots;                     // lanes without a slot redo slot s0 and store nothing
      const int slot = mine ? s0 + sub : s0;
      const int t = t_lo + slot;
      const bool stage = t < S;                                // (t == S: the terminal slot, no control)
      const int tk = stage ? t : S - 1;
      const float* sg = sig_g + slot * TILE;
      float srow[NX], dg[NX], mydiag = 0.0f;
#pragma unroll
      for (int j = 0; j < NX; ++j) {
        srow[j] = sg[row * LD + j];
        dg[j] = sg[j * LD + j];
        mydiag = (j == row) ? dg[j] : mydiag;
      }
      if (live && mine && row < NX) {
        if (cov != nullptr) {
          float* cp = cov + ((bb * (size_t)(S + 1) + (size_t)t) * NX + (size_t)row) * NX;
#pragma unroll
          for (int j = 0; j < NX; ++j) cp[j] = srow[j];
        }
        if (var != nullptr) var[(bb * (size_t)(S + 1) + (size_t)t) * NX + row] = mydiag;
      }
      // var_u[a] = sum_rows K[a][row] (sum_j Sigma[row][j] K[a][j]); the rows of the padding hold zeros
      float pa[NU];
#pragma unroll
      for (int a = 0; a < NU; ++a) pa[a] = 0.0f;
      if (Kb != nullptr) {
        const float* kt = Kb + (size_t)tk * NU * NX;
        const int rk = row < NX ? row : 0;
#pragma unroll
        for (int a = 0; a < NU; ++a) {
          float y = 0.0f;
#pragma unroll
          for (int j = 0; j < NX; ++j) y = fmaf(srow[j], kt[a * NX + j], y);
          pa[a] = (row < NX ? kt[a * NX + rk] : 0.0f) * y;
        }
#pragma unroll
        for (int off = NP / 2; off > 0; off >>= 1) {
#pragma unroll
          for (int a = 0; a < NU; ++a) pa[a] += __shfl_xor(pa[a], off, NP);
        }
      }
      float us[NU];
      load_vec<NU>(ub + (size_t)tk * NU, us);
      double e = 0.0;
      float mine_u = 0.0f;
#pragma unroll
      for (int i = 0; i < NX; ++i) e += (double)(stage ? own.q[i] : (terminal != 0 ? own.qf[i] : 0.0f)) * (double)dg[i];
#pragma unroll
      for (int a = 0; a < NU; ++a) {
        float lu, luu;
        qt_control_cost_derivs(own, own.r[a], us[a], false, &lu, &luu);
        e += stage ? 0.5 * (double)luu * (double)pa[a] : 0.0;
        mine_u = (a == row) ? pa[a] : mine_u;
      }
      if (mine && row == 0) s_e[grp * SLOTS + slot] = e;
      if (live && mine && stage && row < NU && var_u != nullptr) var_u[(bb * (size_t)N + (size_t)t) * NU + row] = mine_u;
    }
    __syncthreads();
    if (r == 0) {
      for (int s = 0; s < nslots; ++s) acc += s_e[grp * SLOTS + s];        // in step order
    }
    __syncthreads();                                           // the stage, the parked Sigma and s_e are rewritten by the next block
  }
  if (live && r == 0 && excess != nullptr) excess[bb] = acc;
}

template <int MODEL>
int launch_track_covariance(const quattro_model_params& p, const float* x, const float* u, int B, int N, int S, const float* K,
                            const float* plant_phys, const float* cost_rows, const float* cov0, const float* noise, int terminal,
                            float* cov, float* var, float* var_u, double* excess, hipStream_t stream) {
  constexpr int PER = ModelDims<MODEL>::NX > 4 ? 1 : 4;
  const dim3 grid((unsigned)((B + PER - 1) / PER)), block(QT_WAVE);
  if (p.integrator == QUATTRO_INTEGRATOR_EULER)
    hipLaunchKernelGGL((track_covariance_kernel<MODEL, false>), grid, block, 0, stream, p, x, u, B, N, S, K, plant_phys, cost_rows,
                       cov0, noise, terminal, cov, var, var_u, excess);
  else if (p.integrator == QUATTRO_INTEGRATOR_RK4)
    hipLaunchKernelGGL((track_covariance_kernel<MODEL, true>), grid, block, 0, stream, p, x, u, B, N, S, K, plant_phys, cost_rows,
                       cov0, noise, terminal, cov, var, var_u, excess);
  else
    return QUATTRO_ERR_UNSUPPORTED;
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

}  // namespace

int quattro_launch_track_covariance(const quattro_model_params& p, const float* x, const float* u, int B, int N, int S,
                                    const float* K, const float* plant_phys, const float* cost_rows, const float* cov0,
                                    const float* noise, int terminal, float* cov, float* var, float* var_u, double* excess,
                                    hipStream_t stream) {
  if (p.model_id == QUATTRO_MODEL_CARTPOLE)
    return launch_track_covariance<QUATTRO_MODEL_CARTPOLE>(p, x, u, B, N, S, K, plant_phys, cost_rows, cov0, noise, terminal, cov,
                                                           var, var_u, excess, stream);
  if (p.model_id == QUATTRO_MODEL_QUADROTOR)
    return launch_track_covariance<QUATTRO_MODEL_QUADROTOR>(p, x, u, B, N, S, K, plant_phys, cost_rows, cov0, noise, terminal, cov,
                                                            var, var_u, excess, stream);
  return QUATTRO_ERR_UNSUPPORTED;
}
