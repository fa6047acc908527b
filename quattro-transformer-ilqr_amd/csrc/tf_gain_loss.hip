// Between the gain predictor's output tokens and the gain stacks of a tracked run, both ways: what a training step on
// the closed-loop cost of the predicted gains needs around quattro_tf_train_step_f32 (forward only), quattro_track_f32,
// quattro_score_f32, quattro_track_gradient_f32 and quattro_tf_train_backward_f32.
//
//   unpack     normalised prediction [B][T][c] -> K [B][N][m][n] and the feed-forward nominal u_ff = u_nom + alpha k [B][N][m]; the rows
//              the predictor does not cover (t >= Tn = min(T, N)) are the logged ones
//   pack_grad  dJ/dK, dJ/du_nom of the tracked cost -> the gradient of the batch loss with respect to the normalised prediction, the
//              loss itself in fp64, and a flag per trajectory that left the finite range (its rows are zero, it is not in the loss)
//
// Token layout: the DATASET's (datagen.create_dataset), element i (1 + n) of a token is k_i and i (1 + n) + 1 + j is K_ij --
// what quattro_tf_gains_* unpack --, NOT the solver's prompt layout [k | K.flat].
//
// Arithmetic: every value is formed by single rounded fp32 operations in a stated order (__fmul_rn / __fadd_rn: nothing contracts to
// an FMA, whatever the flags), the loss by fp64 operations in trajectory order, so that NumPy reproduces every output bit for bit
// (tests/task_loss_cases.py).  Both kernels move a few hundred kB: they are launch-bound, and nothing here is tuned.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/quattro_hip.h"

namespace {

// One thread per output element: the first B N m n threads write K_out, the next B N m write u_ff (consecutive threads, consecutive
// addresses).  Reads of pred_norm are guarded by t < Tn; K_log, k_log, u_nom have the outputs' shapes.
__global__ __launch_bounds__(256) void gains_unpack_kernel(const float* __restrict__ pred, const float* __restrict__ u_mean,
                                                           const float* __restrict__ u_std, const float* __restrict__ K_log,
                                                           const float* __restrict__ k_log, const float* __restrict__ u_nom,
                                                           float alpha, long nK, long nk, int T, int N, int Tn, int n, int m,
                                                           float* __restrict__ K_out, float* __restrict__ u_ff) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int c = m * (1 + n);
  if (idx < nK) {
    const int j = (int)(idx % n);
    const long r = idx / n;                                   // (b N + t) m + i
    const int i = (int)(r % m);
    const long bt = r / m;
    const int t = (int)(bt % N);
    const long b = bt / N;
    float v = K_log[idx];
    if (t < Tn) {
      const int e = i * (1 + n) + 1 + j;
      v = __fadd_rn(__fmul_rn(pred[(b * T + t) * c + e], u_std[e]), u_mean[e]);
    }
    K_out[idx] = v;
  } else if (idx < nK + nk) {
    const long r = idx - nK;                                  // (b N + t) m + i
    const int i = (int)(r % m);
    const long bt = r / m;
    const int t = (int)(bt % N);
    const long b = bt / N;
    float k = k_log[r];
    if (t < Tn) {
      const int e = i * (1 + n);
      k = __fadd_rn(__fmul_rn(pred[(b * T + t) * c + e], u_std[e]), u_mean[e]);
    }
    u_ff[r] = __fadd_rn(u_nom[r], __fmul_rn(alpha, k));
  }
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }      // false for inf and NaN
__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }

// One wave per trajectory (four per workgroup, no barrier: a wave past the batch leaves at once).  The wave first looks at everything
// that decides whether the trajectory is kept -- its cost, its factor, every element of its two gradient blocks -- and votes; only
// then does it write its T c elements of d_pred, lane-strided.  terms[b]: the trajectory's share of the loss (0 when it is left out).
__global__ __launch_bounds__(256) void gains_pack_grad_kernel(const float* __restrict__ grad_K, const float* __restrict__ grad_u,
                                                              const double* __restrict__ cost, const float* __restrict__ scale,
                                                              const float* __restrict__ u_std, float alpha, float task_weight,
                                                              const float* __restrict__ pred, const float* __restrict__ target,
                                                              float mse_weight, int B, int T, int N, int Tn, int n, int m,
                                                              float* __restrict__ d_pred, int32_t* __restrict__ diverged,
                                                              double* __restrict__ terms) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;
  const int c = m * (1 + n);
  const long nK = (long)N * m * n, nk = (long)N * m, np = (long)T * c;
  const float* gK = grad_K + (long)b * nK;
  const float* gu = grad_u + (long)b * nk;
  const double cb = cost[b];
  const double sb = scale != nullptr ? (double)scale[b] : 1.0;
  const double fd = (double)task_weight * sb / (double)B;
  const float f = (float)fd;
  bool ok = finite_d(cb) && finite_f(f);
  for (long q = lane; q < nK; q += 64) ok = ok && finite_f(gK[q]);
  for (long q = lane; q < nk; q += 64) ok = ok && finite_f(gu[q]);
  const bool keep = __all(ok);
  float* dp = d_pred + (long)b * np;
  if (!keep) {
    for (long q = lane; q < np; q += 64) dp[q] = 0.0f;
    if (lane == 0) {
      diverged[b] = 1;
      terms[b] = 0.0;
    }
    return;
  }
  const bool with_mse = mse_weight != 0.0f && pred != nullptr && target != nullptr;
  const float inv = 1.0f / (float)((long)B * np);              // mse_kernel's 1 / n
  double sq = 0.0;
  for (long q = lane; q < np; q += 64) {
    const int t = (int)(q / c), e = (int)(q % c);
    float v = 0.0f;
    if (t < Tn) {
      const int i = e / (1 + n), r = e % (1 + n);
      const float g = r == 0 ? __fmul_rn(gu[(long)t * m + i], alpha) : gK[((long)t * m + i) * n + (r - 1)];
      v = __fmul_rn(__fmul_rn(g, f), u_std[e]);
    }
    if (with_mse) {
      const float err = __fsub_rn(pred[(long)b * np + q], target[(long)b * np + q]);
      v = __fadd_rn(v, __fmul_rn(mse_weight, __fmul_rn(__fmul_rn(2.0f, err), inv)));
      sq += (double)err * (double)err;
    }
    dp[q] = v;
  }
  if (with_mse) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
  }
  if (lane == 0) {
    diverged[b] = 0;
    double term = (double)task_weight * sb * cb / (double)B;
    if (with_mse) term += (double)mse_weight * (sq / (double)((long)B * np));
    terms[b] = term;
  }
}

// loss = terms[0] + terms[1] + ... in that order: one lane, so that the sum is the same on every run and NumPy's sequential sum
// (B is a mini-batch: hundreds of additions)
__global__ void loss_sum_kernel(const double* __restrict__ terms, int B, double* __restrict__ loss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double acc = 0.0;
  for (int b = 0; b < B; ++b) acc += terms[b];
  *loss = acc;
}

bool dims_ok(int B, int T, int N, int n, int m) {
  return B > 0 && T > 0 && N > 0 && n > 0 && m > 0 && (long)B * N * m * (n + 1) < (1L << 40) && (long)B * T * m * (n + 1) < (1L << 40);
}

}  // namespace

extern "C" {

int quattro_tf_gains_unpack_f32(const float* pred_norm, const float* u_mean, const float* u_std, const float* K_log,
                                const float* k_log, const float* u_nom, float alpha, int B, int T, int N, int n, int m,
                                float* K_out, float* u_ff, void* stream) {
  if (!pred_norm || !u_mean || !u_std || !K_log || !k_log || !u_nom || !K_out || !u_ff || !dims_ok(B, T, N, n, m))
    return QUATTRO_ERR_BAD_ARG;
  const long nK = (long)B * N * m * n, nk = (long)B * N * m;
  const long blocks = (nK + nk + 255) / 256;
  if (blocks > 0x7fffffffL) return QUATTRO_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gains_unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pred_norm, u_mean, u_std, K_log,
                     k_log, u_nom, alpha, nK, nk, T, N, T < N ? T : N, n, m, K_out, u_ff);
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

int quattro_tf_gains_pack_grad_f32(const float* grad_K, const float* grad_u_nom, const double* cost, const float* scale,
                                   const float* u_std, float alpha, float task_weight, const float* pred_norm,
                                   const float* target_norm, float mse_weight, int B, int T, int N, int n, int m, float* d_pred,
                                   int32_t* diverged, double* terms, double* loss, void* stream) {
  if (!grad_K || !grad_u_nom || !cost || !u_std || !d_pred || !diverged || !terms || !loss || !dims_ok(B, T, N, n, m))
    return QUATTRO_ERR_BAD_ARG;
  if (mse_weight != 0.0f && (!pred_norm || !target_norm)) return QUATTRO_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gains_pack_grad_kernel, dim3((B + 3) / 4), dim3(256), 0, st, grad_K, grad_u_nom, cost, scale, u_std, alpha,
                     task_weight, pred_norm, target_norm, mse_weight, B, T, N, T < N ? T : N, n, m, d_pred, diverged, terms);
  hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(64), 0, st, terms, B, loss);
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

}  // extern "C"
