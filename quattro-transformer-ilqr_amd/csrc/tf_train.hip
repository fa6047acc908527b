// Training step of the gain predictor on the device, fp32: forward with saved activations, MSE loss,
// backward, Adam — hand-written kernels, no BLAS, no autograd.
//
// Replaces, for one mini-batch, the body of the training loop of TransformerILQR.fit
// (quattro_ilqr_tf/transformer_ilqr.py:150-172: model(x, u_prompt) -> MSELoss -> loss.backward() -> Adam.step()) around
// the architecture of quattro_ilqr_tf/transformer_model.py:85-138 (state / control embeddings, learnable target tokens,
// sinusoidal positions + dropout, post-LayerNorm encoder layers with causal self-attention and a ReLU feed-forward,
// dropout on the attention weights and after each sub-block, linear head on the last T tokens).
//
// Arithmetic: fp32 throughout, like the reference's training (torch default dtype).  Every matrix product of the step —
// the linear layers forward, their input gradients and their weight gradients — is ONE strided kernel built on
// v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulation: gradients agree with fp32 autograd to ~1e-6, so the tests can
// be tight); the weight-gradient products reduce over all B L tokens and are split along that dimension across
// workgroups (fp32 atomic accumulation).  Attention (L ~ 100, head dimension 32) runs one workgroup per (sequence, head)
// out of LDS, on the same fp32 MFMA with transposed tiles whose accumulators feed the next product directly.  This is not the inference hot path (that is tf_stream.hip, bf16): a training step at
// batch 256 is ~0.1 TFLOP and the target here is correctness first, then "not the bottleneck of fit()".
//
// Dropout masks are a counter hash of (seed, site, element index), recomputed wherever they are needed (forward and
// backward see the same mask without storing it); quattro_tf_train_dropout_mask_f32 materialises one for tests.
//
// The step is written as two halves, train_forward and train_backward, with the MSE kernel between them.  quattro_tf_train_backward_f32
// is the backward half on its own, started from a gradient d(scalar)/d(pred) the caller supplies (a task loss: csrc/tf_gain_loss.hip)
// after a forward-only call of the step has filled the workspace.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/quattro_hip.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Drop {
  uint64_t seed;
  float p, inv_keep;   // p = 0: no dropout (evaluation, or a model trained without)
};

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}
// 0 (dropped) or 1 / (1 - p) (kept) for element `idx` of dropout site `site`
__device__ __forceinline__ float keep_scale(const Drop& d, uint32_t site, uint64_t idx) {
  if (d.p <= 0.0f) return 1.0f;
  uint32_t h = mix32((uint32_t)idx + 0x9e3779b9U * (site + 1u));
  h = mix32(h ^ (uint32_t)(idx >> 32) ^ (uint32_t)d.seed);
  h = mix32(h + (uint32_t)(d.seed >> 32));
  const float u = (float)(h >> 8) * (1.0f / 16777216.0f);
  return u >= d.p ? d.inv_keep : 0.0f;
}

// ------------------------------------------------------------------------------------------------ strided GEMM
// C[i][j] (=, +=, atomic +=) sum_r A(i, r) B(r, j) (+ bias[j]),  A(i, r) = A[i sai + r sar],  B(r, j) = B[r sbr + j sbj].
// Workgroup of four waves (2 x 2); a wave owns WTM x WTN 32 x 32 MFMA tiles, so the workgroup tile is 64 WTM x 64 WTN
// (64 x 64 is what runs: see gemm() below); 32 reduction steps per LDS stage; the next stage's global loads are issued before the MFMAs of the
// current one and land in registers meanwhile.  blockIdx.z selects a slice [z kchunk, (z + 1) kchunk) of the reduction
// (weight gradients: mode ATOMIC).  arowsum (may be null): arowsum[i] += sum_r A(i, r) — with A = dY^T that is the bias
// gradient, for free beside dW.
constexpr int BK = 32;
constexpr int MODE_STORE = 0, MODE_ACC = 1, MODE_ATOMIC = 2;

template <int WTM, int WTN>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ A, long sai, long sar,
                                                       const float* __restrict__ B, long sbr, long sbj,
                                                       float* __restrict__ C, long ldc, int M, int N, int K, int kchunk,
                                                       const float* __restrict__ bias, int mode,
                                                       float* __restrict__ arowsum) {
  constexpr int BM = 64 * WTM, BN = 64 * WTN, PA = BM + 4, PB = BN + 4, NLA = BM * BK / 256, NLB = BN * BK / 256;
  __shared__ float As[BK * PA], Bs[BK * PB];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, wm = wv >> 1, wn = wv & 1;
  const int i0 = blockIdx.y * BM, j0 = blockIdx.x * BN;
  const int r_begin = blockIdx.z * kchunk, r_end = min(K, r_begin + kchunk);
  // tile loaders: consecutive threads along whichever index is contiguous in memory; slot p of a thread is element
  // (r, i) = (ar + p adr, ai + p adi) of the A tile (likewise B)
  const bool a_rfast = (sar == 1), b_rfast = (sbr == 1);
  const int ar = a_rfast ? (tid & 31) : (tid / BM), ai = a_rfast ? (tid >> 5) : (tid % BM);
  const int adr = a_rfast ? 0 : 256 / BM, adi = a_rfast ? 8 : 0;
  const int br = b_rfast ? (tid & 31) : (tid / BN), bj = b_rfast ? (tid >> 5) : (tid % BN);
  const int bdr = b_rfast ? 0 : 256 / BN, bdj = b_rfast ? 8 : 0;
  const float* abase = A + (long)(i0 + ai) * sai + (long)ar * sar;
  const float* bbase = B + (long)br * sbr + (long)(j0 + bj) * sbj;
  const long astep = (long)adi * sai + (long)adr * sar, bstep = (long)bdr * sbr + (long)bdj * sbj;
  float ra[NLA], rb[NLB];
  const bool ij_inside = (i0 + BM <= M) && (j0 + BN <= N);   // workgroup-uniform: the tile needs no row / column guards
  auto fetch = [&](int r0) {
    const float* ap = abase + (long)r0 * sar;
    const float* bp = bbase + (long)r0 * sbr;
    if (ij_inside && r0 + BK <= r_end) {                       // interior stage (almost all of them): plain loads
#pragma unroll
      for (int p = 0; p < NLA; ++p) ra[p] = ap[p * astep];
#pragma unroll
      for (int p = 0; p < NLB; ++p) rb[p] = bp[p * bstep];
      return;
    }
#pragma unroll
    for (int p = 0; p < NLA; ++p) {
      const bool ok = (i0 + ai + p * adi < M) && (r0 + ar + p * adr < r_end);
      ra[p] = ok ? ap[p * astep] : 0.0f;
    }
#pragma unroll
    for (int p = 0; p < NLB; ++p) {
      const bool ok = (j0 + bj + p * bdj < N) && (r0 + br + p * bdr < r_end);
      rb[p] = ok ? bp[p * bstep] : 0.0f;
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int p = 0; p < NLA; ++p) As[(ar + p * adr) * PA + ai + p * adi] = ra[p];
#pragma unroll
    for (int p = 0; p < NLB; ++p) Bs[(br + p * bdr) * PB + bj + p * bdj] = rb[p];
  };
  f32x16 acc[WTM][WTN];
#pragma unroll
  for (int tm = 0; tm < WTM; ++tm)
#pragma unroll
    for (int tn = 0; tn < WTN; ++tn)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[tm][tn][e] = 0.0f;
  float rowsum = 0.0f;
  const bool do_rowsum = arowsum != nullptr && blockIdx.x == 0 && tid < BM;
  fetch(r_begin);
  stash();
  __syncthreads();
  for (int r0 = r_begin; r0 < r_end; r0 += BK) {
    const bool more = r0 + BK < r_end;
    if (more) fetch(r0 + BK);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      float a[WTM], b[WTN];
#pragma unroll
      for (int tm = 0; tm < WTM; ++tm) a[tm] = As[(kk + (lane >> 5)) * PA + (wm * WTM + tm) * 32 + (lane & 31)];
#pragma unroll
      for (int tn = 0; tn < WTN; ++tn) b[tn] = Bs[(kk + (lane >> 5)) * PB + (wn * WTN + tn) * 32 + (lane & 31)];
#pragma unroll
      for (int tm = 0; tm < WTM; ++tm)
#pragma unroll
        for (int tn = 0; tn < WTN; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
    }
    if (do_rowsum) {
#pragma unroll
      for (int r = 0; r < BK; ++r) rowsum += As[r * PA + tid];
    }
    __syncthreads();
    if (more) {
      stash();
      __syncthreads();
    }
  }
  if (do_rowsum && i0 + tid < M) atomicAdd(arowsum + i0 + tid, rowsum);
  // C/D layout of a 32 x 32 tile: register e of lane l holds row 8 (e / 4) + 4 (l / 32) + e % 4, column l % 32
#pragma unroll
  for (int tn = 0; tn < WTN; ++tn) {
    const int gj = j0 + (wn * WTN + tn) * 32 + (lane & 31);
    if (gj >= N) continue;
    const float bjv = (bias != nullptr && blockIdx.z == 0) ? bias[gj] : 0.0f;
#pragma unroll
    for (int tm = 0; tm < WTM; ++tm) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int gi = i0 + (wm * WTM + tm) * 32 + 8 * (e >> 2) + 4 * (lane >> 5) + (e & 3);
        if (gi >= M) continue;
        float* c = C + (long)gi * ldc + gj;
        const float v = acc[tm][tn][e] + bjv;
        if (mode == MODE_STORE) *c = v;
        else if (mode == MODE_ACC) *c += v;
        else atomicAdd(c, v);
      }
    }
  }
}

template <int WTM, int WTN>
void gemm_launch(hipStream_t st, const float* A, long sai, long sar, const float* B, long sbr, long sbj, float* C, long ldc,
                 int M, int N, int K, const float* bias, int mode, float* arowsum) {
  constexpr int BM = 64 * WTM, BN = 64 * WTN;
  const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  int splits = 1;
  if (mode == MODE_ATOMIC) {
    splits = 1024 / tiles;
    const int max_splits = (K + 127) / 128;
    if (splits > max_splits) splits = max_splits;
    if (splits < 1) splits = 1;
  }
  int kchunk = (K + splits - 1) / splits;
  kchunk = ((kchunk + BK - 1) / BK) * BK;
  splits = (K + kchunk - 1) / kchunk;
  hipLaunchKernelGGL((gemm_f32_kernel<WTM, WTN>), dim3((N + BN - 1) / BN, (M + BM - 1) / BM, splits), dim3(256), 0, st, A, sai,
                     sar, B, sbr, sbj, C, ldc, M, N, K, kchunk, bias, mode, arowsum);
}

void gemm(hipStream_t st, const float* A, long sai, long sar, const float* B, long sbr, long sbj, float* C, long ldc,
          int M, int N, int K, const float* bias, int mode, float* arowsum = nullptr) {
  // 64 x 64 tiles only.  Measured on one box (scripts/time_train.py, B = 256, whole step): 3.37 ms, with 128 x 64 tiles allowed
  // 3.92, with 128 x 128 allowed 4.23 — the larger tiles need 179 / 237 registers (two waves per SIMD) and this kernel hides its
  // load -> LDS -> MFMA phases by occupancy, not by a deeper pipeline.
  gemm_launch<1, 1>(st, A, sai, sar, B, sbr, sbj, C, ldc, M, N, K, bias, mode, arowsum);
}
// Y[M][N] = X[M][K] W[N][K]^T + b
void linear_fwd(hipStream_t st, const float* X, const float* W, const float* b, float* Y, int M, int N, int K) {
  gemm(st, X, K, 1, W, 1, K, Y, N, M, N, K, b, MODE_STORE);
}
// dX[M][K] (=, +=) dY[M][N] W[N][K]
void linear_bwd_input(hipStream_t st, const float* dY, const float* W, float* dX, int M, int N, int K, bool accumulate) {
  gemm(st, dY, N, 1, W, K, 1, dX, K, M, K, N, nullptr, accumulate ? MODE_ACC : MODE_STORE);
}
// dW[N][K] += dY[M][N]^T X[M][K],  db[N] += column sums of dY   (both zeroed by the caller)
void linear_bwd_weight(hipStream_t st, const float* dY, const float* X, float* dW, float* db, int M, int N, int K) {
  gemm(st, dY, 1, N, X, K, 1, dW, K, N, K, M, nullptr, MODE_ATOMIC, db);
}

// ------------------------------------------------------------------------------------------------ embeddings
// h0[b][t] = drop(token(b, t) + pe[t]): state embedding rows, prompt embedding rows, learnable target rows
// (transformer_model.py:125-132, PositionalEncoding :77-80)
__global__ __launch_bounds__(256) void embed_fwd_kernel(const float* __restrict__ xe, const float* __restrict__ ue,
                                                        const float* __restrict__ tgt, const float* __restrict__ pe,
                                                        float* __restrict__ h0, int Bn, int NS, int P, int T, int d, Drop dr) {
  const int L = NS + P + T;
  const long n = (long)Bn * L * d;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int e = (int)(idx % d);
    const long row = idx / d;
    const int t = (int)(row % L), b = (int)(row / L);
    float v;
    if (t < NS) v = xe[((long)b * NS + t) * d + e];
    else if (t < NS + P) v = ue[((long)b * P + (t - NS)) * d + e];
    else v = tgt[(long)(t - NS - P) * d + e];
    h0[idx] = (v + pe[(long)t * d + e]) * keep_scale(dr, 0u, (uint64_t)idx);
  }
}
__global__ __launch_bounds__(256) void embed_bwd_kernel(const float* __restrict__ dh0, float* __restrict__ dxe,
                                                        float* __restrict__ due, float* __restrict__ dtgt, int Bn, int NS,
                                                        int P, int T, int d, Drop dr) {
  const int L = NS + P + T;
  const long n = (long)Bn * L * d;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int e = (int)(idx % d);
    const long row = idx / d;
    const int t = (int)(row % L), b = (int)(row / L);
    const float g = dh0[idx] * keep_scale(dr, 0u, (uint64_t)idx);
    if (t < NS) dxe[((long)b * NS + t) * d + e] = g;
    else if (t < NS + P) due[((long)b * P + (t - NS)) * d + e] = g;
    else atomicAdd(dtgt + (long)(t - NS - P) * d + e, g);
  }
}

// rows [L - T, L) of every sequence <-> a dense [B T][d] array (the head reads only the target rows)
__global__ __launch_bounds__(256) void tail_gather_kernel(const float* __restrict__ h, float* __restrict__ out, int Bn, int L,
                                                          int T, int d) {
  const long n = (long)Bn * T * d;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int e = (int)(idx % d);
    const long row = idx / d;
    const int t = (int)(row % T), b = (int)(row / T);
    out[idx] = h[((long)b * L + (L - T) + t) * d + e];
  }
}
__global__ __launch_bounds__(256) void tail_scatter_kernel(const float* __restrict__ dout, float* __restrict__ dh, int Bn, int L,
                                                           int T, int d) {
  const long n = (long)Bn * L * d;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const int e = (int)(idx % d);
    const long row = idx / d;
    const int t = (int)(row % L), b = (int)(row / L);
    dh[idx] = t >= L - T ? dout[((long)b * T + (t - (L - T))) * d + e] : 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------ attention on the MFMA pipe
// softmax(Q K^T / sqrt(hd) + causal mask) V with dropout on the attention weights (torch.nn.MultiheadAttention as configured
// at transformer_model.py:104-111), every product on v_mfma_f32_32x32x2_f32 (fp32 operands).  One workgroup per (sequence, head),
// wave w owns the 32 queries of tile w; everything is computed TRANSPOSED (keys x queries), so a lane holds one query's
// column: its keys sit in the 16 accumulator registers of each key tile — softmax statistics are sums over registers plus
// one exchange between the two lane halves, and the probability tile is, as it stands, the B operand of the next product
// (O^T = V^T P^T, dQ^T = K^T dS^T): nothing moves between the products.  The forward keeps only the row statistics
// (max, 1 / sum) for the backward, which recomputes the probabilities (no [L][L] array in memory).
constexpr int HD = 32, HDP = HD + 1;   // largest head dimension (one tile); LDS row pitch
constexpr int LP = 128;   // padded sequence length: four tiles of 32 (rows >= L are zero)
__device__ __forceinline__ int acc_row(int e, int hl) { return 8 * (e >> 2) + 4 * hl + (e & 3); }   // row held by register e
__device__ __forceinline__ float half_max(float v) { return fmaxf(v, __shfl_xor(v, 32)); }
__device__ __forceinline__ float half_sum(float v) { return v + __shfl_xor(v, 32); }
__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ f32x16 zero_acc() {
  f32x16 z;
#pragma unroll
  for (int e = 0; e < 16; ++e) z[e] = 0.0f;
  return z;
}

__global__ __launch_bounds__(256) void attn_fwd_mfma_kernel(const float* __restrict__ qkv, float* __restrict__ stats,
                                                            float* __restrict__ out, int L, int d, int H, int hd, float scale,
                                                            Drop dr, uint32_t site) {
  extern __shared__ float sm[];
  float* Qs = sm;                    // [LP][HDP] each; Q already times 1 / sqrt(hd)
  float* Ks = Qs + LP * HDP;
  float* Vs = Ks + LP * HDP;
  float* Ts = Vs + LP * HDP;         // [4 waves][32][HDP]: a wave's O tile on its way out
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hl = lane >> 5, lc = lane & 31;
  const long row0 = (long)b * L;
  for (int idx = tid; idx < LP * HD; idx += 256) {
    const int j = idx / HD, e = idx % HD;
    float q = 0.0f, k = 0.0f, v = 0.0f;
    if (j < L && e < hd) {                                   // head dimensions below 32: the tile's other columns stay zero
      const float* src = qkv + (row0 + j) * 3 * d + h * hd + e;
      q = src[0] * scale;
      k = src[d];
      v = src[2 * d];
    }
    Qs[j * HDP + e] = q;
    Ks[j * HDP + e] = k;
    Vs[j * HDP + e] = v;
  }
  __syncthreads();
  if (32 * w >= L) return;           // (no barrier below)
  const int nt = w + 1, qi = 32 * w + lc;
  const long pbase = ((long)b * H + h) * L * L;
  f32x16 S[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    S[jt] = zero_acc();
    if (jt < nt) {
#pragma unroll
      for (int kk = 0; kk < HD / 2; ++kk)
        S[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[(32 * jt + lc) * HDP + 2 * kk + hl], Qs[qi * HDP + 2 * kk + hl], S[jt], 0, 0,
                                                     0);
    }
  }
  float mx = -3.0e38f;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = 32 * jt + acc_row(e, hl);
      const float sv = (jt < nt && key <= qi && key < L) ? S[jt][e] : -3.0e38f;
      S[jt][e] = sv;
      mx = fmaxf(mx, sv);
    }
  mx = half_max(mx);
  float sum = 0.0f;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float ex = S[jt][e] > -1.0e38f ? expf(S[jt][e] - mx) : 0.0f;
      S[jt][e] = ex;
      sum += ex;
    }
  sum = half_sum(sum);
  const float inv = 1.0f / sum;
  if (hl == 0 && qi < L) {
    stats[(((long)b * H + h) * L + qi) * 2 + 0] = mx;
    stats[(((long)b * H + h) * L + qi) * 2 + 1] = inv;
  }
  f32x16 O = zero_acc();
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    if (jt < nt) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = 32 * jt + acc_row(e, hl);
        float pd = S[jt][e] * inv;
        if (dr.p > 0.0f && key <= qi && qi < L) pd *= keep_scale(dr, site, (uint64_t)(pbase + (long)qi * L + key));
        O = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[key * HDP + lc], pd, O, 0, 0, 0);
      }
    }
  }
  // O^T[dim = acc_row(e, hl)][query = lc] -> rows of 32 contiguous floats
  float* Tw = Ts + w * 32 * HDP;
#pragma unroll
  for (int e = 0; e < 16; ++e) Tw[lc * HDP + acc_row(e, hl)] = O[e];
  wave_fence();
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int q = 2 * r + hl;
    if (32 * w + q < L && lc < hd) out[(row0 + 32 * w + q) * d + h * hd + lc] = Tw[q * HDP + lc];
  }
}

// Backward of the same: P is recomputed from the saved row statistics, D_i = dO_i . O_i.  Two sweeps over the causal tile
// pairs, neither needs another wave's results: (A) wave w as QUERY tile w, transposed tiles (lane = query), accumulates
// dQ^T over its key tiles; (B) wave w as KEY tile w, untransposed tiles (lane = key), accumulates dK^T and dV^T over the
// query tiles at or after it.  dS and P feed the accumulating products straight from their accumulator registers.
__global__ __launch_bounds__(256) void attn_bwd_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ stats,
                                                            const float* __restrict__ o, const float* __restrict__ dout,
                                                            float* __restrict__ dqkv, int L, int d, int H, int hd, float scale,
                                                            Drop dr, uint32_t site) {
  extern __shared__ float sm[];
  float* Qs = sm;                    // [LP][HDP] each; Q already times 1 / sqrt(hd)
  float* Ks = Qs + LP * HDP;
  float* Vs = Ks + LP * HDP;
  float* Gs = Vs + LP * HDP;         // dO
  float* Ts = Gs + LP * HDP;         // [4 waves][32][HDP] output staging
  float* Ms = Ts + 4 * 32 * HDP;     // [LP] row max, 1 / row sum, D
  float* Is = Ms + LP;
  float* Ds = Is + LP;
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hl = lane >> 5, lc = lane & 31;
  const long row0 = (long)b * L;
  for (int idx = tid; idx < LP * HD; idx += 256) {
    const int j = idx / HD, e = idx % HD;
    float q = 0.0f, k = 0.0f, v = 0.0f, g = 0.0f;
    if (j < L && e < hd) {
      const float* src = qkv + (row0 + j) * 3 * d + h * hd + e;
      q = src[0] * scale;
      k = src[d];
      v = src[2 * d];
      g = dout[(row0 + j) * d + h * hd + e];
    }
    Qs[j * HDP + e] = q;
    Ks[j * HDP + e] = k;
    Vs[j * HDP + e] = v;
    Gs[j * HDP + e] = g;
  }
  if (tid < LP) {
    float mval = 0.0f, ival = 0.0f, dval = 0.0f;
    if (tid < L) {
      mval = stats[(((long)b * H + h) * L + tid) * 2 + 0];
      ival = stats[(((long)b * H + h) * L + tid) * 2 + 1];
      const float* po = o + (row0 + tid) * d + h * hd;
      const float* pg = dout + (row0 + tid) * d + h * hd;
      for (int e = 0; e < hd; ++e) dval = fmaf(pg[e], po[e], dval);
    }
    Ms[tid] = mval;
    Is[tid] = ival;
    Ds[tid] = dval;
  }
  __syncthreads();
  if (32 * w >= L) return;           // (no barrier below)
  const int ntiles = (L + 31) / 32;
  const long pbase = ((long)b * H + h) * L * L;
  float* Tw = Ts + w * 32 * HDP;
  auto flush = [&](const f32x16& acc, int col_off, float mul) __attribute__((always_inline)) {
    // acc[dim = acc_row(e, hl)][row = lc] -> dqkv[(row0 + 32 w + row)][col_off + h HD + dim], rows of 32 contiguous floats
#pragma unroll
    for (int e = 0; e < 16; ++e) Tw[lc * HDP + acc_row(e, hl)] = acc[e] * mul;
    wave_fence();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = 2 * r + hl;
      if (32 * w + q < L && lc < hd) dqkv[(row0 + 32 * w + q) * 3 * d + col_off + h * hd + lc] = Tw[q * HDP + lc];
    }
    wave_fence();
  };
  {  // ---- (A) query tile w: dQ
    const int qi = 32 * w + lc;
    const float mq = Ms[qi], iq = Is[qi], dq_ = Ds[qi];
    f32x16 dQ = zero_acc();
    for (int jt = 0; jt <= w; ++jt) {
      f32x16 S = zero_acc(), dP = zero_acc();
#pragma unroll
      for (int kk = 0; kk < HD / 2; ++kk) {
        S = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[(32 * jt + lc) * HDP + 2 * kk + hl], Qs[qi * HDP + 2 * kk + hl], S, 0, 0, 0);
        dP = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[(32 * jt + lc) * HDP + 2 * kk + hl], Gs[qi * HDP + 2 * kk + hl], dP, 0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = 32 * jt + acc_row(e, hl);
        const bool valid = key <= qi && qi < L;
        const float pv = valid ? expf(S[e] - mq) * iq : 0.0f;
        const float ks = (valid && dr.p > 0.0f) ? keep_scale(dr, site, (uint64_t)(pbase + (long)qi * L + key)) : 1.0f;
        const float ds = pv * (dP[e] * ks - dq_);
        dQ = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[key * HDP + lc], ds, dQ, 0, 0, 0);
      }
    }
    flush(dQ, 0, scale);
  }
  {  // ---- (B) key tile w: dK, dV
    const int kj = 32 * w + lc;
    f32x16 dK = zero_acc(), dV = zero_acc();
    for (int it = w; it < ntiles; ++it) {
      f32x16 S = zero_acc(), dP = zero_acc();
#pragma unroll
      for (int kk = 0; kk < HD / 2; ++kk) {
        S = __builtin_amdgcn_mfma_f32_32x32x2f32(Qs[(32 * it + lc) * HDP + 2 * kk + hl], Ks[kj * HDP + 2 * kk + hl], S, 0, 0, 0);
        dP = __builtin_amdgcn_mfma_f32_32x32x2f32(Gs[(32 * it + lc) * HDP + 2 * kk + hl], Vs[kj * HDP + 2 * kk + hl], dP, 0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int qr = 32 * it + acc_row(e, hl);
        const bool valid = kj <= qr && qr < L;
        const float pv = valid ? expf(S[e] - Ms[qr]) * Is[qr] : 0.0f;
        const float ks = (valid && dr.p > 0.0f) ? keep_scale(dr, site, (uint64_t)(pbase + (long)qr * L + kj)) : 1.0f;
        const float ds = pv * (dP[e] * ks - Ds[qr]);
        dV = __builtin_amdgcn_mfma_f32_32x32x2f32(Gs[qr * HDP + lc], pv * ks, dV, 0, 0, 0);
        dK = __builtin_amdgcn_mfma_f32_32x32x2f32(Qs[qr * HDP + lc], ds, dK, 0, 0, 0);
      }
    }
    flush(dK, d, 1.0f);
    flush(dV, 2 * d, 1.0f);
  }
}

// ------------------------------------------------------------------------------------------------ LayerNorm (+ residual)
// s = a + drop(b);  y = (s - mean) rstd g + beta.   One wave per row; d a multiple of 64, at most 512.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
constexpr int LN_MAXE = 8, LN_BWD_ROWS = 16;   // rows per workgroup of the backward: four per wave, ~6 waves per SIMD at batch 256

__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ a, const float* __restrict__ bsrc,
                                                     float* __restrict__ s_out, float* __restrict__ y,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                     const float* __restrict__ g, const float* __restrict__ beta, int M, int d,
                                                     Drop dr, uint32_t site) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const int E = (d + 63) >> 6;   // elements per lane; the last one is partial when d is not a multiple of 64
  float v[LN_MAXE];
  float sum = 0.0f;
#pragma unroll
  for (int e = 0; e < LN_MAXE; ++e) {
    v[e] = 0.0f;
    if (e < E && lane + 64 * e < d) {
      const long idx = (long)row * d + lane + 64 * e;
      v[e] = a[idx] + bsrc[idx] * keep_scale(dr, site, (uint64_t)idx);
      sum += v[e];
    }
  }
  const float mean = wave_sum(sum) / (float)d;
  float sq = 0.0f;
#pragma unroll
  for (int e = 0; e < LN_MAXE; ++e)
    if (e < E && lane + 64 * e < d) sq = fmaf(v[e] - mean, v[e] - mean, sq);
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)d + 1.0e-5f);
#pragma unroll
  for (int e = 0; e < LN_MAXE; ++e) {
    if (e < E && lane + 64 * e < d) {
      const int c = lane + 64 * e;
      const long idx = (long)row * d + c;
      s_out[idx] = v[e];
      y[idx] = (v[e] - mean) * rstd * g[c] + beta[c];
    }
  }
  if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
}

// ds = rstd (dxh - mean(dxh) - xh mean(dxh xh)), dxh = dy g;  per block of LN_BWD_ROWS rows the partial sums of dy xh and dy go
// to `part` [block][2][d]; ln_bwd_reduce_kernel adds them up (hundreds of blocks adding atomically to the same 2 d
// addresses serialised in L2: 38 us per call instead of ~12)
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ s,
                                                     const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                     const float* __restrict__ g, float* __restrict__ ds,
                                                     float* __restrict__ part, int M, int d) {
  __shared__ float sh[2][4][64 * LN_MAXE];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int E = (d + 63) >> 6;   // elements per lane; the last one is partial when d is not a multiple of 64
  float ag[LN_MAXE], ab[LN_MAXE];
#pragma unroll
  for (int e = 0; e < LN_MAXE; ++e) { ag[e] = 0.0f; ab[e] = 0.0f; }
  constexpr int rows_per_block = LN_BWD_ROWS;
  for (int rr = wv; rr < rows_per_block; rr += 4) {
    const int row = blockIdx.x * rows_per_block + rr;
    if (row >= M) break;
    const float mean = mean_in[row], rstd = rstd_in[row];
    float xh[LN_MAXE], dxh[LN_MAXE];
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int e = 0; e < LN_MAXE; ++e) {
      xh[e] = 0.0f;
      dxh[e] = 0.0f;
      if (e < E && lane + 64 * e < d) {
        const int c = lane + 64 * e;
        const long idx = (long)row * d + c;
        const float gy = dy[idx];
        xh[e] = (s[idx] - mean) * rstd;
        dxh[e] = gy * g[c];
        s1 += dxh[e];
        s2 = fmaf(dxh[e], xh[e], s2);
        ag[e] = fmaf(gy, xh[e], ag[e]);
        ab[e] += gy;
      }
    }
    const float m1 = wave_sum(s1) / (float)d, m2 = wave_sum(s2) / (float)d;
#pragma unroll
    for (int e = 0; e < LN_MAXE; ++e)
      if (e < E && lane + 64 * e < d) ds[(long)row * d + lane + 64 * e] = rstd * (dxh[e] - m1 - xh[e] * m2);
  }
#pragma unroll
  for (int e = 0; e < LN_MAXE; ++e) {
    if (e < E) {
      sh[0][wv][lane + 64 * e] = ag[e];
      sh[1][wv][lane + 64 * e] = ab[e];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < d; c += 256) {
    part[((long)blockIdx.x * 2 + 0) * d + c] = sh[0][0][c] + sh[0][1][c] + sh[0][2][c] + sh[0][3][c];
    part[((long)blockIdx.x * 2 + 1) * d + c] = sh[1][0][c] + sh[1][1][c] + sh[1][2][c] + sh[1][3][c];
  }
}
// dg[c] += sum_blocks part[.][0][c], dbeta[c] += sum_blocks part[.][1][c]: blockIdx.y takes a slice of the blocks
// (64 adders per address instead of one per 16 rows)
constexpr int LN_RED_SLICES = 64;
__global__ __launch_bounds__(256) void ln_bwd_reduce_kernel(const float* __restrict__ part, int nblocks, int d,
                                                            float* __restrict__ dg, float* __restrict__ dbeta) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2 * d) return;
  const int which = idx / d, c = idx % d;
  const int per = (nblocks + LN_RED_SLICES - 1) / LN_RED_SLICES;
  const int b0 = blockIdx.y * per, b1 = min(nblocks, b0 + per);
  float acc = 0.0f;
#pragma unroll 8
  for (int b = b0; b < b1; ++b) acc += part[((long)b * 2 + which) * d + c];
  if (b1 > b0) atomicAdd((which == 0 ? dg : dbeta) + c, acc);
}

// ------------------------------------------------------------------------------------------------ element-wise pieces
// f = drop(relu(a)) in place (transformer_model.py:104-111: activation relu, dropout inside the feed-forward)
__global__ __launch_bounds__(256) void relu_drop_kernel(float* __restrict__ a, long n, Drop dr, uint32_t site) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256)
    a[idx] = fmaxf(a[idx], 0.0f) * keep_scale(dr, site, (uint64_t)idx);
}
// da = df where the unit was kept and positive (f > 0), times 1 / (1 - p)
__global__ __launch_bounds__(256) void relu_drop_bwd_kernel(float* __restrict__ df, const float* __restrict__ f, long n,
                                                            float inv_keep) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256)
    df[idx] = f[idx] > 0.0f ? df[idx] * inv_keep : 0.0f;
}
// dst = src * mask(site)   (gradient through a dropout on a sub-block's output)
__global__ __launch_bounds__(256) void drop_bwd_kernel(float* __restrict__ dst, const float* __restrict__ src, long n, Drop dr,
                                                       uint32_t site) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256)
    dst[idx] = src[idx] * keep_scale(dr, site, (uint64_t)idx);
}
__global__ __launch_bounds__(256) void add_kernel(float* __restrict__ dst, const float* __restrict__ src, long n) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) dst[idx] += src[idx];
}
__global__ __launch_bounds__(256) void mask_kernel(float* __restrict__ out, long n, Drop dr, uint32_t site) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256)
    out[idx] = keep_scale(dr, site, (uint64_t)idx);
}

// loss += mean((pred - y)^2); dpred = 2 (pred - y) / n     (nn.MSELoss, transformer_ilqr.py:139)
__global__ __launch_bounds__(256) void mse_kernel(const float* __restrict__ pred, const float* __restrict__ y, long n,
                                                  float* __restrict__ dpred, float* __restrict__ loss) {
  __shared__ float red[4];
  float acc = 0.0f;
  const float inv = 1.0f / (float)n;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const float e = pred[idx] - y[idx];
    acc = fmaf(e, e, acc);
    if (dpred != nullptr) dpred[idx] = 2.0f * e * inv;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(loss, (red[0] + red[1] + red[2] + red[3]) * inv);
}

// torch.optim.Adam defaults (transformer_ilqr.py:140): no weight decay, bias-corrected moments
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long n, float lr, float b1, float b2, float eps,
                                                   float c1, float c2) {
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long)gridDim.x * 256) {
    const float gi = g[idx];
    const float mi = b1 * m[idx] + (1.0f - b1) * gi;
    const float vi = b2 * v[idx] + (1.0f - b2) * gi * gi;
    m[idx] = mi;
    v[idx] = vi;
    p[idx] -= lr * (mi / c1) / (sqrtf(vi / c2) + eps);
  }
}

inline int ew_blocks(long n) {
  long b = (n + 255) / 256;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

// ------------------------------------------------------------------------------------------------ layout
struct LayerOff {
  long wqkv, bqkv, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2;
};
struct ParamOff {
  long tgt, ws, bs, wc, bc, wout, bout;
  LayerOff layer[QUATTRO_TF_MAX_LAYERS];
  long total;
};
ParamOff param_offsets(const quattro_tf_train_desc& D) {
  ParamOff o;
  long at = 0;
  auto take = [&](long n) { const long r = at; at += (n + 3) / 4 * 4; return r; };   // 16-byte aligned blocks
  const long d = D.d_model, ff = D.d_ff, c = D.control_dim, n = D.state_dim;
  o.tgt = take((long)D.target_len * d);
  o.ws = take(d * n);
  o.bs = take(d);
  o.wc = take(d * c);
  o.bc = take(d);
  o.wout = take(c * d);
  o.bout = take(c);
  for (int l = 0; l < D.n_layers; ++l) {
    LayerOff& q = o.layer[l];
    q.wqkv = take(3 * d * d);
    q.bqkv = take(3 * d);
    q.wo = take(d * d);
    q.bo = take(d);
    q.w1 = take(ff * d);
    q.b1 = take(ff);
    q.w2 = take(d * ff);
    q.b2 = take(d);
    q.g1 = take(d);
    q.be1 = take(d);
    q.g2 = take(d);
    q.be2 = take(d);
  }
  o.total = at;
  return o;
}

// head dimensions the attention kernels take: up to one 32-wide tile (8, 16, 32 in practice)
bool head_dim_ok(int hd) { return hd >= 1 && hd <= HD; }

bool desc_ok(const quattro_tf_train_desc* D) {
  return D && D->state_dim > 0 && D->control_dim > 0 && D->d_model > 0 && D->d_model <= 64 * LN_MAXE &&
         D->nhead > 0 && D->d_model % D->nhead == 0 && head_dim_ok(D->d_model / D->nhead) && D->d_ff > 0 && D->n_layers > 0 &&
         D->n_layers <= QUATTRO_TF_MAX_LAYERS && D->n_state_tok > 0 && D->prompt_len > 0 && D->target_len > 0 &&
         D->n_state_tok + D->prompt_len + D->target_len <= LP && D->dropout >= 0.0f && D->dropout < 1.0f;
}

struct LayerWs {
  float *qkv, *P, *ao, *o, *s1, *mean1, *rstd1, *h1, *f1, *f2, *s2, *mean2, *rstd2, *h2;
};
struct Ws {
  float *xe, *ue, *h0, *tail, *pred, *dpred, *loss_pad;
  LayerWs layer[QUATTRO_TF_MAX_LAYERS];
  float *dh, *dtmp, *dbranch, *dqkv, *df, *dao, *dtail, *dxe, *due, *lnpart;
  size_t total;
};
Ws carve(const quattro_tf_train_desc& D, int Bn, char* base) {
  Ws w;
  size_t at = 0;
  auto take = [&](size_t floats) {
    float* p = base ? reinterpret_cast<float*>(base + at) : nullptr;
    at += (floats * sizeof(float) + 255) / 256 * 256;
    return p;
  };
  const size_t L = D.n_state_tok + D.prompt_len + D.target_len, M = (size_t)Bn * L, d = D.d_model, ff = D.d_ff;
  const size_t Mt = (size_t)Bn * D.target_len;
  w.xe = take((size_t)Bn * D.n_state_tok * d);
  w.ue = take((size_t)Bn * D.prompt_len * d);
  w.h0 = take(M * d);
  w.tail = take(Mt * d);
  w.pred = take(Mt * D.control_dim);
  w.dpred = take(Mt * D.control_dim);
  w.loss_pad = take(64);
  for (int l = 0; l < D.n_layers; ++l) {
    LayerWs& q = w.layer[l];
    q.qkv = take(M * 3 * d);
    q.P = take((size_t)Bn * D.nhead * L * 2);      // row statistics (max, 1 / sum) of the softmax
    q.ao = take(M * d);
    q.o = take(M * d);
    q.s1 = take(M * d);
    q.mean1 = take(M);
    q.rstd1 = take(M);
    q.h1 = take(M * d);
    q.f1 = take(M * ff);
    q.f2 = take(M * d);
    q.s2 = take(M * d);
    q.mean2 = take(M);
    q.rstd2 = take(M);
    q.h2 = take(M * d);
  }
  w.dh = take(M * d);
  w.dtmp = take(M * d);
  w.dbranch = take(M * d);
  w.dqkv = take(M * 3 * d);
  w.df = take(M * ff);
  w.dao = take(M * d);
  w.dtail = take(Mt * d);
  w.dxe = take((size_t)Bn * D.n_state_tok * d);
  w.due = take((size_t)Bn * D.prompt_len * d);
  w.lnpart = take(((M + LN_BWD_ROWS - 1) / LN_BWD_ROWS) * 2 * d);
  w.total = at;
  return w;
}

size_t attn_mfma_fwd_lds() { return (size_t)(3 * LP * HDP + 4 * 32 * HDP) * sizeof(float); }
size_t attn_mfma_bwd_lds() { return (size_t)(4 * LP * HDP + 4 * 32 * HDP + 3 * LP) * sizeof(float); }

// the attention kernels' dynamic LDS exceeds the default limit: raised before the first launch of a call
void raise_attn_lds() {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                      (int)attn_mfma_fwd_lds());
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_bwd_mfma_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                      (int)attn_mfma_bwd_lds());
}

// The two halves of the step.  Both carve the same workspace for (D, batch): the forward half leaves every saved activation there,
// the backward half reads them and the gradient `dpred` [B T][c] of a scalar with respect to the normalised prediction.
void train_forward(const quattro_tf_train_desc& D, const float* params, void* workspace, const float* x_norm,
                   const float* prompt_norm, const float* pe, int batch, uint64_t dropout_seed, int training, float* pred,
                   hipStream_t st) {
  const ParamOff po = param_offsets(D);
  const Ws w = carve(D, batch, reinterpret_cast<char*>(workspace));
  const int Bn = batch, NS = D.n_state_tok, P = D.prompt_len, T = D.target_len, L = NS + P + T, M = Bn * L, Mt = Bn * T;
  const int d = D.d_model, ff = D.d_ff, c = D.control_dim, n = D.state_dim, H = D.nhead;
  const int hd = d / H;
  const float scale = 1.0f / sqrtf((float)hd);
  Drop dr;
  dr.seed = dropout_seed;
  dr.p = (training && D.dropout > 0.0f) ? D.dropout : 0.0f;
  dr.inv_keep = 1.0f / (1.0f - dr.p);
  auto site = [](int layer, int kind) { return (uint32_t)(1 + 4 * layer + kind); };   // 0: positions; per layer: attention
                                                                                       // weights, out-proj, ff hidden, ff out
  // ---------------------------------------------------------------- forward
  linear_fwd(st, x_norm, params + po.ws, params + po.bs, w.xe, Bn * NS, d, n);
  linear_fwd(st, prompt_norm, params + po.wc, params + po.bc, w.ue, Bn * P, d, c);
  hipLaunchKernelGGL(embed_fwd_kernel, dim3(ew_blocks((long)M * d)), dim3(256), 0, st, w.xe, w.ue, params + po.tgt, pe, w.h0, Bn,
                     NS, P, T, d, dr);
  const float* hin = w.h0;
  for (int l = 0; l < D.n_layers; ++l) {
    const LayerOff& q = po.layer[l];
    const LayerWs& a = w.layer[l];
    linear_fwd(st, hin, params + q.wqkv, params + q.bqkv, a.qkv, M, 3 * d, d);
    hipLaunchKernelGGL(attn_fwd_mfma_kernel, dim3(H, Bn), dim3(256), attn_mfma_fwd_lds(), st, a.qkv, a.P, a.ao, L, d, H, hd, scale, dr,
                       site(l, 0));
    linear_fwd(st, a.ao, params + q.wo, params + q.bo, a.o, M, d, d);
    hipLaunchKernelGGL(ln_fwd_kernel, dim3((M + 3) / 4), dim3(256), 0, st, hin, a.o, a.s1, a.h1, a.mean1, a.rstd1,
                       params + q.g1, params + q.be1, M, d, dr, site(l, 1));
    linear_fwd(st, a.h1, params + q.w1, params + q.b1, a.f1, M, ff, d);
    hipLaunchKernelGGL(relu_drop_kernel, dim3(ew_blocks((long)M * ff)), dim3(256), 0, st, a.f1, (long)M * ff, dr, site(l, 2));
    linear_fwd(st, a.f1, params + q.w2, params + q.b2, a.f2, M, d, ff);
    hipLaunchKernelGGL(ln_fwd_kernel, dim3((M + 3) / 4), dim3(256), 0, st, a.h1, a.f2, a.s2, a.h2, a.mean2, a.rstd2,
                       params + q.g2, params + q.be2, M, d, dr, site(l, 3));
    hin = a.h2;
  }
  hipLaunchKernelGGL(tail_gather_kernel, dim3(ew_blocks((long)Mt * d)), dim3(256), 0, st, hin, w.tail, Bn, L, T, d);
  linear_fwd(st, w.tail, params + po.wout, params + po.bout, pred, Mt, c, d);
}

void train_backward(const quattro_tf_train_desc& D, const float* params, float* grads, void* workspace, const float* x_norm,
                    const float* prompt_norm, const float* dpred, int batch, uint64_t dropout_seed, int training,
                    hipStream_t st) {
  const ParamOff po = param_offsets(D);
  const Ws w = carve(D, batch, reinterpret_cast<char*>(workspace));
  const int Bn = batch, NS = D.n_state_tok, P = D.prompt_len, T = D.target_len, L = NS + P + T, M = Bn * L, Mt = Bn * T;
  const int d = D.d_model, ff = D.d_ff, c = D.control_dim, n = D.state_dim, H = D.nhead;
  const int hd = d / H;
  const float scale = 1.0f / sqrtf((float)hd);
  Drop dr;
  dr.seed = dropout_seed;
  dr.p = (training && D.dropout > 0.0f) ? D.dropout : 0.0f;
  dr.inv_keep = 1.0f / (1.0f - dr.p);
  auto site = [](int layer, int kind) { return (uint32_t)(1 + 4 * layer + kind); };   // 0: positions; per layer: attention
                                                                                       // weights, out-proj, ff hidden, ff out
  const bool dropping = dr.p > 0.0f;
  // ---------------------------------------------------------------- backward
  (void)hipMemsetAsync(grads, 0, (size_t)po.total * sizeof(float), st);
  linear_bwd_weight(st, dpred, w.tail, grads + po.wout, grads + po.bout, Mt, c, d);
  linear_bwd_input(st, dpred, params + po.wout, w.dtail, Mt, c, d, false);
  hipLaunchKernelGGL(tail_scatter_kernel, dim3(ew_blocks((long)M * d)), dim3(256), 0, st, w.dtail, w.dh, Bn, L, T, d);
  for (int l = D.n_layers - 1; l >= 0; --l) {
    const LayerOff& q = po.layer[l];
    const LayerWs& a = w.layer[l];
    const float* lin = l == 0 ? w.h0 : w.layer[l - 1].h2;
    // LayerNorm 2: dh -> ds2 (in dtmp); s2 = h1 + drop(f2)
    hipLaunchKernelGGL(ln_bwd_kernel, dim3((M + LN_BWD_ROWS - 1) / LN_BWD_ROWS), dim3(256), 0, st, w.dh, a.s2, a.mean2, a.rstd2, params + q.g2, w.dtmp,
                       w.lnpart, M, d);
    hipLaunchKernelGGL(ln_bwd_reduce_kernel, dim3((2 * d + 255) / 256, LN_RED_SLICES), dim3(256), 0, st, w.lnpart, (M + LN_BWD_ROWS - 1) / LN_BWD_ROWS, d, grads + q.g2,
                       grads + q.be2);
    const float* df2 = w.dtmp;
    if (dropping) {
      hipLaunchKernelGGL(drop_bwd_kernel, dim3(ew_blocks((long)M * d)), dim3(256), 0, st, w.dbranch, w.dtmp, (long)M * d, dr,
                         site(l, 3));
      df2 = w.dbranch;
    }
    linear_bwd_weight(st, df2, a.f1, grads + q.w2, grads + q.b2, M, d, ff);
    linear_bwd_input(st, df2, params + q.w2, w.df, M, d, ff, false);
    hipLaunchKernelGGL(relu_drop_bwd_kernel, dim3(ew_blocks((long)M * ff)), dim3(256), 0, st, w.df, a.f1, (long)M * ff,
                       dr.inv_keep);
    linear_bwd_weight(st, w.df, a.h1, grads + q.w1, grads + q.b1, M, ff, d);
    // dh1 = ds2 (residual) + da1 W1
    linear_bwd_input(st, w.df, params + q.w1, w.dtmp, M, ff, d, true);
    // LayerNorm 1: dh1 (dtmp) -> ds1 (dh); s1 = hin + drop(o)
    hipLaunchKernelGGL(ln_bwd_kernel, dim3((M + LN_BWD_ROWS - 1) / LN_BWD_ROWS), dim3(256), 0, st, w.dtmp, a.s1, a.mean1, a.rstd1, params + q.g1, w.dh,
                       w.lnpart, M, d);
    hipLaunchKernelGGL(ln_bwd_reduce_kernel, dim3((2 * d + 255) / 256, LN_RED_SLICES), dim3(256), 0, st, w.lnpart, (M + LN_BWD_ROWS - 1) / LN_BWD_ROWS, d, grads + q.g1,
                       grads + q.be1);
    const float* dob = w.dh;
    if (dropping) {
      hipLaunchKernelGGL(drop_bwd_kernel, dim3(ew_blocks((long)M * d)), dim3(256), 0, st, w.dbranch, w.dh, (long)M * d, dr,
                         site(l, 1));
      dob = w.dbranch;
    }
    linear_bwd_weight(st, dob, a.ao, grads + q.wo, grads + q.bo, M, d, d);
    linear_bwd_input(st, dob, params + q.wo, w.dao, M, d, d, false);
    hipLaunchKernelGGL(attn_bwd_mfma_kernel, dim3(H, Bn), dim3(256), attn_mfma_bwd_lds(), st, a.qkv, a.P, a.ao, w.dao, w.dqkv, L, d,
                       H, hd, scale, dr, site(l, 0));
    linear_bwd_weight(st, w.dqkv, lin, grads + q.wqkv, grads + q.bqkv, M, 3 * d, d);
    // d(lin) = ds1 (residual, in dh) + dqkv Wqkv
    linear_bwd_input(st, w.dqkv, params + q.wqkv, w.dh, M, 3 * d, d, true);
  }
  hipLaunchKernelGGL(embed_bwd_kernel, dim3(ew_blocks((long)M * d)), dim3(256), 0, st, w.dh, w.dxe, w.due, grads + po.tgt, Bn, NS,
                     P, T, d, dr);
  linear_bwd_weight(st, w.dxe, x_norm, grads + po.ws, grads + po.bs, Bn * NS, d, n);
  linear_bwd_weight(st, w.due, prompt_norm, grads + po.wc, grads + po.bc, Bn * P, d, c);
}

}  // namespace

extern "C" {

size_t quattro_tf_train_param_count(const quattro_tf_train_desc* D) {
  return desc_ok(D) ? (size_t)param_offsets(*D).total : 0;
}

long quattro_tf_train_param_offset(const quattro_tf_train_desc* D, int which, int layer) {
  if (!desc_ok(D)) return -1;
  const ParamOff o = param_offsets(*D);
  switch (which) {
    case QUATTRO_TF_P_TARGET: return o.tgt;
    case QUATTRO_TF_P_STATE_W: return o.ws;
    case QUATTRO_TF_P_STATE_B: return o.bs;
    case QUATTRO_TF_P_CTRL_W: return o.wc;
    case QUATTRO_TF_P_CTRL_B: return o.bc;
    case QUATTRO_TF_P_OUT_W: return o.wout;
    case QUATTRO_TF_P_OUT_B: return o.bout;
    default: break;
  }
  if (layer < 0 || layer >= D->n_layers) return -1;
  const LayerOff& q = o.layer[layer];
  switch (which) {
    case QUATTRO_TF_P_QKV_W: return q.wqkv;
    case QUATTRO_TF_P_QKV_B: return q.bqkv;
    case QUATTRO_TF_P_O_W: return q.wo;
    case QUATTRO_TF_P_O_B: return q.bo;
    case QUATTRO_TF_P_FF1_W: return q.w1;
    case QUATTRO_TF_P_FF1_B: return q.b1;
    case QUATTRO_TF_P_FF2_W: return q.w2;
    case QUATTRO_TF_P_FF2_B: return q.b2;
    case QUATTRO_TF_P_LN1_G: return q.g1;
    case QUATTRO_TF_P_LN1_B: return q.be1;
    case QUATTRO_TF_P_LN2_G: return q.g2;
    case QUATTRO_TF_P_LN2_B: return q.be2;
    default: return -1;
  }
}

size_t quattro_tf_train_workspace_bytes(const quattro_tf_train_desc* D, int batch) {
  if (!desc_ok(D) || batch <= 0) return 0;
  return carve(*D, batch, nullptr).total;
}

int quattro_tf_train_step_f32(const quattro_tf_train_desc* D, const float* params, float* grads, void* workspace,
                              size_t workspace_bytes, const float* x_norm, const float* prompt_norm,
                              const float* target_norm, const float* pe, int batch, uint64_t dropout_seed, int training,
                              float* loss, float* pred_out, void* stream) {
  if (!desc_ok(D)) return D ? QUATTRO_ERR_UNSUPPORTED : QUATTRO_ERR_BAD_ARG;
  if (!params || !workspace || !x_norm || !prompt_norm || !pe || batch <= 0) return QUATTRO_ERR_BAD_ARG;
  if ((grads != nullptr || loss != nullptr) && !target_norm) return QUATTRO_ERR_BAD_ARG;
  if (((uintptr_t)workspace & 255) != 0 || workspace_bytes < carve(*D, batch, nullptr).total) return QUATTRO_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  raise_attn_lds();
  const Ws w = carve(*D, batch, reinterpret_cast<char*>(workspace));
  const long npred = (long)batch * D->target_len * D->control_dim;
  float* pred = pred_out ? pred_out : w.pred;
  train_forward(*D, params, workspace, x_norm, prompt_norm, pe, batch, dropout_seed, training, pred, st);
  if (loss != nullptr || grads != nullptr) {
    float* lossp = loss ? loss : w.loss_pad;
    (void)hipMemsetAsync(lossp, 0, sizeof(float), st);
    hipLaunchKernelGGL(mse_kernel, dim3(ew_blocks(npred) > 256 ? 256 : ew_blocks(npred)), dim3(256), 0, st, pred, target_norm,
                       npred, grads ? w.dpred : nullptr, lossp);
  }
  if (grads != nullptr) train_backward(*D, params, grads, workspace, x_norm, prompt_norm, w.dpred, batch, dropout_seed, training, st);
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

int quattro_tf_train_backward_f32(const quattro_tf_train_desc* D, const float* params, float* grads, void* workspace,
                                  size_t workspace_bytes, const float* x_norm, const float* prompt_norm, const float* d_pred,
                                  int batch, uint64_t dropout_seed, int training, void* stream) {
  if (!desc_ok(D)) return D ? QUATTRO_ERR_UNSUPPORTED : QUATTRO_ERR_BAD_ARG;
  if (!params || !grads || !workspace || !x_norm || !prompt_norm || !d_pred || batch <= 0) return QUATTRO_ERR_BAD_ARG;
  if (((uintptr_t)workspace & 255) != 0 || workspace_bytes < carve(*D, batch, nullptr).total) return QUATTRO_ERR_WORKSPACE;
  raise_attn_lds();
  train_backward(*D, params, grads, workspace, x_norm, prompt_norm, d_pred, batch, dropout_seed, training, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

int quattro_tf_adam_f32(float* params, const float* grads, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                        float eps, int step, void* stream) {
  if (!params || !grads || !m || !v || step < 1) return QUATTRO_ERR_BAD_ARG;
  if (n == 0) return QUATTRO_OK;
  // bias corrections in double, as torch.optim.Adam computes them: in fp32, 1 - 0.999^step cancels catastrophically at small
  // step (5e-5 relative at step 1), a systematic difference the parameter tests are too coarse to see
  const float c1 = (float)(1.0 - pow((double)beta1, (double)step)), c2 = (float)(1.0 - pow((double)beta2, (double)step));
  hipLaunchKernelGGL(adam_kernel, dim3(ew_blocks((long)n)), dim3(256), 0, (hipStream_t)stream, params, grads, m, v, (long)n, lr,
                     beta1, beta2, eps, c1, c2);
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

int quattro_tf_train_dropout_mask_f32(uint64_t dropout_seed, float p, int site, size_t n, float* out, void* stream) {
  if (!out || p < 0.0f || p >= 1.0f || site < 0) return QUATTRO_ERR_BAD_ARG;
  if (n == 0) return QUATTRO_OK;
  Drop dr;
  dr.seed = dropout_seed;
  dr.p = p;
  dr.inv_keep = 1.0f / (1.0f - p);
  hipLaunchKernelGGL(mask_kernel, dim3(ew_blocks((long)n)), dim3(256), 0, (hipStream_t)stream, out, (long)n, dr, (uint32_t)site);
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}

}  // extern "C"
