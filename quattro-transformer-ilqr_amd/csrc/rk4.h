// Classic RK4 with zero-order-hold u, stated once: the value step, the four points the rate function is evaluated at, and the
// push of one direction through the four stages.  Nothing here knows a model: the caller passes the rate function (or its
// directional derivative) as a callable that is told the stage index s = 0..3, so it can pick per-stage data (a stage point,
// a QuadStage, a cheaper rate function after stage 0).  Every rollout and every RK4 linearisation of the library goes through
// these three functions; the operation order below — fmaf(0.5 dt, k, x) for the stage points, x + (dt / 6) (k1 + 2 k2 + 2 k3 + k4)
// for the value, fmaf(dt / 6, acc + dk4, dx0) with acc = dk1 + 2 dk2 + 2 dk3 built by fmaf for a tangent — is what decides the
// bits they share.  (user_model.h's qt_user::step is NOT one of them: see the note there.)
// No device intrinsics: with QT_RK4_HOST defined the header compiles for the host (tests/test_rk4_host_cpu.py).
#pragma once
#ifdef QT_RK4_HOST
#include <math.h>
#define __device__
#define __forceinline__ inline
#endif

// xn = x + dt/6 (k1 + 2 k2 + 2 k3 + k4);  rate(s, xs, k): k = rate function at stage point s, which is xs
template <int NX, class Rate>
__device__ __forceinline__ void rk4_step(float dt, const float* x, float* xn, Rate rate) {
  float k1[NX], k2[NX], k3[NX], k4[NX], xs[NX];
  rate(0, x, k1);
#pragma unroll
  for (int i = 0; i < NX; ++i) xs[i] = fmaf(0.5f * dt, k1[i], x[i]);
  rate(1, xs, k2);
#pragma unroll
  for (int i = 0; i < NX; ++i) xs[i] = fmaf(0.5f * dt, k2[i], x[i]);
  rate(2, xs, k3);
#pragma unroll
  for (int i = 0; i < NX; ++i) xs[i] = fmaf(dt, k3[i], x[i]);
  rate(3, xs, k4);
#pragma unroll
  for (int i = 0; i < NX; ++i) xn[i] = x[i] + (dt / 6.0f) * (k1[i] + 2.0f * k2[i] + 2.0f * k3[i] + k4[i]);
}

// the four stage points of the step from x: xp[0] = x, xp[1..3] as rk4_step forms them (the value chain of a linearisation,
// computed once and shared by all directions)
template <int NX, class Rate>
__device__ __forceinline__ void rk4_points(float dt, const float* x, float (*xp)[NX], Rate rate) {
  float k[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) xp[0][i] = x[i];
  rate(0, xp[0], k);
#pragma unroll
  for (int i = 0; i < NX; ++i) xp[1][i] = fmaf(0.5f * dt, k[i], x[i]);
  rate(1, xp[1], k);
#pragma unroll
  for (int i = 0; i < NX; ++i) xp[2][i] = fmaf(0.5f * dt, k[i], x[i]);
  rate(2, xp[2], k);
#pragma unroll
  for (int i = 0; i < NX; ++i) xp[3][i] = fmaf(dt, k[i], x[i]);
}

// col = d x_next / d z along one direction whose state part is dx0;  jvp(s, dxs, dk): dk = (d rate / d x) dxs + (d rate / d u) du
// at stage point s (the caller's du and stage data are captured)
template <int NX, class Jvp>
__device__ __forceinline__ void rk4_tangent(float dt, const float* dx0, float* col, Jvp jvp) {
  float dk[NX], dxs[NX], acc[NX];
  jvp(0, dx0, dk);
#pragma unroll
  for (int i = 0; i < NX; ++i) { acc[i] = dk[i]; dxs[i] = fmaf(0.5f * dt, dk[i], dx0[i]); }
  jvp(1, dxs, dk);
#pragma unroll
  for (int i = 0; i < NX; ++i) { acc[i] = fmaf(2.0f, dk[i], acc[i]); dxs[i] = fmaf(0.5f * dt, dk[i], dx0[i]); }
  jvp(2, dxs, dk);
#pragma unroll
  for (int i = 0; i < NX; ++i) { acc[i] = fmaf(2.0f, dk[i], acc[i]); dxs[i] = fmaf(dt, dk[i], dx0[i]); }
  jvp(3, dxs, dk);
#pragma unroll
  for (int i = 0; i < NX; ++i) col[i] = fmaf(dt / 6.0f, acc[i] + dk[i], dx0[i]);
}
