// Device functions of the adjoint sweeps and the covariance recursion (cost_gradient.hip, track_gradient.hip, track_covariance.hip):
// what a lane forms off the serial chain -- an entry of Lf_x, the l_u of one control, a column of [A | B] or of [A + B K | B] with the
// matching entry of l_z.  Moved here unchanged from cost_gradient.hip and (track_item) from track_gradient.hip, whose kernels compile to
// the same instructions as before.
#pragma once
#include "rollout_body.h"

namespace {

// entry j of Lf_x(x_N)
template <int MODEL>
__device__ __forceinline__ float grad_terminal_entry(const quattro_model_params& own, const float* xN, const int j) {
  constexpr int NX = ModelDims<MODEL>::NX;
#ifdef QT_USER_MODEL_HEADER
  if constexpr (MODEL == QUATTRO_MODEL_USER) {
    using D = qtad::Dual<float>;
    D xd[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xd[i] = D(xN[i], i == j ? 1.0f : 0.0f);
    return qt_user::final_cost<D>(own, xd).d;
  } else
#endif
  {
    float v = 0.0f;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const float g = qt_terminal_vx(own, i, xN[i]);
      v = (i == j) ? g : v;
    }
    return v;
  }
}

// l_u of ONE control (weight ra, value ua): the expression of qt_control_cost_derivs with a softplus that is accurate RELATIVE to
// itself.  qt_softplus forms log(1 + e) on the hardware v_exp_f32 / v_log_f32; the absolute error 6e-8 of forming 1 + e is harmless
// next to the cost it is added to, but away from the barrier (beta u of 3 or more) with a small r the barrier is all of l_u and, over
// a short horizon, most of g_t: 2.7e-6 of the entry on the cart-pole (beta = 3, r = 0.004, N = 2).  Here, on the same two hardware
// instructions: the rounding of x log2(e) is compensated (e (1 + r ln 2)), and log1p(e) = log(w) e / (w - 1) with w = 1 + e rounded
// (w - 1 is exact, and the quotient undoes the rounding of w).  About 25 instructions; the math library's expf / log1pf gave the
// same accuracy at about 150, which every pass of every wave runs whether its lane holds a control or not.
// NOT the bits of the l_u in the records of quattro_linearize_f32: the two agree to fp32 round-off where the barrier is active and to
// about 1e-6 relative away from it, where the record's is the less accurate one.
__device__ __forceinline__ float grad_control_lu(const quattro_model_params& own, float ra, float ua) {
#pragma clang fp contract(off)
  float lu = 2.0f * ra * ua;
  if (own.barrier_alpha != 0.0f) {
    const float bz = -own.barrier_beta * ua;
    const float a = -fabsf(bz);
    const float t = a * 1.44269504f;                                       // log2(e) = 1.44269504f + 1.92596299e-8
    const float r = fmaf(a, 1.44269504f, -t) + a * 1.92596299e-8f;
    float e = exp2f(t);
    e = fmaf(e, r * 0.693147181f, e);                                      // exp(a) = 2^t 2^r
    const float w = 1.0f + e;
    const float l1p = (w == 1.0f) ? e : __logf(w) * __fdividef(e, w - 1.0f);
    const float sp = (fmaxf(bz, 0.0f) + l1p) * (1.0f / own.barrier_beta);
    const float sg = __fdividef(bz >= 0.0f ? 1.0f : e, w);                 // logistic(bz)
    lu = fmaf(own.barrier_alpha, -2.0f * sp * sg, lu);
  }
  return lu;
}

// column j of [A | B] at (xs, us) -> col[NX], and entry j of l_z = (l_x, l_u) (returned)
template <int MODEL, bool RK4>
__device__ __forceinline__ float grad_item(const quattro_model_params& own, const float* xs, const float* us, const int j,
                                           float* col) {
  constexpr int NX = ModelDims<MODEL>::NX, NU = ModelDims<MODEL>::NU;
#ifdef QT_USER_MODEL_HEADER
  if constexpr (MODEL == QUATTRO_MODEL_USER) {
    using D = qtad::Dual<float>;
    D xd[NX], ud[NU], xn[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xd[i] = D(xs[i], i == j ? 1.0f : 0.0f);
#pragma unroll
    for (int a = 0; a < NU; ++a) ud[a] = D(us[a], NX + a == j ? 1.0f : 0.0f);
    qt_user::step<D, RK4>(own, xd, ud, xn);
#pragma unroll
    for (int i = 0; i < NX; ++i) col[i] = xn[i].d;
    return qt_user::stage_cost<D>(own, xd, ud).d;
  } else
#endif
  {
    const float dt = own.dt;
    float dx0[NX], du[NU];
#pragma unroll
    for (int i = 0; i < NX; ++i) dx0[i] = (i == j) ? 1.0f : 0.0f;
#pragma unroll
    for (int a = 0; a < NU; ++a) du[a] = (NX + a == j) ? 1.0f : 0.0f;
    if constexpr (!RK4) {
      float dk[NX];
      qt_rate_jvp<MODEL>(own, xs, us, dx0, du, dk);
#pragma unroll
      for (int i = 0; i < NX; ++i) col[i] = fmaf(dt, dk[i], dx0[i]);
    } else if constexpr (MODEL == QUATTRO_MODEL_QUADROTOR) {
      QuadStage st[4];
      quad_rk4_stages(own, own.phys, xs, us, [&](int s, const QuadStage& q) __attribute__((always_inline)) { st[s] = q; });
      rk4_tangent<NX>(dt, dx0, col, [&](int s, const float* dxs, float* dk) __attribute__((always_inline)) {
        quad_jvp_at(st[s], own, dxs, du, dk);
      });
    } else {
      float xp[4][NX];
      rk4_points<NX>(dt, xs, xp, [&](int, const float* xst, float* k) __attribute__((always_inline)) { qt_rate<MODEL>(own, xst, us, k); });
      rk4_tangent<NX>(dt, dx0, col, [&](int s, const float* dxs, float* dk) __attribute__((always_inline)) {
        qt_rate_jvp<MODEL>(own, xp[s], us, dxs, du, dk);
      });
    }
    // l_z[j]: the lane's own state entry, or its own control (quadratic term + barrier)
    float v = 0.0f, ra = own.r[0], ua = us[0];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const float g = 2.0f * own.q[i] * (xs[i] - own.x_ref[i]);
      v = (i == j) ? g : v;
    }
#pragma unroll
    for (int a = 1; a < NU; ++a) {
      ra = (NX + a == j) ? own.r[a] : ra;
      ua = (NX + a == j) ? us[a] : ua;
    }
    return j >= NX ? grad_control_lu(own, ra, ua) : v;
  }
}

// column j of [A + B K | B] at (xs, us) -> col[NX], given the lane's control seed du (state lane j: K[:, j]; control lane a: e_a),
// and the matching staged entry: l_x[j] + du^T l_u for a state lane, l_u[a] for a control lane (returned)
template <int MODEL, bool RK4>
__device__ __forceinline__ float track_item(const quattro_model_params& own, const float* xs, const float* us, const int j,
                                            const float* du, float* col) {
  constexpr int NX = ModelDims<MODEL>::NX, NU = ModelDims<MODEL>::NU;
#ifdef QT_USER_MODEL_HEADER
  if constexpr (MODEL == QUATTRO_MODEL_USER) {
    using D = qtad::Dual<float>;
    D xd[NX], ud[NU], xn[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xd[i] = D(xs[i], i == j ? 1.0f : 0.0f);
#pragma unroll
    for (int a = 0; a < NU; ++a) ud[a] = D(us[a], du[a]);
    qt_user::step<D, RK4>(own, xd, ud, xn);
#pragma unroll
    for (int i = 0; i < NX; ++i) col[i] = xn[i].d;
    return qt_user::stage_cost<D>(own, xd, ud).d;
  } else
#endif
  {
    const float dt = own.dt;
    float dx0[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) dx0[i] = (i == j) ? 1.0f : 0.0f;
    if constexpr (!RK4) {
      float dk[NX];
      qt_rate_jvp<MODEL>(own, xs, us, dx0, du, dk);
#pragma unroll
      for (int i = 0; i < NX; ++i) col[i] = fmaf(dt, dk[i], dx0[i]);
    } else if constexpr (MODEL == QUATTRO_MODEL_QUADROTOR) {
      QuadStage st[4];
      quad_rk4_stages(own, own.phys, xs, us, [&](int s, const QuadStage& q) __attribute__((always_inline)) { st[s] = q; });
      rk4_tangent<NX>(dt, dx0, col, [&](int s, const float* dxs, float* dk) __attribute__((always_inline)) {
        quad_jvp_at(st[s], own, dxs, du, dk);
      });
    } else {
      float xp[4][NX];
      rk4_points<NX>(dt, xs, xp, [&](int, const float* xst, float* k) __attribute__((always_inline)) { qt_rate<MODEL>(own, xst, us, k); });
      rk4_tangent<NX>(dt, dx0, col, [&](int s, const float* dxs, float* dk) __attribute__((always_inline)) {
        qt_rate_jvp<MODEL>(own, xp[s], us, dxs, du, dk);
      });
    }
    // the lane's own l_x entry (0 for a control lane), then du^T l_u: with du = e_a that is l_u[a] itself (1 * l_u[a] + 0, exact)
    float v = 0.0f;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const float g = 2.0f * own.q[i] * (xs[i] - own.x_ref[i]);
      v = (i == j) ? g : v;
    }
#pragma unroll
    for (int a = 0; a < NU; ++a) v = fmaf(du[a], grad_control_lu(own, own.r[a], us[a]), v);
    return v;
  }
}

}  // namespace
