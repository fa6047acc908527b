// The two built-in rate functions and the integrator step stated once for ANY scalar type: plain float, or dual.h's Dual<float>
// carrying a derivative along one seeded direction.  The only user is the parameter gradient (cost_param_gradient.hip), which
// seeds ONE physical parameter and reads the derivative part of the step: d f / d theta_k at (x_t, u_t; theta).
//
// NOT the bits of the rollouts: the float rates of models_device.h multiply by reciprocals hoisted out of their loops, use fmaf in
// the integrator (rk4.h) and a Newton-refined 1 / cos; these statements divide where the formula divides and step as
// x + k * dt (qt_user::step's scheme).  With every type float the VALUE agrees with qt_step to fp32 round-off, no closer, and
// nothing may rely on more: only the derivative part is used, and it is checked against fp64 central differences of the oracle's
// step (tests/pgrad_cases.py).  models_device.h and every kernel built on it stay as they are.
//
// A rate is stated in three parts, rate(phys, x, u) = combine(coefs(phys), terms(x, u), x, u):
//   coefs    the quotients and products of the physical parameters alone (they are the same for every step of a trajectory: the
//            kernel forms them, with their derivatives along every parameter, once per wave)
//   terms    everything that reads the state and the control but no parameter (the trigonometry: in an Euler step about a given
//            (x, u) it carries no derivative and is formed once for all parameters)
//   combine  the rate from the two
// and over four scalar types, so that a quantity that carries no derivative costs no derivative arithmetic:
//   P  the parameters' coefficients    X  the state and its terms    U  the control    O  the rate (a product of the three)
// With all four the same T, GenericRate::rate is `rate(const T* phys, const T* x, const T* u, T* xd)`.  Every mixed operation used
// below exists in dual.h (Dual op Dual, Dual op float, float op Dual).  `float` may be `double` throughout (GenericRate::Scalar):
// dual.h's operators are generic over the underlying type, and generic_sincos below supplies the one function that is not.
#pragma once
#include "dual.h"

template <int MODEL>
struct GenericRate;

// the plain number type underneath a scalar (for constants that must not be rounded to float under double)
template <class T>
struct BaseScalar {
  using type = T;
};
template <class T>
struct BaseScalar<qtad::Dual<T>> {
  using type = typename BaseScalar<T>::type;
};

// sin and cos for the four scalars used here.  float and Dual<float> are dual.h's (qt_sincos underneath); double goes to the math
// library, and Dual<double> is written out because dual.h's template looks up the float overload only.
__device__ __forceinline__ void generic_sincos(float a, float* s, float* c) { qtad::sincos(a, s, c); }
__device__ __forceinline__ void generic_sincos(const qtad::Dual<float>& a, qtad::Dual<float>* s, qtad::Dual<float>* c) {
  qtad::sincos(a, s, c);
}
__device__ __forceinline__ void generic_sincos(double a, double* s, double* c) { ::sincos(a, s, c); }
__device__ __forceinline__ void generic_sincos(const qtad::Dual<double>& a, qtad::Dual<double>* s, qtad::Dual<double>* c) {
  double sv, cv;
  ::sincos(a.v, &sv, &cv);
  *s = qtad::Dual<double>(sv, cv * a.d);
  *c = qtad::Dual<double>(cv, -(sv * a.d));
}

// cart-pole (cartpole_terms of models_device.h; examples/cartpole/cartpole_dynamics.py:48-71)
template <>
struct GenericRate<QUATTRO_MODEL_CARTPOLE> {
  static constexpr int NX = 4, NU = 1;
  static constexpr int NP = 4;      // m_cart, m_pole, length, gravity
  static constexpr int NC = 5, NG = 3;
  // The parameter gradient forms this model's terms in double.  d(theta'')/d(length) is proportional to g sin(th) - cos(th) F / mt,
  // which cancels where the pole is nearly in balance under the force: forty-fold in one of the tested states, where the fp32
  // roundings of sin, cos and the two products alone were 6e-6 of the derivative (bound: 2e-6).  No reordering in fp32 helps (the
  // roundings of sin and cos are enough), so the few hundred operations of this small model run in fp64; the term is rounded to
  // fp32 once, at the end.
  using Scalar = double;
  template <class P>
  static __device__ __forceinline__ void coefs(const P* ph, P* c) {
    const P M = ph[0], mp = ph[1], l = ph[2], g = ph[3];
    const P mt = M + mp;
    c[0] = 1.0f / mt;
    c[1] = mp * l / mt;
    c[2] = mp / mt;
    c[3] = l;
    c[4] = g;
  }
  template <class X, class U>
  static __device__ __forceinline__ void terms(const X* x, const U* u, X* g) {
    generic_sincos(x[2], &g[0], &g[1]);
    g[2] = x[3] * x[3] * g[0];                       // thd^2 sin(th)
  }
  template <class P, class X, class U, class O>
  static __device__ __forceinline__ void combine(const P* c, const X* g, const X* x, const U* u, O* xd) {
    const X s = g[0], cs = g[1];
    const O tmp = u[0] * c[0] + c[1] * g[2];         // (F + mp l thd^2 s) / (M + mp)
    using Bs = typename BaseScalar<O>::type;
    const O den = c[3] * (Bs(4) / Bs(3) - c[2] * (cs * cs));
    const O thdd = (cs * tmp - c[4] * s) / den;
    xd[0] = x[1];
    xd[1] = tmp - c[1] * (thdd * cs);
    xd[2] = x[3];
    xd[3] = thdd;
  }
};

// quadrotor (qt_rate<QUADROTOR> of models_device.h; examples/quadrotor/quadrotor_dynamics.py:63-164)
template <>
struct GenericRate<QUATTRO_MODEL_QUADROTOR> {
  static constexpr int NX = 12, NU = 4;
  static constexpr int NP = 7;      // mass, Ix, Iy, Iz, arm, gravity, k_yaw
  static constexpr int NC = 8, NG = 9;
  using Scalar = float;
  template <class P>
  static __device__ __forceinline__ void coefs(const P* ph, P* c) {
    const P mass = ph[0], Ix = ph[1], Iy = ph[2], Iz = ph[3], arm = ph[4], grav = ph[5], kyaw = ph[6];
    c[0] = 1.0f / mass;
    c[1] = (Iy - Iz) / Ix;
    c[2] = (Iz - Ix) / Iy;
    c[3] = (Ix - Iy) / Iz;
    c[4] = arm / Ix;
    c[5] = arm / Iy;
    c[6] = kyaw / Iz;
    c[7] = grav;
  }
  template <class X, class U>
  static __device__ __forceinline__ void terms(const X* x, const U* u, X* g) {
    X sph, cph, sth, cth, sps, cps;
    generic_sincos(x[6], &sph, &cph);
    generic_sincos(x[7], &sth, &cth);
    generic_sincos(x[8], &sps, &cps);
    const X sec = 1.0f / cth, tth = sth * sec;
    const X wp = x[9], wq = x[10], wr = x[11];
    const U thrust = u[0] + u[1] + u[2] + u[3];
    g[0] = (sps * sph + cps * sth * cph) * thrust;
    g[1] = (cps * sph - sps * sth * cph) * thrust;
    g[2] = (cth * cph) * thrust;
    const X mix = wq * sph + wr * cph;
    g[3] = wp + mix * tth;
    g[4] = wq * cph - wr * sph;
    g[5] = mix * sec;
    g[6] = wq * wr;
    g[7] = wp * wr;
    g[8] = wp * wq;
  }
  template <class P, class X, class U, class O>
  static __device__ __forceinline__ void combine(const P* c, const X* g, const X* x, const U* u, O* xd) {
    xd[0] = x[3];
    xd[1] = x[4];
    xd[2] = x[5];
    xd[3] = c[0] * g[0];
    xd[4] = c[0] * g[1];
    xd[5] = c[0] * g[2] - c[7];
    xd[6] = g[3];
    xd[7] = g[4];
    xd[8] = g[5];
    xd[9] = c[1] * g[6] + c[4] * ((u[1] + u[2]) - (u[0] + u[3]));
    xd[10] = c[2] * g[7] + c[5] * ((u[0] + u[1]) - (u[2] + u[3]));
    xd[11] = c[3] * g[8] + c[6] * (u[0] - u[1] + u[2] - u[3]);
  }
};

// the whole statement for one scalar type
template <int MODEL, class T>
__device__ __forceinline__ void generic_rate(const T* phys, const T* x, const T* u, T* xd) {
  using R = GenericRate<MODEL>;
  T c[R::NC], g[R::NG];
  R::coefs(phys, c);
  R::terms(x, u, g);
  R::combine(c, g, x, u, xd);
}

// xn = f(x, u; phys): explicit Euler or classic RK4 with zero-order-hold u about a plain (x, u), from the coefficients c (type P) and
// the terms g1 of (x, u) itself; the stage points of an RK4 step after the first take the rate's type O.  qt_user::step's scheme
// (no fmaf), see the note at the top.
template <int MODEL, bool RK4, class S, class P, class O>
__device__ __forceinline__ void generic_step(S dt, const P* c, const S* g1, const S* x, const S* u, O* xn) {
  using R = GenericRate<MODEL>;
  constexpr int NX = R::NX;
  O k1[NX];
  R::combine(c, g1, x, u, k1);
  if constexpr (!RK4) {
#pragma unroll
    for (int i = 0; i < NX; ++i) xn[i] = x[i] + k1[i] * dt;
  } else {
    O k2[NX], k3[NX], k4[NX], xs[NX], g[R::NG];
#pragma unroll
    for (int i = 0; i < NX; ++i) xs[i] = x[i] + k1[i] * (S(0.5) * dt);
    R::terms(xs, u, g);
    R::combine(c, g, xs, u, k2);
#pragma unroll
    for (int i = 0; i < NX; ++i) xs[i] = x[i] + k2[i] * (S(0.5) * dt);
    R::terms(xs, u, g);
    R::combine(c, g, xs, u, k3);
#pragma unroll
    for (int i = 0; i < NX; ++i) xs[i] = x[i] + k3[i] * dt;
    R::terms(xs, u, g);
    R::combine(c, g, xs, u, k4);
#pragma unroll
    for (int i = 0; i < NX; ++i) xn[i] = x[i] + (k1[i] + k2[i] * S(2) + k3[i] * S(2) + k4[i]) * (dt / S(6));
  }
}
