// Device-side bodies of the quadrotor rollouts (four lanes — one DPP quad — per trajectory / line-search candidate), shared
// by rollout_quad.hip (one launch per call) and solve_quad.hip (the device-resident solve loop).  Design notes:
// rollout_quad.hip.
#pragma once
#include <type_traits>

#include "models_device.h"

namespace {

constexpr int NX = 12, NU = 4, CS = 16;   // candidate record: x'_{t+1} (12) | u'_t (4)

#define QT_QP(a, b, c, d) ((a) | ((b) << 2) | ((c) << 4) | ((d) << 6))
template <int CTRL>
__device__ __forceinline__ float quad_perm(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int I>
__device__ __forceinline__ float quad_bcast(float v) {   // value of lane I of this quad, in every lane of the quad
  return quad_perm<QT_QP(I, I, I, I)>(v);
}
__device__ __forceinline__ double quad_sum(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  return v;
}

// per-lane constants, selected once from the model parameters
struct LaneConst {
  bool is0, is1;          // axis 0 / axis 1 (else axis 2); lane 3 counts as axis 0
  int a, j;
  float qw[4], qfw[4], xr[4];   // weights / reference of the own states (p_a, v_a, angle_a, omega_a); 0 weights on lane 3
  float rj;                     // R weight of control j
  float tc[4];                  // omega'_a = gy * (omega_b omega_c) + sum_i tc[i] u_i     (torque row / inertia)
  float gy, gz, inv_mass, dt;
  __device__ __forceinline__ float sel(float v0, float v1, float v2) const { return is0 ? v0 : (is1 ? v1 : v2); }
};

// the torque row as VALUES in registers.  tc[3] is -gain in every role, and left to itself the compiler keeps gain and negates it at
// each use that cannot take a source modifier -- QuadDrive's DPP multiply-adds: a v_xor per step.
__device__ __forceinline__ void pin_torque_row(LaneConst& L) {
  asm("" : "+v"(L.tc[0]), "+v"(L.tc[1]), "+v"(L.tc[2]), "+v"(L.tc[3]));   // (not volatile: a row nobody reads still drops out)
}

__device__ __forceinline__ LaneConst lane_const(const quattro_model_params& p, int j) {
  LaneConst L;
  L.j = j;
  L.a = j == 3 ? 0 : j;
  L.is0 = L.a == 0;
  L.is1 = L.a == 1;
  const float live = j == 3 ? 0.0f : 1.0f;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    L.qw[g] = live * L.sel(p.q[3 * g], p.q[3 * g + 1], p.q[3 * g + 2]);
    L.qfw[g] = live * L.sel(p.qf[3 * g], p.qf[3 * g + 1], p.qf[3 * g + 2]);
    L.xr[g] = L.sel(p.x_ref[3 * g], p.x_ref[3 * g + 1], p.x_ref[3 * g + 2]);
  }
  L.rj = p.r[j];   // (indexed, not a chain of selects: the compiler turns those into a phi of POINTERS into the parameter block,
                   //  which pins a private copy of the whole block in scratch memory inside the fused solve kernel)
  const float Ix = p.phys[1], Iy = p.phys[2], Iz = p.phys[3], arm = p.phys[4], kyaw = p.phys[6];
  // tau_phi = arm((u1+u2)-(u0+u3)), tau_theta = arm((u0+u1)-(u2+u3)), tau_psi = kyaw(u0-u1+u2-u3)   (quadrotor_dynamics.py:139-154)
  const float s0 = L.sel(-1.0f, 1.0f, 1.0f), s1 = L.sel(1.0f, 1.0f, -1.0f), s2 = L.sel(1.0f, -1.0f, 1.0f),
              s3 = L.sel(-1.0f, -1.0f, -1.0f);
  const float gain = L.sel(arm / Ix, arm / Iy, kyaw / Iz);
  L.tc[0] = s0 * gain; L.tc[1] = s1 * gain; L.tc[2] = s2 * gain; L.tc[3] = s3 * gain;
  pin_torque_row(L);
  L.gy = L.sel((Iy - Iz) / Ix, (Iz - Ix) / Iy, (Ix - Iy) / Iz);
  L.gz = L.sel(0.0f, 0.0f, -p.phys[5]);
  L.inv_mass = 1.0f / p.phys[0];
  L.dt = p.dt;
  return L;
}

// The lane constants of a PLANT (quattro_track_f32, quattro_mpc_run_plant_f32): lane_const's role and rate-function constants —
// a plant has no cost, its weights stay zero and unused.  The parameters are the plant's own or, with plant_phys, row bb of that
// array: chosen as VALUES behind a wave-uniform branch, never as a pointer into either block (lane_const's note on pointer phis).
// (The formulas are lane_const's, restated: routing lane_const itself through a shared helper reorders its parameter loads, and
//  the line-search kernels' register allocation follows that order — one more VGPR in rollout_quad_kernel.)
__device__ __forceinline__ LaneConst lane_const_plant(const PlantSpec& plant, const float* __restrict__ plant_phys, size_t bb,
                                                      float dt, int j) {
  float ph[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) ph[i] = plant.phys[i];
  if (plant_phys != nullptr) {
#pragma unroll
    for (int i = 0; i < 7; ++i) ph[i] = plant_phys[bb * 8 + i];
  }
  const float mass = ph[0], Ix = ph[1], Iy = ph[2], Iz = ph[3], arm = ph[4], grav = ph[5], kyaw = ph[6];
  LaneConst L{};
  L.j = j;
  L.a = j == 3 ? 0 : j;
  L.is0 = L.a == 0;
  L.is1 = L.a == 1;
  const float s0 = L.sel(-1.0f, 1.0f, 1.0f), s1 = L.sel(1.0f, 1.0f, -1.0f), s2 = L.sel(1.0f, -1.0f, 1.0f),
              s3 = L.sel(-1.0f, -1.0f, -1.0f);
  const float gain = L.sel(arm / Ix, arm / Iy, kyaw / Iz);
  L.tc[0] = s0 * gain; L.tc[1] = s1 * gain; L.tc[2] = s2 * gain; L.tc[3] = s3 * gain;
  pin_torque_row(L);
  L.gy = L.sel((Iy - Iz) / Ix, (Iz - Ix) / Iy, (Ix - Iy) / Iz);
  L.gz = L.sel(0.0f, 0.0f, -grav);
  L.inv_mass = 1.0f / mass;
  L.dt = dt;
  return L;
}

// The lane constants of a trajectory with parameters of its own (quattro_ilqr_solve_phys_f32, quattro_mpc_run_phys_f32): the cost
// weights and dt are p's, as lane_const selects them; the rate-function constants come from row bb of model_phys [B][8], read as
// values -- the quads of a wave work on different trajectories, so these are vector loads.  lane_const's formulas restated on the
// row, like lane_const_plant's and for its reason: lane_const itself, and with it every kernel that calls it, stays as it is (what it
// derives from p.phys is dead here and removed).
__device__ __forceinline__ LaneConst lane_const_phys(const quattro_model_params& p, const float* __restrict__ model_phys, size_t bb,
                                                     int j) {
  LaneConst L = lane_const(p, j);
  float ph[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) ph[i] = model_phys[bb * 8 + i];
  const float mass = ph[0], Ix = ph[1], Iy = ph[2], Iz = ph[3], arm = ph[4], grav = ph[5], kyaw = ph[6];
  const float s0 = L.sel(-1.0f, 1.0f, 1.0f), s1 = L.sel(1.0f, 1.0f, -1.0f), s2 = L.sel(1.0f, -1.0f, 1.0f),
              s3 = L.sel(-1.0f, -1.0f, -1.0f);
  const float gain = L.sel(arm / Ix, arm / Iy, kyaw / Iz);
  L.tc[0] = s0 * gain; L.tc[1] = s1 * gain; L.tc[2] = s2 * gain; L.tc[3] = s3 * gain;
  pin_torque_row(L);
  L.gy = L.sel((Iy - Iz) / Ix, (Iz - Ix) / Iy, (Ix - Iy) / Iz);
  L.gz = L.sel(0.0f, 0.0f, -grav);
  L.inv_mass = 1.0f / mass;
  return L;
}

template <bool PHYS>
__device__ __forceinline__ LaneConst lane_const_of(const quattro_model_params& p, const float* __restrict__ model_phys, size_t bb,
                                                   int j) {
  if constexpr (PHYS) return lane_const_phys(p, model_phys, bb, j);
  else return lane_const(p, j);
}

// the four controls of the quad: lane j holds u_j (`own`).  Round 6: they are broadcast to every lane (`c`, four DPP moves, as
// rounds 2 - 5 did for every step) only where the step's store wants all four in one lane anyway -- lane 3's record, the control
// row of gather_quarter: Store::ALL_U.  A step that stores its own lane's values (simulate, the tracked plant, a cost-only
// rollout) keeps `own` alone, and the rate function reads the quad through DPP operands (QuadDrive).
struct QuadU {
  float own;
  bool all;
  float c[4];
  __device__ __forceinline__ explicit QuadU(float uo, bool want_all = false) : own(uo), all(want_all) {
    if (all) { c[0] = quad_bcast<0>(uo); c[1] = quad_bcast<1>(uo); c[2] = quad_bcast<2>(uo); c[3] = quad_bcast<3>(uo); }
  }
};

// what the rate function takes from the controls, once per step (the four stage calls of RK4 share it): thrust / mass and this
// lane's torque row.  From the broadcast copies where the step has them.  Where not: v_add_f32_dpp / v_mul_f32_dpp /
// v_fmac_f32_dpp on the own-control register -- gain_dot's idiom, its leading s_nop for the VALU-write -> DPP-read hazard
// included -- with one move left (the sum's first term; only src0 can be the DPP operand): 9 issue slots for the 11 of four moves
// and seven operations.  (With the four moves needed anyway it would be 13: measured, the line search 0.6 us slower.)  Same values
// either way: a + b and a * b commute bit for bit, the sum keeps its association ((u0 + u1) + u2) + u3 and the row its order
// tc0 u0, + tc1 u1, + tc2 u2, + tc3 u3, fused as before.
struct QuadDrive {
  float tm, tau;
  __device__ __forceinline__ QuadDrive(const LaneConst& L, const QuadU& U) {
    if (U.all) {
      tm = (U.c[0] + U.c[1] + U.c[2] + U.c[3]) * L.inv_mass;
      tau = fmaf(L.tc[3], U.c[3], fmaf(L.tc[2], U.c[2], fmaf(L.tc[1], U.c[1], L.tc[0] * U.c[0])));
      return;
    }
    float s, t;
#define QT_DP(l) " quad_perm:[" l "," l "," l "," l "] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
    asm volatile("s_nop 1\n\t"
                 "v_mov_b32_dpp %0, %2" QT_DP("0")
                 "v_mul_f32_dpp %1, %2, %3" QT_DP("0")
                 "v_add_f32_dpp %0, %2, %0" QT_DP("1")
                 "v_fmac_f32_dpp %1, %2, %4" QT_DP("1")
                 "v_add_f32_dpp %0, %2, %0" QT_DP("2")
                 "v_fmac_f32_dpp %1, %2, %5" QT_DP("2")
                 "v_add_f32_dpp %0, %2, %0" QT_DP("3")
                 "v_fmac_f32_dpp %1, %2, %6" QT_DP("3")
                 : "=&v"(s), "=&v"(t)
                 : "v"(U.own), "v"(L.tc[0]), "v"(L.tc[1]), "v"(L.tc[2]), "v"(L.tc[3]));
#undef QT_DP
    tm = s * L.inv_mass;
    tau = t;
  }
};

// time derivative of the own states xo = (p_a, v_a, angle_a, omega_a) given the quad's controls
// sin / cos of the own angle at an RK4 stage point from the step's base values by angle addition: the stage angle is the base
// angle + delta with |delta| = O(dt * rate), so sin(delta), cos(delta) are short Taylor polynomials (odd to delta^7, even to
// delta^6: below 1 ulp of the result for |delta| <= 0.25; beyond that — a tumbling candidate — the full reduction runs, behind a
// wave-uniform branch).  A full qt_sincos is ~25 instructions on the serial chain, this is 11.
struct TrigBase {
  float a, s, c;      // base angle and its sin / cos
};
__device__ __forceinline__ void stage_sincos(const TrigBase& b, float x, float* s, float* c) {
  const float d = x - b.a;
  if (__builtin_expect(__any(!(fabsf(d) <= 0.25f)), 0)) {
    qt_sincos(x, s, c);
    return;
  }
  const float z = d * d;
  const float sd = d * fmaf(z, fmaf(z, fmaf(z, -1.9841270e-4f, 8.3333333e-3f), -1.6666667e-1f), 1.0f);
  const float cd = fmaf(z, fmaf(z, fmaf(z, -1.3888889e-3f, 4.1666667e-2f), -0.5f), 1.0f);
  *s = fmaf(b.s, cd, b.c * sd);
  *c = fmaf(b.c, cd, -(b.s * sd));
}

template <bool STAGE>
__device__ __forceinline__ void quad_rate(const LaneConst& L, const float* xo, const QuadDrive& D, float* xd, TrigBase& tb) {
  const float tm = D.tm, tau = D.tau;
  float so, co;
  if constexpr (STAGE) {
    stage_sincos(tb, xo[2], &so, &co);
  } else {
    qt_sincos_chain(xo[2], &so, &co);
    tb.a = xo[2]; tb.s = so; tb.c = co;
  }
  const float sph = quad_bcast<0>(so), cph = quad_bcast<0>(co), sth = quad_bcast<1>(so), cth = quad_bcast<1>(co),
              sps = quad_bcast<2>(so), cps = quad_bcast<2>(co);
  const float y = __builtin_amdgcn_rcpf(cth);
  const float sec = fmaf(fmaf(-cth, y, 1.0f), y, y);       // 1 / cos(theta): reciprocal + one Newton step
  const float tth = sth * sec;
  const float wp = quad_bcast<0>(xo[3]), wq = quad_bcast<1>(xo[3]), wr = quad_bcast<2>(xo[3]);
  xd[0] = xo[1];
  // v' = (T/m) [sps sph + cps sth cph, cps sph - sps sth cph, cth cph] - [0, 0, g]
  const float ca = L.sel(sps, cps, 0.0f), cb = L.sel(cps * sth, -(sps * sth), cth);
  xd[1] = fmaf(tm, fmaf(ca, sph, cb * cph), L.gz);
  // Euler-angle rates
  const float mix = fmaf(wq, sph, wr * cph);
  xd[2] = L.sel(fmaf(mix, tth, wp), fmaf(wq, cph, -(wr * sph)), mix * sec);
  // body rates: the lane's product omega_b omega_c -- wq wr, wp wr, wp wq by axis, lane 3 as axis 0 -- as a product of two quad
  // permutations of the body-rate register, [q, p, p, q] x [r, r, q, r]: the operands and their order per lane are those of the
  // role select over three products that stood here (two multiplies and two selects in the ISA)
  xd[3] = fmaf(L.gy, quad_perm<QT_QP(1, 0, 0, 1)>(xo[3]) * quad_perm<QT_QP(2, 2, 1, 2)>(xo[3]), tau);
}

template <bool RK4>
__device__ __forceinline__ void quad_step(const LaneConst& L, const float* xo, const QuadU& uo, float* xn) {
  const QuadDrive D(L, uo);
  TrigBase tb;
  if constexpr (!RK4) {
    float k1[4];
    quad_rate<false>(L, xo, D, k1, tb);
#pragma unroll
    for (int g = 0; g < 4; ++g) xn[g] = fmaf(L.dt, k1[g], xo[g]);
  } else {   // stage 0 sets the trig base, the later stages reach their angles from it by angle addition
    rk4_step<4>(L.dt, xo, xn, [&](int s, const float* xs, float* k) __attribute__((always_inline)) {
      if (s == 0) quad_rate<false>(L, xs, D, k, tb);
      else quad_rate<true>(L, xs, D, k, tb);
    });
  }
}

// The lanes whose barrier term counts, as lane_stage_cost takes them: the lanes of rollouts whose result is used -- or none where
// the problem has no barrier.  Taken once, outside the step loop.  The test is p.barrier_alpha != 0.0f on the BITS (true for NaN,
// false for +-0): as a float compare inside the step the compiler kept the wave-uniform, loop-invariant answer as a 0/1 VGPR and
// compared it again every step (v_cndmask, v_cmp, s_andn2, s_cbranch).  Folded into the mask, the step's one remaining test --
// may the short cut be taken -- answers both.
__device__ __forceinline__ unsigned long long barrier_lanes(const quattro_model_params& p, bool counted) {
  const bool on = (__float_as_uint(p.barrier_alpha) << 1) != 0u;
  unsigned long long m = on ? __builtin_amdgcn_ballot_w64(counted) : 0ull;
  asm volatile("" : "+s"(m));   // (a value from here on: the select is not carried into the loop)
  return m;
}

// this lane's share of L(x,u): its four state terms, its control's R and barrier terms.  `counted` = lane belongs to a
// rollout whose result is used (the wave-uniform barrier shortcut must not be vetoed by idle quads), as a lane mask the caller
// takes once, outside its loop: barrier_lanes(p, counted), which is empty where p has no barrier -- the term is then never added,
// as `if (p.barrier_alpha != 0.0f)` around it had it.
// SHORTCUT = false (the line search's candidates, round 8): no test at all.  A wave of candidates takes the short cut in 8 % of its
// steps (the large alphas push a control below 20 / beta almost at once), so the two compares, two ballots, the
// multiply, the mask arithmetic and the branch that splits the step's block bought next to nothing there.  The term is computed in
// every lane and kept where the problem has a barrier (`counted` non-empty: barrier_lanes' bit test; one select on a scalar
// condition).  The same bits: that is what makes the short cut exact.
template <bool SHORTCUT = true>
__device__ __forceinline__ float lane_stage_cost(const quattro_model_params& p, const LaneConst& L, const float* xo,
                                                 float uo, unsigned long long counted) {
  float c = 0.0f;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float d = xo[g] - L.xr[g];
    c = fmaf(L.qw[g] * d, d, c);
  }
  c = fmaf(L.rj * uo, uo, c);
  if constexpr (!SHORTCUT) {
    const float sp = qt_softplus(-uo, p.barrier_beta);
    const float cb = fmaf(p.barrier_alpha, sp * sp, c);
    float cost = counted != 0ull ? cb : c;
    // (pinned to its step: without the branch nothing holds the cost in place, and left alone the compiler sinks the four costs
    //  of the unrolled steps to the end of the group behind the last step's recurrence -- 25 registers more and the line search
    //  34.4 instead of 32.5 us, against 33.2 with the test)
    asm volatile("" : "+v"(cost));
    return cost;
  }
  // exact shortcut, per lane (see qt_stage_cost): with beta*u > 20 the lane's barrier term is below
  // alpha * 4.25e-18 / beta^2; when that is under half an ulp of c the fmaf below returns c unchanged
  const float ib = 1.0f / p.barrier_beta;
  // (the wave-wide test as lane masks of the two raw compares combined on the scalar unit: `__all(a && b)` makes the
  // compiler materialise the conjunction as a 0/1 VGPR and compare it again)
  const unsigned long long big = __builtin_amdgcn_ballot_w64(p.barrier_beta * uo > 20.0f);
  const unsigned long long tiny = __builtin_amdgcn_ballot_w64(fabsf(p.barrier_alpha) * 4.25e-18f * ib * ib < c * 2.9e-8f);
  if ((counted & ~(big & tiny)) != 0ull) {
    const float sp = qt_softplus(-uo, p.barrier_beta);
    c = fmaf(p.barrier_alpha, sp * sp, c);
  }
  return c;
}

__device__ __forceinline__ float lane_final_cost(const LaneConst& L, const float* xo) {
  float c = 0.0f;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float d = xo[g] - L.xr[g];
    c = fmaf(L.qfw[g] * d, d, c);
  }
  return c;
}

// Where a wave's nominal data lives: the arrays of the wave's trajectories as wave-uniform buffer resources plus this lane's
// loop-invariant 32-bit byte offsets; the step is a SCALAR offset.  (Round 4: as 64-bit pointers per lane the four address
// computations were ~8 of a step's ~165 vector instructions, in a kernel that is bound by exactly those.)
// `wb` = the wave's first trajectory (wave-uniform), `li` = this lane's trajectory minus wb (0 for a lane that only runs along),
// `nwt` = trajectories a wave spans.
struct NomSrc {
  __amdgpu_buffer_rsrc_t rx, ru, rK, rk;
  int vx, vu, vK;
  __device__ __forceinline__ NomSrc(const LaneConst& L, const float* x_nom, const float* u_nom, const float* K, const float* k,
                                    int N, int wb, int li, int nwt) {
    const size_t w = (size_t)wb;
    rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x_nom) + w * (N + 1) * NX, 0, nwt * (N + 1) * NX * 4, 0x00020000);
    ru = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(u_nom) + w * N * NU, 0, nwt * N * NU * 4, 0x00020000);
    rK = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(K) + w * N * NU * NX, 0, nwt * N * NU * NX * 4, 0x00020000);
    rk = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(k) + w * N * NU, 0, nwt * N * NU * 4, 0x00020000);
    vx = 4 * (li * (N + 1) * NX + L.a);
    vu = 4 * (li * N * NU + L.j);
    vK = 4 * NX * (li * N * NU + L.j);
  }
};

// nominal data of one step as this lane needs it: own states, own control, own gain row
struct NomLane {
  float x[4], u, k;
  float4 K[3];
  __device__ __forceinline__ void load(const NomSrc& s, int t) {
#pragma unroll
    for (int g = 0; g < 4; ++g) x[g] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(s.rx, s.vx + 12 * g, t * (NX * 4), 0));
    u = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(s.ru, s.vu, t * (NU * 4), 0));
    k = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(s.rk, s.vu, t * (NU * 4), 0));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const auto q = __builtin_amdgcn_raw_buffer_load_b128(s.rK, s.vK + 16 * i, t * (NU * NX * 4), 0);
      K[i] = make_float4(__int_as_float(q[0]), __int_as_float(q[1]), __int_as_float(q[2]), __int_as_float(q[3]));
    }
  }
  // the same without the feed-forward term (a tracked plant step follows the nominal itself: k plays no part, `k` stays unset)
  __device__ __forceinline__ void load_track(const NomSrc& s, int t) {
#pragma unroll
    for (int g = 0; g < 4; ++g) x[g] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(s.rx, s.vx + 12 * g, t * (NX * 4), 0));
    u = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(s.ru, s.vu, t * (NU * 4), 0));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const auto q = __builtin_amdgcn_raw_buffer_load_b128(s.rK, s.vK + 16 * i, t * (NU * NX * 4), 0);
      K[i] = make_float4(__int_as_float(q[0]), __int_as_float(q[1]), __int_as_float(q[2]), __int_as_float(q[3]));
    }
  }
};

// REF (quattro_ilqr_solve_ref_f32, quattro_mpc_run_ref_f32): LaneConst::xr becomes a value of the STEP.  Where the rows of a wave's
// trajectories live, NomSrc's way: one wave-uniform buffer resource over the rows of the wave's trajectories ([nwt][R][12] from
// trajectory wb on), this lane's loop-invariant byte offset (its trajectory, its axis), and the step's row — qt_ref_row, the
// clamp — as a SCALAR offset.  (Offsets are 32-bit: the C entries bound R.)
struct NoRefSrc {
  static constexpr bool ON = false;
  __device__ __forceinline__ NoRefSrc() {}
  __device__ __forceinline__ NoRefSrc(const LaneConst&, const RefRows&, int, int, int) {}
};
struct RefSrc {
  static constexpr bool ON = true;
  __amdgpu_buffer_rsrc_t r;
  int v;
  RefRows rr;
  __device__ __forceinline__ RefSrc(const LaneConst& L, const RefRows& rr_, int wb, int li, int nwt) : rr(rr_) {
    r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rr_.rows) + (size_t)wb * rr_.R * NX, 0, nwt * rr_.R * NX * 4, 0x00020000);
    v = 4 * (li * rr_.R * NX + L.a);
  }
};
// this lane's four components (a, 3 + a, 6 + a, 9 + a) of the row that horizon step t reads; every quad of a trajectory — all
// candidates of a line search — loads the same four
struct RefLane {
  float xr[4];
  __device__ __forceinline__ void load(const RefSrc& s, int t) {
    const int row = qt_ref_row(s.rr, t);
#pragma unroll
    for (int g = 0; g < 4; ++g) xr[g] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(s.r, s.v + 12 * g, row * (NX * 4), 0));
  }
  __device__ __forceinline__ void load(const NoRefSrc&, int) {}
};
// L with the step's reference in place of the problem's: a copy in registers, so that lane_stage_cost / lane_final_cost (and with
// them every kernel without rows) stay as they are
template <class RefS>
__device__ __forceinline__ LaneConst with_ref(const LaneConst& L, const RefLane& rl) {
  if constexpr (RefS::ON) {
    LaneConst Lt = L;
#pragma unroll
    for (int g = 0; g < 4; ++g) Lt.xr[g] = rl.xr[g];
    return Lt;
  } else {
    return L;
  }
}

// Stores.  One 16-byte store per lane per step: the x' row (12 floats, state 3g+a in lane a / register g) is transposed
// inside the quad so that lane j < 3 holds x'[4j .. 4j+3] and lane 3 holds (u'_0..u'_3).  Per-state dword stores were
// 5 requests of 12-16 bytes per quad and step; at 2048 waves that request rate, not bandwidth, cost 45 us per line
// search once the caches were cold.  Stores are predicated by `en`, never branched around a rollout: the DPP exchanges
// and the wave-uniform barrier shortcut need every quad of the wave on the same path, so idle quads (alpha slot >=
// n_alpha, inactive trajectory) run along on valid data and simply do not store.
__device__ __forceinline__ float4 gather_quarter(const LaneConst& L, const QuadU& U, const float* xn) {
  const float t0 = L.sel(xn[0], xn[1], xn[2]);                                       // own lane: states 0, 4, 8
  const float t1 = quad_perm<QT_QP(1, 2, 0, 3)>(L.sel(xn[3], xn[0], xn[1]));         // states 1, 5, 9
  const float t2 = quad_perm<QT_QP(2, 0, 1, 3)>(L.sel(xn[2], xn[3], xn[0]));         // states 2, 6, 10
  const float t3 = L.sel(xn[1], xn[2], xn[3]);                                       // own lane: states 3, 7, 11
  const bool l3 = L.j == 3;
  return make_float4(l3 ? U.c[0] : t0, l3 ? U.c[1] : t1, l3 ? U.c[2] : t2, l3 ? U.c[3] : t3);
}

struct NoStore {
  static constexpr bool ALL_U = false;
  __device__ __forceinline__ void operator()(const LaneConst&, int, const QuadU&, const float*) const {}
};
struct ArrayStore {     // x_new [N+1][12], u_new [N][4]
  static constexpr bool ALL_U = true;
  float* base;          // lanes 0..2: x_new + 12 + 4j (row t+1 at + 12 t); lane 3: u_new (row t at + 4 t)
  int stride;
  bool en;
  __device__ __forceinline__ ArrayStore(const LaneConst& L, float* xo, float* uo, bool en_)
      : base(L.j < 3 ? xo + NX + 4 * L.j : uo), stride(L.j < 3 ? NX : NU), en(en_) {}
  __device__ __forceinline__ void operator()(const LaneConst& L, int t, const QuadU& U, const float* xnext) const {
    const float4 v = gather_quarter(L, U, xnext);
    if (en) *reinterpret_cast<float4*>(base + (size_t)t * stride) = v;
  }
};
// Candidate records of the fused line search [t][CS], AXIS-major: lane a < 3 writes its own four states as they sit in
// its registers — floats 4a .. 4a+3 = x'[a], x'[3+a], x'[6+a], x'[9+a] — and lane 3 the four controls: no transposition
// inside the quad on the serial chain (it was ~16 of a step's ~175 vector instructions, for all six candidates); the
// one candidate that is accepted is put back into natural order by the copy that commits it.
struct ScratchStore {
  static constexpr bool ALL_U = true;
  float* s;
  bool en, l3;
  __device__ __forceinline__ ScratchStore(const LaneConst& L, float* rec, bool en_) : s(rec + 4 * L.j), en(en_), l3(L.j == 3) {}
  __device__ __forceinline__ void operator()(const LaneConst&, int t, const QuadU& U, const float* xnext) const {
    const float4 v = make_float4(l3 ? U.c[0] : xnext[0], l3 ? U.c[1] : xnext[1], l3 ? U.c[2] : xnext[2], l3 ? U.c[3] : xnext[3]);
    if (en) *reinterpret_cast<float4*>(s + (size_t)t * CS) = v;
  }
};

// 12-term dot product K_j,: dx with dx spread over the axis lanes: state 3g+a lives in lane a, register g.
// Written as v_fmac_f32_dpp (the broadcast is the DPP modifier of the multiply-add's first source): the compiler does
// not fold a quad_perm move into v_fmac, and 12 extra moves plus their hazard no-ops were 9 % of a step.  The leading
// s_nop covers the VALU-write -> DPP-read hazard for dx, which the hazard recogniser cannot see inside inline asm.
__device__ __forceinline__ float gain_dot(const float4* K, const float* dx, float acc) {
#define QT_FD(k, d, l) "v_fmac_f32_dpp %0, " d ", " k " quad_perm:[" l "," l "," l "," l "] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
  asm volatile("s_nop 1\n\t"
               QT_FD("%5", "%1", "0") QT_FD("%6", "%1", "1") QT_FD("%7", "%1", "2")
               QT_FD("%8", "%2", "0") QT_FD("%9", "%2", "1") QT_FD("%10", "%2", "2")
               QT_FD("%11", "%3", "0") QT_FD("%12", "%3", "1") QT_FD("%13", "%3", "2")
               QT_FD("%14", "%4", "0") QT_FD("%15", "%4", "1") QT_FD("%16", "%4", "2")
               : "+v"(acc)
               : "v"(dx[0]), "v"(dx[1]), "v"(dx[2]), "v"(dx[3]), "v"(K[0].x), "v"(K[0].y), "v"(K[0].z), "v"(K[0].w),
                 "v"(K[1].x), "v"(K[1].y), "v"(K[1].z), "v"(K[1].w), "v"(K[2].x), "v"(K[2].y), "v"(K[2].z), "v"(K[2].w));
#undef QT_FD
  return acc;
}

// Tracked plant steps by a quad, stated ONCE for this lane mapping: track_quad_kernel (rollout_quad.hip) and the persistent loop's
// mpc_advance (solve_quad.hip) both run this function, which is why they agree bit for bit.  For j < steps:
//   u_app = u_nom[j] (+ K[j] (x - x_nom[j]) with feedback),   x <- f_plant(x, u_app) (+ disturbance[j])
// with f_plant the quadrotor step of L (lane_const_plant) under the plant's integrator — a wave-uniform runtime branch, so the
// callers need no template dimension for it.  xh: the quad's state, in and out.  Lane j stores u_app_j at urows[j * NU], an axis
// lane its four states of row j + 1 at xrows[(j + 1) * NX + 3 g]; dist (or NULL): this lane's element of the first step's
// disturbance row, the next step's dist_stride floats on.  Every quad of the wave runs along (the DPP exchanges need it); only
// `live` ones store.  No implicit fma contraction: the two translation units must round alike.
__device__ __forceinline__ void quad_track_body(const LaneConst& L, const bool rk4, const bool feedback, const NomSrc& nom,
                                                float* xh, const int steps, const float* __restrict__ dist,
                                                const size_t dist_stride, const bool live, float* __restrict__ xrows,
                                                float* __restrict__ urows) {
#pragma clang fp contract(off)
  for (int j = 0; j < steps; ++j) {
    NomLane nb;
    nb.load_track(nom, j);
    float ua = nb.u;
    if (feedback) {
      float dx[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) dx[g] = xh[g] - nb.x[g];
      ua = gain_dot(nb.K, dx, ua);
    }
    const QuadU U(ua);
    float xn[4];
    if (rk4) quad_step<true>(L, xh, U, xn);
    else quad_step<false>(L, xh, U, xn);
    if (dist != nullptr) {
#pragma unroll
      for (int g = 0; g < 4; ++g) xn[g] += dist[(size_t)j * dist_stride + 3 * g];
    }
    if (live) {
      urows[(size_t)j * NU] = ua;
      if (L.j < 3) {
#pragma unroll
        for (int g = 0; g < 4; ++g) xrows[(size_t)(j + 1) * NX + 3 * g] = xn[g];
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) xh[g] = xn[g];
  }
}

// One closed-loop rollout by a quad.  Returns this LANE's partial of sum_t L + Lf (fp64); quad_sum() gives the total.
// What a step issues (round 6, Euler, gfx950, by the SQ counters per wave over N = 50, prologue and commit included): the line
// search 136 vector / 19 scalar instructions and 5.4 branches per step (6 798 / 963 / 269 per wave), simulate_quad_body's step
// 80 / 11 / 4.1 (4 008 / 565 / 205); of the line search's ~120 in the loop body 12 are K dx, ~16 the stage cost with its short
// cut, ~48 the rate function including its in-quad broadcasts, 4 + 1 the record.  Round 8, SHORTCUT = false (the stand-alone line
// search, without the barrier test): 130 vector / 16 scalar instructions per step (6 505 / 814 per wave) and one branch fewer in
// every step; the stage cost is ~12 of the loop body's instructions.
// PRIO: the state recurrence of a step at wave priority 1, the stage cost, the store and the loads that hang off it at 0
// (rollout_quad.hip); without it the step runs at the caller's priority throughout and adds its stage cost ahead of the rate function.
// RefS = RefSrc: stage and terminal cost against the step's row.  The row's four floats are requested with the step's nominal data,
// PF steps ahead, and the terminal row before the loop: the cost is not on the recurrence, and neither are its loads.
// SHORTCUT: lane_stage_cost's -- false for the Euler line-search candidates (linesearch_quad_kernel, rollout_quad_kernel, the
// persistent loop's line-search phase); rollout_quad.hip has the numbers.
template <bool RK4, int PF, bool PRIO, bool SHORTCUT, class Store, class RefS = NoRefSrc>
__device__ __forceinline__ double quad_rollout_closed(const quattro_model_params& p, const LaneConst& L,
                                                      const NomSrc& src, float alpha, int N, bool counted, Store store,
                                                      const RefS& ref = RefS()) {
  // nominal data is requested PF steps ahead (PF register buffers, loop unrolled by PF): the loads come from HBM / the
  // far cache (K was written by the sweep, 39 MB per 4096 trajectories) and a step is only ~0.5 us of issue.  PF = 4 in
  // the stand-alone kernels; 2 inside the device-resident solve loop, where the gains were written by the same workgroup a
  // moment ago (L2-resident) and the loop shares its 128 registers with the sweep.
  const unsigned long long counted_mask = barrier_lanes(p, counted);
  NomLane nb[PF];
#pragma unroll
  for (int d = 0; d < PF; ++d) nb[d].load(src, d < N ? d : N - 1);
  RefLane rl[PF], rlN;
#pragma unroll
  for (int d = 0; d < PF; ++d) rl[d].load(ref, d < N ? d : N - 1);
  rlN.load(ref, N);
  float xh[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) xh[g] = nb[0].x[g];
  double J = 0.0;
  auto step = [&](const NomLane& b, const RefLane& rt, int t) __attribute__((always_inline)) {
    if constexpr (PRIO) __builtin_amdgcn_s_setprio(1);
    float dx[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) dx[g] = xh[g] - b.x[g];
    const float du = gain_dot(b.K, dx, b.k);
    const float uh = fmaf(alpha, du, b.u);
    if constexpr (!PRIO) J += (double)lane_stage_cost<SHORTCUT>(p, with_ref<RefS>(L, rt), xh, uh, counted_mask);
    float xnext[4];
    const QuadU U(uh, Store::ALL_U);
    quad_step<RK4>(L, xh, U, xnext);
    if constexpr (PRIO) {
      __builtin_amdgcn_s_setprio(0);
      J += (double)lane_stage_cost<SHORTCUT>(p, with_ref<RefS>(L, rt), xh, uh, counted_mask);
    }
    store(L, t, U, xnext);
#pragma unroll
    for (int g = 0; g < 4; ++g) xh[g] = xnext[g];
  };
  int t = 0;
  for (; t + PF <= N; t += PF) {
#pragma unroll
    for (int d = 0; d < PF; ++d) {
      step(nb[d], rl[d], t + d);
      nb[d].load(src, t + d + PF < N ? t + d + PF : N - 1);
      rl[d].load(ref, t + d + PF < N ? t + d + PF : N - 1);
    }
  }
#pragma unroll
  for (int d = 0; d < PF - 1; ++d)
    if (t + d < N) step(nb[d], rl[d], t + d);          // wave-uniform tail (N % PF steps)
  J += (double)lane_final_cost(with_ref<RefS>(L, rlN), xh);
  return J;
}

// simulate: quad per trajectory, 16 trajectories per wave
// `gid` = 4 * trajectory + lane-in-quad; `live` = this quad has a trajectory to roll out (idle quads run along on
// trajectory 0 without storing: the DPP exchanges and the wave-uniform barrier shortcut need every quad on the same path)
// PHYS: the quad's physical parameters are row b of model_phys (lane_const_phys); the cost stays p's
// REF: the cost of step t against the row of rr that step reads (RefSrc), prefetched with the controls, RING steps ahead
// RING (round 9; SIM_RING in the stand-alone kernel): the controls sit in a register ring this many steps deep, the loop unrolled to match.  At two steps ahead
// (rounds 2 - 8) a control was waited for a step and a half after its load issued, ~700 cycles of cover against the 900 of a miss
// to HBM -- and a 128-byte line holds eight steps of a trajectory's controls, so every wave of a launch misses together every
// eighth step.  A step issues one control load and four state stores, so the wait for a control is vmcnt(5 SIM_RING - 1 or so):
// inside the counter's six bits up to a ring of twelve.
// The persistent loops run this body once per solve, as one phase among many in a kernel that is short of registers: they keep
// RING = 2 and ENTRY = false, which compiles to the code of rounds 6 - 8 (the same instructions but for a commuted operand or two; a
// ring of four there, with the other bodies' prologues, cost ten closed-loop control steps 0.7 %).
// ENTRY: the body is a kernel's whole, its prologue on every wave's critical path -- x0's row is written after the prologue's wait.
constexpr int SIM_RING = 4;
template <bool RK4, bool PHYS = false, bool REF = false, int RING = 2, bool ENTRY = false>
__device__ __forceinline__ void simulate_quad_body(const quattro_model_params& p, const float* __restrict__ x0,
                                                   const float* __restrict__ u, int N, float* __restrict__ x,
                                                   double* __restrict__ cost, const int gid, const bool live,
                                                   const float* __restrict__ model_phys = nullptr, const RefRows& rr = RefRows{}) {
  using RefS = std::conditional_t<REF, RefSrc, NoRefSrc>;
  const int b = gid >> 2;
  const size_t bb = live ? b : 0;
  const LaneConst L = lane_const_of<PHYS>(p, model_phys, bb, gid & 3);
  float* xo = x + bb * (N + 1) * NX + L.a;
  float xh[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) xh[g] = x0[bb * NX + 3 * g + L.a];
  const bool writer = live && L.j < 3;
  const int bw = __builtin_amdgcn_readfirstlane(b);         // the wave's first trajectory (gid grows with the lane)
  const __amdgpu_buffer_rsrc_t rsx =
      __builtin_amdgcn_make_buffer_rsrc(x + (size_t)bw * (N + 1) * NX, 0, 16 * (N + 1) * NX * 4, 0x00020000);
  // (a lane that writes nothing: an offset the range check drops, with room for the stores' immediate offsets above it -- the
  //  resource is 16 (N + 1) 48 bytes, far below 2^30)
  const int vox = writer ? 4 * ((b - bw) * (N + 1) * NX + L.a) : 0x40000000;
  // Round 6: the controls come the same way, NomSrc's: the wave's 16 trajectories as one wave-uniform resource, this lane's
  // loop-invariant byte offset, the (clamped) step as a SCALAR offset -- a 64-bit address per lane and step was a vector shift-add
  // and two scalar instructions of a kernel that pays for every issue slot.  An idle quad reads the wave's first trajectory's.
  // The step is carried as a byte offset of its own (`ou`, RING steps ahead, one add and one min per step), and the resource's
  // flag word is pinned in a register of its own: sharing rsx's, the compiler copied it into place again in every step.
  int uflags = 0x00020000;
  asm("" : "+s"(uflags));
  const __amdgpu_buffer_rsrc_t rsu =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(u) + (size_t)bw * N * NU, 0, 16 * N * NU * 4, uflags);
  const int vou = 4 * ((live ? b - bw : 0) * N * NU + L.j);
  const int ou_last = (N - 1) * (NU * 4);
  auto control = [&](int ofs) __attribute__((always_inline)) {     // the control at byte offset ofs of the row, clamped to the last
    return __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsu, vou, ofs < ou_last ? ofs : ou_last, 0));
  };
  if constexpr (!ENTRY) {
    if (writer) {
#pragma unroll
      for (int g = 0; g < 4; ++g) xo[3 * g] = xh[g];
    }
  }
  const RefS ref(L, rr, bw, live ? b - bw : 0, 16);
  RefLane rq[RING], rN;
  qt_static_for<RING>([&](auto d) __attribute__((always_inline)) { rq[d].load(ref, d < N ? d : 0); });   // (a row past the horizon is requested and never read: row 0 will do, also for N = 0)
  rN.load(ref, N);
  double J = 0.0;
  const unsigned long long live_mask = barrier_lanes(p, live);
  float uq[RING];
  qt_static_for<RING>([&](auto d) __attribute__((always_inline)) { uq[d] = control(d * (NU * 4)); });
  int ou = RING * (NU * 4);
  auto step = [&](float ut, const RefLane& rt, int t) __attribute__((always_inline)) {
    J += (double)lane_stage_cost(p, with_ref<RefS>(L, rt), xh, ut, live_mask);
    float xn[4];
    const QuadU U(ut);
    quad_step<RK4>(L, xh, U, xn);
    // Round 4: the lane's four states go out as they sit in its registers (x[t+1][3g + a], four dword stores).  The in-quad
    // transposition that made one 16-byte store per lane of them (gather_quarter: two DPP permutes and ten selects) was 27 %
    // of this kernel by an ablation build (since removed) — a lone wave per SIMD pays for every instruction it issues,
    // and at 256 waves the request rate that made dword stores expensive in the line search (2048 waves) is no issue.
    // ... through buffer stores: the wave's 16 trajectories are one wave-uniform resource, the row a scalar offset, and a lane
    // that writes nothing (the quad's control lane, a lane past the batch) carries an out-of-range offset the range check drops.
    // No exec-mask branch around the stores — which matters beyond the branch: with the stores behind a branch the compiler's
    // wait-count pass must assume they may NOT have been issued, and the wait for the next control (loaded BEFORE them) comes out
    // as vmcnt(1) instead of the full count — every step then waits for the previous step's stores to be acknowledged.
    // (round 6: the row is ONE scalar offset and the four states' 0 / 12 / 24 / 36 ride in the instruction's immediate field; as
    //  part of the scalar offset each store had a scalar add of its own per step)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_int(xn[g]), rsx, vox + 12 * g, (t + 1) * (NX * 4), 0);
#pragma unroll
    for (int g = 0; g < 4; ++g) xh[g] = xn[g];
  };
  // Everything loaded so far (the lane's constants, x0, the first RING controls: ONE batch of requests, round 9) lands HERE,
  // through the builtin the compiler's wait-count pass understands: otherwise the loop header inherits those loads as pending and
  // every step carries the decreasing `s_waitcnt vmcnt(4..1)` the first one needs — which from the second step on wait for the
  // PREVIOUS step's four state stores to be acknowledged (the counter retires in order): a store round trip on the chain of every step.
  // (the empty asm "uses" x0 and the prefetched controls, so their loads cannot sink below the wait)
  if constexpr (ENTRY) {
    asm volatile("" : "+v"(xh[0]), "+v"(xh[1]), "+v"(xh[2]), "+v"(xh[3]));
#pragma unroll
    for (int d = 0; d < RING; ++d) asm volatile("" : "+v"(uq[d]));      // (a loop: an asm operand does not capture in a lambda)
  } else {
    static_assert(ENTRY || RING == 2, "the persistent loops' form");
    asm volatile("" : "+v"(uq[0]), "+v"(uq[1]));
  }
  if constexpr (REF) {
    if constexpr (ENTRY) {
#pragma unroll
      for (int d = 0; d < RING; ++d)
#pragma unroll
        for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(rq[d].xr[g]));
#pragma unroll
      for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(rN.xr[g]));
    } else {
#pragma unroll
      for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(rq[0].xr[g]), "+v"(rq[1].xr[g]), "+v"(rN.xr[g]));
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0f70);        // vmcnt(0), nothing else
  // Row 0 of x is x0, written AFTER that wait (round 9; it used to be requested before it, so that the loop was entered only once
  // the store had been acknowledged: a third round trip behind the arguments and x0).  Stores carry no register the loop reads,
  // so pending ones cost its waits nothing.  Through the steps' resource: a lane that writes nothing is dropped by the range check.
  if constexpr (ENTRY) {
#pragma unroll
    for (int g = 0; g < 4; ++g) __builtin_amdgcn_raw_buffer_store_b32(__float_as_int(xh[g]), rsx, vox + 12 * g, 0, 0);
  }
  int t = 0;
  for (; t + (RING - 1) < N; t += RING) {
    qt_static_for<RING>([&](auto d) __attribute__((always_inline)) {
      step(uq[d], rq[d], t + d);
      uq[d] = control(ou);
      ou += NU * 4;
      rq[d].load(ref, t + d + RING < N ? t + d + RING : N - 1);
    });
  }
  qt_static_for<RING - 1>([&](auto d) __attribute__((always_inline)) {
    if (t + d < N) step(uq[d], rq[d], t + d);          // wave-uniform tail (N % RING steps)
  });
  J += (double)lane_final_cost(with_ref<RefS>(L, rN), xh);
  J = quad_sum(J);
  if (live && L.j == 0 && cost != nullptr) cost[b] = J;
}

// Fused line search: 8 candidate quads = 32 lanes per trajectory, 2 trajectories per wave.  Every candidate leaves its
// (x', u') in the scratch; after the ballot the trajectory's 32 lanes copy the accepted candidate over the nominal.
// `gid` = 32 * trajectory + lane-in-trajectory for this lane (the 64 lanes of a wave hold two consecutive trajectories);
// `force` treats every trajectory as active whatever its flag says (fixed-iteration benchmarking runs).
// PHYS: the candidates of trajectory b roll out under row b of model_phys (lane_const_phys); the cost stays p's
// REF: every candidate's cost against the rows of rr (quad_rollout_closed with a RefSrc)
// SHORTCUT: lane_stage_cost's barrier test -- the callers switch it off for Euler (rollout_quad.hip)
// ENTRY: the body is a kernel's whole (linesearch_quad_kernel): the requests that need the arguments alone go out in one batch ahead
// of the early exit.  The persistent loops, where this is one phase of an iteration, keep the order of rounds 2 - 8.
template <bool RK4, int PF, bool PRIO, bool PHYS = false, bool REF = false, bool SHORTCUT = true, bool ENTRY = false>
__device__ __forceinline__ void linesearch_quad_body(const quattro_model_params& p, float* x_nom, float* u_nom,
                                                     const float* __restrict__ K, const float* __restrict__ k,
                                                     const AlphaList& al, int n_alpha, int B, int N, double tol,
                                                     double* cost, int32_t* __restrict__ alpha_idx, int32_t* active,
                                                     int32_t* iters, float* __restrict__ scratch, const int gid,
                                                     const bool force, const float* __restrict__ model_phys = nullptr,
                                                     const RefRows& rr = RefRows{}) {
  const int b = gid >> 5, ai = (gid >> 2) & 7, l32 = gid & 31;
  // Round 9 (ENTRY): whatever the arguments alone address is requested in ONE batch, ahead of the early exit -- the trajectory's flag,
  // its cost so far (as a value: which trajectory a lane works on is known only with the flag, but a live lane's is b) and, where the
  // lane constants are the problem's, their lane-indexed entries.  The flag used to be fetched and waited for alone, then J0, then
  // the constants.  The nominal data is NOT requested here: its addresses take `live`, and a wave with no live trajectory (most waves
  // of a solve's late iterations) leaves below without having asked for any of it.
  bool live;
  double J0 = 0.0;
  LaneConst L;
  if constexpr (ENTRY) {
    const int bc = b < B ? b : 0;
    // (the flag from an address that is valid with or without an array of flags -- without, a word of the cost, read and ignored: a
    //  load behind `active != nullptr` sits in a block of its own and is waited for there, alone.  A lane past the batch reads
    //  trajectory 0's flag and cost, which that trajectory's wave may be writing at the same moment: an unsynchronised read whose
    //  value is dropped -- `live` is false for such a lane whatever it read)
    const int32_t* const fp = active != nullptr ? active + bc : reinterpret_cast<const int32_t*>(cost + bc);
    const bool flag = (*fp != 0) | force | (active == nullptr);
    J0 = cost[bc];
    if constexpr (!PHYS) {
      L = lane_const(p, gid & 3);
      asm volatile("" : "+v"(L.rj));              // (the constant's load stays ahead of the exit, with the two above)
    }
    asm volatile("" : "+v"(J0));
    live = (b < B) && flag;
  } else {
    live = (b < B) && (force || active == nullptr || active[b < B ? b : 0] != 0);
  }
  if (!__any(live)) return;   // both trajectories of the wave converged / out of range: nothing to do (late iterations
                              // of a solve run mostly such waves)
  const bool mine = live && ai < n_alpha;
  const size_t bb = live ? b : 0;
  const int aa = mine ? ai : 0;
  if constexpr (!ENTRY || PHYS) L = lane_const_of<PHYS>(p, model_phys, bb, gid & 3);
  if constexpr (ENTRY) J0 = live ? J0 : 0.0;
  float* xn = x_nom + bb * (N + 1) * NX;
  float* un = u_nom + bb * N * NU;
  const int wb = __builtin_amdgcn_readfirstlane(b);    // the wave's first trajectory (gid grows with the lane; wb < B: a lane is live)
  const NomSrc nom(L, x_nom, u_nom, K, k, N, wb, live ? b - wb : 0, 2);
  float* sc = scratch + (bb * 8) * (size_t)N * CS;     // this trajectory's 8 candidate slots
  float alpha = al.a[0];
#pragma unroll
  for (int i = 1; i < QUATTRO_MAX_ALPHAS; ++i) alpha = (aa == i) ? al.a[i] : alpha;
  if constexpr (!ENTRY) J0 = live ? cost[bb] : 0.0;
  using RefS = std::conditional_t<REF, RefSrc, NoRefSrc>;
  double J = quad_rollout_closed<RK4, PF, PRIO, SHORTCUT>(p, L, nom, alpha, N, mine, ScratchStore(L, sc + (size_t)aa * N * CS, mine),
                                                RefS(L, rr, wb, live ? b - wb : 0, 2));
  J = quad_sum(J);
  const bool ok = mine && (J <= J0);     // false for NaN, like the reference's comparison
  // first accepted alpha among this trajectory's 8 quads (bit 4*ai of its 32-bit half of the ballot)
  const unsigned long long bal = __ballot(ok);
  const int lane = threadIdx.x & 63;
  const unsigned grp = (unsigned)((bal >> (lane & 32)) & 0x11111111ull);
  const int first = grp ? ((__ffs((int)grp) - 1) >> 2) : -1;
  if (live && first >= 0) {
    // The candidate records were stored by OTHER lanes of this wave.  For a workgroup-scope release gfx950 emits
    // s_waitcnt lgkmcnt(0) only (the CU is assumed to perform its vector-memory operations in order); the explicit vmcnt(0)
    // makes the hand-over independent of that assumption: every scratch store of this wave is complete (written through to
    // L2) before any lane loads a record (one wait per line search).
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // Lane pair (e, e + 16) of the trajectory's 32 lanes takes element e of two consecutive records: e < 12 is state e
    // (natural order) read from its axis-major slot 4 (e % 3) + e / 3, e >= 12 is control e - 12.  Stores are contiguous
    // runs of 12 (4) floats per record; the reads stay inside the record's 64 bytes.
    const float* src = sc + (size_t)first * N * CS;
    const int e = l32 & 15, half = l32 >> 4;
    const bool isx = e < 12;
    const int slot = isx ? 4 * (e % 3) + e / 3 : e;
    float* dst = isx ? xn + NX + e : un + (e - 12);
    const int dstride = isx ? NX : NU;
    // COPY_U records per lane in flight: all of a block's loads are issued before its first store (a dword load / wait / store
    // per record, as the plain loop compiles, is a round trip to L2 per four records: 10 % of the kernel by ablation).  25 = the
    // headline's N = 50 in ONE round (13 took two, behind the wait above); the rollout's registers are dead here, there is room.
    constexpr int COPY_U = 25;
    for (int t0 = half; t0 < N; t0 += 2 * COPY_U) {
      float v[COPY_U];
#pragma unroll
      for (int q = 0; q < COPY_U; ++q) {
        const int t = t0 + 2 * q;
        v[q] = src[(size_t)(t < N ? t : t0) * CS + slot];
      }
#pragma unroll
      for (int q = 0; q < COPY_U; ++q) {
        const int t = t0 + 2 * q;
        if (t < N) dst[(size_t)t * dstride] = v[q];
      }
    }
    if (ai == first && L.j == 0) {
      cost[b] = J;
      if (active != nullptr && fabs(J0 - J) < tol) active[b] = 0;   // converged
    }
  }
  if (live && l32 == 0) {
    if (alpha_idx != nullptr) alpha_idx[b] = first;
    if (iters != nullptr) iters[b] += 1;
    if (first < 0 && active != nullptr) active[b] = 0;            // no improving step
  }
}

}  // namespace
