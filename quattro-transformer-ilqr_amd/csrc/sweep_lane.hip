// Cart-pole-shaped problems (n = 4, m = 1): linearisation + Riccati-like sweep, one stand-alone launch.
//
// Arithmetic replaced: _compute_dynamics_jacobians / _compute_cost_derivatives / _finite_diff_*_final +
// iLQR_TF.backward_pass / backward_pass_segment (quattro_ilqr_tf/quattro_ilqr_tf.py:149-275, :290-317, :336-364).
//
// A 4 x 4 value function, a 4 x 5 [A | B] and a scalar Q_uu are ~150 multiply-adds per step: handing such a problem a
// whole 64-lane wave (sweep_generic_kernel: LDS-staged blocks, seven workgroup barriers per step) spends the step on
// synchronisation, not on arithmetic — 42 us for B = 1024, N = 50, plus a 13 us linearisation launch in front.  Here a
// trajectory gets one 16-lane DPP row, four trajectories per wave (cartpole_body.h, which the device-resident solve loop
// shares): the rows form their step records with the SAME device-model code the record kernels use
// (EulerRecord::fill_const / fill_state, or the RK4 forward-mode columns) and run the recursion on them with the generic
// kernel's formulas term for term (the gains agree with quattro_linearize_f32 + quattro_riccati_sweep_f32 through
// ROWMAJOR records to fp32 round-off).  No record buffer and no workgroup barrier.
#include "cartpole_body.h"

namespace {

// sixteen lanes (one DPP row) per trajectory, four trajectories per wave: cartpole_body.h
template <bool RK4>
__global__ __launch_bounds__(QT_WAVE) void sweep16_cartpole_kernel(const quattro_model_params p, const float* __restrict__ x,
                                                                    const float* __restrict__ u, int B, int N, int t_start,
                                                                    float reg, float* __restrict__ Kout,
                                                                    float* __restrict__ kout, int32_t* __restrict__ status,
                                                                    const int32_t* __restrict__ active, int k_rows) {
  __shared__ __attribute__((aligned(16))) float s_stage[4 * cp16::STAGE_FLOATS];
  const int lane = threadIdx.x;
  const int b = blockIdx.x * 4 + (lane >> 4);
  const bool live = b < B && (active == nullptr || active[b < B ? b : 0] != 0);
  if (!__any(live)) return;
  sweep16_cartpole_body<RK4>(p, x, u, N, t_start, reg, Kout, kout, status, b, live, lane, s_stage + (lane >> 4) * cp16::STAGE_FLOATS,
                             k_rows);
}

}  // namespace

int quattro_launch_sweep_lane_cartpole(const quattro_model_params& p, const float* x, const float* u, int B, int N,
                                       int t_start, float reg, float* K, float* k, int k_rows, int32_t* status,
                                       const int32_t* active, hipStream_t stream) {
  const int blocks = (B + 3) / 4;                          // sixteen lanes per trajectory
  if (p.integrator == QUATTRO_INTEGRATOR_RK4)
    hipLaunchKernelGGL(sweep16_cartpole_kernel<true>, dim3(blocks), dim3(QT_WAVE), 0, stream, p, x, u, B, N, t_start, reg, K, k,
                       status, active, k_rows);
  else
    hipLaunchKernelGGL(sweep16_cartpole_kernel<false>, dim3(blocks), dim3(QT_WAVE), 0, stream, p, x, u, B, N, t_start, reg, K,
                       k, status, active, k_rows);
  return hipGetLastError() == hipSuccess ? QUATTRO_OK : QUATTRO_ERR_LAUNCH;
}
