// Host stand-ins for the two device functions csrc/dual.h takes from models_device.h, so that the header's algebra can be
// compiled and checked on a CPU (tests/test_dual_host_cpu.py).  Plain libm: no quadrant reduction of our own, no hardware
// exp / log; the large-argument conventions of the device qt_sincos are not reproduced here.
#pragma once
#include <math.h>

static inline void qt_sincos(float x, float* s, float* c) {
  *s = sinf(x);
  *c = cosf(x);
}
static inline float qt_softplus(float z, float beta) {
  const float bz = beta * z;
  return (fmaxf(bz, 0.0f) + log1pf(expf(-fabsf(bz)))) / beta;
}
