"""csrc/rk4.h compiled for the host (QT_RK4_HOST) and applied to a linear rate function x' = A x + B u, where classic RK4 with
zero-order-hold u is known in closed form: with Z = h A,

    x_next = Phi x + Gamma u,   Phi = I + Z + Z^2/2 + Z^3/6 + Z^4/24,   Gamma = h (I + Z/2 + Z^2/6 + Z^3/24) B,

and the n + m tangent columns of the step are the columns of [Phi | Gamma].  rk4_step, rk4_points and rk4_tangent run in fp32
(-O1 -ffp-contract=off: only the header's own fmaf calls are fused); the reference is fp64 numpy on the fp32-rounded inputs.

Tolerance 5e-6 of the largest reference entry: an output ends a chain of about 60 fp32 roundings (four rate evaluations of
n + m fused multiply-adds each, the stage updates, the final combination), each at most 2^-24 of an intermediate no larger
than about twice the output scale when ||Z|| <= 1 (60 * 2 * 2^-24 = 7e-6 only if every rounding went the same way; measured
errors are around 1e-7).  The inputs are scaled to ||Z||_2 = 0.95 so that every term of Phi matters: the test asserts, from
numpy alone, that the smallest one (Z^4/24) has an entry above 1e-3, two hundred times the tolerance — a dropped or
mis-weighted stage cannot pass.  (With h = 0.01 and a unit-scale A that term is 2e-8 and a wrong scheme would.)"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "quattro-transformer-ilqr_amd", "csrc")
CLANG = "/opt/rocm/llvm/bin/clang++"            # the host compiler that ships with the device toolchain
TOL = 5e-6
H = 0.1
Z_NORM = 0.95

DRIVER = r"""
#define QT_RK4_HOST
#include "rk4.h"
#include <stdio.h>
#include <vector>

// stdin: n m dt A[n][n] B[n][m] x[n] u[m] as hex floats -> one line: x_next[n], the stage points [4][n], columns [n + m][n]
template <int N, int M>
static int run() {
  float dt, A[N][N], B[N][M], x[N], u[M];
  if (scanf("%a", &dt) != 1) return 1;
  for (auto& r : A) for (auto& v : r) if (scanf("%a", &v) != 1) return 1;
  for (auto& r : B) for (auto& v : r) if (scanf("%a", &v) != 1) return 1;
  for (auto& v : x) if (scanf("%a", &v) != 1) return 1;
  for (auto& v : u) if (scanf("%a", &v) != 1) return 1;
  auto lin = [&](const float* xs, const float* us, float* k) {
    for (int i = 0; i < N; ++i) {
      float s = 0.0f;
      for (int j = 0; j < N; ++j) s = fmaf(A[i][j], xs[j], s);
      for (int a = 0; a < M; ++a) s = fmaf(B[i][a], us[a], s);
      k[i] = s;
    }
  };
  float xn[N], xp[4][N];
  rk4_step<N>(dt, x, xn, [&](int, const float* xs, float* k) { lin(xs, u, k); });
  rk4_points<N>(dt, x, xp, [&](int, const float* xs, float* k) { lin(xs, u, k); });
  for (float v : xn) printf("%a ", v);
  for (auto& r : xp) for (float v : r) printf("%a ", v);
  for (int j = 0; j < N + M; ++j) {
    float dx0[N], du[M], col[N];
    for (int i = 0; i < N; ++i) dx0[i] = i == j ? 1.0f : 0.0f;
    for (int a = 0; a < M; ++a) du[a] = N + a == j ? 1.0f : 0.0f;
    rk4_tangent<N>(dt, dx0, col, [&](int, const float* dxs, float* dk) { lin(dxs, du, dk); });
    for (float v : col) printf("%a ", v);
  }
  printf("\n");
  return 0;
}

int main() {
  int n, m;
  if (scanf("%d %d", &n, &m) != 2) return 1;
  if (n == 4 && m == 1) return run<4, 1>();
  if (n == 12 && m == 4) return run<12, 4>();
  return 2;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    work = tmp_path_factory.mktemp("rk4_host")
    (work / "driver.cpp").write_text(DRIVER)
    r = subprocess.run([CLANG, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I", CSRC, str(work / "driver.cpp"),
                        "-o", str(work / "driver")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(h, A, B, x, u):
        n, m = B.shape
        vals = np.concatenate([[h], A.ravel(), B.ravel(), x, u])
        text = f"{n} {m}\n" + " ".join(float(v).hex() for v in vals) + "\n"
        out = subprocess.run([str(work / "driver")], input=text, capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr[-4000:]
        t = np.array([float.fromhex(s) for s in out.stdout.split()])
        assert t.size == n + 4 * n + (n + m) * n
        return t[:n], t[n:5 * n].reshape(4, n), t[5 * n:].reshape(n + m, n).T       # x_next, points, [d x_next / d z] (n x (n + m))
    return run


def _problem(n, m, seed):
    """fp32-rounded inputs, as fp64 arrays: A with ||h A||_2 = Z_NORM (symmetric part plus half as much skew part, so that the
    powers of Z do not decay faster than the norm says), B, x, u of unit scale."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    A = (G + G.T) / 2 + 0.5 * (G - G.T) / 2
    A *= Z_NORM / (H * np.linalg.norm(A, 2))
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    return float(f32(H)), f32(A), f32(rng.standard_normal((n, m))), f32(rng.standard_normal(n)), f32(rng.standard_normal(m))


@pytest.mark.parametrize("n,m,seed", [(4, 1, 41), (12, 4, 124)])
def test_rk4_header_matches_closed_form_on_linear_system(driver, n, m, seed):
    h, A, B, x, u = _problem(n, m, seed)
    Z = h * A
    I = np.eye(n)
    P = [np.linalg.matrix_power(Z, k) for k in range(5)]
    # the condition on the inputs: every term of Phi is large against the tolerance
    assert 0.5 <= np.linalg.norm(Z, 2) <= 1.0
    terms = [P[1], P[2] / 2, P[3] / 6, P[4] / 24]
    assert min(np.max(np.abs(t)) for t in terms) > 1e-3, [np.max(np.abs(t)) for t in terms]
    Phi = I + sum(terms)
    Gam = h * (I + P[1] / 2 + P[2] / 6 + P[3] / 24) @ B
    f = lambda xs: A @ xs + B @ u
    pts = [x, x + 0.5 * h * f(x)]
    pts.append(x + 0.5 * h * f(pts[1]))
    pts.append(x + h * f(pts[2]))
    pts = np.array(pts)

    xn, xp, J = driver(h, A, B, x, u)
    ref_x, ref_J = Phi @ x + Gam @ u, np.hstack([Phi, Gam])
    err_x = np.max(np.abs(xn - ref_x)) / np.max(np.abs(ref_x))
    err_p = np.max(np.abs(xp - pts)) / np.max(np.abs(pts))
    err_J = np.max(np.abs(J - ref_J)) / np.max(np.abs(ref_J))
    print(f"n = {n}, m = {m}: ||Z||_2 = {np.linalg.norm(Z, 2):.3f}, smallest term of Phi {np.max(np.abs(terms[3])):.1e}; "
          f"error / largest entry: x_next {err_x:.1e}, stage points {err_p:.1e}, [Phi | Gamma] {err_J:.1e}  (bound {TOL})")
    assert err_x <= TOL and err_p <= TOL and err_J <= TOL, (err_x, err_p, err_J)
    assert np.array_equal(xp[0], x)                          # the first point is the state itself
