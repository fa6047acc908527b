"""One problem family for user-compiled models, written once for any (n, m), on the grid of dimensions at which the library of a
user model takes another compile-time path; its fp64 restatement, the seeded inputs, the bounds and the mutants that the tests
must be able to tell apart.  A plain helper module (like tests/param_cases.py and tests/dual_probe.py), used by

  * scripts/prebuild_user_models.py (the 13 libraries of the grid),
  * tests/test_user_grid_cpu.py (density, conditioning and pivot swaps of the reference, the fp32 emulation of the reference
    formulas against the bounds, every mutant's multiple, header compile and layout),
  * tests/test_user_grid_gpu.py (every kernel of a user model's library against this reference).

The three C++ bodies loop over NX / NU, so the same source text serves every grid point; a library depends on the bodies and
(n, m) only: integrator, dt and every parameter are run-time fields, so both integrators and both variants share a library.

The family.  With C (n x n), D (n x m) matrices of eighths in [0.25, 1], sx = C x / n, sv = D u / m:

    rate_i = P0 sin(sx_i) + P1 tanh(sv_i) + P2 exp(sx_i / 2) softplus_2(sv_i) + P3 sqrt(1 + sv_i^2) / (2 + cos(sx_i)) - x_i
    L      = default_stage_cost + 2 softplus_1(z / 2) + sum_ai E_ai x_i u_a + sum_a u_a u_{a+1} / 8 + P4 u_0 sum_{a>=1} b_a u_a
    Lf     = default_final_cost + (a . x)^2 / 2,        z = a . x + b . u

a alternates in sign (|a_i| in [0.5, 1]), b is positive, E (1/128 .. 5/128) carries the sign of a.  Every partial derivative of the rate with
respect to sx_i and sv_i is positive over the range the inputs reach (the quotient's, whose sign is sin(sx)'s, is a tenth of
the others), so every entry of A and B is bounded away from zero; the rank-one Hessian of the softplus term makes l_xx, l_uu and
l_ux dense, the bilinear term has the sign of the softplus term's entry, and (a . x)^2 makes V_xx(N) dense.  Variant `convex`
has P4 = 0, P5 = 1.  u_0 enters the rate and z as P5 u_0: variant `pivot` (m >= 2) sets r[0] = 0, P4 = 0.6 and P5 = 1 / 128, which
makes u_0 nearly the slack of tests/test_user_model_gpu.py (Q_uu[0][0] is a few reg) without emptying its column of B: Q_uu + reg I
is indefinite, its partial pivoting swaps rows, and an elimination without pivoting loses its digits in fp32.

Inputs are rounded to fp32 and handed back as fp64: the device and the reference start from the same numbers.
"""
import numpy as np

# (n, m) -> what it is the edge of
GRID = {
    (1, 1): "NZ = 2, generic, scalar everything",
    (4, 1): "NZ = 5: just below the tile rule, generic",
    (3, 2): "NZ = 5: just below the tile rule, generic",
    (5, 1): "NZ = 6: first tile shape",
    (2, 4): "NZ = 6: first tile shape, m > n",
    (4, 4): "NZ = 8: last LPI = 8; all float4 paths",
    (7, 2): "NZ = 9: first LPI = 16; all scalar paths",
    (12, 4): "NZ = 16: last LPI = 16, last tile",
    (13, 4): "NZ = 17: first LPI = 32; n > 12, generic",
    (12, 5): "NZ = 17; m > 4, generic",
    (1, 8): "m >> n, generic, n + 1 = 2 gain columns",
    (16, 1): "widest state with one control",
    (16, 8): "the maximum, with a dense cost",
}
POINTS = tuple(GRID)
TILE_POINTS = ((5, 1), (2, 4), (4, 4), (7, 2), (12, 4))          # the table of the issue, stated independently of is_tile()
VARIANTS = ("convex", "pivot")
INTEGRATORS = ("euler", "rk4")
BATCHES = (1, 3)
HORIZONS = (1, 2, 9)
B_FULL, N_FULL = 3, 10
DT = 0.25
ALPHAS = (1.0, 0.5, 0.25, 0.1, 0.05, 0.01)
REG = 1e-6
# A second sweep at a regularisation that is visible (K_reg, k_reg): what tells Q_uu from Q_uu + reg I in the V update, which at
# reg = 1e-6 moves nothing.  Variant `convex` only: an indefinite Q_uu may have an eigenvalue next to -REG_BIG.
REG_BIG = 5e-2


def is_tile(n, m):
    """The rule of csrc/capi.hip: quattro_model_layout and csrc/solve_user.hip: TILE."""
    return n <= 12 and m <= 4 and n + m >= 6


def lanes_per_item(n, m):
    nz = n + m
    return 8 if nz <= 8 else 16 if nz <= 16 else 32


def variants(n, m):
    return VARIANTS if m >= 2 else ("convex",)


def cases():
    """Every (n, m, variant, integrator) of the grid."""
    return [(n, m, v, i) for (n, m) in POINTS for v in variants(n, m) for i in INTEGRATORS]


def case_id(c):
    return f"{c[0]}x{c[1]}-{c[2]}-{c[3]}"


# ---------------------------------------------------------------------------------------------------------------- the bodies
HELPERS = """
__device__ __forceinline__ float g_cx(int i, int j) { return (2 + (3 * i + 5 * j) % 7) * 0.125f; }
__device__ __forceinline__ float g_cu(int i, int a) { return (2 + (2 * i + 3 * a) % 5) * 0.125f; }
__device__ __forceinline__ float g_sg(int i) { return (i & 1) ? -1.0f : 1.0f; }
__device__ __forceinline__ float g_a(int i) { return g_sg(i) * (4 + (3 * i) % 5) * 0.125f; }
__device__ __forceinline__ float g_b(int a) { return (3 + (2 * a) % 5) * 0.125f; }
__device__ __forceinline__ float g_e(int a, int i) { return g_sg(i) * (1 + (3 * a + 2 * i) % 5) * 0.0078125f; }
"""
RATE = """
const float sn = (float)(1.0 / NX), sm = (float)(1.0 / NU);
const T u0 = u[0] * P[5];
#pragma nounroll
for (int i = 0; i < NX; ++i) {
  T sx(0.0f), sv(0.0f);
#pragma nounroll
  for (int j = 0; j < NX; ++j) sx = sx + x[j] * g_cx(i, j);
#pragma nounroll
  for (int a = 0; a < NU; ++a) sv = sv + (a == 0 ? u0 : u[a]) * g_cu(i, a);
  sx = sx * sn;
  sv = sv * sm;
  xd[i] = sin(sx) * P[0] + tanh(sv) * P[1] + exp(sx * 0.5f) * softplus(sv, 2.0f) * P[2]
        + sqrt(sv * sv + 1.0f) / (cos(sx) + 2.0f) * P[3] - x[i];
}
"""
STAGE = """
T c = default_stage_cost<T>(p, x, u);
T z(0.0f);
#pragma nounroll
for (int i = 0; i < NX; ++i) z = z + x[i] * g_a(i);
#pragma nounroll
for (int a = 0; a < NU; ++a) z = z + (a == 0 ? u[0] * P[5] : u[a]) * g_b(a);
c = c + softplus(z * 0.5f, 1.0f) * 2.0f;
#pragma nounroll
for (int a = 0; a < NU; ++a) {
#pragma nounroll
  for (int i = 0; i < NX; ++i) c = c + x[i] * u[a] * g_e(a, i);
}
#pragma nounroll
for (int a = 0; a + 1 < NU; ++a) c = c + u[a] * u[a + 1] * 0.125f;
#pragma nounroll
for (int a = 1; a < NU; ++a) c = c + u[0] * u[a] * (P[4] * g_b(a));
return c;
"""
FINAL = """
T s(0.0f);
#pragma nounroll
for (int i = 0; i < NX; ++i) s = s + x[i] * g_a(i);
return default_final_cost<T>(p, x) + s * s * 0.5f;
"""


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def coefficients(n, m):
    """The integer-built coefficient arrays of HELPERS (all exact in fp32): C (n, n), D (n, m), a (n,), b (m,), E (m, n)."""
    i, j, a = np.arange(n), np.arange(n), np.arange(m)
    sg = np.where(i % 2 == 1, -1.0, 1.0)
    return dict(C=(2 + (3 * i[:, None] + 5 * j[None, :]) % 7) * 0.125, D=(2 + (2 * i[:, None] + 3 * a[None, :]) % 5) * 0.125,
                a=sg * (4 + (3 * i) % 5) * 0.125, b=(3 + (2 * a) % 5) * 0.125,
                E=sg[None, :] * (1 + (3 * a[:, None] + 2 * i[None, :]) % 5) * 0.0078125,
                sn=float(np.float32(1.0 / n)), sm=float(np.float32(1.0 / m)))


PHYS = (0.9, 0.6, 0.35, 0.25)        # P[0..3], pairwise distinct; P[4] is the variant's coupling
PIVOT_COUPLING = 0.6
PIVOT_SLACK = 1.0 / 128.0     # P[5]: what is left of u[0] in the rate and in z (1 in variant `convex`)


def params(n, m, variant):
    """Every run-time field of the model as fp32-representable fp64, pairwise distinct within each vector."""
    i, a = np.arange(n), np.arange(m)
    r = 0.25 + 0.05 * a
    p4, p5 = 0.0, 1.0
    if variant == "pivot":
        assert m >= 2
        # r[0] = 0 as in the slack problem, and the other weights small (0.03, 0.04, ...): the diagonal of Q_uu + reg I stays below
        # the couplings beside it after the first elimination step too, so that later pivots swap as well (m >= 3)
        r = 0.02 + 0.01 * a
        r[0] = 0.0
        p4, p5 = PIVOT_COUPLING, PIVOT_SLACK
    return dict(P=_f32(PHYS + (p4, p5)), q=_f32(0.3 + 0.04 * i), r=_f32(r), qf=_f32(1.0 + 0.15 * i),
                x_ref=_f32(0.4 * np.sin(1.0 + 1.7 * i)), dt=DT)


def model(n, m, variant="convex", integrator="rk4", p=None):
    """The compiled model of a grid point (one library per (n, m): hipcc cross-compiles without a GPU)."""
    import quattro_ilqr_amd as q
    p = params(n, m, variant) if p is None else p
    return q.compile_model(f"grid{n}x{m}", n, m, rate=RATE, stage_cost=STAGE, final_cost=FINAL, helpers=HELPERS, dt=p["dt"],
                           integrator=integrator, phys=tuple(p["P"]), q=p["q"], r=p["r"], qf=p["qf"], x_ref=p["x_ref"])


def all_models():
    """The 13 models of the grid (their libraries are independent of one another: four are compiled at a time)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=4) as ex:
        return list(ex.map(lambda nm: model(*nm), POINTS))


# Seeds of the inputs, by (n, m, variant).  What variant `pivot` needs (every trajectory has a step whose partial pivoting swaps
# at p = 0 and, for m >= 3, at a p >= 1 of the same inversion; tests/test_user_grid_cpu.py asserts it) was searched on the CPU over
# the weights r and the couplings above; with those chosen, the first seed gives it at every point, so one pinned seed serves all.
SEED_DEFAULT = 3
SEEDS = {(n, m, v): SEED_DEFAULT for (n, m) in GRID for v in VARIANTS}


def inputs(n, m, variant, N, B=B_FULL):
    """x0 (B, n), u (B, N, m): the first B rows and N steps of one seeded batch, so that B = 1 is row 0 of the larger batch."""
    assert B <= B_FULL and N <= N_FULL
    rng = np.random.default_rng(1000 * n + 10 * m + SEEDS.get((n, m, variant), SEED_DEFAULT))
    p = params(n, m, variant)
    x0 = p["x_ref"] + 0.3 * rng.standard_normal((B_FULL, n))
    u = 0.5 + 0.3 * rng.standard_normal((B_FULL, N_FULL, m))
    return _f32(x0[:B]), _f32(u[:B, :N])


# ---------------------------------------------------------------------------------------------------------------- the reference
def _softplus(z, beta):
    """(max(beta z, 0) + log(1 + exp(-|beta z|))) / beta, as csrc/dual.h; branches on the real part (complex step)."""
    bz = z * beta
    pos = np.real(bz) > 0
    return (bz * pos + np.log1p(np.exp(np.where(pos, -bz, bz)))) / beta


class Problem:
    """The family at one (n, m) with parameter dict p, as NumPy functions over arrays with any leading axes.  dtype float32
    emulates the device's storage and arithmetic (the formulas as written here, not the kernels' order of operations)."""

    def __init__(self, n, m, p, integrator="rk4", dtype=np.float64):
        self.n, self.m, self.p, self.integrator, self.dtype = n, m, p, integrator, dtype
        c = coefficients(n, m)
        cast = (lambda v: np.asarray(v, dtype=dtype)) if dtype != np.float64 else (lambda v: np.asarray(v, dtype=np.float64))
        self.C, self.D, self.a, self.b, self.E = (cast(c[k]) for k in ("C", "D", "a", "b", "E"))
        self.sn, self.sm = dtype(c["sn"]), dtype(c["sm"])
        self.P, self.q, self.r, self.qf, self.x_ref = (cast(p[k]) for k in ("P", "q", "r", "qf", "x_ref"))
        self.dt = dtype(p["dt"])
        self.u_scale = cast(np.concatenate([self.P[5:6], np.ones(m - 1)]))      # u[0] enters the rate and z through P[5]
        self.h = dtype  # scalar constructor: constants take the working precision

    def rate(self, x, u):
        h = self.h
        sx = (x @ self.C.T) * self.sn
        sv = ((u * self.u_scale) @ self.D.T) * self.sm
        P = self.P
        return (np.sin(sx) * P[0] + np.tanh(sv) * P[1] + np.exp(sx * h(0.5)) * _softplus(sv, h(2.0)) * P[2]
                + np.sqrt(sv * sv + h(1.0)) / (np.cos(sx) + h(2.0)) * P[3] - x)

    def step(self, x, u, integrator=None, hold_x=False):
        """hold_x: the mutant whose stages 2-4 see the step's first state instead of the advanced one."""
        dt, h = self.dt, self.h
        k1 = self.rate(x, u)
        if (integrator or self.integrator) == "euler":
            return x + k1 * dt
        adv = (lambda k, c: x) if hold_x else (lambda k, c: x + k * c)
        k2 = self.rate(adv(k1, h(0.5) * dt), u)
        k3 = self.rate(adv(k2, h(0.5) * dt), u)
        k4 = self.rate(adv(k3, dt), u)
        return x + (k1 + k2 * h(2.0) + k3 * h(2.0) + k4) * (dt / h(6.0))

    def L(self, x, u):
        h = self.h
        d = x - self.x_ref
        c = np.sum(d * d * self.q, axis=-1) + np.sum(u * u * self.r, axis=-1)
        z = x @ self.a + (u * self.u_scale) @ self.b
        c = c + _softplus(z * h(0.5), h(1.0)) * h(2.0)
        c = c + np.sum((u @ self.E) * x, axis=-1)
        if self.m > 1:
            c = c + np.sum(u[..., :-1] * u[..., 1:], axis=-1) * h(0.125)
            c = c + u[..., 0] * (u[..., 1:] @ self.b[1:]) * self.P[4]
        return c

    def Lf(self, x):
        d = x - self.x_ref
        s = x @ self.a
        return np.sum(d * d * self.qf, axis=-1) + s * s * self.h(0.5)

    # ---- one trajectory at a time, for oracle.ilqr.optimize
    def f1(self, x, u):
        return self.step(x, u)

    # ---- rollouts (costs are summed in fp64, as on the device)
    def total_cost(self, xs, u):
        return (np.sum(np.asarray(self.L(xs[:, :-1], u), dtype=np.float64), axis=1)
                + np.asarray(self.Lf(xs[:, -1]), dtype=np.float64))

    def rollout(self, x0, u, hold_x=False):
        xs = [np.asarray(x0, dtype=self.dtype)]
        u = np.asarray(u, dtype=self.dtype)
        for t in range(u.shape[1]):
            xs.append(self.step(xs[-1], u[:, t], hold_x=hold_x))
        xs = np.stack(xs, axis=1)
        return xs, self.total_cost(xs, u)

    def closed_loop(self, x0, x_nom, u_nom, k, K, alpha, about_next=False, alpha_on_k_only=False, hold_x=False):
        """u'_t = u_t + alpha (k_t + K_t (x'_t - x_t)), x'_{t+1} = f(x'_t, u'_t) -> x', u', cost.  The two flags are mutants."""
        dt = self.dtype
        x_nom, u_nom, k, K = (np.asarray(v, dtype=dt) for v in (x_nom, u_nom, k, K))
        al = dt(alpha)
        xs, us = [np.asarray(x0, dtype=dt)], []
        for t in range(u_nom.shape[1]):
            dx = xs[-1] - x_nom[:, t + 1 if about_next else t]
            fb = np.einsum("bij,bj->bi", K[:, t], dx)
            du = k[:, t] * al + fb if alpha_on_k_only else (k[:, t] + fb) * al
            us.append(u_nom[:, t] + du)
            xs.append(self.step(xs[-1], us[-1], hold_x=hold_x))
        xs, us = np.stack(xs, axis=1), np.stack(us, axis=1)
        return xs, us, self.total_cost(xs, us)

    # ---- exact derivatives (fp64 only)
    def records(self, xs, u, integrator=None):
        """Blocks about the nominal in the layout of oracle.ilqr.riccati_sweep_batched: first order by complex step, second
        order by Richardson-extrapolated central differences of the complex-step gradient (tests/test_user_grid_cpu.py holds
        them to 1e-9 of the block scale against the closed form, hessian_closed_form)."""
        n = self.n
        z = np.concatenate([xs[:, :-1], u], axis=-1)
        F = complex_step_jac(lambda w: self.step(w[..., :n], w[..., n:], integrator=integrator), z)
        gL = lambda w: complex_step_jac(lambda v: self.L(v[..., :n], v[..., n:])[..., None], w)[..., 0, :]
        g, H = gL(z), richardson_hessian(gL, z)
        gF = lambda w: complex_step_jac(lambda v: self.Lf(v)[..., None], w)[..., 0, :]
        xN = xs[:, -1]
        return dict(A=F[..., :n], B=F[..., n:], lx=g[..., :n], lu=g[..., n:], lxx=H[..., :n, :n], luu=H[..., n:, n:],
                    lux=H[..., n:, :n], VxN=gF(xN), VxxN=richardson_hessian(gF, xN))

    def hessian_closed_form(self, xs, u):
        """l_xx, l_uu, l_ux, V_xx(N) written out by hand: an independent check of the numerical second derivatives."""
        n, m = self.n, self.m
        z = 0.5 * (xs[:, :-1] @ self.a + (u * self.u_scale) @ self.b)
        s = 1.0 / (1.0 + np.exp(-z))
        w = (0.5 * s * (1.0 - s))[..., None, None]
        lxx = w * np.outer(self.a, self.a) + np.diag(2.0 * self.q)
        lux = w * np.outer(self.b * self.u_scale, self.a) + self.E
        T = np.diag(2.0 * self.r)
        for a in range(m - 1):
            T[a, a + 1] += 0.125; T[a + 1, a] += 0.125
        for a in range(1, m):
            T[0, a] += self.P[4] * self.b[a]; T[a, 0] += self.P[4] * self.b[a]
        luu = w * np.outer(self.b * self.u_scale, self.b * self.u_scale) + T
        VxxN = np.broadcast_to(np.diag(2.0 * self.qf) + np.outer(self.a, self.a), (xs.shape[0], n, n))
        return dict(lxx=lxx, luu=luu, lux=lux, VxxN=VxxN)


def complex_step_jac(fun, z, h=1e-30):
    """fun: (..., nz) -> (..., k), analytic.  -> (..., k, nz), exact to fp64 round-off."""
    nz = z.shape[-1]
    zp = z[..., None, :].astype(np.complex128) + 1j * h * np.eye(nz)
    return np.swapaxes(np.imag(fun(zp)) / h, -1, -2)


def richardson_hessian(grad, z, h=2e-3):
    """grad: (..., nz) -> (..., nz), exact.  Central differences at h and h / 2, extrapolated (error O(h^4)), symmetrised."""
    nz = z.shape[-1]
    def central(step):
        e = step * np.eye(nz)
        return (grad(z[..., None, :] + e) - grad(z[..., None, :] - e)) / (2 * step)
    H = (4.0 * central(0.5 * h) - central(h)) / 3.0
    return 0.5 * (H + np.swapaxes(H, -1, -2))


# ---------------------------------------------------------------------------------------------------------------- the sweep
def invert_bubble(a, pivot=True):
    """Gauss-Jordan inverse of (..., m, m) in a's dtype with the bubble-order partial pivoting of csrc/sweep_generic_body.h:
    invert_gj (row r > p is swapped up whenever it is larger than what row p holds by then), or with none (the tile sweep's
    elimination).  -> inverse, swaps (..., m) = how many rows were swapped up at pivot p."""
    a = np.array(a)
    m = a.shape[-1]
    w = np.broadcast_to(np.eye(m, dtype=a.dtype), a.shape).copy()
    swaps = np.zeros(a.shape[:-2] + (m,), dtype=np.int64)
    for p in range(m):
        if pivot:
            for r in range(p + 1, m):
                sw = np.abs(a[..., r, p]) > np.abs(a[..., p, p])
                swaps[..., p] += sw
                s3 = sw[..., None]
                for M in (a, w):
                    rp, rr = M[..., p, :].copy(), M[..., r, :].copy()
                    M[..., p, :] = np.where(s3, rr, rp)
                    M[..., r, :] = np.where(s3, rp, rr)
        ip = a.dtype.type(1.0) / a[..., p, p]
        a[..., p, :] *= ip[..., None]
        w[..., p, :] *= ip[..., None]
        for r in range(m):
            if r != p:
                f = a[..., r, p].copy()
                a[..., r, :] -= f[..., None] * a[..., p, :]
                w[..., r, :] -= f[..., None] * w[..., p, :]
    return w, swaps


def unpivoted_pivot_ratio(quu):
    """(..., m, m) -> (...): the smallest pivot of the elimination without pivoting relative to the diagonal entry it started
    as.  The tile sweep flags QUATTRO_TRAJ_ILLCOND where this is <= 1e-6 (csrc/sweep_tile16.hip)."""
    a = np.array(quu, dtype=np.float64)
    m = a.shape[-1]
    worst = np.full(a.shape[:-2], np.inf)
    for p in range(m):
        piv = a[..., p, p].copy()
        worst = np.minimum(worst, piv / np.abs(np.asarray(quu)[..., p, p]))
        a[..., p, :] /= piv[..., None]
        for r in range(m):
            if r != p:
                a[..., r, :] -= a[..., r, p].copy()[..., None] * a[..., p, :]
    return worst


def sweep(d, reg=REG, dtype=np.float64, inverse="linalg", reg_in_update=False, symmetrise=True, info=None):
    """oracle.ilqr.riccati_sweep_batched with the inverse to choose ("linalg", "pivot" = invert_bubble, "nopivot") and two
    mutant switches.  info: a dict that receives quu (B, S, m, m) = Q_uu + reg I and swaps (B, S, m)."""
    c = lambda key: np.asarray(d[key]).astype(dtype)
    A, Bm, lx, lu, lxx, luu, lux, Vx, Vxx = (c(k) for k in ("A", "B", "lx", "lu", "lxx", "luu", "lux", "VxN", "VxxN"))
    Bt, S, n, m = A.shape[0], A.shape[1], A.shape[2], Bm.shape[3]
    k_out, K_out = np.zeros((Bt, S, m), dtype=dtype), np.zeros((Bt, S, m, n), dtype=dtype)
    quu_all, swaps_all = np.zeros((Bt, S, m, m)), np.zeros((Bt, S, m), dtype=np.int64)
    eye = np.eye(m, dtype=dtype)
    T = lambda M: np.swapaxes(M, -1, -2)
    mv = lambda M, v: np.einsum("bij,bj->bi", M, v)
    for s in reversed(range(S)):
        At, Bt_ = T(A[:, s]), T(Bm[:, s])
        Qx, Qu = lx[:, s] + mv(At, Vx), lu[:, s] + mv(Bt_, Vx)
        Qxx = lxx[:, s] + At @ Vxx @ A[:, s]
        Qux = lux[:, s] + Bt_ @ Vxx @ A[:, s]
        Quu = luu[:, s] + Bt_ @ Vxx @ Bm[:, s]
        Qr = Quu + dtype(reg) * eye
        quu_all[:, s] = Qr
        if inverse == "linalg":
            W = np.linalg.inv(Qr)
        else:
            W, swaps_all[:, s] = invert_bubble(Qr, pivot=inverse == "pivot")
        k, K = -mv(W, Qu), -(W @ Qux)
        k_out[:, s], K_out[:, s] = k, K
        Qv = Qr if reg_in_update else Quu
        Vx = Qx + mv(T(K) @ Qv, k) + mv(T(K), Qu) + mv(T(Qux), k)
        Vxx = Qxx + T(K) @ Qv @ K + T(K) @ Qux + T(Qux) @ K
        if symmetrise:
            Vxx = dtype(0.5) * (Vxx + T(Vxx))
    if info is not None:
        info.update(quu=quu_all, swaps=swaps_all)
    return k_out, K_out


# ---------------------------------------------------------------------------------------------------------------- bounds
# No bound is new.  Each quantity takes the bound the suite already asserts for it: param_cases.BOUNDS for the rollouts,
# 1e-6 max(1, max|block|) per record entry (test_user_model_derivative_records_are_exact), per-step 2e-5 for K and 5e-5 for k
# (test_tile_sweep_on_rowmajor_records_of_any_dims...), 2e-4 on x for a whole solve (the chain test).
RECORD_NAMES = ("A", "B", "lx", "lu", "lxx", "luu", "lux", "VxN", "VxxN")
BOUNDS = dict(sim_x=2e-6, sim_cost=2e-6, cl_x=1e-5, cl_u=1e-5, cl_cost=1e-5, K=2e-5, k=5e-5, K_reg=2e-5, k_reg=5e-5,
              **{name: 1e-6 for name in RECORD_NAMES})
SOLVE_X_BOUND = 2e-4
FAMILIES = dict(rollout=("sim_x", "sim_cost", "cl_x", "cl_u", "cl_cost"), records=RECORD_NAMES, gains=("K", "k", "K_reg", "k_reg"))
ALL = ("rollout", "records", "gains")

# The error of the reference formulas evaluated in NumPy float32 on the same inputs, against fp64: worst over every case, batch
# and horizon of the grid (tests/test_user_grid_cpu.py recomputes them and holds each to a quarter of its bound).
FP32_EMULATION = dict(sim_x=1.3e-7, sim_cost=1.4e-7, cl_x=1.0e-7, cl_u=2.2e-7, cl_cost=1.9e-7, K=8.5e-7, k=2.3e-6)


def _per_step(a, b, floor):
    """Worst per-step relative Frobenius error of (B, S, ...) arrays over the batch: conftest.per_step_rel / per_step_rel_floor."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    a, b = a.reshape(a.shape[0], a.shape[1], -1), b.reshape(b.shape[0], b.shape[1], -1)
    den = np.linalg.norm(b, axis=2)
    if floor:
        den = np.maximum(den, 0.01 * np.maximum(den.max(axis=1, keepdims=True), 1e-300))
    else:
        den = np.where(den > 0, den, 1.0)
    return float(np.max(np.linalg.norm(a - b, axis=2) / den))


def error(name, got, ref):
    """The error measure the bound of `name` applies to.
    sim_x, cl_x, cl_u: per component of every step, over max(1, the largest component of that trajectory) -- the states of one
      step are coupled through a dense Jacobian, so a component's fp32 error scales with the state, not with itself (a
      component that passes through zero keeps the error its neighbours give it).  A leading alpha axis is folded into the batch.
    *_cost: relative, per trajectory.   Records: per entry over max(1, max|block|), per (b, t) block.
    K: per step, relative Frobenius; k: the same with the denominator floored at 1 % of the trajectory's largest step."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if name.endswith("cost"):
        return float(np.max(np.abs(got - ref) / np.abs(ref)))
    if name in ("sim_x", "cl_x", "cl_u"):
        got, ref = got.reshape((-1,) + got.shape[-2:]), ref.reshape((-1,) + ref.shape[-2:])
        scale = np.maximum(1.0, np.max(np.abs(ref), axis=(1, 2), keepdims=True))
        return float(np.max(np.abs(got - ref) / scale))
    if name in ("K", "K_reg"):
        return _per_step(got, ref, floor=False)
    if name in ("k", "k_reg"):
        return _per_step(got, ref, floor=True)
    lead = 1 if name in ("VxN", "VxxN") else 2
    g, r = got.reshape(got.shape[:lead] + (-1,)), ref.reshape(ref.shape[:lead] + (-1,))
    return float(np.max(np.max(np.abs(g - r), axis=-1) / np.maximum(1.0, np.max(np.abs(r), axis=-1))))


# ---------------------------------------------------------------------------------------------------------------- evaluation
def evaluate(n, m, variant, integrator, N, B=B_FULL, mutant=None, about=None, dtype=np.float64):
    """Every quantity the GPU tests compare, as the reference gives it, or as mutant `mutant` of it does.
    about: dict(nom=, K=, k= [, rec=]) -- linearise and close the loop about this nominal with these gains (and sweep these
    records) instead of the evaluation's own: a mutant is evaluated about the true nominal with the true gains, as a wrong kernel
    is; the float32 emulation (dtype: rollouts in float32, the sweep in float32 with the pivoted inverse of invert_gj) and its
    fp64 counterpart start from the same fp32-rounded nominal, records and gains, as the device and its reference do."""
    mut = MUTANTS[mutant] if mutant else {}
    about = about or {}
    p = params(n, m, variant)
    if "params" in mut:
        mut["params"](p)
    pr = Problem(n, m, p, integrator, dtype)
    x0, u = inputs(n, m, variant, N, B)
    ro = mut.get("rollout", {})
    xs, J = pr.rollout(x0, u, hold_x=ro.get("hold_x", False))
    out = dict(sim_x=xs, sim_cost=J)
    nom = np.asarray(about.get("nom", xs), dtype=np.float64)
    if "rec" in about:
        rec = about["rec"]
    else:
        p64 = Problem(n, m, p, integrator)
        rec = p64.records(nom, u, integrator=mut.get("integrator"))
        if "records" in mut:
            mut["records"](rec, p64, nom, u)
    out.update(rec)
    sw = dict(mut.get("sweep", {}))
    post = sw.pop("post", None)
    sw_dtype = np.float32 if mut.get("fp32") else dtype
    if sw_dtype != np.float64:
        sw.setdefault("inverse", "pivot")
    info = {}
    for tag, reg in ((("", REG), ("_reg", REG_BIG)) if variant == "convex" else (("", REG),)):
        k, K = sweep(rec, reg=reg, dtype=sw_dtype, info=info if tag == "" else None, **sw)
        if post:
            k, K = post(k, K)
        out["k" + tag], out["K" + tag] = k, K
    out["quu"], out["swaps"] = info["quu"], info["swaps"]
    gk, gK = about.get("k", out["k"]), about.get("K", out["K"])
    cl = [pr.closed_loop(x0, nom, u, gk, gK, al, about_next=ro.get("about_next", False),
                         alpha_on_k_only=ro.get("alpha_on_k_only", False), hold_x=ro.get("hold_x", False)) for al in ALPHAS]
    out["cl_x"], out["cl_u"], out["cl_cost"] = (np.stack([c[i] for c in cl]) for i in range(3))
    return out


def rounded(ev):
    """The `about` of an evaluation with nominal, records and gains rounded to fp32: what a device hands its reference."""
    return dict(nom=_f32(ev["sim_x"]), K=_f32(ev["K"]), k=_f32(ev["k"]), rec={name: _f32(ev[name]) for name in RECORD_NAMES})


def is_noop(name, n, m, variant, integrator, N):
    """Where mutant `name` changes nothing (asserted, not skipped), or does not apply at all (`only`)."""
    mut = MUTANTS[name]
    if "only" in mut and not mut["only"](n, m, variant, integrator, N):
        return None
    return bool(mut.get("noop") and mut["noop"](n, m, variant, integrator, N))


# ---------------------------------------------------------------------------------------------------------------- mutants
def _swap(key, i, j):
    def fn(p):
        v = p[key].copy(); v[i], v[j] = v[j], v[i]; p[key] = v
    return fn


def _xref0(p):
    v = p["x_ref"].copy(); v[0] = 0.0; p["x_ref"] = v


def _rec_lux_zero(rec, pr, xs, u):
    rec["lux"] = np.zeros_like(rec["lux"])


def _rec_lux_shift(rec, pr, xs, u):
    rec["lux"] = np.roll(rec["lux"], -1, axis=-1)                  # l_ux[a, i] := l_ux[a, (i + 1) % n]


def _rec_B_rot(rec, pr, xs, u):
    rec["B"] = np.roll(rec["B"], 1, axis=-1)


def _rec_Vxx_default(rec, pr, xs, u):
    rec["VxxN"] = np.broadcast_to(np.diag(2.0 * pr.qf), rec["VxxN"].shape).copy()


def _rec_lxx_rows(rec, pr, xs, u):
    rec["lxx"] = np.roll(rec["lxx"], -1, axis=-2)                  # row j from seed j + 1


def _post_K_order(k, K):
    return k, np.swapaxes(K, -1, -2).reshape(K.shape)              # K written in (n, m) order into the (m, n) buffer


def _post_k_sign(k, K):
    return -k, K


# name -> dict(family, one of: params / records / integrator / sweep / rollout, noop(n, m, variant, integrator, N))
MUTANTS = {
    "l_ux zeroed": dict(family="records", records=_rec_lux_zero),
    "l_ux[a, (i+1) % n]": dict(family="records", records=_rec_lux_shift, noop=lambda n, m, v, i, N: n == 1),
    "B columns rotated": dict(family="records", records=_rec_B_rot, noop=lambda n, m, v, i, N: m == 1),
    "A, B of the Euler step under RK4": dict(family="records", integrator="euler", noop=lambda n, m, v, i, N: i == "euler"),
    "V_xx(N) of default_final_cost": dict(family="records", records=_rec_Vxx_default),
    "l_xx row j from seed j+1": dict(family="records", records=_rec_lxx_rows, noop=lambda n, m, v, i, N: n == 1),
    "Q_uu + reg I in the V update": dict(family="gains", sweep=dict(reg_in_update=True), noop=lambda n, m, v, i, N: N == 1,
                                         only=lambda n, m, v, i, N: v == "convex"),
    # V' = Q_xx + K^T Q_uu K + K^T Q_ux + Q_ux^T K is symmetric whatever K is once l_xx, l_uu and V_xx(N) are: with exact second
    # derivatives (the device's, and this reference's) the symmetrisation only removes round-off.  It mattered to the reference's
    # own finite differences, whose Hessians are not symmetric; here it is a no-op to fp64 round-off at every grid point.
    "V_xx not symmetrised": dict(family="gains", sweep=dict(symmetrise=False), noop=lambda n, m, v, i, N: True, roundoff=True),
    "K in (n, m) order": dict(family="gains", sweep=dict(post=_post_K_order), noop=lambda n, m, v, i, N: n == 1 or m == 1),
    "sign of k": dict(family="gains", sweep=dict(post=_post_k_sign)),
    "unpivoted fp32 elimination": dict(family="gains", sweep=dict(inverse="nopivot"), fp32=True,
                                       only=lambda n, m, v, i, N: v == "pivot"),
    "feedback about x_nom[t+1]": dict(family="rollout", rollout=dict(about_next=True)),
    # (N = 1: the only step starts on the nominal, x'_0 - x_0 = 0, and the feedback term is zero whatever multiplies it)
    "alpha on k only": dict(family="rollout", rollout=dict(alpha_on_k_only=True), noop=lambda n, m, v, i, N: N == 1),
    "RK4 stages 2-4 hold x": dict(family="rollout", rollout=dict(hold_x=True), noop=lambda n, m, v, i, N: i == "euler"),
    "P[0] <-> P[1]": dict(family=ALL, params=_swap("P", 0, 1)),
    "q[0] <-> q[n-1]": dict(family=ALL, params=lambda p: _swap("q", 0, -1)(p), noop=lambda n, m, v, i, N: n == 1),
    "r[0] <-> r[m-1]": dict(family=ALL, params=lambda p: _swap("r", 0, -1)(p), noop=lambda n, m, v, i, N: m == 1),
    "x_ref[0] := 0": dict(family=ALL, params=_xref0),
}
