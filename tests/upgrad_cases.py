"""The cost gradient with respect to a trajectory's rows for USER-COMPILED models (compile_model(..., param_grad=True),
csrc/user_param_gradient.hip): the models, the fp64 reference, the error measure, the fp32 restatement, the mutants and the bound.
A plain helper module (like tests/pgrad_cases.py), used by scripts/prebuild_user_models.py, tests/test_user_param_gradient_cpu.py
and tests/test_user_param_gradient_gpu.py.

Models (all compiled with param_grad=True):
    grid1x1, grid4x4, grid16x8   the family of tests/user_grid_cases.py (its P[4], P[5] enter both rate and cost; (16, 8) is the
                                 register and LDS maximum), variant `convex`
    quad                         the quadrotor typed in again (tests/test_user_model_gpu.py's QUAD_RATE with `const T` for
                                 `const float`): (12, 4), NP = 7, default costs, the skew set of tests/param_cases.py
    probe                        (2, 1), NP = 3: a damped pendulum whose L reads qf, whose Lf reads q and a product of two weights,
                                 and both read P and x_ref through something other than (x - x_ref)^2: a closed-form weight or
                                 target partial is visibly wrong here

Reference (fp64, about the fp32-rounded (x, u) and the fp32 values of the rows): lambda from grad_cases.adjoint over exact blocks
(complex step through step / L / Lf in (x, u)); df/dtheta and every partial of L and Lf by the complex step in the parameter block
(phys, q, qf, r, x_ref complex; tests/user_grid_cases.Problem is analytic and its softplus branches on the real part):

    grad_phys[k]      = sum_{t<N} [ lambda_{t+1} . df/dtheta_k (x_t, u_t) + dL/dtheta_k (x_t, u_t) ] + dLf/dtheta_k (x_N)
    grad_weights[e]   = sum_{t<N} dL/de + dLf/de                 e over [q | qf | r]
    grad_targets[rho] = sum_{t<N, min(t,R-1)=rho} dL/dx_ref + [min(N,R-1)=rho] dLf/dx_ref

Error measure (DESIGN 4.7.8's, with the cost's own terms added to the parameters'): each entry against the sum of the absolute
values of its terms -- grad_phys[k] against sum_t ( sum_i Lambda_i |df_i/dtheta_k(t)| + |dL/dtheta_k(t)| ) + |dLf/dtheta_k|,
Lambda_i = max_t |lambda_{t,i}|; the others against sum |term|.  A zero denominator asks for exactly +0.0.
"""
import numpy as np

import grad_cases as gc
import param_cases as pc
import user_grid_cases as g

f32 = gc.f32
INTEGRATORS = ("euler", "rk4")
B_FULL = 3
BATCHES = (1, 3)
HORIZONS = (1, 2, 9, 63, 64)           # 63: the 64 slots fill one pass exactly; 64: the terminal slot is alone in a second pass
N_MAX = 64


def ref_counts(N):
    return (None, 1, 3, N + 1, N + 3)


# ---------------------------------------------------------------------------------------------------------------- bodies
QUAD_RATE_T = """
const T mass = P[0], Ix = P[1], Iy = P[2], Iz = P[3], arm = P[4], grav = P[5], kyaw = P[6];
T sph, cph, sth, cth, sps, cps;
sincos(x[6], &sph, &cph);  sincos(x[7], &sth, &cth);  sincos(x[8], &sps, &cps);
const T sec = 1.0f / cth, tth = sth * sec;
const T wp = x[9], wq = x[10], wr = x[11];
const T tm = (u[0] + u[1] + u[2] + u[3]) / mass;
xd[0] = x[3];  xd[1] = x[4];  xd[2] = x[5];
xd[3] = tm * (sps * sph + cps * sth * cph);
xd[4] = tm * (cps * sph - sps * sth * cph);
xd[5] = tm * (cth * cph) - grav;
const T mix = wq * sph + wr * cph;
xd[6] = wp + mix * tth;
xd[7] = wq * cph - wr * sph;
xd[8] = mix * sec;
xd[9] = (wq * wr) * ((Iy - Iz) / Ix) + ((u[1] + u[2]) - (u[0] + u[3])) * (arm / Ix);
xd[10] = (wp * wr) * ((Iz - Ix) / Iy) + ((u[0] + u[1]) - (u[2] + u[3])) * (arm / Iy);
xd[11] = (wp * wq) * ((Ix - Iy) / Iz) + (u[0] - u[1] + u[2] - u[3]) * (kyaw / Iz);
"""
# the body that breaks the rule of quattro_ilqr_amd/user_model.py (a local that holds a parameter is declared float)
QUAD_RATE_FLOAT = QUAD_RATE_T.replace("const T mass", "const float mass")

PROBE_RATE = """
xd[0] = x[1];
xd[1] = -(sin(x[0]) * P[0]) - x[1] * P[1] + u[0] * P[2];
"""
PROBE_STAGE = """
const T s0 = atan(x[0] - p.x_ref[0]), d1 = x[1] - p.x_ref[1];
return s0 * s0 * p.q[0] + d1 * d1 * (p.q[1] + p.qf[1] * 0.05f) + u[0] * u[0] * (p.r[0] + P[1] * 0.3f);
"""
PROBE_FINAL = """
const T t0 = tanh(x[0] - p.x_ref[0]), d1 = x[1] - p.x_ref[1];
return t0 * t0 * p.qf[0] + d1 * d1 * (p.qf[1] + p.q[1] * 0.5f + p.r[0] * p.qf[0] * 0.25f) + x[1] * x[1] * (P[2] * 0.1f);
"""
# (every partial of the probe's costs is one product or a sum of terms of one sign, and atan and tanh vanish at 0 only, where x - x_ref
#  is exact: a target row's only term would otherwise be measured against itself next to a zero that fp32 places elsewhere)


# ---------------------------------------------------------------------------------------------------------------- functions
class Fns:
    """step / L / Lf of one model under one parameter block, over arrays with any leading axes.  blk: dict(P, q, qf, r, x_ref) whose
    entries may be complex (the complex step) or float32 / complex64 (the fp32 restatement: the imaginary part of a complex64
    evaluation is the dual arithmetic in fp32); x_ref may carry the leading axes of x (a target row per step).  rate_terms: the
    additive terms of the rate (..., n, K), so that a derivative that is a difference can be told from one that is not."""

    def __init__(self, model, blk, integ):
        self.model, self.integ = model, integ
        self.P, self.q, self.qf, self.r, self.x_ref = (blk[k] for k in ("P", "q", "qf", "r", "x_ref"))
        self.dt, self.alpha, self.beta = model.dt, model.barrier_alpha, model.barrier_beta

    def rate(self, x, u):
        return np.sum(self.rate_terms(x, u), axis=-1)

    def step(self, x, u, stage1_only=False):
        dt = self.dt
        k1 = self.rate(x, u)
        if self.integ == "euler" or stage1_only:
            return x + k1 * dt
        k2 = self.rate(x + k1 * (0.5 * dt), u)
        k3 = self.rate(x + k2 * (0.5 * dt), u)
        k4 = self.rate(x + k3 * dt, u)
        return x + (k1 + k2 * 2.0 + k3 * 2.0 + k4) * (dt / 6.0)

    def default_L(self, x, u):
        d = x - self.x_ref
        c = np.sum(d * d * self.q, axis=-1) + np.sum(u * u * self.r, axis=-1)
        if self.alpha != 0.0:
            sp = g._softplus(-u, self.beta)
            c = c + np.sum(sp * sp, axis=-1) * self.alpha
        return c

    def default_Lf(self, x):
        d = x - self.x_ref
        return np.sum(d * d * self.qf, axis=-1)

    L, Lf = default_L, default_Lf


class GridFns(Fns):
    def __init__(self, model, blk, integ):
        super().__init__(model, blk, integ)
        dtype = np.float32 if np.asarray(blk["P"]).dtype in (np.float32, np.complex64) else np.float64
        pr = g.Problem(model.n, model.m, g.params(model.n, model.m, "convex"), integ, dtype)
        pr.P, pr.q, pr.qf, pr.r, pr.x_ref = self.P, self.q, self.qf, self.r, self.x_ref
        pr.u_scale = np.concatenate([self.P[5:6], np.ones(model.m - 1, dtype=dtype)])
        self.pr = pr

    def rate_terms(self, x, u):
        pr, P = self.pr, self.P
        sx = (x @ pr.C.T) * pr.sn
        sv = ((u * pr.u_scale) @ pr.D.T) * pr.sm
        return np.stack([np.sin(sx) * P[0], np.tanh(sv) * P[1], np.exp(sx * 0.5) * g._softplus(sv, 2.0) * P[2],
                         np.sqrt(sv * sv + 1.0) / (np.cos(sx) + 2.0) * P[3], -x], axis=-1)

    def rate(self, x, u):
        return self.pr.rate(x, u)

    def L(self, x, u):
        return self.pr.L(x, u)

    def Lf(self, x):
        return self.pr.Lf(x)


class QuadFns(Fns):
    def rate_terms(self, x, u):
        mass, Ix, Iy, Iz, arm, grav, kyaw = (self.P[k] for k in range(7))
        sph, cph, sth, cth, sps, cps = (f(x[..., i]) for i in (6, 7, 8) for f in (np.sin, np.cos))
        sec = 1.0 / cth
        tth = sth * sec
        wp, wq, wr = x[..., 9], x[..., 10], x[..., 11]
        u0, u1, u2, u3 = (u[..., a] for a in range(4))
        tm = (u0 + u1 + u2 + u3) / mass
        mix = wq * sph + wr * cph
        z = tm * 0.0
        first = [x[..., 3] + z, x[..., 4] + z, x[..., 5] + z, tm * (sps * sph + cps * sth * cph), tm * (cps * sph - sps * sth * cph),
                 tm * (cth * cph), wp + mix * tth, wq * cph - wr * sph, mix * sec, (wq * wr) * ((Iy - Iz) / Ix),
                 (wp * wr) * ((Iz - Ix) / Iy), (wp * wq) * ((Ix - Iy) / Iz)]
        second = [z, z, z, z, z, z - grav, z, z, z, ((u1 + u2) - (u0 + u3)) * (arm / Ix), ((u0 + u1) - (u2 + u3)) * (arm / Iy),
                  (u0 - u1 + u2 - u3) * (kyaw / Iz)]
        return np.stack([np.stack(first, axis=-1), np.stack(second, axis=-1)], axis=-1)


class ProbeFns(Fns):
    def rate_terms(self, x, u):
        P = self.P
        z = x[..., 0] * 0.0
        return np.stack([np.stack([x[..., 1] + z, -(np.sin(x[..., 0]) * P[0])], axis=-1), np.stack([z, -(x[..., 1] * P[1])], axis=-1),
                         np.stack([z, u[..., 0] * P[2] + z], axis=-1)], axis=-1)

    def L(self, x, u):
        xr = self.x_ref
        s0, d1 = np.arctan(x[..., 0] - xr[..., 0]), x[..., 1] - xr[..., 1]
        return s0 * s0 * self.q[0] + d1 * d1 * (self.q[1] + self.qf[1] * 0.05) + u[..., 0] * u[..., 0] * (self.r[0] + self.P[1] * 0.3)

    def Lf(self, x):
        xr = self.x_ref
        t0, d1 = np.tanh(x[..., 0] - xr[..., 0]), x[..., 1] - xr[..., 1]
        return (t0 * t0 * self.qf[0] + d1 * d1 * (self.qf[1] + self.q[1] * 0.5 + self.r[0] * self.qf[0] * 0.25)
                + x[..., 1] * x[..., 1] * (self.P[2] * 0.1))


# ---------------------------------------------------------------------------------------------------------------- models
class Model:
    def __init__(self, name, n, m, fns, base, dt, bodies, barrier=(0.0, 1.0), x0_spread=0.3, u_mean=0.5, u_spread=0.3, seed=3,
                 n_roll=None):
        self.name, self.n, self.m, self.fns_cls, self.dt, self.bodies = name, n, m, fns, float(np.float32(dt)), bodies
        self.base = {k: f32(v) for k, v in base.items()}          # P, q, qf, r, x_ref as the device holds them
        self.NP = self.base["P"].size
        self.barrier_alpha, self.barrier_beta = (float(np.float32(v)) for v in barrier)
        self.x0_spread, self.u_mean, self.u_spread, self.seed = x0_spread, u_mean, u_spread, seed
        self.n_roll = n_roll            # a longer horizon repeats the rollout of this many steps (the outputs are defined about any sequences)

    def fns(self, blk, integ):
        return self.fns_cls(self, blk, integ)

    def device(self, integ, param_grad=True):
        """The compiled model (one library per model and per param_grad: hipcc cross-compiles without a GPU)."""
        import quattro_ilqr_amd as q
        b = self.base
        kw = dict(param_grad=True) if param_grad else {}
        return q.compile_model(self.name, self.n, self.m, dt=self.dt, integrator=integ, phys=tuple(b["P"]), q=b["q"], r=b["r"],
                               qf=b["qf"], x_ref=b["x_ref"], barrier_alpha=self.barrier_alpha, barrier_beta=self.barrier_beta,
                               **self.bodies, **kw)

    # ---- seeded inputs and rows
    def rows(self, B=B_FULL, R=None, hetero=True):
        """Per-trajectory blocks (list of dict) and target rows (B, R, n) or None: phys and weights scaled per entry by 0.8 .. 1.25,
        targets the model's x_ref plus 0.2 N(0, 1); all fp32 values.  hetero=False: the model's own values, R ignored."""
        rng = np.random.default_rng(100 + self.seed)
        scale = lambda v: f32(v * np.exp(rng.uniform(np.log(0.8), np.log(1.25), (B_FULL,) + v.shape)))
        P, q, qf, r = (scale(self.base[k]) for k in ("P", "q", "qf", "r"))
        tg = f32(self.base["x_ref"] + 0.2 * rng.standard_normal((B_FULL, N_MAX + 4, self.n)))
        if not hetero:
            return [dict(self.base) for _ in range(B)], None
        blks = [dict(P=P[b], q=q[b], qf=qf[b], r=r[b], x_ref=self.base["x_ref"]) for b in range(B)]
        return blks, (None if R is None else tg[:B, :R])

    def inputs(self, N, B=B_FULL):
        rng = np.random.default_rng(self.seed)
        x0 = self.base["x_ref"] + self.x0_spread * rng.standard_normal((B_FULL, self.n))
        u = self.u_mean + self.u_spread * rng.standard_normal((B_FULL, N_MAX, self.m))
        return f32(x0[:B]), f32(u[:B, :N])


def _grid(n, m):
    p = g.params(n, m, "convex")
    return Model(f"pgrid{n}x{m}", n, m, GridFns, dict(P=p["P"], q=p["q"], qf=p["qf"], r=p["r"], x_ref=p["x_ref"]), p["dt"],
                 dict(rate=g.RATE, stage_cost=g.STAGE, final_cost=g.FINAL, helpers=g.HELPERS))


def _quad():
    s = pc.SETS["quadrotor"]["skew"]
    base = dict(P=[s["phys"][k] for k in pc.PHYS_NAMES["quadrotor"]], q=s["q"], qf=s["qf"], r=s["r"], x_ref=s["x_ref"])
    # d(rate)/d(Ix, Iy, Iz) is a difference of the gyroscopic and the torque term (DESIGN 4.7.8's cart-pole lesson): the rotors are
    # biased so that each torque stays 4 sigma away from zero, the body rates start small and the rollout is short, which keeps the
    # gyroscopic term a fraction of the torque's at every state (tests/test_user_param_gradient_cpu.py asserts the ratio)
    spread = np.array([.3, .3, .3, .5, .5, .5, .3, .3, .5, .05, .05, .05])
    return Model("pquad", 12, 4, QuadFns, base, s["dt"], dict(rate=QUAD_RATE_T), barrier=(s["barrier_alpha"], s["barrier_beta"]),
                 x0_spread=spread, u_mean=3.1 + np.array([0.6, -0.4, 0.6, -0.8]), u_spread=0.05, seed=QUAD_SEED, n_roll=9)


QUAD_SEED = 11
MODELS = {
    "grid1x1": _grid(1, 1), "grid4x4": _grid(4, 4), "grid16x8": _grid(16, 8), "quad": _quad(),
    "probe": Model("pprobe", 2, 1, ProbeFns, dict(P=(4.0, 0.35, 1.6), q=(1.2, 0.3), qf=(9.0, 2.5), r=(0.15,), x_ref=(0.7, -0.2)), 0.05,
                   dict(rate=PROBE_RATE, stage_cost=PROBE_STAGE, final_cost=PROBE_FINAL), x0_spread=0.5, u_mean=0.2, u_spread=0.8),
}
NAMES = tuple(MODELS)


def all_models():
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=4) as ex:
        return list(ex.map(lambda md: md.device("rk4"), MODELS.values()))


# ---------------------------------------------------------------------------------------------------------------- the reference
def window(rows, blks, N):
    """The x_ref that slot t = 0 .. N reads, per trajectory: (B, N + 1, n)."""
    if rows is None:
        return np.stack([np.tile(b["x_ref"], (N + 1, 1)) for b in blks])
    R = rows.shape[1]
    return rows[:, [min(t, R - 1) for t in range(N + 1)]]


def rollout(model, blks, integ, x0, u, win=None, dtype=np.float64):
    """-> x (B, N+1, n), J (B,) per trajectory under its own block (win: the cost against these targets)."""
    B, N = u.shape[:2]
    xs, J = [], []
    for b in range(B):
        f = model.fns(blks[b], integ)
        x = [np.asarray(x0[b], dtype=dtype)]
        for t in range(N):
            x.append(f.step(x[-1], u[b, t]))
        x = np.stack(x)
        xs.append(x)
        w = np.tile(blks[b]["x_ref"], (N + 1, 1)) if win is None else win[b]
        fs = model.fns(dict(blks[b], x_ref=w[:N]), integ)
        fN = model.fns(dict(blks[b], x_ref=w[N]), integ)
        J.append(np.sum(fs.L(x[:N], u[b])) + fN.Lf(x[N]))
    return np.stack(xs), np.stack(J)


def blocks(model, blks, integ, x, u, win):
    """Exact fp64 blocks about (x, u) in grad_cases.adjoint's layout."""
    n = model.n
    parts = []
    for b in range(u.shape[0]):
        N = u.shape[1]
        fs = model.fns(dict(blks[b], x_ref=win[b, :N, None, :]), integ)
        fN = model.fns(dict(blks[b], x_ref=win[b, N]), integ)
        z = np.concatenate([x[b, :N], u[b]], axis=-1)
        F = g.complex_step_jac(lambda w: fs.step(w[..., :n], w[..., n:]), z)
        gl = g.complex_step_jac(lambda w: fs.L(w[..., :n], w[..., n:])[..., None], z)[..., 0, :]
        gN = g.complex_step_jac(lambda w: fN.Lf(w)[..., None], x[b, N])[0]
        parts.append(dict(A=F[..., :n], B=F[..., n:], lx=gl[..., :n], lu=gl[..., n:], VxN=gN))
    return {k: np.stack([p[k] for p in parts]) for k in parts[0]}


H = 1e-30


def _seeded(blk, key, i, lead=()):
    """blk with entry i of `key` moved by i H (x_ref may carry leading axes: every step's row is seeded at once)."""
    v = np.array(blk[key], dtype=np.complex64 if np.asarray(blk[key]).dtype == np.float32 else np.complex128)
    v[..., i] += 1j * H
    return dict(blk, **{key: v})


def partials(model, blk, integ, x, u, w, stage1_only=False, dtype=np.float64):
    """One trajectory: x (N+1, n), u (N, m), w (N+1, n) the targets of its slots.  -> df (N, n, NP), and the partials of L (N, .) and
    Lf (.) in P (NP), the weights [q | qf | r] (2n + m) and the slot's own target (n).  dtype float32: everything in float32 /
    complex64, the fp32 restatement of the dual arithmetic."""
    n, m, NP, N = model.n, model.m, model.NP, u.shape[0]
    cast = lambda v: np.asarray(v, dtype=dtype)
    blk = {k: cast(v) for k, v in blk.items()}
    x, u, w = cast(x), cast(u), cast(w)
    bs, bN = dict(blk, x_ref=w[:N]), dict(blk, x_ref=w[N])
    im = lambda v: np.asarray(np.imag(v), dtype=np.float64) / H
    out = dict(df=np.zeros((N, n, NP)), L_P=np.zeros((N, NP)), Lf_P=np.zeros(NP), L_w=np.zeros((N, 2 * n + m)), Lf_w=np.zeros(2 * n + m))
    for k in range(NP):
        fs, fN = model.fns(_seeded(bs, "P", k), integ), model.fns(_seeded(bN, "P", k), integ)
        out["df"][:, :, k] = im(fs.step(x[:N], u, stage1_only=stage1_only))
        out["L_P"][:, k], out["Lf_P"][k] = im(fs.L(x[:N], u)), im(fN.Lf(x[N]))
    for e, (key, i) in enumerate([("q", i) for i in range(n)] + [("qf", i) for i in range(n)] + [("r", a) for a in range(m)]):
        out["L_w"][:, e] = im(model.fns(_seeded(bs, key, i), integ).L(x[:N], u))
        out["Lf_w"][e] = im(model.fns(_seeded(bN, key, i), integ).Lf(x[N]))
    out["L_ref"] = np.stack([im(model.fns(_seeded(bs, "x_ref", i), integ).L(x[:N], u)) for i in range(n)], axis=-1)
    out["Lf_ref"] = np.stack([im(model.fns(_seeded(bN, "x_ref", i), integ).Lf(x[N])) for i in range(n)], axis=-1)
    return out


MUTANTS = ("lambda_t for lambda_t+1", "the cost's own dL/dtheta dropped", "terminal slot dropped from q, r and phys",
           "weights by the closed form", "row rule off by one", "q and qf exchanged", "rk4 differentiated at stage 1 only",
           "the seed of theta_k+1")


def reference(model, blks, integ, x, u, lam, rows=None, mutant=None, restate=False):
    """x (B, N+1, n), u (B, N, m), lam (B, N+1, n); blks, rows: Model.rows().  -> dict(grad_phys (B, NP), grad_weights (B, 2n+m),
    grad_targets (B, R, n), den_*).  restate: the fp32 restatement (tangents in float32, lambda and every term rounded to fp32, the
    sums in fp64)."""
    B, N, m = u.shape
    n, NP = model.n, model.NP
    R = 1 if rows is None else rows.shape[1]
    rnd = f32 if restate else (lambda a: a)
    win = window(rows, blks, N)
    off = mutant == "row rule off by one"
    idx = [min(t + 1 if off else t, R - 1) for t in range(N + 1)]
    win_used = win if not off else (win if rows is None else rows[:, idx])
    out = {k: [] for k in ("grad_phys", "den_phys", "grad_weights", "den_weights", "grad_targets", "den_targets")}
    for b in range(B):
        pa = partials(model, blks[b], integ, x[b], u[b], win_used[b], stage1_only=mutant == "rk4 differentiated at stage 1 only",
                      dtype=np.float32 if restate else np.float64)
        lm = rnd(lam[b])
        nxt = lm[:N] if mutant == "lambda_t for lambda_t+1" else lm[1:]
        own, ownN = (0.0 * pa["L_P"], 0.0 * pa["Lf_P"]) if mutant == "the cost's own dL/dtheta dropped" else (pa["L_P"], pa["Lf_P"])
        tp = rnd(rnd(np.einsum("ti,tik->tk", nxt, pa["df"])) + own)
        tN, wN = rnd(ownN), rnd(pa["Lf_w"])
        if mutant == "terminal slot dropped from q, r and phys":
            tN = 0.0 * tN
            wN = np.concatenate([0.0 * wN[:n], wN[n:2 * n], 0.0 * wN[2 * n:]])
        gp = np.sum(tp, axis=0) + tN
        if mutant == "the seed of theta_k+1":
            gp = np.roll(gp, -1)
        Lam = np.max(np.abs(lam[b]), axis=0)
        out["grad_phys"].append(gp)
        out["den_phys"].append(np.einsum("i,tik->k", Lam, np.abs(pa["df"])) + np.sum(np.abs(pa["L_P"]), axis=0) + np.abs(pa["Lf_P"]))
        tw = rnd(pa["L_w"])
        gw = np.sum(tw, axis=0) + wN
        if mutant == "weights by the closed form":
            d = x[b] - win[b]
            gw = np.concatenate([np.sum(d[:N] ** 2, axis=0), d[N] ** 2, np.sum(u[b] ** 2, axis=0)])
        if mutant == "q and qf exchanged":
            gw = np.concatenate([gw[n:2 * n], gw[:n], gw[2 * n:]])
        out["grad_weights"].append(gw)
        out["den_weights"].append(np.sum(np.abs(pa["L_w"]), axis=0) + np.abs(pa["Lf_w"]))
        tt, tf = rnd(pa["L_ref"]), rnd(pa["Lf_ref"])
        gt, den = np.zeros((R, n)), np.zeros((R, n))
        for t in range(N):
            gt[idx[t]] += tt[t]
            den[min(t, R - 1)] += np.abs(pa["L_ref"][t])
        gt[idx[N]] += tf
        den[min(N, R - 1)] += np.abs(pa["Lf_ref"])
        out["grad_targets"].append(gt)
        out["den_targets"].append(den)
    return {k: np.stack(v) for k, v in out.items()}


def errors(got, ref):
    """pgrad_cases.errors: the measure above per output, the largest over the batch and the entries."""
    import pgrad_cases as pg
    return pg.errors(got, ref)


def worst(errs):
    return max(errs.values())


_CACHE = {}


def case(name, integ, N, R=None, B=B_FULL, hetero=True):
    """-> dict(model, blks, rows, x0, x (fp32-rounded rollout under each trajectory's own block), u, lam (fp64 adjoint), d) -- computed
    once and shared; nothing in it is modified by its users."""
    key = (name, integ, N, R, B, hetero)
    if key not in _CACHE:
        model = MODELS[name]
        blks, rows = model.rows(B, R, hetero)
        x0, u = model.inputs(N, B)
        if model.n_roll is not None and N > model.n_roll:
            nr = model.n_roll
            x = f32(rollout(model, blks, integ, x0, u[:, :nr])[0])
            x, u = x[:, [t % (nr + 1) for t in range(N + 1)]], u[:, [t % nr for t in range(N)]]
        else:
            x = f32(rollout(model, blks, integ, x0, u)[0])
        d = blocks(model, blks, integ, x, u, window(rows, blks, N))
        _CACHE[key] = dict(model=model, blks=blks, rows=rows, x0=x0, x=x, u=u, d=d, lam=gc.adjoint(d)["costate"])
    return _CACHE[key]


def row_arrays(c):
    """The rows of a case in the forms ops takes: model_phys (B, NP), weights (B, 2n + m), targets (B, R, n) or None; float32."""
    P = np.stack([b["P"] for b in c["blks"]]).astype(np.float32)
    w = np.stack([np.concatenate([b["q"], b["qf"], b["r"]]) for b in c["blks"]]).astype(np.float32)
    return P, w, None if c["rows"] is None else c["rows"].astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- conditioning
CANCEL_MAX = 4.0


def cancellation(c, integ):
    """The worst ratio sum_terms |d term_i / d theta_k| / |d rate_i / d theta_k| over the stage-1 points of a case (entries whose terms
    are all zero do not depend on theta_k and are left out): > 1 only where a parameter derivative is a difference."""
    model, worst_ratio = c["model"], 1.0
    for b, blk in enumerate(c["blks"]):
        N = c["u"].shape[1]
        for k in range(model.NP):
            t = np.imag(model.fns(_seeded(blk, "P", k), integ).rate_terms(c["x"][b, :N], c["u"][b])) / H
            num, den = np.sum(np.abs(t), axis=-1), np.abs(np.sum(t, axis=-1))
            live = num > 0
            if np.any(live):
                worst_ratio = max(worst_ratio, float(np.max(num[live] / den[live])))
    return worst_ratio


# ---------------------------------------------------------------------------------------------------------------- bounds
# E: the distance of the fp32 restatement from fp64 under the measure above: the worst over every model, both integrators, N in
# HORIZONS and R in (none, 3, N + 1), B = B_FULL, measured on the CPU (tests/test_user_param_gradient_cpu.py recomputes it and holds
# the restatement to this figure).  The GPU tests assert the project's rule: the larger of 4 x E (DESIGN 4.7.8's factor) and the fp32
# floor of the rollout comparisons, param_cases.BOUNDS["sim_x"].
# Measured: grid1x1 1.84e-7 (phys), grid4x4 1.64e-7 (targets), grid16x8 1.72e-7 (weights), quad 5.57e-7 (phys, Euler, N = 2), probe 2.09e-7.
E = {"grid1x1": 1.9e-7, "grid4x4": 1.7e-7, "grid16x8": 1.8e-7, "quad": 5.6e-7, "probe": 2.1e-7}
FLOOR = pc.BOUNDS["sim_x"]


def gpu_bound(name):
    return max(4.0 * E[name], FLOOR)


# The reference against complex-step derivatives of the fp64 rollout cost (re-rolled from x0, u under the perturbed entry):
# FD_WORST is the worst relative to the measure's denominator over the CPU test's cases; asserted: 10 x that.
FD_WORST = 8e-15
FD_BOUND = 10.0 * FD_WORST

# Every mutant stands >= 10 x above gpu_bound in the case named here: mutant -> (model, integrator, N, R).
TEETH = {
    "lambda_t for lambda_t+1": ("grid4x4", "euler", 9, 3),
    "the cost's own dL/dtheta dropped": ("probe", "euler", 9, 3),
    "terminal slot dropped from q, r and phys": ("probe", "euler", 9, 3),
    "weights by the closed form": ("probe", "euler", 9, 3),
    "row rule off by one": ("probe", "euler", 9, 3),
    "q and qf exchanged": ("probe", "euler", 9, 3),
    "rk4 differentiated at stage 1 only": ("grid4x4", "rk4", 9, 3),
    "the seed of theta_k+1": ("quad", "euler", 9, 3),
}


def total_derivative(c, integ, entries):
    """Complex-step derivative of the fp64 rollout cost of each trajectory in the named entries: ("P", k), ("q" | "qf" | "r", i),
    ("row", rho, i).  -> list of (B,) arrays."""
    model, blks, rows = c["model"], c["blks"], c["rows"]
    B, N = c["u"].shape[:2]
    out = []
    for ent in entries:
        vals = []
        for b in range(B):
            if ent[0] == "row":
                rw = np.array(window(rows, blks, N)[b], dtype=np.complex128)
                R = 1 if rows is None else rows.shape[1]
                for t in range(N + 1):
                    if min(t, R - 1) == ent[1]:
                        rw[t, ent[2]] += 1j * H
                J = rollout(model, [blks[b]], integ, c["x0"][b:b + 1], c["u"][b:b + 1], win=rw[None], dtype=np.complex128)[1]
            else:
                wn = window(rows, blks, N)[b:b + 1]
                J = rollout(model, [_seeded(blks[b], ent[0], ent[1])], integ, c["x0"][b:b + 1], c["u"][b:b + 1], win=wn,
                            dtype=np.complex128)[1]
            vals.append(np.imag(J[0]) / H)
        out.append(np.array(vals))
    return out


# ---------------------------------------------------------------------------------------------------------------- the use case
# One gradient step on model_phys of the probe model (DESIGN 4.7.8's step rule): the log is the fp64 rollout under the model's own
# parameters, the loss of trajectory b its cost against that log (targets = the log, R = N + 1) as a function of its phys row, which
# starts at Model.rows() (every entry off by a factor in 0.8 .. 1.25).  theta' = theta - s g with s = RHO min_k |theta_k / g_k|,
# halved until the fp64 cost of the rollout under theta' is below that under theta, at most HALVINGS times.
SYSID_N, SYSID_RHO, SYSID_HALVINGS = 26, 0.25, 30


def sysid_case(name, integ):
    model = MODELS[name]
    own, _ = model.rows(hetero=False)
    off, _ = model.rows()
    x0, u = model.inputs(SYSID_N)
    log = rollout(model, own, integ, x0, u)[0].astype(np.float32)
    return dict(model=model, x0=x0, u=u, log=log, theta=np.stack([b["P"] for b in off]).astype(np.float32))


def sysid_cost(c, integ, theta):
    model = c["model"]
    blks = [dict(model.base, P=np.asarray(theta[b], dtype=np.float64)) for b in range(theta.shape[0])]
    return rollout(model, blks, integ, c["x0"], c["u"], win=c["log"].astype(np.float64))[1]


def sysid_reference_gradient(c, integ):
    model = c["model"]
    theta = c["theta"].astype(np.float64)
    blks = [dict(model.base, P=theta[b]) for b in range(theta.shape[0])]
    rows = c["log"].astype(np.float64)
    x = rollout(model, blks, integ, c["x0"], c["u"])[0]
    d = blocks(model, blks, integ, x, c["u"], window(rows, blks, SYSID_N))
    return reference(model, blks, integ, x, c["u"], gc.adjoint(d)["costate"], rows=rows)["grad_phys"]


def sysid_descends(c, integ, grad):
    theta, grad = c["theta"].astype(np.float64), np.asarray(grad, dtype=np.float64)
    J0 = sysid_cost(c, integ, theta)
    s = SYSID_RHO * np.min(np.abs(theta) / np.maximum(np.abs(grad), 1e-300), axis=1)
    out = np.full(theta.shape[0], -1)
    for h in range(SYSID_HALVINGS + 1):
        J = sysid_cost(c, integ, theta - s[:, None] * grad)
        out = np.where((out < 0) & (J < J0), h, out)
        if np.all(out >= 0):
            break
        s = s * 0.5
    return out
