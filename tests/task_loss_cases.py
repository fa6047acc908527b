"""The tracking loss of the gain predictor (quattro_tf_train_backward_f32, quattro_tf_gains_unpack_f32, quattro_tf_gains_pack_grad_f32,
train_hip.HipTrainer.forward / backward / tracking_step, training.tracking_loss): the cases, NumPy restatements of the two entries
between predictor tokens and gain stacks with their named mutants, the fp64 chain and the error measure.  A plain helper module (like
tests/policy_cases.py and tests/train_cases.py, which it composes), CPU only; used by tests/test_task_loss_cpu.py and
tests/test_task_loss_gpu.py.

Case (name, integrator): policy_cases.case(model, "skew", integ, N = 7, B = 5) gives the nominal x_nom, u_nom, the Riccati gains K of
the fp64 oracle about it (rounded to fp32) and the perturbed start x0; the feed-forward k of the same sweep completes the "logged"
gains.  The predictor is train_cases' recipe (predictor_cases.random_model(sharp=True)) at (n, c = m (1 + n)), d_model 32, 4 heads,
1 layer, d_ff 64, over N + 1 state tokens, P prompt rows and T target rows:
    cartpole      n = 4,  m = 1, c = 5,  N = 7, P = 3, T = 5 < N
    quadrotor     n = 12, m = 4, c = 52, N = 7, P = 1, T = 7 = N
    quadrotor_T8  the same with T = 8 > N: one predicted row that no step uses
Normaliser: u_mean = the logged rows' mean, u_std = 0.1 x their std (+ 1e-6), so that a prediction of order one unpacks to gains near
the logged ones and the closed loop stays in the regime policy_cases measures; test_task_loss_cpu.py asserts on these inputs, in fp64,
that every trajectory's cost is finite and below COST_CAP x the cost of its logged gains.  The inputs of the predictor are the
normalised x_nom, the last P normalised logged rows (prompt) and the first min(T, N) (target; a row past N is zero).

Token layout: the data set's -- element i (1 + n) of a token is k_i, element i (1 + n) + 1 + j is K_ij.

Error measure of d_pred: divided by its exact factors (f_b u_std[e], and alpha in the k slots) it is grad_K / grad_u_nom of
policy_cases, whose `errors` are taken about the run the gradient was formed about (rows t >= min(T, N) of those arrays, which d_pred
does not carry, are taken from the reference); rows min(T, N) <= t < T of d_pred must be exactly +0.0, else the measure is inf.
"""
import functools

import numpy as np
import torch

import grad_cases as gc
import param_cases as pc
import policy_cases as pol
import predictor_cases as prc
import train_cases as tc
from oracle import ilqr as o_ilqr
from oracle import linearize as o_lin

f32 = np.float32
SET = "skew"
SHAPES = {"cartpole": ("cartpole", 7, 3, 5), "quadrotor": ("quadrotor", 7, 1, 7), "quadrotor_T8": ("quadrotor", 7, 1, 8)}
NAMES = tuple(SHAPES)
D_MODEL, NHEAD, LAYERS, D_FF = 32, 4, 1, 64
B_CASE = 5                  # a last wave with idle groups in the gradient kernel (four trajectories per wave)
ALPHAS = (1.0, 0.5)
COST_CAP = 10.0             # every trajectory's cost under the predicted gains stays below this multiple of its logged-gains cost
PACK_ROUNDINGS = 2e-7       # three fp32 roundings of the pack (the factor f_b and two products), each <= 2^-24 of a value no larger than
                            # the measure's denominator: 3 x 6e-8
UNPACK_MUTANTS = ("prompt layout", "u_mean left out of unpack", "logged rows t >= Tn overwritten by the prediction")
PACK_MUTANTS = ("prompt layout", "u_std left out of the gradient", "alpha not applied to the k slot", "rows t >= Tn given a gradient",
                "scale of trajectory b + 1", "division by B T c")
MUTANTS = UNPACK_MUTANTS + PACK_MUTANTS[1:]


def gpu_bound(model):
    return pol.gpu_bound(model) + PACK_ROUNDINGS


class Case:
    pass


def dataset_rows(k, K):
    """(B, N, m), (B, N, m, n) -> (B, N, m (1 + n)) in the data set's layout."""
    return np.concatenate([k[..., None], K], axis=-1).reshape(k.shape[0], k.shape[1], -1)


@functools.lru_cache(maxsize=None)
def case(name, integ, B=B_CASE):
    model, N, P, T = SHAPES[name]
    n, m = pc.DIMS[model]
    c = m * (1 + n)
    pcs = pol.case(model, SET, integ, N, B=B)
    spec = pc.spec(model, SET, integ)
    k, K = o_ilqr.riccati_sweep_batched(o_lin.linearize_analytic(spec, pcs["x_nom"], pcs["u_nom"]))
    cs = Case()
    cs.name, cs.model, cs.integ, cs.spec = name, model, integ, spec
    cs.n, cs.m, cs.c, cs.N, cs.P, cs.T, cs.Tn, cs.B = n, m, c, N, P, T, min(T, N), B
    cs.x_nom, cs.u_nom, cs.x0 = f32(pcs["x_nom"]), f32(pcs["u_nom"]), f32(pcs["x0"])
    cs.K_log, cs.k_log = f32(K), f32(k)
    assert np.array_equal(cs.K_log, f32(pcs["K"]))
    rows = dataset_rows(cs.k_log, cs.K_log).astype(np.float64)
    cs.u_mean, cs.u_std = f32(rows.mean(axis=(0, 1))), f32(0.1 * rows.std(axis=(0, 1)) + 1e-6)
    xm, xs = cs.x_nom.astype(np.float64).mean(axis=(0, 1)), cs.x_nom.astype(np.float64).std(axis=(0, 1)) + 1e-6
    rows_norm = f32((rows - cs.u_mean) / cs.u_std)
    cs.x_norm = np.ascontiguousarray(f32((cs.x_nom - xm) / xs))
    cs.prompt_norm = np.ascontiguousarray(rows_norm[:, N - P:])
    cs.target_norm = np.zeros((B, T, c), dtype=f32)
    cs.target_norm[:, :cs.Tn] = rows_norm[:, :cs.Tn]
    seed = 700 + NAMES.index(name)
    w, _, _ = prc.random_model(n, c, N + 1, P, T, D_FF, LAYERS, seed, sharp=True, d_model=D_MODEL, nhead=NHEAD)
    cs.train = tc.Case(name, (n, c, D_MODEL, NHEAD, LAYERS, D_FF, N + 1, P, T), B, tc._state_dict(w), w["pos_encoder.pe"][0], seed)
    cs.train.batch = lambda draw=0: (cs.x_norm, cs.prompt_norm, cs.target_norm)
    cs.pred_norm = predict(cs, np.float32)
    cs.phys = np.tile(np.array([pc.SETS[model][SET]["phys"][q] for q in pc.PHYS_NAMES[model]], dtype=np.float64), (B, 1))
    return cs


def predict(cs, dtype=np.float64, params=None):
    """The predictor's normalised output (B, T, c) on the case's inputs: train_cases.restated on the CPU in `dtype`."""
    td = torch.float64 if dtype == np.float64 else torch.float32
    W = {key: torch.as_tensor(np.asarray(v), dtype=td) for key, v in (cs.train.params if params is None else params).items()}
    with tc._one_thread(), torch.no_grad():
        out = tc.restated(W, torch.as_tensor(cs.train.pe, dtype=td), torch.as_tensor(cs.x_norm, dtype=td),
                          torch.as_tensor(cs.prompt_norm, dtype=td), NHEAD)
    return np.ascontiguousarray(out.numpy().astype(dtype))


# ---------------------------------------------------------------------------------------------------------------- restatements
def unpack(pred, u_mean, u_std, K_log, k_log, u_nom, alpha, dtype=np.float32, mutant=None):
    """quattro_tf_gains_unpack_f32 in NumPy: every value one rounded product then one rounded sum in `dtype`.  -> (K, u_ff)."""
    d = dtype
    pred, u_mean, u_std, K_log, k_log, u_nom = (np.asarray(a).astype(d) for a in (pred, u_mean, u_std, K_log, k_log, u_nom))
    Bt, N, m, n = K_log.shape
    T = pred.shape[1]
    Tn = min(T, N)
    mean = np.zeros_like(u_mean) if mutant == "u_mean left out of unpack" else u_mean
    raw = (pred * u_std[None, None, :]).astype(d) + mean[None, None, :]
    if mutant == "prompt layout":
        kp, Kp = raw[..., :m], raw[..., m:].reshape(Bt, T, m, n)
    else:
        rows = raw.reshape(Bt, T, m, 1 + n)
        kp, Kp = rows[..., 0], rows[..., 1:]
    K, k = K_log.copy(), k_log.copy()
    K[:, :Tn], k[:, :Tn] = Kp[:, :Tn], kp[:, :Tn]
    if mutant == "logged rows t >= Tn overwritten by the prediction" and Tn < N:
        K[:, Tn:], k[:, Tn:] = Kp[:, T - 1:T], kp[:, T - 1:T]
    u_ff = u_nom + (d(alpha) * k).astype(d)
    return K.astype(d), u_ff.astype(d)


def factors(scale, Bt, task_weight=1.0, dtype=np.float32, mutant=None, Tc=1):
    """f_b = dtype(task_weight scale_b / B), formed in fp64 from the fp32 values."""
    s = np.ones(Bt) if scale is None else np.asarray(scale, dtype=f32).astype(np.float64)
    if mutant == "scale of trajectory b + 1":
        s = np.roll(s, -1)
    div = Bt * Tc if mutant == "division by B T c" else Bt
    return (np.float64(f32(task_weight)) * s / div).astype(dtype)


def pack(grad_K, grad_u, cost, scale, u_std, alpha, T, task_weight=1.0, pred=None, target=None, mse_weight=0.0, dtype=np.float32,
         mutant=None):
    """quattro_tf_gains_pack_grad_f32 in NumPy -> dict(d_pred, diverged, terms, loss)."""
    d = dtype
    gK, gu, u_std = (np.asarray(a).astype(d) for a in (grad_K, grad_u, u_std))
    cost = np.asarray(cost, dtype=np.float64)
    Bt, N, m, n = gK.shape
    c, Tn = m * (1 + n), min(T, N)
    f = factors(scale, Bt, task_weight, d, mutant, T * c)
    ok = np.isfinite(cost) & np.isfinite(f) & np.isfinite(gK).reshape(Bt, -1).all(axis=1) & np.isfinite(gu).reshape(Bt, -1).all(axis=1)
    a = d(1.0) if mutant == "alpha not applied to the k slot" else d(alpha)
    with np.errstate(all="ignore"):
        gk = (gu * a).astype(d)
        if mutant == "prompt layout":
            g = np.concatenate([gk, gK.reshape(Bt, N, m * n)], axis=-1)
        else:
            g = np.concatenate([gk[..., None], gK], axis=-1).reshape(Bt, N, c)
        rows = (g * f[:, None, None]).astype(d)
        if mutant != "u_std left out of the gradient":
            rows = (rows * u_std[None, None, :]).astype(d)
    d_pred = np.zeros((Bt, T, c), dtype=d)
    d_pred[:, :Tn] = rows[:, :Tn]
    if mutant == "rows t >= Tn given a gradient" and T > Tn:
        d_pred[:, Tn:] = rows[:, Tn - 1:Tn]
    s = np.ones(Bt) if scale is None else np.asarray(scale, dtype=f32).astype(np.float64)
    terms = np.float64(f32(task_weight)) * s * cost / Bt
    if mse_weight != 0.0:
        pr, tg = np.asarray(pred).astype(d), np.asarray(target).astype(d)
        err = (pr - tg).astype(d)
        inv = d(1.0) / d(Bt * T * c)
        d_pred = d_pred + (d(mse_weight) * ((d(2.0) * err).astype(d) * inv).astype(d)).astype(d)
        terms = terms + np.float64(f32(mse_weight)) * ((err.astype(np.float64) ** 2).reshape(Bt, -1).sum(axis=1) / (Bt * T * c))
    d_pred[~ok] = 0.0
    terms = np.where(ok, terms, 0.0)
    loss = np.float64(0.0)
    for b in range(Bt):
        loss = loss + terms[b]
    return dict(d_pred=d_pred.astype(d), diverged=(~ok).astype(np.int32), terms=terms, loss=float(loss))


def unpack_grad(d_pred, ref, scale, u_std, alpha, N, m, n, fdtype=np.float32):
    """d_pred (B, T, c) divided by its exact factors -> dict(grad_K, grad_u_nom) in policy_cases' shapes (rows t >= min(T, N) from
    `ref`; fdtype: the type f_b was rounded to), or None when a row min(T, N) <= t < T is not exactly +0.0."""
    dp = np.asarray(d_pred, dtype=np.float64)
    Bt, T, c = dp.shape
    Tn = min(T, N)
    tail = dp[:, Tn:]
    if tail.size and not (np.all(tail == 0.0) and not np.any(np.signbit(tail))):
        return None
    f = factors(scale, Bt, dtype=fdtype).astype(np.float64)
    rows = (dp[:, :Tn] / f[:, None, None] / np.asarray(u_std, dtype=np.float64)[None, None, :]).reshape(Bt, Tn, m, 1 + n)
    gK, gu = np.array(ref["grad_K"], dtype=np.float64), np.array(ref["grad_u_nom"], dtype=np.float64)
    gK[:, :Tn], gu[:, :Tn] = rows[..., 1:], rows[..., 0] / float(alpha)
    return dict(grad_K=gK, grad_u_nom=gu)


# ---------------------------------------------------------------------------------------------------------------- the fp64 chain
def run64(cs, K, u_ff):
    """The oracle's closed loop (k = 0, alpha = 1 about the feed-forward nominal u_ff) from the case's start -> (x, u, cost)."""
    K, u_ff = np.asarray(K, dtype=np.float64), np.asarray(u_ff, dtype=np.float64)
    return o_lin.closed_loop_rollout_batched(cs.spec, cs.x0.astype(np.float64), cs.x_nom.astype(np.float64), u_ff, np.zeros_like(u_ff),
                                             K, 1.0)


def reference_about(cs, x, u, K):
    """policy_cases.reference in fp64 about the run (x, u) under gains K -> (d, ref)."""
    x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
    d = gc.blocks_per_trajectory([cs.spec] * x.shape[0], x, u)
    return d, pol.reference(d, x, cs.x_nom.astype(np.float64), np.asarray(K, dtype=np.float64), cs.N)


def logged_cost(cs):
    """fp64 cost per trajectory of the logged gains through the same path: pred = the normalised logged rows."""
    rows = (dataset_rows(cs.k_log, cs.K_log).astype(np.float64) - cs.u_mean) / cs.u_std
    pred = np.zeros((cs.B, cs.T, cs.c))
    pred[:, :cs.Tn] = rows[:, :cs.Tn]
    K, u_ff = unpack(pred, cs.u_mean, cs.u_std, cs.K_log, cs.k_log, cs.u_nom, 1.0, dtype=np.float64)
    return run64(cs, K, u_ff)[2]


def scale_of(cs):
    return f32(1.0 / logged_cost(cs))


def chain64(cs, pred=None, alpha=1.0, scale=None, unpack_mutant=None, pack_mutant=None):
    """fp64: pred_norm -> unpack -> closed loop -> cost, loss; adjoint about that run -> pack.  -> dict."""
    pred = cs.pred_norm if pred is None else pred
    K, u_ff = unpack(pred, cs.u_mean, cs.u_std, cs.K_log, cs.k_log, cs.u_nom, alpha, dtype=np.float64, mutant=unpack_mutant)
    x, u, cost = run64(cs, K, u_ff)
    d, ref = reference_about(cs, x, u, K)
    out = pack(ref["grad_K"], ref["grad_u_nom"], cost, scale, cs.u_std, alpha, cs.T, dtype=np.float64, mutant=pack_mutant)
    out.update(K=K, u_ff=u_ff, x=x, u=u, cost=cost, d=d, ref=ref)
    return out


def d_pred_errors(cs, d_pred, about, alpha=1.0, scale=None, fdtype=np.float32):
    """policy_cases.errors of d_pred about the fp64 reference `about` (a dict with d, ref, x, K) -> worst of grad_K, grad_u_nom."""
    got = unpack_grad(d_pred, about["ref"], scale, cs.u_std, alpha, cs.N, cs.m, cs.n, fdtype)
    if got is None:
        return np.inf
    e = pol.errors(got, about["ref"], about["d"], about["x"], cs.x_nom.astype(np.float64), about["K"])
    return max(e["grad_K"], e["grad_u_nom"])


# mutant -> (case name, alpha) on which it must move d_pred to >= 10 x gpu_bound (measured values: tests/test_task_loss_cpu.py)
TEETH = {
    "prompt layout": ("quadrotor", 1.0),
    "u_std left out of the gradient": ("quadrotor", 1.0),
    "u_mean left out of unpack": ("quadrotor", 1.0),
    "alpha not applied to the k slot": ("quadrotor", 0.5),
    "rows t >= Tn given a gradient": ("quadrotor_T8", 1.0),
    "logged rows t >= Tn overwritten by the prediction": ("cartpole", 1.0),
    "scale of trajectory b + 1": ("quadrotor", 1.0),
    "division by B T c": ("quadrotor", 1.0),
}


def mutant_error(name, mutant, integ="rk4"):
    cs_name, alpha = TEETH[mutant]
    cs = case(cs_name, integ)
    scale = scale_of(cs)
    base = chain64(cs, alpha=alpha, scale=scale)
    mut = chain64(cs, alpha=alpha, scale=scale, unpack_mutant=mutant if mutant in UNPACK_MUTANTS else None,
                  pack_mutant=mutant if mutant in PACK_MUTANTS else None)
    return d_pred_errors(cs, mut["d_pred"], base, alpha, scale, fdtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------- finite differences
FD_H = pol.FD_H
FD_DIRECTIONS = 3
# Measured (every case name, both integrators, alpha 1 and 0.5): the worst relative difference between the fp64 chain's d_pred and central
# differences of the loss through unpack along FD_DIRECTIONS seeded directions in pred_norm; asserted: 10 x that.
FD_WORST = {"cartpole": 5.2e-8, "quadrotor": 6.3e-9}
FD_BOUND = {model: 10.0 * v for model, v in FD_WORST.items()}


def fd_error(cs, alpha=1.0, seed=5):
    """Central differences (FD_H) of the loss mean_b(scale_b closed_loop_cost_b) through unpack along random directions in pred_norm,
    against sum(d_pred * direction) of the fp64 chain: the worst relative difference."""
    scale = scale_of(cs)
    base = chain64(cs, alpha=alpha, scale=scale)
    s = scale.astype(np.float64)

    def loss(pred):
        K, u_ff = unpack(pred, cs.u_mean, cs.u_std, cs.K_log, cs.k_log, cs.u_nom, alpha, dtype=np.float64)
        return float(np.sum(s * pol.closed_loop_cost(cs.model, cs.integ, cs.x0.astype(np.float64), cs.x_nom.astype(np.float64), u_ff, K,
                                                     cs.phys)) / cs.B)

    rng = np.random.default_rng(seed)
    p0 = cs.pred_norm.astype(np.float64)
    worst = 0.0
    for _ in range(FD_DIRECTIONS):
        v = rng.standard_normal(p0.shape)
        fd = (loss(p0 + FD_H * v) - loss(p0 - FD_H * v)) / (2.0 * FD_H)
        an = float(np.sum(base["d_pred"] * v))
        worst = max(worst, abs(fd - an) / abs(an))
    return worst


# ---------------------------------------------------------------------------------------------------------------- backward from a given gradient
def evaluate_linear(params, pe, x, u, d_pred, nhead, dtype=torch.float64, masks=None, micro=False):
    """train_cases.evaluate for the scalar (pred * d_pred).sum(), whose gradient with respect to pred is d_pred: dict(loss, pred,
    grads) of train_cases.restated in `dtype`, returned as fp64.  micro=True: the gradient accumulated over single-sequence backward
    passes (another summation order over the tokens), as train_cases' floor does."""
    with tc._one_thread():
        W = {key: torch.as_tensor(np.asarray(v), dtype=dtype).clone().requires_grad_(True) for key, v in params.items()}
        pe, x, u, dp = (torch.as_tensor(np.asarray(a), dtype=dtype) for a in (pe, x, u, d_pred))
        if not micro:
            pred = tc.restated(W, pe, x, u, nhead, masks)
            loss = (pred * dp).sum()
            loss.backward()
        else:
            preds, loss = [], torch.zeros((), dtype=dtype)
            for b in range(x.shape[0]):
                mb = None if masks is None else {s: m[b:b + 1] for s, m in masks.items()}
                pb = tc.restated(W, pe, x[b:b + 1], u[b:b + 1], nhead, mb, None, b0=b)
                lb = (pb * dp[b:b + 1]).sum()
                lb.backward()
                preds.append(pb.detach())
                loss = loss + lb.detach()
            pred = torch.cat(preds)
        grads = {key: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy() for key, v in W.items()}
    return dict(loss=float(loss.detach().double()), pred=pred.detach().double().numpy(), grads=grads)


def grad_compare(got, ref):
    """train_cases.compare without the loss (the backward entry computes none): the prediction and every parameter block."""
    q = tc.compare(dict(got, loss=ref["loss"]), ref)
    q.pop("loss")
    return q


def floor_linear(tcs, d_pred, draws, masks=None):
    """train_cases.floor_of's procedure for the scalar of evaluate_linear -> (floor, [fp64 reference per draw]): the largest distance to
    the fp64 reference of two fp32 CPU evaluations (whole batch; single-sequence micro-batches), maximised over the draws."""
    worst, refs = {}, []
    for draw in range(draws):
        x, u, _ = tcs.batch(draw)
        ref = evaluate_linear(tcs.params, tcs.pe, x, u, d_pred, tcs.H, masks=masks)
        refs.append(ref)
        for micro in (False, True):
            q = grad_compare(evaluate_linear(tcs.params, tcs.pe, x, u, d_pred, tcs.H, dtype=torch.float32, masks=masks, micro=micro), ref)
            worst = {key: max(worst.get(key, 0.0), v) for key, v in q.items()}
    return worst, refs


def within(tag, q, fl):
    """Print the worst distance / floor and assert every distance of q within MARGIN x floor (train_cases.bound_of)."""
    bd = {key: v for key, v in tc.bound_of(dict(fl, loss=1.0)).items() if key != "loss"}
    scale = {key: v / tc.MARGIN for key, v in bd.items()}
    key, r = tc.worst_ratio(q, scale)
    print(f"RATIO {tag}: worst distance / floor {r:.2f} at {key} ({q[key]:.2e})")
    over = {key: (q[key], bd[key]) for key in q if not q[key] <= bd[key]}
    assert not over, (tag, over)


# ---------------------------------------------------------------------------------------------------------------- direction of descent
DESCENT_CASE = ("cartpole", "rk4")
DESCENT_STEPS = (0.3, 0.1, 0.03, 0.01, 0.003, 0.001)
TRUNCATION_CAP, NOISE_CAP, DESCENT_TOL = 0.005, 0.01, 0.05


def flat(grads, names):
    return np.concatenate([np.asarray(grads[name], dtype=np.float64).ravel() for name in names])


def moved(params, names, direction, h):
    """params + h direction (a flat vector over `names`), fp64 arrays."""
    out, at = {}, 0
    for name in names:
        v = np.asarray(params[name], dtype=np.float64)
        out[name] = v + h * direction[at:at + v.size].reshape(v.shape)
        at += v.size
    return out


@functools.lru_cache(maxsize=None)
def descent_step():
    """-> dict(h, truncation, noise, gnorm, loss): the largest h of DESCENT_STEPS at which, in the fp64 chain along the fp64 gradient g of
    the whole loss with respect to the predictor's parameters, the central difference of the loss stands within TRUNCATION_CAP of |g|
    (relative) and the fp32 loss noise 2 x 2^-23 x loss / h stays below NOISE_CAP |g|."""
    cs = case(*DESCENT_CASE)
    scale = scale_of(cs)
    names = sorted(cs.train.params)
    ch = chain64(cs, pred=predict(cs, np.float64), scale=scale)
    g = flat(evaluate_linear(cs.train.params, cs.train.pe, cs.x_norm, cs.prompt_norm, ch["d_pred"], NHEAD)["grads"], names)
    gnorm = float(np.linalg.norm(g))
    loss = lambda p: chain64(cs, pred=predict(cs, np.float64, p), scale=scale)["loss"]
    for h in DESCENT_STEPS:
        fd = (loss(moved(cs.train.params, names, g / gnorm, h)) - loss(moved(cs.train.params, names, g / gnorm, -h))) / (2.0 * h)
        trunc, noise = abs(fd - gnorm) / gnorm, 2.0 * 2.0 ** -23 * ch["loss"] / h / gnorm
        if trunc < TRUNCATION_CAP and noise < NOISE_CAP:
            return dict(h=h, truncation=trunc, noise=noise, gnorm=gnorm, loss=ch["loss"])
    raise AssertionError("no step of DESCENT_STEPS meets both caps")
