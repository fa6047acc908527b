"""The gradient of the tracked closed-loop cost on the GPU (quattro_track_gradient_f32, ops.track_gradient, autograd.tracking_cost):
   1. every output against the fp64 reference, built-in models, both integrators, policy_cases.parity_cases: N = 7 with n_steps = 7, 5
      and 1, N = 26, B = 5 (a last wave with idle groups), terminal on and off, with and without rows, a plant with the other integrator;
   2. the same for user-compiled models at policy_cases.USER_POINTS (8-, 16- and 32-lane groups);
   3. bit-for-bit identities: a trajectory of a batch against its own B = 1 call, rows past n_steps are +0.0, an output does not depend
      on which others are asked for, lambda_0 == costate[:, 0];
   4. K = None against ops.cost_gradient within the bound (whether the bits agree is printed, not asserted);
   5. autograd.tracking_cost: the forward value, the five gradients against the entry's results scaled by the incoming gradient,
      plant_phys.grad against the fp64 reference, and no ops.cost_param_gradient launch without a row that asks for one.
The bound of 1, 2 and 4 is policy_cases.gpu_bound: the larger of 4 x E (the fp32 restatement's distance from fp64, measured on the CPU)
and the project's fp32 floor 2e-6; every measured value is printed before it is asserted.  Reference, measures, mutants:
tests/policy_cases.py, tests/test_track_gradient_cpu.py."""
import numpy as np
import pytest

import grad_cases as gc
import param_cases as pc
import pgrad_cases as pgc
import policy_cases as pol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _pkg():
    import quattro_ilqr_amd as q
    return q


def dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def host(out):
    return {key: v.double().cpu().numpy() for key, v in out.items()}


def _same(a, b, tag):
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a, b), tag


def _call(q, md, c, plant_integ=None, **over):
    """ops.track_gradient on a case of policy_cases -> the dict of device tensors."""
    kw = dict(plant=None if plant_integ is None else md.with_(integrator=plant_integ), plant_phys=c.get("phys"), targets=c.get("rows"),
              weights=c.get("w"), terminal=c["terminal"], want_costate=True)
    kw.update(over)
    return q.ops.track_gradient(md, dev32(c["x"]), dev32(c["u"]), dev32(c["x_nom"]), dev32(c["K"]), **kw)


# ------------------------------------------------------------------------------------------------ 1. parity, built-in models
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_gradient_matches_the_fp64_reference(model, integ):
    q = _pkg()
    bound = pol.gpu_bound(model)
    bad = []
    for kw in [k for k in pol.parity_cases(model) if k["integ"] == integ]:
        c = pol.case(model, **kw)
        md = pc.device_model(q.models, model, kw["set_name"], integ)
        got = host(_call(q, md, c, kw.get("plant_integ")))
        assert set(got) == set(pol.KEYS)
        errs = pol.case_errors(c, got)
        print(f"[track grad {model} {pol.case_id(kw)}] " + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
        bad += [(pol.case_id(kw), k, e) for k, e in errs.items() if not e < bound]
    assert not bad, (bound, bad)


# ------------------------------------------------------------------------------------------------ 2. parity, user models
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("point", pol.USER_POINTS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_user_model_gradient_matches_the_fp64_reference(point, integ):
    import user_grid_cases as g
    q = _pkg()
    n, m = point
    md = g.model(n, m, "convex", integ)
    bound = max(4.0 * pol.USER_E, pol.FLOOR)
    bad = []
    for N, S in pol.USER_STEPS:
        for terminal in (True, False):
            c = pol.user_case(n, m, integ, N, S, terminal=terminal)
            for B in (1, pol.USER_B):
                got = host(_call(q, md, {k: (v[:B] if isinstance(v, np.ndarray) else v) for k, v in c.items()}))
                cb = dict(c, d={k: v[:B] for k, v in c["d"].items()}, ref={k: v[:B] for k, v in c["ref"].items()}, x=c["x"][:B],
                          x_nom=c["x_nom"][:B], K=c["K"][:B])
                errs = pol.case_errors(cb, got)
                print(f"[track grad user {n}x{m} {integ}] N={N} S={S} terminal={terminal} B={B}: "
                      + " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
                bad += [(N, S, terminal, B, k, e) for k, e in errs.items() if not e < bound]
    assert not bad, (bound, bad)


# ------------------------------------------------------------------------------------------------ 3. identities
def _identity_case(name, integ):
    """-> (DeviceModel, case dict with N = 7, S = 5 and every kind of row)."""
    q = _pkg()
    if name == "user":
        import user_grid_cases as g
        import weight_cases as wc
        n, m = 12, 4
        md = g.model(n, m, "convex", integ)
        c = pol.user_case(n, m, integ, 9, 4)
        B = pol.USER_B
        f = np.exp(np.random.default_rng(23).uniform(np.log(0.8), np.log(1.25), (B, len(md.phys))))
        c.update(phys=(np.asarray(md.phys)[None, :] * f).astype(np.float32), w=wc.rows_about(np.concatenate([md.q, md.qf, md.r]), B),
                 rows=(np.asarray(md.x_ref)[None, None, :] + 0.05 * np.random.default_rng(29).standard_normal((B, 3, n))).astype(np.float32))
        return md, c
    return pc.device_model(q.models, name, "skew", integ), pol.case(name, "skew", integ, 7, 5, hetero=("weights", "phys"), R=4)


@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("name", ("cartpole", "quadrotor", "user"))
def test_gradient_identities_bit_for_bit(name, integ):
    q = _pkg()
    md, c = _identity_case(name, integ)
    B, N, S = c["x"].shape[0], c["N"], c["S"]
    assert S < N
    full = _call(q, md, c)
    _same(full["grad_x0"], full["costate"][:, 0].contiguous(), "lambda_0 is costate[:, 0]")
    # rows the tracked steps did not read are +0.0
    for key, first in (("grad_u_nom", S), ("grad_K", S), ("grad_x_nom", S)):
        tail = full[key][:, first:]
        assert tail.numel() > 0 and bool((tail == 0).all()) and not bool(torch.signbit(tail).any()), key
        assert bool((full[key][:, :first] != 0).any()), key
    # every trajectory is its own B = 1 call
    for b in range(B):
        one = _call(q, md, {k: (v[b:b + 1] if isinstance(v, np.ndarray) else v) for k, v in c.items()})
        for key in full:
            _same(one[key], full[key][b:b + 1], f"trajectory {b} {key}")
    # an output does not depend on which others are asked for
    for want in ((), ("K",), ("x_nom",), ("x0",), ("K", "x0"), ("x_nom", "K")):
        for lam in (False, True):
            got = _call(q, md, c, want=want, want_costate=lam)
            assert set(got) == {"grad_u_nom"} | {"grad_" + w for w in want} | ({"costate"} if lam else set()), (want, lam)
            for key in got:
                _same(got[key], full[key], f"want={want} costate={lam}: {key}")
    # the rows matter, each of them, and so does the terminal flag
    for drop in ("phys", "w", "rows"):
        assert not torch.equal(_call(q, md, dict(c, **{drop: None}))["grad_u_nom"], full["grad_u_nom"]), drop
    assert not torch.equal(_call(q, md, dict(c, terminal=False))["grad_u_nom"], full["grad_u_nom"])


# ------------------------------------------------------------------------------------------------ 4. feedback off
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_without_gains_it_is_the_open_loop_gradient(model, integ):
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    spec = pc.spec(model, "skew", integ)
    for N in (7, 26):
        x, u = gc.nominal(model, "skew", integ, N, pol.B_CASE)
        d = gc.blocks(spec, x, u)
        ref = gc.adjoint(d)
        got = q.ops.track_gradient(md, dev32(x), dev32(u), want_costate=True)
        assert set(got) == {"grad_u_nom", "grad_x0", "costate"}
        open_loop = q.ops.cost_gradient(md, dev32(x), dev32(u), want_costate=True)
        errs = gc.errors(dict(grad_u=got["grad_u_nom"].double().cpu().numpy(), grad_x0=got["grad_x0"].double().cpu().numpy(),
                              costate=got["costate"].double().cpu().numpy()), ref, d)
        bits = {k: torch.equal(got["grad_u_nom" if k == "grad_u" else k], open_loop[k]) for k in open_loop}
        print(f"[track grad K=None {model} {integ}] N={N}: " + " ".join(f"{k} {e:.1e}" for k, e in errs.items())
              + f"; equal to ops.cost_gradient bit for bit: {bits}")
        assert gc.worst(errs) < pol.gpu_bound(model), errs
        lo = host(open_loop)
        errs = gc.errors(dict(grad_u=got["grad_u_nom"].double().cpu().numpy(), grad_x0=got["grad_x0"].double().cpu().numpy(),
                              costate=got["costate"].double().cpu().numpy()),
                         dict(grad_u=lo["grad_u"], grad_x0=lo["grad_x0"], costate=lo["costate"]), d)
        assert gc.worst(errs) < pol.gpu_bound(model), ("against ops.cost_gradient", errs)


# ------------------------------------------------------------------------------------------------ 5. autograd
@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_tracking_cost_backward_is_the_gradient_kernel(model, integ, monkeypatch):
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    other = "rk4" if integ == "euler" else "euler"
    N, S = 7, 5
    c = pol.case(model, "skew", integ, N, S, hetero=("weights", "phys"), R=4)
    B, n = c["x0"].shape
    dist = (1e-3 * np.random.default_rng(3).standard_normal((S, B, n))).astype(np.float32)
    launches = []
    real = q.ops.cost_param_gradient
    monkeypatch.setattr(q.ops, "cost_param_gradient", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    up = torch.linspace(0.5, 2.0, B, device=DEV, dtype=torch.float64)
    for plant, terminal, feedback in ((None, True, True), (md.with_(integrator=other), False, True), (None, True, False)):
        leaves = [dev32(c[k]).requires_grad_(True) for k in ("x0", "x_nom", "u_nom", "K")] + [dev32(dist).requires_grad_(True)]
        x0, x_nom, u_nom, K, dd = leaves
        kw = dict(steps=S, plant=plant, plant_phys=c["phys"], targets=c["rows"], weights=c["w"], terminal=terminal, feedback=feedback)
        J = q.tracking_cost(md, x0, x_nom, u_nom, K, disturbance=dd, **kw)
        assert J.dtype == torch.float64 and tuple(J.shape) == (B,)
        (J * up).sum().backward()
        assert not launches, "no row asks for a gradient: no ops.cost_param_gradient launch"
        with torch.no_grad():
            x, u = q.ops.track(md, x0, x_nom, u_nom, K, S, plant=plant, plant_phys=c["phys"], feedback=feedback, disturbance=dd)
            total, _ = q.ops.score(md, x, u, targets=c["rows"], weights=c["w"], model_phys=c["phys"], terminal=terminal, ref_hold=1,
                                   want_stage=False)
            _same(J.detach(), total, "forward value is ops.score's total of ops.track's run")
            ref = q.ops.track_gradient(md, x, u, x_nom if feedback else None, K if feedback else None, plant=plant, plant_phys=c["phys"],
                                       targets=c["rows"], weights=c["w"], terminal=terminal, want_costate=True)
        w = up.float()
        _same(x0.grad, ref["grad_x0"] * w[:, None], "x0.grad")
        _same(u_nom.grad[:, :S].contiguous(), (ref["grad_u_nom"] * w[:, None, None])[:, :S].contiguous(), "u_nom.grad")
        assert tuple(u_nom.grad.shape) == (B, N, md.m) and bool((u_nom.grad[:, S:] == 0).all())
        _same(dd.grad, (ref["costate"][:, 1:] * w[:, None, None]).transpose(0, 1).contiguous(), "disturbance.grad")
        if feedback:
            _same(x_nom.grad, ref["grad_x_nom"] * w[:, None, None], "x_nom.grad")
            _same(K.grad, ref["grad_K"] * w[:, None, None, None], "K.grad")
            assert bool((K.grad[:, :S] != 0).any()) and bool((K.grad[:, S:] == 0).all())
        else:
            assert x_nom.grad is None and K.grad is None


@pytest.mark.parametrize("integ", gc.INTEGRATORS)
@pytest.mark.parametrize("model", pc.MODELS)
def test_tracking_cost_plant_phys_gradient_matches_the_fp64_reference(model, integ, monkeypatch):
    q = _pkg()
    md = pc.device_model(q.models, model, "skew", integ)
    other = "rk4" if integ == "euler" else "euler"
    N = 7
    launches = []
    real = q.ops.cost_param_gradient
    monkeypatch.setattr(q.ops, "cost_param_gradient", lambda *a, **k: (launches.append(1), real(*a, **k))[1])
    for plant_integ in (None, other):
        c = pol.case(model, "skew", integ, N, N, plant_integ=plant_integ, hetero=("phys",))
        plant = None if plant_integ is None else md.with_(integrator=plant_integ)
        B = c["x0"].shape[0]
        x0, x_nom, u_nom, K = (dev32(c[k]) for k in ("x0", "x_nom", "u_nom", "K"))
        phys = dev32(c["phys"]).requires_grad_(True)
        K.requires_grad_(True)
        del launches[:]
        J = q.tracking_cost(md, x0, x_nom, u_nom, K, plant=plant, plant_phys=phys)
        J.sum().backward()
        assert len(launches) == 1 and tuple(phys.grad.shape) == (B, len(md.phys)) and phys.grad.dtype == torch.float32
        # the fp64 reference about the run the device made: the closed-loop costate over the plant's blocks, then the parameter terms
        with torch.no_grad():
            x, u = q.ops.track(md, x0, x_nom, u_nom, K, N, plant=plant, plant_phys=phys.detach())
            _same(K.grad, q.ops.track_gradient(md, x, u, x_nom, K.detach(), plant=plant, plant_phys=phys.detach(), want=("K",))["grad_K"],
                  "K.grad beside a row gradient")
        xh, uh = x.double().cpu().numpy(), u.double().cpu().numpy()
        d = gc.blocks_per_trajectory(c["specs"], xh, uh)
        lam = pol.reference(d, xh, c["x_nom"], c["K"], N)["costate"]
        ref = pgc.reference(model, c["specs"][0], xh, uh, lam, phys=c["phys"].astype(np.float64))
        e = pgc.errors(dict(grad_phys=phys.grad.double().cpu().numpy()), ref)["grad_phys"]
        print(f"[tracking_cost grad_phys {model} {integ} plant {plant_integ or integ}] {e:.1e}")
        assert e < pgc.gpu_bound(model), e
        # a second call without a row that requires a gradient: no launch more
        del launches[:]
        K2 = dev32(c["K"]).requires_grad_(True)
        q.tracking_cost(md, x0, x_nom, u_nom, K2, plant=plant, plant_phys=phys.detach()).sum().backward()
        assert not launches
        _same(K2.grad, K.grad, "the same K.grad without the row gradient")
