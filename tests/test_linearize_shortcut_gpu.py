"""The linearisation's exact short cuts: the barrier terms of l_u / l_uu are skipped when every lane of a wave finds them
below half an ulp of what they are added to (qt_barrier_derivs_negligible, models_device.h), and the range reduction of the
sines and cosines when every lane's |angle| <= 0.78 (qt_sincos_chain).  "Exact" is what is tested, by the poison-lane
technique: the same steps are linearised once in waves that take the short cut and once in waves where a neighbouring lane
holds a step that forces the full path wave-wide, and the records must agree bit for bit.

Record path: the poisoned launch carries the steps of the clean one at its EVEN steps and a poison step at every odd one (a
record depends on its own (x_t, u_t) only, and the kernels lay consecutive steps into consecutive lanes or lane groups), so
that every wave, whatever its width in steps, holds one.  Fused sweep: lowering u_0 alone forces the full path in the refill
batch of steps 0 .. 24 and can change the gains of step 0 only, which is swept last (the refill votes in launches of more than
1024 trajectories; smaller ones run the full path throughout and must agree all the same).

Against the fp64 oracle the bounds are those of tests/test_model_params_gpu.py (param_cases.BOUNDS)."""
import numpy as np
import pytest

import param_cases as pc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import linearize as o_lin  # noqa: E402

DEV = "cuda:0"
BETA = 10.0                                    # the quadrotor's barrier_beta
CART_BETA = 3.0                                # param_cases' cart-pole set with a barrier


def _ops():
    from quattro_ilqr_amd import _lib, models, ops
    return _lib, models, ops


def _dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _f64(t):
    return t.double().cpu().numpy()


def _model(model, integ):
    _lib, models, ops = _ops()
    if model == "quadrotor":
        return models.quadrotor_model(integrator=integ)
    return pc.device_model(models, "cartpole", "skew_barrier", integ)


def _spec(md, model, integ):
    p = dict(dt=md.dt, phys=dict(zip(pc.PHYS_NAMES[model], md.phys)), x_ref=md.x_ref, q=md.q, r=md.r, qf=md.qf,
             barrier_alpha=md.barrier_alpha, barrier_beta=md.barrier_beta)
    return pc.spec_from(model, p, integ)


def _layouts(md):
    _lib, _, ops = _ops()
    lays = [ops.model_layout(md), _lib.LAYOUT_ROWMAJOR] + ([_lib.LAYOUT_TILE16] if md.n == 12 else [])
    return list(dict.fromkeys(lays))


def _blocks(md, x, u, layout):
    _, _, ops = _ops()
    rec, _, _, _ = ops.linearize(md, x, u, layout=layout)
    return ops.unpack_derivs(rec, u.shape[0], md.n, md.m, layout)


def _interleave(x, u, xp, up):
    """(x, u) of horizon N -> horizon 2 N: step 2 t is step t of (x, u), step 2 t + 1 the poison step (xp[t], up[t])."""
    B, N, m = u.shape
    n = x.shape[2]
    x2 = np.zeros((B, 2 * N + 1, n))
    u2 = np.zeros((B, 2 * N, m))
    x2[:, 0:2 * N:2], x2[:, 1:2 * N:2], x2[:, 2 * N] = x[:, :N], xp, x[:, N]
    u2[:, 0::2], u2[:, 1::2] = u, up
    return x2, u2


def _clean_vs_poisoned(md, x, u, xp, up, label):
    """-> the clean launch's blocks per layout; asserts that the poisoned launch reproduces them at its even steps"""
    x2, u2 = _interleave(x, u, xp, up)
    out = {}
    for layout in _layouts(md):
        clean = _blocks(md, _dev32(x), _dev32(u), layout)
        mixed = _blocks(md, _dev32(x2), _dev32(u2), layout)
        torch.cuda.synchronize()
        for key, v in clean.items():
            assert torch.equal(_bits(v), _bits(mixed[key][:, 0::2])), (label, layout, key)
        out[layout] = (clean, mixed)
    return out


def _quad_inputs(rng, B, N, lo=20.5, hi=40.0):
    md_ref = np.zeros(12)
    md_ref[2] = 0.5
    x = md_ref + 0.2 * rng.standard_normal((B, N + 1, 12))
    u = rng.uniform(lo, hi, (B, N, 4)) / BETA
    return x, u


# ------------------------------------------------------------------------------------------------------------- record path
@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("model", ["quadrotor", "cartpole"])
def test_records_with_and_without_the_barrier_short_cut(model, integ):
    """Every control well inside the short cut (beta u in [20.5, 40]); the poison steps hold a control at beta u = 5."""
    md = _model(model, integ)
    for B in (1, 2, 3):
        for N in (1, 4, 26):
            rng = np.random.default_rng(100 * N + B)
            if model == "quadrotor":
                x, u = _quad_inputs(rng, B, N)
                xp, up = x[:, :N] + 0.01, u.copy()
                up[..., 1] = 5.0 / BETA
            else:
                x = np.asarray(md.x_ref) + 0.3 * rng.standard_normal((B, N + 1, 4))
                u = rng.uniform(20.5, 40.0, (B, N, 1)) / CART_BETA
                xp, up = x[:, :N] + 0.01, np.full((B, N, 1), 5.0 / CART_BETA)
            _clean_vs_poisoned(md, x, u, xp, up, (model, integ, B, N))


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_records_with_and_without_the_angle_short_cut(integ):
    """Small angles everywhere; the poison steps hold angles of 0.9 and 40.0.  Both launches against the oracle."""
    md = _model("quadrotor", integ)
    spec = _spec(md, "quadrotor", integ)
    rng = np.random.default_rng(5)
    B, N = 3, 26
    x, u = _quad_inputs(rng, B, N)
    xp = x[:, :N] + 0.01
    xp[:, 0::3, 6], xp[:, 1::3, 7], xp[:, 2::3, 8] = 40.0, 0.9, 40.0
    xp[:, 1::3, 6], xp[:, 2::3, 7] = 0.9, -0.9
    up = u.copy()
    for layout, (clean, mixed) in _clean_vs_poisoned(md, x, u, xp, up, ("angles", integ)).items():
        for got, (xx, uu) in ((clean, (x, u)), (mixed, _interleave(x, u, xp, up))):
            f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)     # noqa: E731
            ref = o_lin.linearize_analytic(spec, f32(xx), f32(uu))
            for key in ("A", "B", "lx", "lu", "lxx", "luu"):
                e = pc.change(key, _f64(got[key]), ref[key])
                print(f"[angles {integ} layout {layout}] {key} {e:.1e}")
                assert e < pc.BOUNDS[key], (integ, layout, key, e)


# ------------------------------------------------------------------------------------------------------------- fused sweep
@pytest.mark.parametrize("what", ["control", "angle"])
@pytest.mark.parametrize("B", [1, 2, 1030])                 # (1030: the launch that fills the chip, whose refill has the short cuts)
@pytest.mark.parametrize("N", [26, 51])
def test_fused_sweep_with_and_without_the_short_cuts(N, B, what):
    _lib, _, ops = _ops()
    md = _model("quadrotor", "euler")
    assert ops.model_fuses_sweep(md)
    rng = np.random.default_rng(10 * N + B)
    x, u = _quad_inputs(rng, B, N)
    x2, u2 = x.copy(), u.copy()
    if what == "control":
        u2[:, 0, 2] = 5.0 / BETA
    else:
        x2[:, 0, 6] = 0.9
    xd, ud = _dev32(x), _dev32(u)
    K, k, st = ops.linearize_sweep(md, xd, ud)
    K2, k2, st2 = ops.linearize_sweep(md, _dev32(x2), _dev32(u2))
    rec, VxN, VxxN, _ = ops.linearize(md, xd, ud, layout=_lib.LAYOUT_TILE16C)
    Kc, kc, sc = ops.riccati_sweep(rec, VxN, VxxN, 12, 4, _lib.LAYOUT_TILE16C)
    torch.cuda.synchronize()
    assert int(st.abs().sum()) == 0 and int(st2.abs().sum()) == 0
    assert torch.equal(_bits(K[:, 1:]), _bits(K2[:, 1:])) and torch.equal(_bits(k[:, 1:]), _bits(k2[:, 1:]))
    assert not torch.equal(_bits(K[:, 0]), _bits(K2[:, 0]))                 # (the modified step did reach the sweep)
    assert torch.equal(_bits(K), _bits(Kc)) and torch.equal(_bits(k), _bits(kc)) and torch.equal(st, sc)


# ---------------------------------------------------------------------------------------------------------------- boundary
@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_boundary_of_the_barrier_short_cut(integ):
    """Controls at beta u = 5 (the barrier term is a tenth of l_u: a threshold that lets it through shows against the oracle),
    19.9, 20.0, 20.1 and 22, a weight r = 1e-9 (the l_uu bound fails the vote) and a NaN control:
    records against the oracle in param_cases' bounds, the NaN where the oracle has it, and the status of either sweep
    flags the NaN trajectory alone."""
    _lib, _, ops = _ops()
    base = _model("quadrotor", integ)
    rng = np.random.default_rng(11)
    N = 7
    zs = (5.0, 19.9, 20.0, 20.1, 22.0)
    x, u = _quad_inputs(rng, len(zs) + 1, N, 22.0, 30.0)
    for b, z in enumerate(zs):
        u[b] = z / BETA
    u[len(zs), 3, 1] = np.nan
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)     # noqa: E731
    for md in (base, base.with_(r=(1e-9, 0.01, 0.01, 0.01))):
        spec = _spec(md, "quadrotor", integ)
        u_fin = np.nan_to_num(u, nan=2.5)                  # the oracle's step with the NaN is not compared: see below
        ref = o_lin.linearize_analytic(spec, f32(x), f32(u_fin))
        bn, tn, an = len(zs), 3, 1                         # where the NaN sits
        for layout in _layouts(md):
            got = {k_: _f64(v) for k_, v in _blocks(md, _dev32(x), _dev32(u), layout).items()}
            # the step with the NaN: l_u and l_uu of that control are NaN, those of the other three are the finite 2 r u, 2 r
            lu, luu = got["lu"][bn, tn], np.diagonal(got["luu"][bn, tn])
            assert np.isnan(lu[an]) and np.isnan(luu[an]), (integ, layout, lu, luu)
            others = [a for a in range(4) if a != an]
            r = np.asarray(md.r, dtype=np.float32).astype(np.float64)
            assert np.allclose(lu[others], (2.0 * r * f32(u_fin)[bn, tn])[others], rtol=1e-6, atol=0.0), (integ, layout, lu)
            assert np.allclose(luu[others], (2.0 * r)[others], rtol=1e-6, atol=0.0), (integ, layout, luu)
            for key in ("A", "B", "lx", "lu", "lxx", "luu"):
                g, w = got[key].copy(), ref[key].copy()
                g[bn, tn], w[bn, tn] = 0.0, 0.0
                assert np.isfinite(g).all(), (integ, layout, key)
                e = pc.change(key, g, w)
                print(f"[boundary {integ} r0 {md.r[0]:g} layout {layout}] {key} {e:.1e}")
                assert e < pc.BOUNDS[key], (integ, layout, key, e)
        want = [0] * len(zs) + [_lib.TRAJ_NONFINITE]
        rec, VxN, VxxN, lay = ops.linearize(md, _dev32(x), _dev32(u))
        _, _, st = ops.riccati_sweep(rec, VxN, VxxN, 12, 4, lay)
        assert [int(v) & _lib.TRAJ_NONFINITE for v in st.cpu()] == want, (integ, st)
        _, _, st = ops.linearize_sweep(md, _dev32(x), _dev32(u))
        assert [int(v) & _lib.TRAJ_NONFINITE for v in st.cpu()] == want, (integ, "fused", st)
