"""Every operator and function of csrc/dual.h on the device against fp64 derivatives (no finite differences anywhere).

The probe libraries of tests/dual_probe.py are compiled user models whose rows each exercise one form; their weights are
runtime parameters, so a one-hot q (qf) makes the stage (final) cost equal to one row:

  T = float                ops.simulate with N = 1: the returned cost is g(x0, u0), and x1 - x0 = dt g (Euler)
  T = Dual<Dual<float>>    ops.linearize: l_x, l_u, l_xx, l_uu, l_ux and V_x(N), V_xx(N) against the exact gradient and Hessian
  T = Dual<float>          A, B: I + dt grad g row by row (Euler); the complex-step Jacobian of the whole RK4 map

References: sympy derivatives evaluated in mpmath; kinked functions through the closed form of the branch taken.  Errors are
|got - ref| / S with S = max(1, |reference value, gradient and Hessian entries|) of the row at the point; the bound is
8 x max(E_row, 2^-23), E_row the error of the textbook formulas in numpy float32 (dual_probe.tolerances).  The float value
of a softplus row alone is held to 2e-6 of S (hardware exp / log in qt_softplus, csrc/models_device.h).  Each test prints
the device maxima per row (DESIGN.md 4.8 records them)."""
import numpy as np
import pytest

import dual_probe as dp
from test_user_model_gpu import complex_step_jac

pytestmark = pytest.mark.gpu

ALL = [L.name for L in dp.all_libs()]
DT32 = float(np.float32(dp.DT))


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda:0")


def _reference_is_usable(L):
    """Random libraries: every reference jet finite and of scale < 1e4 — asserted on the reference alone, before the device
    is looked at (nothing is skipped or filtered afterwards)."""
    if not L.overlap:
        return
    for r in L.rows:
        for p in range(dp.NPTS):
            a, b, w = r.point(p)
            for ww in (w, dp.f32(dp.WF)):
                j = dp.jet_ref(r.fn, (a, b, ww))
                assert j.finite() and j.scale < dp.RANDOM_SCALE_MAX, (r.name, p, j.scale)


def _linearize(md, x0, u0):
    """Records of single-step items: x0 (P, n), u0 (P, 1) -> blocks (P, ...) as fp64 numpy, V_x(N), V_xx(N) at x0 too."""
    from quattro_ilqr_amd import _lib, ops
    P, n = x0.shape
    x = np.stack([x0, x0], axis=1)
    rec, VxN, VxxN, layout = ops.linearize(md, _t(x), _t(u0.reshape(P, 1, 1)))
    blocks = {k: v.double().cpu().numpy()[:, 0] for k, v in ops.unpack_derivs(rec, P, n, 1, layout, lib=_lib.load_for(md)).items()}
    return blocks, VxN.double().cpu().numpy(), VxxN.double().cpu().numpy()


def _full(blocks, i):
    """Gradient (n + 1,) and Hessian (n + 1, n + 1) over z = (x, u) of item i."""
    g = np.concatenate([blocks["lx"][i], blocks["lu"][i]])
    H = np.block([[blocks["lxx"][i], blocks["lux"][i].T], [blocks["lux"][i], blocks["luu"][i]]])
    return g, H


def _embed(jet, idx, nz, x_only=False):
    """The row's jet over (a, b, w) placed into z = (x, u) (or into x alone)."""
    g, H = np.zeros(nz), np.zeros((nz, nz))
    for s, i in enumerate(idx):
        if i is None or (x_only and s == 2):
            continue
        g[i] = jet.g[s]
        for t, j in enumerate(idx):
            if j is None or (x_only and t == 2):
                continue
            H[i, j] = jet.H[s, t]
    return g, H


def _value_tol(row, tol):
    return dp.SOFTPLUS_VALUE_TOL if row.name.startswith("softplus") else tol[0]


@pytest.mark.parametrize("libname", ALL)
def test_float_instantiation_values(libname):
    """T = float: the cost of a one-step rollout with a one-hot q is the row's value; the Euler step moves the row's slot by
    dt times it."""
    from quattro_ilqr_amd import ops
    L = dp.lib(libname)
    _reference_is_usable(L)
    md = L.model("euler")
    x0, u0 = L.states()
    for r in L.rows + [None]:
        x, cost = ops.simulate(L.select(md, r), _t(x0), _t(u0.reshape(-1, 1, 1)))
        cost, x = cost.cpu().numpy(), x.double().cpu().numpy()
        if r is None:                                   # the control term h(u[0]) alone
            ref = [dp.h_jet(float(w)) for w in u0[:, 0]]
            err = max(abs(c - j.v) / j.scale for c, j in zip(cost, ref))
            print(f"{L.name}/h(u): float value error / S {err:.1e}")
            assert err <= dp.FACTOR * dp.EPS32
            continue
        pts = [r.point(p) for p in range(dp.NPTS)]
        tol = dp.tolerances(r.fn, pts)
        refs = [dp.jet_ref(r.fn, at) for at in pts]
        err = max(abs(c - j.v) / j.scale for c, j in zip(cost, refs))
        step = max(abs(x[p, 1, r.ia] - (x[p, 0, r.ia] + DT32 * j.v)) / max(1.0, DT32 * j.scale) for p, j in enumerate(refs))
        print(f"{L.name}/{r.name}: float value error / S {err:.1e} (bound {_value_tol(r, tol):.1e}); Euler step {step:.1e}")
        assert err <= _value_tol(r, tol), (r.name, err)
        assert step <= max(_value_tol(r, tol), tol[0]), (r.name, step)


@pytest.mark.parametrize("libname", ALL)
def test_second_order_duals_give_the_exact_gradient_and_hessian(libname):
    """T = Dual<Dual<float>>: with a one-hot q the stage-cost blocks are the row's gradient and Hessian over (x, u), zero
    outside its own slots; with a one-hot qf V_x(N), V_xx(N) are those of the final cost (u[0] -> phys[0]).  l_xx must be
    symmetric and l_ux the transposed mixed partials: lanes j and c compute H[j, c] and H[c, j] independently."""
    L = dp.lib(libname)
    _reference_is_usable(L)
    md = L.model("euler")
    x0, u0 = L.states()
    n, nz = L.n, L.n + 1
    for r in L.rows:
        w = [0.0] * n
        w[r.ia] = 1.0
        blocks, Vx, Vxx = _linearize(md.with_(q=tuple(w), r=(0.0,), qf=tuple(w)), x0, u0)
        pts = [r.point(p) for p in range(dp.NPTS)]
        ptsN = [(a, b, dp.f32(dp.WF)) for a, b, _ in pts]
        tol, tolN = dp.tolerances(r.fn, pts), dp.tolerances(r.fn, ptsN)
        idx = r.z_index(n)
        worst = np.zeros(5)
        for p in range(dp.NPTS):
            ref = dp.jet_ref(r.fn, pts[p])
            g_ref, H_ref = _embed(ref, idx, nz)
            g, H = _full(blocks, p)
            e = np.array([np.max(np.abs(g - g_ref)), np.max(np.abs(H - H_ref)), np.max(np.abs(blocks["lxx"][p] - blocks["lxx"][p].T))]) / ref.scale
            assert e[0] <= tol[1] and e[1] <= tol[2] and e[2] <= 2 * tol[2], (r.name, pts[p], e, tol)
            refN = dp.jet_ref(r.fn, ptsN[p])
            gN, HN = _embed(refN, idx, n, x_only=True)
            eN = np.array([np.max(np.abs(Vx[p] - gN)), np.max(np.abs(Vxx[p] - HN))]) / refN.scale
            assert eN[0] <= tolN[1] and eN[1] <= tolN[2] and np.max(np.abs(Vxx[p] - Vxx[p].T)) / refN.scale <= 2 * tolN[2], (r.name, ptsN[p], eN, tolN)
            worst = np.maximum(worst, np.concatenate([e, eN]))
        print(f"{L.name}/{r.name}: gradient {worst[0]:.1e} (bound {tol[1]:.1e})  Hessian {worst[1]:.1e} (bound {tol[2]:.1e})  "
              f"asymmetry {worst[2]:.1e}  V_x {worst[3]:.1e}  V_xx {worst[4]:.1e}")
    # the control term: l_u = h'(u), l_uu = h''(u), everything else zero
    blocks, _, _ = _linearize(L.select(md, None), x0, u0)
    for p in range(dp.NPTS):
        j = dp.h_jet(float(u0[p, 0]))
        g, H = _full(blocks, p)
        g_ref, H_ref = np.zeros(nz), np.zeros((nz, nz))
        g_ref[n], H_ref[n, n] = j.g[2], j.H[2, 2]
        assert max(np.max(np.abs(g - g_ref)), np.max(np.abs(H - H_ref))) / j.scale <= dp.FACTOR * dp.EPS32


@pytest.mark.parametrize("integrator", ["euler", "rk4"])
@pytest.mark.parametrize("libname", ALL)
def test_first_order_duals_give_the_exact_step_jacobian(libname, integrator):
    """T = Dual<float>: [A | B] of the whole integrator step.  Euler: I + dt grad g, row by row, from the rows' exact
    gradients.  RK4: the complex-step Jacobian of the RK4 map in fp64 (kinked functions branch on the real part).  An entry's
    error is dt x (error of a first derivative) plus the rounding of a number near 1 (6e-8), so the rows' first-derivative
    bound holds for it in units of max(1, dt S, |J|)."""
    L = dp.lib(libname)
    _reference_is_usable(L)
    md = L.model(integrator).with_(dt=dp.DT)
    x0, u0 = L.states()
    n = L.n
    blocks, _, _ = _linearize(md, x0, u0)
    J = np.concatenate([blocks["A"], blocks["B"]], axis=2)                    # (P, n, n + 1)
    tols = {r.name: dp.tolerances(r.fn, [r.point(p) for p in range(dp.NPTS)]) for r in L.rows}
    if integrator == "euler":
        for r in L.rows:
            worst = 0.0
            for p in range(dp.NPTS):
                ref = dp.jet_ref(r.fn, r.point(p))
                row = np.zeros(n + 1)
                row[r.ia] = 1.0
                for s, i in enumerate(r.z_index(n)):
                    if i is not None:
                        row[i] += DT32 * ref.g[s]
                worst = max(worst, np.max(np.abs(J[p, r.ia] - row)) / max(1.0, DT32 * ref.scale))
            print(f"{L.name}/{r.name}: Euler [A | B] row error {worst:.1e} (bound {tols[r.name][1]:.1e})")
            assert worst <= tols[r.name][1], (r.name, worst)
        if not L.overlap:                                 # an owned second slot has no rate of its own: its row is the identity's
            for r in L.rows:
                if r.nx == 2:
                    assert np.array_equal(J[:, r.ib], np.tile(np.eye(n + 1)[r.ib], (dp.NPTS, 1)))
        return
    f = dp.step_fn(L.rate_fn(dp.ComplexMath()), "rk4", DT32)
    bound = max(t[1] for t in tols.values())
    worst = 0.0
    for p in range(dp.NPTS):
        z = np.concatenate([x0[p], u0[p]]).astype(np.float64)
        J_ref = complex_step_jac(lambda zz: f(zz[:n], zz[n:]), z)
        S = max(dp.jet_ref(r.fn, r.point(p)).scale for r in L.rows)
        worst = max(worst, np.max(np.abs(J[p] - J_ref)) / max(1.0, DT32 * S, np.max(np.abs(J_ref))))
    print(f"{L.name}: RK4 [A | B] error {worst:.1e} (bound {bound:.1e})")
    assert worst <= bound


# ---------------------------------------------------------------------------------------------------------------- edges
EDGES = dp.edges()


@pytest.mark.parametrize("edge", EDGES, ids=[e.id for e in EDGES])
def test_edges(edge):
    """One case each: exact ties and kinks (fabs(0); fmax(a, a), fmin(a, a) and the mixed forms take the first argument's
    branch; == / != at equality), sincos at multiples of pi / 4 +- 1 ulp, around 2048, at 1e6, 1e9, 1e15, beyond (sin = 0, cos = 1:
    the jet at angle 0) and at +-inf (NaN), softplus at beta z = +-100 and +-1e4, tanh / atan saturated, sqrt / log at 1e-6, pow
    with a negative base and at a zero base for e = 0, 1, 2, 3.  All three scalar types; the other rows of the library sit at
    their first main point, the step is taken with dt = 0 so that the (deselected) final cost sees the same state."""
    from quattro_ilqr_amd import ops
    L = dp.lib(edge.lib)
    r = L.row(edge.row)
    a, b, w = edge.at
    x0, _ = L.states()
    x0 = x0[:1].copy()
    x0[0, r.ia] = a
    if r.nx == 2:
        x0[0, r.ib] = b
    u0 = np.array([[w]], dtype=np.float32)
    n, nz = L.n, L.n + 1
    md = L.model("euler").with_(dt=0.0, phys=(w,))
    sel = [0.0] * n
    sel[r.ia] = 1.0
    _, cost = ops.simulate(L.select(md, r), _t(x0), _t(u0.reshape(1, 1, 1)))
    cost = float(cost[0])
    blocks, Vx, Vxx = _linearize(md.with_(q=tuple(sel), r=(0.0,), qf=tuple(sel)), x0, u0)
    dyn, _, _ = _linearize(md.with_(dt=dp.DT), x0, u0)
    g, H = _full(blocks, 0)
    if edge.kind == "nan":
        assert np.isnan(cost) and np.isnan(g[r.ia]) and np.isnan(H[r.ia, r.ia]) and np.isnan(Vx[0, r.ia]) and np.isnan(dyn["A"][0, r.ia, r.ia])
        return
    ref, tol = dp.edge_reference(edge)
    assert ref.finite()
    idx = r.z_index(n)
    g_ref, H_ref = _embed(ref, idx, nz)
    gN, HN = _embed(ref, idx, n, x_only=True)
    S = ref.scale
    e = dict(value=abs(cost - ref.v) / S, gradient=np.max(np.abs(g - g_ref)) / S, hessian=np.max(np.abs(H - H_ref)) / S,
             Vx=np.max(np.abs(Vx[0] - gN)) / S, Vxx=np.max(np.abs(Vxx[0] - HN)) / S)
    row = np.zeros(nz)
    row[r.ia] = 1.0
    for s, i in enumerate(idx):
        if i is not None:
            row[i] += DT32 * ref.g[s]
    e["AB"] = np.max(np.abs(np.concatenate([dyn["A"][0, r.ia], dyn["B"][0, r.ia]]) - row)) / max(1.0, DT32 * S)
    print(f"{edge.id} at {edge.at}: " + "  ".join(f"{k} {v:.1e}" for k, v in e.items()) + f"  (S {S:.3g}, bounds {tol})")
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(H)) and np.isfinite(cost)
    assert e["value"] <= _value_tol(r, tol) and e["gradient"] <= tol[1] and e["hessian"] <= tol[2], e
    assert e["Vx"] <= tol[1] and e["Vxx"] <= tol[2] and e["AB"] <= tol[1], e
    assert np.max(np.abs(blocks["lxx"][0] - blocks["lxx"][0].T)) / S <= 2 * tol[2]
    if r.name.startswith("softplus"):                     # saturated: first derivative -> 1 or 0, second -> 0
        assert abs(g[r.ia] - (1.0 if edge.at[0] > edge.at[2] else 0.0)) <= tol[1] * S and abs(H[r.ia, r.ia]) <= tol[2] * S


# ------------------------------------------------------------------------------------------- the wave-uniform branch
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_one_large_angle_does_not_change_its_neighbours(B):
    """qt_sincos takes its large-argument reduction behind one wave-uniform __any branch: one item with |angle| > 2048 makes
    its whole wave take it.  The records, terminal pairs, states and costs of every OTHER item must equal, bit for bit, those
    of the same batch with that item at a small angle — with the large item first, in the middle and last in a wave and in
    the batch (n + m = 8: eight lanes per linearisation item, eight items per wave); the large item's own derivative of
    the sincos row is checked against the exact one."""
    import torch
    from quattro_ilqr_amd import _lib, ops
    L = dp.lib("dual_probe_c")
    r = L.row("sincos_mix")
    n = L.n
    md = L.model("rk4").with_(q=(1.0,) * n, r=(1.0,), qf=(1.0,) * n)
    xm, um = L.states()
    x0 = xm[np.arange(B) % dp.NPTS].copy()
    u0 = um[np.arange(B) % dp.NPTS].copy().reshape(B, 1, 1)
    x0[:, r.ia] = (0.1 + 0.01 * np.arange(B)).astype(np.float32)
    lib = _lib.load_for(md)

    def run(x0):
        x, cost = ops.simulate(md, _t(x0), _t(u0))
        xin = torch.stack([_t(x0), _t(x0)], dim=1).contiguous()           # linearise about x0 at both ends
        rec, VxN, VxxN, layout = ops.linearize(md, xin, _t(u0))
        out = dict(ops.unpack_derivs(rec, B, n, 1, layout, lib=lib), VxN=VxN, VxxN=VxxN, x=x, cost=cost)
        torch.cuda.synchronize()
        return out

    base = run(x0)
    big = np.float32(5000.25)
    for pos in sorted({0, 3, 7, B // 2, B - 2, B - 1} & set(range(B))):
        xb = x0.copy()
        xb[pos, r.ia] = big
        got = run(xb)
        others = torch.ones(B, dtype=torch.bool, device="cuda:0")
        others[pos] = False
        for key, v in got.items():
            assert torch.equal(v[others], base[key][others]), (B, pos, key)
        at = (float(big), float(xb[pos, r.ib]), float(u0[pos, 0, 0]))
        ref, tol = dp.jet_ref(r.fn, at), dp.tolerances(r.fn, [at])
        lx = got["lx"][pos, 0].double().cpu().numpy()
        assert not torch.equal(got["lx"][pos], base["lx"][pos])
        assert abs(lx[r.ia] - ref.g[0]) / ref.scale <= tol[1] and abs(float(got["lxx"][pos, 0, r.ia, r.ia]) - ref.H[0, 0]) / ref.scale <= tol[2]
