"""The user-model grid (tests/user_grid_cases.py) on the fp64 reference alone: what tests/test_user_grid_gpu.py relies on.

  1. The grid is the table: 13 points, tile rule and lanes per item on both sides of every edge.
  2. The reference is dense and well conditioned; variant `pivot` is indefinite with row swaps at p = 0 and p >= 1.
  3. The numerical second derivatives agree with the closed form to 1e-9 of the block scale.
  4. The reference formulas in NumPy float32 stay within a quarter of every bound (so the bounds may be used at these inputs).
  5. Every mutant moves a quantity of its family by 10 x its bound (parameters: 100 x) wherever it is not an enumerated no-op.
  6. Every grid model's generated header compiles here, and quattro_model_layout answers what the table says.
"""
import ctypes
import functools

import numpy as np
import pytest

import user_grid_cases as g

CASES = g.cases()
IDS = [g.case_id(c) for c in CASES]


@functools.lru_cache(maxsize=None)
def base(n, m, variant, integrator, N):
    return g.evaluate(n, m, variant, integrator, N)


def test_the_grid_is_the_table_of_the_issue():
    assert len(g.POINTS) == 13 and len(set(g.POINTS)) == 13
    assert tuple(p for p in g.POINTS if g.is_tile(*p)) == g.TILE_POINTS
    assert {n + m for n, m in g.POINTS} >= {2, 5, 6, 8, 9, 16, 17, 24}
    assert [g.lanes_per_item(*p) for p in ((4, 4), (7, 2), (12, 4), (13, 4), (12, 5))] == [8, 16, 16, 32, 32]
    assert not g.is_tile(4, 1) and not g.is_tile(3, 2) and g.is_tile(5, 1) and g.is_tile(2, 4)           # NZ = 5 | 6
    assert g.is_tile(12, 4) and not g.is_tile(13, 4) and not g.is_tile(12, 5)
    for n, m in g.POINTS:                                                    # float4 path iff N % 4 == 0 (rollout_body.h)
        assert ((n % 4 == 0, m % 4 == 0) == (True, True)) == ((n, m) in ((4, 4), (12, 4), (16, 8)))
    for n, m in g.POINTS:
        for v in g.variants(n, m):
            p = g.params(n, m, v)
            for key in ("q", "r", "qf", "x_ref"):
                assert len(set(p[key].tolist())) == len(p[key]), (n, m, v, key)
            assert len(set(p["P"][:4].tolist())) == 4
            x0, u = g.inputs(n, m, v, 9, 3)
            x1, u1 = g.inputs(n, m, v, 2, 1)
            assert np.array_equal(x1, x0[:1]) and np.array_equal(u1, u[:1, :2])          # B = 1 is row 0 of the larger batch
            assert np.array_equal(x0, x0.astype(np.float32).astype(np.float64))


def _min_over_max(block, lead, off_diagonal=False):
    a = np.abs(block)
    if off_diagonal:
        k = a.shape[-1]
        part = a[..., ~np.eye(k, dtype=bool)]
    else:
        part = a.reshape(a.shape[:lead] + (-1,))
    return float(np.min(part.min(-1) / a.reshape(a.shape[:lead] + (-1,)).max(-1)))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_is_dense_conditioned_and_pivots_where_it_should(case):
    n, m, variant, integ = case
    for N in g.HORIZONS:
        ev = base(n, m, variant, integ, N)
        for name in ("A", "B", "lux"):
            assert _min_over_max(ev[name], 2) >= 1e-3, (name, N)
        if n >= 2:
            assert _min_over_max(ev["lxx"], 2, True) >= 1e-3 and _min_over_max(ev["VxxN"], 1, True) >= 1e-3, N
        if m >= 2:
            assert _min_over_max(ev["luu"], 2, True) >= 1e-3, N
        quu = ev["quu"]
        assert float(np.max(np.linalg.cond(quu))) <= 100.0
        eig = np.linalg.eigvalsh(quu)
        _, swaps = g.invert_bubble(quu)
        ratio = g.unpivoted_pivot_ratio(quu)
        if variant == "convex":
            assert float(eig.min()) > 0.0 and int(swaps.sum()) == 0
            assert float(ratio.min()) > 0.5                    # far from the tile sweep's 1e-6: no trajectory is flagged
        else:
            # every trajectory has an indefinite step whose partial pivoting swaps at p = 0 and (m >= 3: with m = 2 there is no row
            # below p = 1) at a p >= 1 of the same inversion; m = 8: at least two swaps in one inversion
            indef = (eig.min(-1) < 0) & (eig.max(-1) > 0)
            want = indef & (swaps[..., 0] > 0)
            if m >= 3:
                want &= swaps[..., 1:].sum(-1) > 0
            if m == 8:
                want &= swaps.sum(-1) >= 2
            assert want.any(axis=1).all(), (N, swaps.tolist())
            assert float(ratio.min(axis=1).max()) < -100.0     # every trajectory is flagged, by a pivot far below zero


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "rk4"], ids=[i for c, i in zip(CASES, IDS) if c[3] == "rk4"])
def test_second_derivatives_are_exact_to_1e_9(case):
    n, m, variant, integ = case
    ev = base(n, m, variant, integ, 9)
    pr = g.Problem(n, m, g.params(n, m, variant), integ)
    x0, u = g.inputs(n, m, variant, 9)
    closed = pr.hessian_closed_form(ev["sim_x"], u)
    for name, ref in closed.items():
        err = np.max(np.abs(ev[name] - ref)) / max(1.0, np.max(np.abs(ref)))
        assert err <= 1e-9, (name, err)
    # and by agreement of two step sizes
    z = np.concatenate([ev["sim_x"][:, :-1], u], axis=-1)
    gL = lambda w: g.complex_step_jac(lambda v: pr.L(v[..., :n], v[..., n:])[..., None], w)[..., 0, :]
    H1, H2 = g.richardson_hessian(gL, z, h=2e-3), g.richardson_hessian(gL, z, h=1e-3)
    assert np.max(np.abs(H1 - H2)) <= 1e-9 * max(1.0, np.max(np.abs(H1)))


EMULATED = ("sim_x", "sim_cost", "cl_x", "cl_u", "cl_cost", "K", "k", "K_reg", "k_reg")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float32_reference_formulas_stay_within_a_quarter_of_the_bounds(case):
    """Rollout, closed-loop rollout and the recursion with the pivoted fp32 inverse, in NumPy float32, from the fp32-rounded
    nominal, records and gains, against the same in fp64: at most a quarter of each bound, at every batch and horizon."""
    n, m, variant, integ = case
    worst = {}
    for N in g.HORIZONS:
        about = g.rounded(base(n, m, variant, integ, N))
        ref = g.evaluate(n, m, variant, integ, N, about=about)
        emu = g.evaluate(n, m, variant, integ, N, about=about, dtype=np.float32)
        for name in EMULATED:
            if name not in ref:                                # (K_reg, k_reg: variant `convex` only)
                continue
            for B in g.BATCHES:
                sl = (slice(None), slice(0, B)) if name.startswith("cl_") else (slice(0, B),)
                worst[name] = max(worst.get(name, 0.0), g.error(name, emu[name][sl], ref[name][sl]))
    print(f"[grid fp32 emulation {g.case_id(case)}]", {k_: f"{v:.1e}" for k_, v in worst.items()})
    for name, e in worst.items():
        assert e <= 0.25 * g.BOUNDS[name], (name, e)
        key = name[:-4] if name.endswith("_reg") else name
        assert e <= g.FP32_EMULATION[key], (name, e, "larger than the figure recorded in user_grid_cases.FP32_EMULATION")


def _multiple(mut_ev, ref_ev, names):
    return max(g.error(name, mut_ev[name], ref_ev[name]) / g.BOUNDS[name] for name in names if name in ref_ev)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_mutant_is_seen_or_is_an_enumerated_noop(case):
    n, m, variant, integ = case
    for N in (1, 9):
        ref = base(n, m, variant, integ, N)
        about = dict(nom=ref["sim_x"], K=ref["K"], k=ref["k"])
        for name, mut in g.MUTANTS.items():
            noop = g.is_noop(name, n, m, variant, integ, N)
            if noop is None:                                   # does not apply here (the unpivoted elimination outside `pivot`)
                continue
            ev = g.evaluate(n, m, variant, integ, N, mutant=name, about=about)
            fams = mut["family"] if isinstance(mut["family"], tuple) else (mut["family"],)
            names = [q for f in fams for q in g.FAMILIES[f]]
            if noop:
                for q in (q for q in names if q in ref):
                    if mut.get("roundoff"):
                        assert g.error(q, ev[q], ref[q]) <= 1e-12, (name, q)
                    else:
                        assert np.array_equal(ev[q], ref[q]), (name, q, N)
                continue
            mult = _multiple(ev, ref, names)
            print(f"[grid mutant {g.case_id(case)} N={N}] {name}: {mult:.0f} x bound")
            assert mult >= (100.0 if "params" in mut else 10.0), (name, N, mult)


@pytest.mark.parametrize("nm", g.POINTS, ids=[f"{n}x{m}" for n, m in g.POINTS])
def test_every_pair_of_parameters_matters(nm):
    """Swapping any two of P[0..3], or two entries of q, r, qf, x_ref, moves some compared quantity by more than 100 x its bound."""
    n, m = nm
    ref = base(n, m, "convex", "rk4", 9)
    about = dict(nom=ref["sim_x"], K=ref["K"], k=ref["k"])
    names = [q for f in g.ALL for q in g.FAMILIES[f]]
    pairs = [("P", i, j) for i in range(4) for j in range(i + 1, 4)]
    pairs += [(key, 0, k - 1) for key, k in (("q", n), ("qf", n), ("x_ref", n), ("r", m)) if k >= 2]
    pairs += [(key, 0, 1) for key, k in (("q", n), ("qf", n), ("x_ref", n), ("r", m)) if k >= 3]
    for key, i, j in pairs:
        g.MUTANTS["_pair"] = dict(family=g.ALL, params=g._swap(key, i, j))
        try:
            ev = g.evaluate(n, m, "convex", "rk4", 9, mutant="_pair", about=about)
        finally:
            del g.MUTANTS["_pair"]
        assert _multiple(ev, ref, names) >= 100.0, (key, i, j)


def test_every_grid_header_compiles_and_reports_the_layout_of_the_table():
    """The host half of the twice-stated tile rule: csrc/capi.hip: quattro_model_layout against the table (the device half,
    csrc/solve_user.hip: TILE, is the bit-for-bit test of tests/test_user_grid_gpu.py)."""
    pytest.importorskip("torch")
    from quattro_ilqr_amd import _lib
    models = g.all_models()                                    # hipcc cross-compiles without a GPU; cached by content
    assert len({md.lib_path for md in models}) == 13
    for md in models:
        lib = _lib.load_for(md)
        p = md.c_params()
        want = _lib.LAYOUT_ROWMAJOR_TILE if (md.n, md.m) in g.TILE_POINTS else _lib.LAYOUT_ROWMAJOR
        assert lib.quattro_model_layout(ctypes.byref(p)) == want, (md.n, md.m)
        assert g.model(md.n, md.m, "pivot" if md.m >= 2 else "convex", "euler").lib_path == md.lib_path   # one library per (n, m)
