"""GPU parity tests: every HIP kernel, called through the C ABI (ctypes -> libquattro_hip.so), against the golden
vectors captured from the reference and against the CPU oracle on the same seeded inputs.

Tolerances (BASELINE.json north_star: 1e-5 relative fp32; SURVEY F6 for where that is meaningful):
  sweep on golden inputs      K, k relative Frobenius <= 2e-6 per trajectory, per-step relative <= 1e-5 (k per step with
                              the denominator floored at 5% of the largest step: the cart-pole's scalar k_t crosses
                              zero, where fp32 NumPy on identical inputs also reads 1.4e-5 "relative")
  linearisation               first derivatives <= 1e-5 rel vs the fp64 analytic oracle
  rollouts                    x, u <= 1e-5 rel, cost <= 1e-5 rel vs the reference's forward_pass
"""
import numpy as np
import pytest

from conftest import load_golden, per_step_rel, per_step_rel_floor, rel_fro

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import ilqr as o_ilqr  # noqa: E402
from oracle import linearize as o_lin  # noqa: E402
from oracle import models as o_models  # noqa: E402

DEV = "cuda:0"
BLOCKS = ["A", "B", "lx", "lu", "lxx", "luu", "lux"]


def _ops():
    from quattro_ilqr_amd import _lib, models, ops
    return _lib, models, ops


def dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _spec(model, integ=0):
    return o_models.cartpole_spec(0.01, integ) if model == "cartpole" else o_models.quadrotor_spec(0.01, integ)


# ---------------------------------------------------------------------------------------------- sweep (G4)
@pytest.mark.parametrize("name,n,m", [("sweep_cartpole_N30.npz", 4, 1), ("sweep_cartpole_N50.npz", 4, 1),
                                      ("sweep_quadrotor_N30.npz", 12, 4), ("sweep_quadrotor_N50.npz", 12, 4)])
def test_sweep_matches_reference_on_golden_inputs(name, n, m):
    _lib, models, ops = _ops()
    g = load_golden(name)
    layouts = [_lib.LAYOUT_ROWMAJOR] + ([_lib.LAYOUT_TILE16] if (n, m) == (12, 4) else [])
    N = g["A"].shape[1]
    for layout in layouts:
        rec, _ = ops.pack_derivs(*[dev32(g[k]) for k in BLOCKS], layout=layout)
        K, k, status = ops.riccati_sweep(rec, dev32(g["VxN"]), dev32(g["VxxN"]), n, m, layout)
        torch.cuda.synchronize()
        assert int(status.abs().sum()) == 0
        K, k = K.cpu().numpy(), k.cpu().numpy()
        for b in range(K.shape[0]):
            # measured on MI355X: rel-Fro 2-4e-7, per-step <= 9e-7 (K) / 1.7e-6 (k): as good as fp32 NumPy
            assert rel_fro(K[b], g["K"][b]) < 2e-6 and rel_fro(k[b], g["k"][b]) < 2e-6, (layout, b)
            assert per_step_rel(K[b], g["K"][b]) < 1e-5, (layout, b, per_step_rel(K[b], g["K"][b]))
            assert per_step_rel_floor(k[b], g["k"][b], 0.05) < 1e-5, (layout, b)
        # tail segments == backward_pass_segment (index t - start_idx)
        for seg in g["seg_lengths"]:
            seg = int(seg)
            rec_s, _ = ops.pack_derivs(*[dev32(g[k_][:, N - seg:]) for k_ in BLOCKS], layout=layout)
            Ks, ks, _ = ops.riccati_sweep(rec_s, dev32(g["VxN"]), dev32(g["VxxN"]), n, m, layout)
            Ks, ks = Ks.cpu().numpy(), ks.cpu().numpy()
            assert Ks.shape == g[f"segK_{seg}"].shape
            for b in range(Ks.shape[0]):
                assert per_step_rel(Ks[b], g[f"segK_{seg}"][b]) < 1e-5
                assert per_step_rel_floor(ks[b], g[f"segk_{seg}"][b], 0.05) < 1e-5


def test_sweep_layouts_agree_and_active_mask():
    """TILE16 (register/MFMA kernel) and ROWMAJOR (LDS kernel) are two implementations of the same recursion."""
    _lib, models, ops = _ops()
    g = load_golden("sweep_quadrotor_N50.npz")
    reps = 32                                    # replicate the 3 golden trajectories with small perturbations
    rng = np.random.default_rng(0)
    blocks = {k: np.repeat(g[k], reps, axis=0) for k in BLOCKS + ["VxN", "VxxN"]}
    for k_ in ["lx", "lu", "VxN"]:
        blocks[k_] = blocks[k_] * (1.0 + 1e-3 * rng.standard_normal(blocks[k_].shape))
    Bt = blocks["A"].shape[0]
    out = {}
    for layout in (_lib.LAYOUT_ROWMAJOR, _lib.LAYOUT_TILE16):
        rec, _ = ops.pack_derivs(*[dev32(blocks[k]) for k in BLOCKS], layout=layout)
        K, k, st = ops.riccati_sweep(rec, dev32(blocks["VxN"]), dev32(blocks["VxxN"]), 12, 4, layout)
        out[layout] = (K.cpu().numpy(), k.cpu().numpy())
        assert int(st.abs().sum()) == 0
    d64 = {k: blocks[k].astype(np.float32).astype(np.float64) for k in blocks}
    ko, Ko = o_ilqr.riccati_sweep_batched(d64)
    for layout, (K, k) in out.items():
        for b in range(Bt):
            assert per_step_rel(K[b], Ko[b]) < 1e-5 and per_step_rel(k[b], ko[b]) < 1e-5
    # active mask: masked-out trajectories keep whatever was in the output buffers
    layout = _lib.LAYOUT_TILE16
    rec, _ = ops.pack_derivs(*[dev32(blocks[k]) for k in BLOCKS], layout=layout)
    active = torch.ones(Bt, dtype=torch.int32, device=DEV)
    active[::3] = 0
    Kbuf = torch.full((Bt, 50, 4, 12), 7.0, dtype=torch.float32, device=DEV)
    kbuf = torch.full((Bt, 50, 4), 7.0, dtype=torch.float32, device=DEV)
    ops.riccati_sweep(rec, dev32(blocks["VxN"]), dev32(blocks["VxxN"]), 12, 4, layout, K=Kbuf, k=kbuf, active=active)
    Kb = Kbuf.cpu().numpy()
    assert np.all(Kb[::3] == 7.0)
    assert np.array_equal(Kb[1::3], out[layout][0][1::3])


def _zero_quu_blocks(reg, name="sweep_cartpole_N30.npz"):
    """Q_uu + reg I exactly zero at every step: l_uu = -reg I, B = 0, on one golden trajectory."""
    g = load_golden(name)
    blocks = {k: g[k][:1].copy() for k in BLOCKS + ["VxN", "VxxN"]}
    blocks["B"][:] = 0.0
    blocks["luu"][:] = -reg * np.eye(blocks["luu"].shape[-1])
    return blocks


def test_sweep_status_flags_singular_and_nonfinite():
    _lib, models, ops = _ops()
    g = load_golden("sweep_cartpole_N30.npz")
    blocks = {k: g[k][:2].copy() for k in BLOCKS + ["VxN", "VxxN"]}
    blocks["lx"][1, 5, 0] = np.nan
    rec, layout = ops.pack_derivs(*[dev32(blocks[k]) for k in BLOCKS])
    _, _, st = ops.riccati_sweep(rec, dev32(blocks["VxN"]), dev32(blocks["VxxN"]), 4, 1, layout)
    st = st.cpu().numpy()
    assert st[0] == 0 and (st[1] & _lib.TRAJ_NONFINITE)
    blocks = _zero_quu_blocks(1e-6)
    rec, layout = ops.pack_derivs(*[dev32(blocks[k]) for k in BLOCKS])
    _, _, st = ops.riccati_sweep(rec, dev32(blocks["VxN"]), dev32(blocks["VxxN"]), 4, 1, layout,
                                 reg=float(np.float32(1e-6)))
    assert int(st.cpu()[0]) & _lib.TRAJ_SINGULAR


# ---------------------------------------------------------------------------------------------- linearisation (G3)
@pytest.mark.parametrize("name,model", [("sweep_cartpole_N50.npz", "cartpole"), ("sweep_quadrotor_N50.npz", "quadrotor")])
def test_linearize_matches_oracle_and_reference(name, model):
    _lib, models, ops = _ops()
    g = load_golden(name)
    spec = _spec(model)
    dm = models.model_by_name(model)
    x, u = dev32(g["x_seq"]), dev32(g["u_seq"])
    x64 = g["x_seq"].astype(np.float32).astype(np.float64)
    u64 = g["u_seq"].astype(np.float32).astype(np.float64)
    a = o_lin.linearize_analytic(spec, x64, u64)
    layouts = [_lib.LAYOUT_ROWMAJOR] + ([_lib.LAYOUT_TILE16] if model == "quadrotor" else [])
    for layout in layouts:
        for t_start in (0, 37):
            rec, VxN, VxxN, _ = ops.linearize(dm, x, u, t_start=t_start, layout=layout)
            want, _ = ops.pack_derivs(*[dev32(a[k][:, t_start:]) for k in BLOCKS], layout=layout)
            got, want = rec.cpu().numpy().astype(np.float64), want.cpu().numpy().astype(np.float64)
            assert got.shape == want.shape
            err = np.abs(got - want) / np.maximum(np.abs(want), 1e-2)
            assert err.max() < 1e-5, (layout, t_start, err.max())
            assert rel_fro(VxN.cpu().numpy(), a["VxN"]) < 1e-6
            assert rel_fro(VxxN.cpu().numpy(), a["VxxN"]) < 1e-6
    # distance to the reference's finite differences on first derivatives (~1e-10 + fp32 rounding)
    rec, _, _, _ = ops.linearize(dm, x, u, layout=_lib.LAYOUT_ROWMAJOR)
    ref, _ = ops.pack_derivs(*[dev32(g[k]) for k in BLOCKS], layout=_lib.LAYOUT_ROWMAJOR)
    n, m = dm.n, dm.m
    nab = n * n + n * m
    got, ref = rec.cpu().numpy(), ref.cpu().numpy()
    assert np.max(np.abs(got[..., :nab] - ref[..., :nab])) < 2e-6          # A, B
    # end to end: device linearisation + device sweep.
    layout = ops.preferred_layout(n, m)
    rec, VxN, VxxN, _ = ops.linearize(dm, x, u, layout=layout)
    K, k, _ = ops.riccati_sweep(rec, VxN, VxxN, n, m, layout)
    K, k = K.cpu().numpy(), k.cpu().numpy()
    # (i) against the exact-derivative fp64 oracle: this is the device path's own accuracy
    k_a, K_a = o_ilqr.riccati_sweep_batched(a)
    assert rel_fro(K, K_a) < 2e-6 and rel_fro(k, k_a) < 5e-6, (rel_fro(K, K_a), rel_fro(k, k_a))
    # (ii) against the reference's FD backward pass: bounded by the REFERENCE's second-difference round-off
    # (4 eps |L| / 4 eps_fd^2).  Control experiment, all fp64: the reference's own sweep with only
    # l_xx/l_uu/l_ux/V_xx(N) replaced by their exact values moves K by the same amount the device differs.
    d_ctrl = {kk: g[kk].astype(np.float64) for kk in BLOCKS + ["VxN", "VxxN"]}
    a64 = o_lin.linearize_analytic(spec, g["x_seq"], g["u_seq"])
    for kk in ["lxx", "luu", "lux", "VxxN"]:
        d_ctrl[kk] = a64[kk]
    _, K_ctrl = o_ilqr.riccati_sweep_batched(d_ctrl)
    floor = rel_fro(K_ctrl, g["K"])                      # 8.9e-5 quadrotor, 1.4e-4 cart-pole on these trajectories
    assert abs(rel_fro(K, g["K"]) - floor) < 2e-6
    assert rel_fro(K, g["K"]) < 5e-4 and rel_fro(k, g["k"]) < 5e-4


# ---------------------------------------------------------------------------------------------- rollouts (G5)
@pytest.mark.parametrize("model", ["cartpole", "quadrotor"])
def test_simulate_and_forward_pass_all_alphas(model):
    _lib, models, ops = _ops()
    g = load_golden(f"fwd_{model}.npz")
    dm = models.model_by_name(model)
    x0, u = dev32(g["x0"]), dev32(g["u_seq"])
    x, J = ops.simulate(dm, x0, u)
    assert rel_fro(x.cpu().numpy(), g["x_seq"]) < 1e-6
    assert np.max(np.abs(J.cpu().numpy() - g["cost0"]) / np.abs(g["cost0"])) < 1e-6
    Jt = ops.total_cost(dm, dev32(g["x_seq"]), u)
    assert np.max(np.abs(Jt.cpu().numpy() - g["cost0"]) / np.abs(g["cost0"])) < 1e-6
    alphas = [float(a) for a in g["alphas"]]
    cost, xn, un = ops.rollout(dm, dev32(g["x_seq"]), u, dev32(g["K"]), dev32(g["k"]), alphas, want_traj=True)
    cost, xn, un = cost.cpu().numpy(), xn.cpu().numpy(), un.cpu().numpy()
    for b in range(g["x0"].shape[0]):
        for ai in range(len(alphas)):
            assert rel_fro(xn[ai, b], g["new_x"][b, ai]) < 1e-5
            assert rel_fro(un[ai, b], g["new_u"][b, ai]) < 1e-5
            assert abs(cost[ai, b] - g["new_cost"][b, ai]) <= 1e-5 * abs(g["new_cost"][b, ai])
    cost_only = ops.rollout(dm, dev32(g["x_seq"]), u, dev32(g["K"]), dev32(g["k"]), alphas)
    assert np.array_equal(cost_only.cpu().numpy(), cost)


@pytest.mark.parametrize("model", ["cartpole", "quadrotor"])
def test_fused_linesearch_semantics(model):
    """First accepted alpha, in-place commit, convergence flags: against the separate-rollout kernel."""
    _lib, models, ops = _ops()
    g = load_golden(f"fwd_{model}.npz")
    dm = models.model_by_name(model)
    reps = 5
    x_nom = dev32(np.repeat(g["x_seq"], reps, axis=0)); u_nom = dev32(np.repeat(g["u_seq"], reps, axis=0))
    K = dev32(np.repeat(g["K"], reps, axis=0))
    # scale the feed-forward term differently per replica so that different alphas get accepted (or none)
    scale = np.tile(np.array([1.0, 3.0, 8.0, 30.0, -50.0]), g["x0"].shape[0])
    k = dev32(np.repeat(g["k"], reps, axis=0) * scale[:, None, None])
    Bt = x_nom.shape[0]
    cost0 = ops.total_cost(dm, x_nom, u_nom)
    cand, xn, un = ops.rollout(dm, x_nom, u_nom, K, k, ops.ALPHAS, want_traj=True)
    cand_h, cost0_h = cand.cpu().numpy(), cost0.cpu().numpy()
    want_idx = np.full(Bt, -1)
    for b in range(Bt):
        acc = np.nonzero(cand_h[:, b] <= cost0_h[b])[0]
        if acc.size:
            want_idx[b] = acc[0]
    assert len(set(want_idx.tolist())) >= 3                     # the test exercises several branches
    active = torch.ones(Bt, dtype=torch.int32, device=DEV)
    active[2] = 0
    iters = torch.zeros(Bt, dtype=torch.int32, device=DEV)
    x_run, u_run, cost_run = x_nom.clone(), u_nom.clone(), cost0.clone()
    tol = 1e-3
    idx = ops.linesearch(dm, x_run, u_run, K, k, cost_run, tol, ops.ALPHAS, active=active, iters=iters)
    idx, act, it = idx.cpu().numpy(), active.cpu().numpy(), iters.cpu().numpy()
    for b in range(Bt):
        if b == 2:
            assert it[b] == 0 and torch.equal(x_run[b], x_nom[b])
            continue
        assert idx[b] == want_idx[b] and it[b] == 1
        if want_idx[b] < 0:
            assert act[b] == 0 and torch.equal(x_run[b], x_nom[b]) and torch.equal(u_run[b], u_nom[b])
        else:
            a = want_idx[b]
            assert torch.equal(x_run[b], xn[a, b]) and torch.equal(u_run[b], un[a, b])
            assert float(cost_run[b]) == cand_h[a, b]
            assert act[b] == (0 if abs(cost0_h[b] - cand_h[a, b]) < tol else 1)


# ---------------------------------------------------------------------------------------------- RK4 discretisation
@pytest.mark.parametrize("name,model", [("sweep_cartpole_N30_rk4.npz", "cartpole"), ("sweep_quadrotor_N30_rk4.npz", "quadrotor")])
def test_rk4_linearisation_and_rollout(name, model):
    """integration_method="rk4" is the default of both MPC classes (quadrotor_mpc.py:12, cartpole_mpc.py:146): the
    forward-mode RK4 Jacobians vs the fp64 oracle's chain rule and vs the reference's finite differences."""
    _lib, models, ops = _ops()
    g = load_golden(name)
    spec = _spec(model, integ=1)
    dm = models.model_by_name(model, integrator="rk4")
    x, u = dev32(g["x_seq"]), dev32(g["u_seq"])
    a = o_lin.linearize_analytic(spec, g["x_seq"].astype(np.float32).astype(np.float64),
                                 g["u_seq"].astype(np.float32).astype(np.float64))
    layouts = [_lib.LAYOUT_ROWMAJOR] + ([_lib.LAYOUT_TILE16] if model == "quadrotor" else [])
    n, m = dm.n, dm.m
    for layout in layouts:
        rec, VxN, VxxN, _ = ops.linearize(dm, x, u, layout=layout)
        want, _ = ops.pack_derivs(*[dev32(a[k]) for k in BLOCKS], layout=layout)
        got, want = rec.cpu().numpy().astype(np.float64), want.cpu().numpy().astype(np.float64)
        err = np.abs(got - want) / np.maximum(np.abs(want), 1e-2)
        assert err.max() < 1e-5, (layout, err.max())
        K, k, st = ops.riccati_sweep(rec, VxN, VxxN, n, m, layout)
        k_a, K_a = o_ilqr.riccati_sweep_batched(a)
        assert int(st.abs().sum()) == 0 and rel_fro(K.cpu().numpy(), K_a) < 2e-6
    rec, _, _, _ = ops.linearize(dm, x, u, layout=_lib.LAYOUT_ROWMAJOR)
    ref, _ = ops.pack_derivs(*[dev32(g[k]) for k in BLOCKS], layout=_lib.LAYOUT_ROWMAJOR)
    nab = n * n + n * m
    assert np.max(np.abs(rec.cpu().numpy()[..., :nab] - ref.cpu().numpy()[..., :nab])) < 2e-6      # A, B vs reference FD
    # RK4 rollout vs the reference's simulate
    xs, _ = ops.simulate(dm, dev32(g["x_seq"][:, 0]), u)
    assert rel_fro(xs.cpu().numpy(), g["x_seq"]) < 1e-6


def test_compact_records_give_the_same_sweep_bit_for_bit():
    """TILE16C (Euler quadrotor: constants of the problem once in a header record, 76 state-dependent floats per step)
    carries exactly the information of the full TILE16 record: linearize + sweep through either layout produce
    identical K, k — ragged sizes, t_start > 0 and the active mask included.  Also pins the hand-written list of
    state-dependent lanes: a dynamic entry missing from it would be dropped and show up here."""
    _lib, models, ops = _ops()
    md = models.quadrotor_model()
    assert ops.model_layout(md) == _lib.LAYOUT_TILE16C
    assert ops.model_layout(models.quadrotor_model(integrator="rk4")) == _lib.LAYOUT_TILE16R
    assert ops.record_stride(12, 4, _lib.LAYOUT_TILE16R) == 156 and ops.record_header(12, 4, _lib.LAYOUT_TILE16R) == 416
    assert ops.model_layout(models.cartpole_model()) == _lib.LAYOUT_ROWMAJOR
    assert ops.record_stride(12, 4, _lib.LAYOUT_TILE16C) == 76 and ops.record_header(12, 4, _lib.LAYOUT_TILE16C) == 416
    assert ops.record_header(12, 4, _lib.LAYOUT_TILE16) == 0
    rng = np.random.default_rng(23)
    # (the fused kernel refills its LDS stage every 25 steps: horizons of exactly one, one-and-a-bit, three, four, five stages)
    for B, N, t_start in ((67, 50, 0), (3, 17, 0), (130, 30, 21), (5, 50, 49), (9, 33, 1), (6, 25, 0), (5, 26, 0), (3, 75, 0),
                          (4, 100, 0), (2, 128, 3)):
        x = dev32(np.asarray(md.x_ref) + 0.4 * rng.standard_normal((B, N + 1, 12)))
        u = dev32(2.4525 + 1.5 * rng.standard_normal((B, N, 4)))          # some controls negative: barrier terms live
        out = {}
        for layout in (_lib.LAYOUT_TILE16, _lib.LAYOUT_TILE16C):
            rec, VxN, VxxN, _ = ops.linearize(md, x, u, t_start=t_start, layout=layout)
            out[layout] = ops.riccati_sweep(rec, VxN, VxxN, 12, 4, layout) + (rec,)
        Kf, kf, sf, rec_full = out[_lib.LAYOUT_TILE16]
        Kc, kc, sc, rec_c = out[_lib.LAYOUT_TILE16C]
        assert torch.equal(Kf, Kc) and torch.equal(kf, kc) and torch.equal(sf, sc)
        assert rec_c.numel() == 416 + B * (N - t_start) * 76
        # header = the entries of a full record that never change (compare two different steps of the full records)
        hdr = rec_c[:416]
        same = (rec_full.reshape(-1, 416) == rec_full.reshape(-1, 416)[0]).all(dim=0)
        assert torch.equal(hdr[same], rec_full.reshape(-1, 416)[0][same])
        active = torch.ones(B, dtype=torch.int32, device=DEV); active[::2] = 0
        Kb = torch.full_like(Kc, -7.0); kb = torch.full_like(kc, -7.0)
        ops.riccati_sweep(rec_c, VxN, VxxN, 12, 4, _lib.LAYOUT_TILE16C, K=Kb, k=kb, active=active)
        assert torch.equal(Kb[1::2], Kc[1::2]) and bool((Kb[::2] == -7.0).all())
        # the fused kernel (the sweep's own wave linearises 16 steps at a time into LDS; no record buffer, terminal pair
        # formed in registers) is the same arithmetic again: bit-identical gains, t_start and the active mask included
        assert ops.model_fuses_sweep(md)
        Kz, kz, sz = ops.linearize_sweep(md, x, u, t_start=t_start)
        assert torch.equal(Kz, Kc) and torch.equal(kz, kc) and torch.equal(sz, sc)
        Kb = torch.full_like(Kc, -7.0); kb = torch.full_like(kc, -7.0)
        ops.linearize_sweep(md, x, u, t_start=t_start, K=Kb, k=kb, active=active)
        assert torch.equal(Kb[1::2], Kc[1::2]) and bool((Kb[::2] == -7.0).all()) and bool((kb[::2] == -7.0).all())
    # not a layout for foreign records or other models
    rk4q = models.quadrotor_model(integrator="rk4")
    assert ops.model_can_fuse_sweep(rk4q) and not ops.model_fuses_sweep(rk4q) and ops.model_fuses_sweep(models.cartpole_model())
    assert ops.linearize_sweep_scratch_bytes(md, 7, 30) == 0
    assert ops.linearize_sweep_scratch_bytes(models.quadrotor_model(integrator="rk4"), 7, 30, 4) == 7 * 26 * 132 * 4
    with pytest.raises(_lib.QuattroError):                   # the RK4 quadrotor's sweep needs its coefficient scratch
        ops.linearize_sweep(models.quadrotor_model(integrator="rk4"), x, u, scratch=torch.empty((16,), dtype=torch.uint8, device=DEV))
    with pytest.raises(NotImplementedError):
        ops.linearize(models.quadrotor_model(integrator="rk4"), x, u, layout=_lib.LAYOUT_TILE16C)
    with pytest.raises(NotImplementedError):
        ops.pack_derivs(*[torch.zeros((1, 2) + s, device=DEV) for s in ((12, 12), (12, 4), (12,), (4,), (12, 12), (4, 4), (4, 12))],
                        layout=_lib.LAYOUT_TILE16C)


@pytest.mark.parametrize("model", ["cartpole", "quadrotor"])
@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_short_and_odd_horizons_against_the_oracle(model, integ):
    """Horizons shorter than / not a multiple of the kernels' prefetch depths (rollouts: 4 steps ahead, sweep: 3 record
    buffers), odd batch sizes that leave half-empty waves: simulate, linearize + sweep, all-alpha rollouts and the fused
    line search against the fp64 oracle on the same inputs."""
    _lib, models, ops = _ops()
    md = models.model_by_name(model, integrator=integ)
    spec = _spec(model, 1 if integ == "rk4" else 0)
    rng = np.random.default_rng(31)
    for N in (1, 2, 3, 5, 7):
        B = 3 if N < 5 else 9
        x0 = np.asarray(md.x_ref) + 0.2 * rng.standard_normal((B, md.n))
        u = (2.4525 if model == "quadrotor" else 0.0) + 0.3 * rng.standard_normal((B, N, md.m))
        xs, cost = ops.simulate(md, dev32(x0), dev32(u))
        x_ref, cost_ref = o_lin.rollout_batched(spec, x0, u)
        assert rel_fro(xs.cpu().numpy(), x_ref) < 2e-6, (N, "simulate")
        assert np.max(np.abs(cost.cpu().numpy() - cost_ref) / np.abs(cost_ref)) < 2e-6
        layout = ops.model_layout(md)
        rec, VxN, VxxN, _ = ops.linearize(md, xs, dev32(u), layout=layout)
        K, k, st = ops.riccati_sweep(rec, VxN, VxxN, md.n, md.m, layout)
        assert int(st.abs().sum()) == 0
        blocks = o_lin.linearize_analytic(spec, xs.double().cpu().numpy(), u)
        kr, Kr = o_ilqr.riccati_sweep_batched(blocks)
        assert rel_fro(K.cpu().numpy(), Kr) < 5e-6 and rel_fro(k.cpu().numpy(), kr) < 5e-6, (N, "sweep")
        cand, xn, un = ops.rollout(md, xs, dev32(u), K, k, ops.ALPHAS, want_traj=True)
        Kh, kh = K.double().cpu().numpy(), k.double().cpu().numpy()
        xh = xs.double().cpu().numpy()
        for ai, a in enumerate(ops.ALPHAS):
            nx, nu, nc = o_lin.closed_loop_rollout_batched(spec, x0.astype(np.float32).astype(np.float64), xh, u.astype(np.float32).astype(np.float64), kh, Kh, a)
            assert rel_fro(xn[ai].cpu().numpy(), nx) < 1e-5 and rel_fro(un[ai].cpu().numpy(), nu) < 1e-5, (N, a)
            assert np.max(np.abs(cand[ai].cpu().numpy() - nc) / np.abs(nc)) < 1e-5, (N, a)
        x_run, u_run, c_run = xs.clone(), dev32(u), cost.clone()
        idx = ops.linesearch(md, x_run, u_run, K, k, c_run, 1e-3)
        cand_h, idx_h = cand.cpu().numpy(), idx.cpu().numpy()
        for b in range(B):
            acc = np.nonzero(cand_h[:, b] <= float(cost[b]))[0]
            assert idx_h[b] == (acc[0] if acc.size else -1)
            if acc.size:
                assert torch.equal(x_run[b], xn[acc[0], b]) and torch.equal(u_run[b], un[acc[0], b])


@pytest.mark.parametrize("model", ["cartpole", "quadrotor"])
def test_line_search_with_one_and_with_eight_step_sizes(model):
    """n_alpha = 1 and n_alpha = QUATTRO_MAX_ALPHAS = 8 (all eight candidate slots of a trajectory in use): the fused
    line search agrees with the separate rollouts; 9 step sizes are refused."""
    _lib, models, ops = _ops()
    md = models.model_by_name(model)
    rng = np.random.default_rng(41)
    B, N = 11, 13
    x0 = dev32(np.asarray(md.x_ref) + 0.2 * rng.standard_normal((B, md.n)))
    u = dev32((2.4525 if model == "quadrotor" else 0.0) + 0.3 * rng.standard_normal((B, N, md.m)))
    xs, cost = ops.simulate(md, x0, u)
    layout = ops.model_layout(md)
    rec, VxN, VxxN, _ = ops.linearize(md, xs, u, layout=layout)
    K, k, _ = ops.riccati_sweep(rec, VxN, VxxN, md.n, md.m, layout)
    for alphas in ((0.3,), (4.0, 2.0, 1.0, 0.5, 0.25, 0.1, 0.05, 0.01)):
        cand, xn, un = ops.rollout(md, xs, u, K, k, alphas, want_traj=True)
        assert cand.shape == (len(alphas), B)
        x_run, u_run, c_run = xs.clone(), u.clone(), cost.clone()
        idx = ops.linesearch(md, x_run, u_run, K, k, c_run, 1e-3, alphas).cpu().numpy()
        cand_h = cand.cpu().numpy()
        for b in range(B):
            acc = np.nonzero(cand_h[:, b] <= float(cost[b]))[0]
            assert idx[b] == (acc[0] if acc.size else -1), (alphas, b)
            if acc.size:
                assert torch.equal(x_run[b], xn[acc[0], b]) and torch.equal(u_run[b], un[acc[0], b])
                assert float(c_run[b]) == cand_h[acc[0], b]
            else:
                assert torch.equal(x_run[b], xs[b]) and torch.equal(u_run[b], u[b])
    with pytest.raises(ValueError):
        ops.rollout(md, xs, u, K, k, tuple(0.1 * i for i in range(1, 10)))


def test_unpack_is_the_inverse_of_pack_and_reads_compact_records():
    """quattro_unpack_derivs_f32: pack -> unpack is the identity for every layout, and unpacking TILE16C records (header
    + state-dependent part) gives exactly the blocks of the full-record linearisation."""
    _lib, models, ops = _ops()
    g = load_golden("sweep_quadrotor_N30.npz")
    blocks = {k_: dev32(g[k_]) for k_ in BLOCKS}
    Bt = g["A"].shape[0]
    for layout in (_lib.LAYOUT_ROWMAJOR, _lib.LAYOUT_TILE16):
        rec, _ = ops.pack_derivs(*[blocks[k_] for k_ in BLOCKS], layout=layout)
        back = ops.unpack_derivs(rec, Bt, 12, 4, layout)
        for k_ in BLOCKS:
            assert torch.equal(back[k_], blocks[k_]), (layout, k_)
    gc = load_golden("sweep_cartpole_N30.npz")
    cb = {k_: dev32(gc[k_]) for k_ in BLOCKS}
    rec, lay = ops.pack_derivs(*[cb[k_] for k_ in BLOCKS])
    back = ops.unpack_derivs(rec, gc["A"].shape[0], 4, 1, lay)
    assert all(torch.equal(back[k_], cb[k_]) for k_ in BLOCKS)
    md = models.quadrotor_model()
    rng = np.random.default_rng(5)
    x = dev32(np.asarray(md.x_ref) + 0.3 * rng.standard_normal((7, 12, 12)))
    u = dev32(2.4525 + rng.standard_normal((7, 11, 4)))
    full = ops.unpack_derivs(ops.linearize(md, x, u, layout=_lib.LAYOUT_TILE16)[0], 7, 12, 4, _lib.LAYOUT_TILE16)
    comp = ops.unpack_derivs(ops.linearize(md, x, u, layout=_lib.LAYOUT_TILE16C)[0], 7, 12, 4, _lib.LAYOUT_TILE16C)
    for k_ in BLOCKS:
        assert torch.equal(full[k_], comp[k_]), k_


@pytest.mark.parametrize("model", ["cartpole", "quadrotor"])
def test_line_search_rejects_non_finite_and_exploding_candidates(model):
    """Gains that are NaN / inf / absurdly large: every candidate's cost is NaN, inf or astronomically high, the comparison
    `cand <= current` is false like in the reference, nothing is committed and the trajectory stops; its neighbours in the
    same wave are unaffected.  (Also exercises the large-argument branch of the device sin/cos: the exploding rollouts
    tumble through thousands of turns.)"""
    _lib, models, ops = _ops()
    md = models.model_by_name(model)
    rng = np.random.default_rng(43)
    B, N = 8, 20
    x0 = dev32(np.asarray(md.x_ref) + 0.1 * rng.standard_normal((B, md.n)))
    u = dev32((2.4525 if model == "quadrotor" else 0.0) + 0.1 * rng.standard_normal((B, N, md.m)))
    xs, cost = ops.simulate(md, x0, u)
    layout = ops.model_layout(md)
    rec, VxN, VxxN, _ = ops.linearize(md, xs, u, layout=layout)
    K, k, _ = ops.riccati_sweep(rec, VxN, VxxN, md.n, md.m, layout)
    good_x, good_u, good_c = xs.clone(), u.clone(), cost.clone()
    ops.linesearch(md, good_x, good_u, K, k, good_c, 1e-3)
    Kb, kb = K.clone(), k.clone()
    kb[1] = float("nan"); kb[3] = float("inf"); kb[4] = 1e6; Kb[6] *= -1e4          # 4: explodes; 6: violently unstable feedback
    x_run, u_run, c_run = xs.clone(), u.clone(), cost.clone()
    active = torch.ones(B, dtype=torch.int32, device=DEV)
    idx = ops.linesearch(md, x_run, u_run, Kb, kb, c_run, 1e-3, active=active).cpu().numpy()
    for b in (1, 3, 4):
        assert idx[b] == -1 and int(active[b]) == 0
        assert torch.equal(x_run[b], xs[b]) and torch.equal(u_run[b], u[b]) and float(c_run[b]) == float(cost[b])
    assert bool(torch.isfinite(x_run).all()) and bool(torch.isfinite(c_run).all())
    for b in (0, 2, 5, 7):                                   # untouched neighbours: same result as the clean run
        assert torch.equal(x_run[b], good_x[b]) and torch.equal(u_run[b], good_u[b])
    cand = ops.rollout(md, xs, u, Kb, kb, ops.ALPHAS)
    assert not bool(torch.isfinite(cand[:, 1]).any()) and not bool(torch.isfinite(cand[:, 3]).any())


def _indefinite_and_ill_conditioned_blocks():
    """Three golden quadrotor trajectories: 0 untouched, 1 with an indefinite, well conditioned l_uu at three steps, 2 with
    l_uu + 2.5e6 at two steps (condition number ~1e8).  -> the blocks, and the same rounded to fp32 and widened to fp64."""
    g = load_golden("sweep_quadrotor_N50.npz")
    blocks = {k: g[k][:3].copy() for k in BLOCKS + ["VxN", "VxxN"]}
    rng = np.random.default_rng(3)
    Qr, _ = np.linalg.qr(rng.standard_normal((4, 4)))
    ind = Qr @ np.diag([0.5, -0.3, 0.2, -0.1]) @ Qr.T
    for s in (49, 43, 10):
        blocks["luu"][1, s] = ind
    for s in (49, 30):
        blocks["luu"][2, s] = blocks["luu"][2, s] + 2.5e6 * np.ones((4, 4))
    d64 = {k: blocks[k].astype(np.float32).astype(np.float64) for k in blocks}
    return blocks, d64


def test_indefinite_and_ill_conditioned_quu_through_pack_derivs():
    """Foreign records (quattro_pack_derivs_f32) with a Q_uu + reg I the unpivoted TILE16 elimination must not be trusted
    on: (1) indefinite but well conditioned (eigenvalues of both signs) at three steps — the reference's np.linalg.inv
    (LAPACK, partial pivoting; quattro_ilqr_tf.py:306) handles it, so must we: the TILE16 kernel raises TRAJ_ILLCOND, the
    ROWMAJOR kernel (which pivots) matches the fp64 oracle, and ops.riccati_sweep(repair=True) reroutes exactly the
    flagged trajectories; (2) positive definite with condition number ~1e8 — beyond fp32 whatever the pivoting: flagged,
    values not compared; (0) the untouched golden trajectory stays unflagged and bit-identical."""
    _lib, models, ops = _ops()
    blocks, d64 = _indefinite_and_ill_conditioned_blocks()
    ko, Ko = o_ilqr.riccati_sweep_batched(d64)
    Quu = d64["luu"][1, 49] + d64["B"][1, 49].T @ d64["VxxN"][1] @ d64["B"][1, 49]
    ev = np.linalg.eigvalsh(0.5 * (Quu + Quu.T))
    assert ev.min() < -0.05 and ev.max() > 0.05 and np.abs(ev).min() > 0.02       # indefinite, comfortably invertible
    args = (dev32(blocks["VxN"]), dev32(blocks["VxxN"]), 12, 4)
    rec_t, _ = ops.pack_derivs(*[dev32(blocks[k]) for k in BLOCKS], layout=_lib.LAYOUT_TILE16)
    rec_r, _ = ops.pack_derivs(*[dev32(blocks[k]) for k in BLOCKS], layout=_lib.LAYOUT_ROWMAJOR)
    Kt, kt, st_t = ops.riccati_sweep(rec_t, *args, _lib.LAYOUT_TILE16)
    Kr, kr, st_r = ops.riccati_sweep(rec_r, *args, _lib.LAYOUT_ROWMAJOR)
    st_t, st_r = st_t.cpu().numpy(), st_r.cpu().numpy()
    assert st_t[0] == 0 and (st_t[1] & _lib.TRAJ_ILLCOND) and (st_t[2] & _lib.TRAJ_ILLCOND), st_t
    assert st_r[0] == 0 and st_r[1] == 0, st_r
    e_K, e_k = per_step_rel(Kr[1].cpu().numpy(), Ko[1]), per_step_rel_floor(kr[1].cpu().numpy(), ko[1], 0.05)
    print(f"indefinite Q_uu, pivoting (ROWMAJOR) kernel vs fp64 oracle: K {e_K:.2e}  k {e_k:.2e}")
    assert e_K < 5e-5 and e_k < 5e-5
    K2, k2, st2 = ops.riccati_sweep(rec_t, *args, _lib.LAYOUT_TILE16, repair=True)
    assert torch.equal(K2[0], Kt[0]) and torch.equal(k2[0], kt[0])                # unflagged: untouched
    assert torch.equal(K2[1], Kr[1]) and torch.equal(k2[1], kr[1])                # flagged: the pivoting kernel's result
    assert int(st2[0]) == 0 and int(st2[1]) == 0
    # the drop-in's backward_pass goes through the same repair (LinAlgError only for a truly singular block)
    e_t = per_step_rel(Kt[1].cpu().numpy(), Ko[1])
    print(f"same block through the unpivoted TILE16 elimination: K {e_t:.2e} (flagged, not used)")


def test_rk4_dense_f_records_against_the_full_record_path():
    """TILE16R (RK4 quadrotor: [A | B] dense per step, cost constants once in a header record, one lane per item with the
    stage points evaluated once) against the full TILE16 records of the 16-lanes-per-item kernel: the same derivative
    blocks to fp32 round-off (the two kernels group the stage arithmetic differently), the same gains through the sweep
    to 1e-5, ragged sizes and t_start > 0 included; the header holds exactly the entries that never change."""
    _lib, models, ops = _ops()
    md = models.quadrotor_model(integrator="rk4")
    rng = np.random.default_rng(31)
    for B, N, t_start in ((70, 50, 0), (3, 17, 0), (65, 30, 19)):
        x = dev32(np.asarray(md.x_ref) + 0.4 * rng.standard_normal((B, N + 1, 12)))
        u = dev32(2.4525 + 1.5 * rng.standard_normal((B, N, 4)))
        rec_f, VxN, VxxN, _ = ops.linearize(md, x, u, t_start=t_start, layout=_lib.LAYOUT_TILE16)
        rec_r, VxN2, VxxN2, lay = ops.linearize(md, x, u, t_start=t_start)
        assert lay == _lib.LAYOUT_TILE16R and rec_r.numel() == 416 + B * (N - t_start) * 156
        assert torch.equal(VxN, VxN2) and torch.equal(VxxN, VxxN2)
        df = ops.unpack_derivs(rec_f, B, 12, 4, _lib.LAYOUT_TILE16)
        dr = ops.unpack_derivs(rec_r, B, 12, 4, _lib.LAYOUT_TILE16R)
        for key in ("lx", "lu", "lxx", "luu", "lux"):
            assert torch.equal(df[key], dr[key]), key
        for key in ("A", "B"):
            err = float((df[key] - dr[key]).abs().max() / df[key].abs().max())
            assert err < 2e-6, (key, err)
        Kf, kf, sf = ops.riccati_sweep(rec_f, VxN, VxxN, 12, 4, _lib.LAYOUT_TILE16)
        Kr, kr, sr = ops.riccati_sweep(rec_r, VxN, VxxN, 12, 4, _lib.LAYOUT_TILE16R)
        assert int(sf.abs().sum()) == 0 and int(sr.abs().sum()) == 0
        for b in range(0, B, max(1, B // 7)):
            assert per_step_rel(Kr[b].cpu().numpy(), Kf[b].cpu().numpy()) < 1e-5, b
            assert per_step_rel_floor(kr[b].cpu().numpy(), kf[b].cpu().numpy(), 0.05) < 1e-5, b
        # the fused kernel (quattro_linearize_sweep_f32: stage points -> Jacobian coefficients by one lane per step, then
        # 4 steps x 16 unit directions per pass; no record buffer, terminal pair in registers): the same gains to 1e-5 per
        # step, every trajectory checked; active mask; status clean
        assert ops.model_can_fuse_sweep(md)
        Kz, kz, sz = ops.linearize_sweep(md, x, u, t_start=t_start)
        assert int(sz.abs().sum()) == 0
        worst_K = max(per_step_rel(Kz[b].cpu().numpy(), Kr[b].cpu().numpy()) for b in range(B))
        worst_k = max(per_step_rel_floor(kz[b].cpu().numpy(), kr[b].cpu().numpy(), 0.05) for b in range(B))
        print(f"fused RK4 sweep vs TILE16R records, B={B} N={N} t_start={t_start}: per-step rel K {worst_K:.2e} k {worst_k:.2e}")
        assert worst_K < 1e-5 and worst_k < 1e-5, (B, N, t_start, worst_K, worst_k)
        active = torch.ones(B, dtype=torch.int32, device=DEV); active[::2] = 0
        Kb = torch.full_like(Kz, -7.0); kb = torch.full_like(kz, -7.0)
        ops.linearize_sweep(md, x, u, t_start=t_start, K=Kb, k=kb, active=active)
        assert torch.equal(Kb[1::2], Kz[1::2]) and torch.equal(kb[1::2], kz[1::2])
        assert bool((Kb[::2] == -7.0).all()) and bool((kb[::2] == -7.0).all())
    with pytest.raises(NotImplementedError):                 # a layout of the RK4 quadrotor only
        ops.linearize(models.quadrotor_model(), x, u, layout=_lib.LAYOUT_TILE16R)


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_cartpole_lane_per_trajectory_sweep_equals_the_record_path(integ):
    """quattro_linearize_sweep_f32 for the cart-pole (a DPP quad of lanes per trajectory, everything in registers, no record buffer)
    against quattro_linearize_f32 + quattro_riccati_sweep_f32 through ROWMAJOR records: the same device-model code and the
    generic kernel's formulas term for term -> the same gains to fp32 round-off (the compiler contracts a few multiply-add
    pairs differently in the two kernels: measured <= 2e-6 per step) and the same status; ragged batch sizes (not a
    multiple of 64), t_start > 0, the active mask, a one-step horizon, and a non-finite input flagged the same way."""
    _lib, models, ops = _ops()
    md = models.cartpole_model(integrator=integ)
    assert ops.model_fuses_sweep(md)
    rng = np.random.default_rng(41)
    for B, N, t_start in ((1024, 50, 0), (67, 30, 0), (3, 17, 5), (130, 30, 29), (5, 1, 0)):
        x = dev32(np.asarray(md.x_ref) + 0.5 * rng.standard_normal((B, N + 1, 4)))
        u = dev32(2.0 * rng.standard_normal((B, N, 1)))
        if B > 3:
            x[3, t_start + (N - t_start) // 2, 2] = float("nan")       # inside the swept range
        rec, VxN, VxxN, lay = ops.linearize(md, x, u, t_start=t_start)
        assert lay == _lib.LAYOUT_ROWMAJOR
        Kr, kr, sr = ops.riccati_sweep(rec, VxN, VxxN, 4, 1, lay)
        Kz, kz, sz = ops.linearize_sweep(md, x, u, t_start=t_start)
        ok = torch.ones(B, dtype=torch.bool, device=DEV)
        if B > 3:
            ok[3] = False
            assert int(sz[3]) & _lib.TRAJ_NONFINITE and int(sr[3]) & _lib.TRAJ_NONFINITE
        assert torch.equal(sz[ok], sr[ok]), (B, N, t_start)
        Kzn, Krn, kzn, krn = (t[ok].cpu().numpy() for t in (Kz, Kr, kz, kr))
        worst = max(per_step_rel(Kzn[i], Krn[i]) for i in range(0, Kzn.shape[0], max(1, Kzn.shape[0] // 40)))
        assert worst < 1e-5, (B, N, t_start, worst)
        assert rel_fro(kzn, krn) < 1e-5
        active = torch.ones(B, dtype=torch.int32, device=DEV); active[::2] = 0
        Kb = torch.full_like(Kr, -7.0); kb = torch.full_like(kr, -7.0)
        ops.linearize_sweep(md, x, u, t_start=t_start, K=Kb, k=kb, active=active)
        assert bool((Kb[::2] == -7.0).all()) and bool((kb[::2] == -7.0).all())
        live = ok.clone(); live[::2] = False
        assert torch.equal(Kb[live], Kz[live]) and torch.equal(kb[live], kz[live])


# ---------------------------------------------------------------------------------------------- fused kernels vs the fp64 oracle, directly
@pytest.mark.parametrize("model,integ,golden", [("quadrotor", "euler", "sweep_quadrotor_N50.npz"), ("quadrotor", "rk4", "sweep_quadrotor_N30_rk4.npz"),
                                                ("cartpole", "euler", "sweep_cartpole_N50.npz"), ("cartpole", "rk4", "sweep_cartpole_N30_rk4.npz")])
def test_fused_linearize_sweep_kernels_against_the_fp64_oracle(model, integ, golden):
    """the kernels the headline and configs[1] actually run — quattro_linearize_sweep_f32 for the Euler
    quadrotor (MODE_FUSED), the RK4 quadrotor (MODE_FUSED_RK4, matrix-pipe forward mode) and the cart-pole (16-lane rows,
    both integrators) — compared DIRECTLY with the fp64 oracle (exact derivatives + fp64 sweep) instead of transitively
    through another HIP path: (i) on the reference's own golden trajectories (x_seq, u_seq of the G3/G4 fixtures), (ii) at
    N = 50 for B = 1024 and a ragged B = 37 of synthetic nominals.  Bound: 5e-6 relative Frobenius per trajectory (measured
    values are printed), t_start > 0 included."""
    _lib, models, ops = _ops()
    md = models.model_by_name(model, integrator=integ)
    spec = _spec(model, 1 if integ == "rk4" else 0)
    g = load_golden(golden)
    worst = {"K": 0.0, "k": 0.0}

    def check(x_np, u_np, t_start, tag):
        x, u = dev32(x_np), dev32(u_np)
        K, k, st = ops.linearize_sweep(md, x, u, t_start=t_start)
        assert int(st.abs().sum()) == 0
        blocks = o_lin.linearize_analytic(spec, x.double().cpu().numpy(), u.double().cpu().numpy(), t_start=t_start)
        kr, Kr = o_ilqr.riccati_sweep_batched(blocks)
        Kh, kh = K.double().cpu().numpy(), k.double().cpu().numpy()
        for b in range(Kh.shape[0]):
            eK, ek = rel_fro(Kh[b], Kr[b]), rel_fro(kh[b], kr[b])
            worst["K"], worst["k"] = max(worst["K"], eK), max(worst["k"], ek)
            assert eK < 5e-6 and ek < 5e-6, (tag, b, eK, ek)

    check(g["x_seq"], g["u_seq"], 0, "golden")
    check(g["x_seq"], g["u_seq"], g["x_seq"].shape[1] - 1 - 5, "golden tail of 5")
    rng = np.random.default_rng(2024)
    for B in (1024, 37):
        N = 50
        x0 = np.asarray(md.x_ref) + rng.uniform(-1, 1, (B, md.n)) * (0.3 if model == "quadrotor" else 0.5)
        u = (2.4525 if model == "quadrotor" else 0.0) + 0.3 * rng.standard_normal((B, N, md.m))
        xs, _ = ops.simulate(md, dev32(x0), dev32(u))
        check(xs.cpu().numpy(), u, 0, f"synthetic B={B}")
        if B == 37:
            check(xs.cpu().numpy(), u, 13, f"synthetic B={B} t_start=13")
    print(f"fused linearize+sweep vs fp64 oracle, {model} {integ}: worst rel-Fro K {worst['K']:.2e} k {worst['k']:.2e} (bound 5e-6)")


def test_rk4_rollouts_with_fast_and_slow_rotation_against_the_oracle():
    """The RK4 rollouts take a stage's sin / cos from the step's base values by angle addition while the stage angle stays
    within 0.25 rad of the base, and by the full reduction beyond (rollout_quad_body.h: stage_sincos).  Both branches against
    the fp64 oracle: gentle trajectories (every lane on the short path), fast-rolling ones (up to 120 rad/s: half a step turns
    the vehicle by 0.6 rad) and a mix inside one wave; open loop and through the closed-loop line search."""
    _lib, models, ops = _ops()
    from oracle import linearize as o_lin
    from oracle import models as o_models
    md = models.quadrotor_model(integrator="rk4")
    spec = o_models.quadrotor_spec(integrator=o_models.INTEGRATOR_RK4)
    rng = np.random.default_rng(77)
    B, N = 48, 20
    x0 = np.asarray(md.x_ref) + 0.2 * rng.standard_normal((B, 12))
    # rows 0-15 gentle, the rest rolling fast: 60-120 rad/s about the body x axis (half a step turns the vehicle by up to
    # 0.6 rad).  Pitch stays small, so the Euler-angle singularity at theta = pi/2 — where fp32 and fp64 part ways whatever the
    # trig — is not what this test measures
    x0[16:, 9] = rng.uniform(60, 120, B - 16) * rng.choice([-1.0, 1.0], B - 16)
    x0[16:32:2, 9] *= 0.3                                         # ... some in between (both branches inside one wave)
    u = 2.4525 + 0.3 * rng.standard_normal((B, N, 4))
    x0_32, u_32 = x0.astype(np.float32).astype(np.float64), u.astype(np.float32).astype(np.float64)
    xs_o, J_o = o_lin.rollout_batched(spec, x0_32, u_32)
    for sel in (slice(0, 16), slice(16, B), slice(0, B)):        # a wave of the simulate kernel holds 16 trajectories
        xs, J = ops.simulate(md, dev32(x0[sel]), dev32(u[sel]))
        xs = xs.double().cpu().numpy()
        scale = np.maximum(1.0, np.abs(xs_o[sel]).max(axis=(1, 2), keepdims=True))
        err = float(np.max(np.abs(xs - xs_o[sel]) / scale))
        assert err < 2e-5, (sel, err)                             # 20 RK4 steps at up to 120 rad/s in fp32
        assert float(np.max(np.abs(J.cpu().numpy() - J_o[sel]) / np.abs(J_o[sel]))) < 2e-5
    # closed loop: zero gains, alpha arbitrary -> every candidate reproduces the nominal; with feedback gains the candidates
    # differ and the oracle's closed-loop rollout is the reference
    K = dev32(0.01 * rng.standard_normal((B, N, 4, 12))); k = dev32(0.05 * rng.standard_normal((B, N, 4)))
    xs_t, _ = ops.simulate(md, dev32(x0), dev32(u))
    cost, x_new, u_new = ops.rollout(md, xs_t, dev32(u), K, k, want_traj=True)
    xs_nom = xs_t.double().cpu().numpy()
    for ai, alpha in enumerate(ops.ALPHAS):
        nx, nu, J = o_lin.closed_loop_rollout_batched(spec, x0_32, xs_nom, u_32, k.double().cpu().numpy(), K.double().cpu().numpy(), alpha)
        scale = np.maximum(1.0, np.abs(nx).max(axis=(1, 2), keepdims=True))
        assert float(np.max(np.abs(x_new[ai].double().cpu().numpy() - nx) / scale)) < 5e-5, alpha
        ok = np.isfinite(J) & (np.abs(J) < 1e12)
        assert float(np.max(np.abs(cost[ai].cpu().numpy()[ok] - J[ok]) / np.abs(J[ok]))) < 5e-5, alpha


def test_rk4_fused_vs_record_sweep_outliers_sit_at_the_euler_angle_singularity():
    """The RK4 quadrotor has two linearisation codes (TILE16R records by forward-mode columns; the fused sweep's stage
    Jacobians on the matrix pipe).  On random trajectories they agree per step to 2e-5 EXCEPT where a pitch angle comes
    within a few degrees of +-pi/2: the Euler-angle rates carry tan(theta) and 1 / cos(theta) (quadrotor_dynamics.py:122-124),
    the Jacobian entries grow like 1 / cos^2, and fp32 round-off of two different evaluation orders is amplified alike in both
    (either code is then equally far from the fp64 oracle).  Pinned here instead of in a script (VERDICT r3 #6b): every
    trajectory that exceeds the bound has min |cos(theta)| below 0.12 (theta within 7 degrees of the singularity), and every
    trajectory that stays clear of it (|cos| >= 0.12 throughout) is within the bound."""
    import quattro_ilqr_amd as q
    from quattro_ilqr_amd import ops
    md = q.quadrotor_model(integrator="rk4")
    rng = np.random.default_rng(3)
    n_out = n_clear = n_all = 0
    worst_clear = 0.0
    for N in (25, 50, 51):
        B = 1024
        x = torch.as_tensor(np.asarray(md.x_ref) + 0.4 * rng.standard_normal((B, N + 1, 12)), dtype=torch.float32, device=DEV).contiguous()
        u = torch.as_tensor(2.4525 + 1.5 * rng.standard_normal((B, N, 4)), dtype=torch.float32, device=DEV).contiguous()
        rec, VxN, VxxN, lay = ops.linearize(md, x, u)
        Kr, kr, sr = ops.riccati_sweep(rec, VxN, VxxN, 12, 4, lay)
        Kf, kf, sf = ops.linearize_sweep(md, x, u)
        e = ((Kf.double() - Kr.double()).flatten(2).norm(dim=2) / Kr.double().flatten(2).norm(dim=2)).max(dim=1).values    # (B,)
        # pitch angles the four RK4 stages of any step can reach: the nominal's, +- a stage's worth of motion
        cos_min = torch.cos(x[:, :-1, 7].double()).abs().min(dim=1).values
        out = e > 2e-5
        clear = cos_min >= 0.12
        assert not bool((out & clear).any()), (N, float(e[out & clear].max()), float(cos_min[out & clear].min()))
        n_out += int(out.sum()); n_clear += int(clear.sum()); n_all += B
        worst_clear = max(worst_clear, float(e[clear].max()))
        assert int(sr.abs().sum()) == 0 and int(sf.abs().sum()) == 0
    print(f"RK4 fused vs records: {n_out} of {n_all} random trajectories above 2e-5, all with min|cos(pitch)| < 0.12; "
          f"{n_clear} clear of the singularity, worst {worst_clear:.2e}")
    assert n_clear > 0.5 * n_all
    # ... and the phenomenon itself: one step of each trajectory pushed to within delta of the singularity
    B, N = 256, 30
    x = np.asarray(md.x_ref) + 0.2 * rng.standard_normal((B, N + 1, 12))
    delta = 10.0 ** rng.uniform(-3.0, -1.0, B)
    t_sing = rng.integers(0, N, B)
    x[np.arange(B), t_sing, 7] = np.where(rng.random(B) < 0.5, 1.0, -1.0) * (np.pi / 2 - delta)
    xt, ut = dev32(x), dev32(2.4525 + 0.5 * rng.standard_normal((B, N, 4)))
    rec, VxN, VxxN, lay = ops.linearize(md, xt, ut)
    Kr, _, _ = ops.riccati_sweep(rec, VxN, VxxN, 12, 4, lay)
    Kf, _, _ = ops.linearize_sweep(md, xt, ut)
    e = ((Kf.double() - Kr.double()).flatten(2).norm(dim=2) / Kr.double().flatten(2).norm(dim=2)).max(dim=1).values.cpu().numpy()
    out = np.nonzero(e > 2e-5)[0]
    assert out.size > 0, "no outlier even at the singularity: the bound of the first part is not being exercised"
    spec = _spec("quadrotor", o_models.INTEGRATOR_RK4)
    xs, us = xt[out].double().cpu().numpy(), ut[out].double().cpu().numpy()
    _, K_o = o_ilqr.riccati_sweep_batched(o_lin.linearize_analytic(spec, xs, us))
    err = lambda K: np.linalg.norm((K[out].double().cpu().numpy() - K_o).reshape(len(out), -1), axis=1) / np.linalg.norm(K_o.reshape(len(out), -1), axis=1)
    er, ef = err(Kr), err(Kf)
    print(f"at the singularity: {out.size} of {B} above 2e-5 (delta {delta[out].min():.1e} .. {delta[out].max():.1e}); distance to the fp64 "
          f"oracle: records median {np.median(er):.1e} max {er.max():.1e}, fused median {np.median(ef):.1e} max {ef.max():.1e}")
    # neither code is the wrong one: their distances to the fp64 oracle are of the same size
    assert np.median(ef) < 5 * np.median(er) + 1e-6 and np.median(er) < 5 * np.median(ef) + 1e-6


# ---------------------------------------------------------------------------------------------- tile sweep for any n <= 12, m <= 4
def _random_lq_problem(rng, B, S, n, m):
    """Random stable-ish dynamics and convex costs (the blocks a linearisation would hand to the sweep)."""
    A = np.eye(n) + 0.1 * rng.standard_normal((B, S, n, n))
    Bm = 0.3 * rng.standard_normal((B, S, n, m))
    def spd(k, lo):
        M = rng.standard_normal((B, S, k, k))
        return M @ np.swapaxes(M, -1, -2) * 0.2 + lo * np.eye(k)
    lxx, luu = spd(n, 0.5), spd(m, 0.3)
    lux = 0.05 * rng.standard_normal((B, S, m, n))
    lx, lu = rng.standard_normal((B, S, n)), 0.3 * rng.standard_normal((B, S, m))
    Mf = rng.standard_normal((B, n, n))
    VxxN = Mf @ np.swapaxes(Mf, -1, -2) * 0.3 + np.eye(n)
    VxN = rng.standard_normal((B, n))
    return dict(A=A, B=Bm, lx=lx, lu=lu, lxx=lxx, luu=luu, lux=lux, VxN=VxN, VxxN=VxxN)


def _rowmajor_records(d, n, m):
    """[A | B | l_xx | l_ux | l_uu | l_x | l_u] per (b, t), stride padded to 4 floats (include/quattro_hip.h)."""
    B, S = d["A"].shape[:2]
    flat = np.concatenate([d[k].reshape(B, S, -1) for k in ("A", "B", "lxx", "lux", "luu", "lx", "lu")], axis=2)
    stride = (flat.shape[2] + 3) // 4 * 4
    rec = np.zeros((B, S, stride))
    rec[:, :, :flat.shape[2]] = flat
    return rec


@pytest.mark.parametrize("n,m", [(12, 4), (6, 2), (4, 1), (7, 3), (12, 1), (3, 4), (1, 1), (11, 2)])
def test_tile_sweep_on_rowmajor_records_of_any_dims_against_the_fp64_oracle(n, m):
    """QUATTRO_LAYOUT_ROWMAJOR_TILE: the MFMA tile recursion on ROWMAJOR records of a problem with n <= 12, m <= 4, padded
    inside the kernel (unit pivots for the controls that are not there).  Against the fp64 oracle of the reference's recursion
    (quattro_ilqr_tf.py:297-317) on random convex problems: per-step gains to fp32 round-off; ragged batch, active mask,
    nothing written for a stopped trajectory."""
    _lib, models, ops = _ops()
    rng = np.random.default_rng(100 * n + m)
    B, S = 37, 23
    d = _random_lq_problem(rng, B, S, n, m)
    k_o, K_o = o_ilqr.riccati_sweep_batched(d)
    assert _lib.load().quattro_record_stride(n, m, _lib.LAYOUT_ROWMAJOR_TILE) == (2 * n * n + 2 * n * m + m * m + n + m + 3) // 4 * 4
    rec = dev32(_rowmajor_records(d, n, m))
    active = torch.ones((B,), dtype=torch.int32, device=DEV)
    active[5] = 0
    K = torch.full((B, S, m, n), -3.0, dtype=torch.float32, device=DEV)
    k = torch.full((B, S, m), -3.0, dtype=torch.float32, device=DEV)
    K, k, status = ops.riccati_sweep(rec, dev32(d["VxN"]), dev32(d["VxxN"]), n, m, _lib.LAYOUT_ROWMAJOR_TILE, K=K, k=k, active=active)
    assert int(status.abs().sum()) == 0
    live = np.arange(B) != 5
    eK = max(per_step_rel(K[b].cpu().numpy(), K_o[b]) for b in range(B) if live[b])
    ek = max(per_step_rel_floor(k[b].cpu().numpy(), k_o[b]) for b in range(B) if live[b])
    print(f"tile sweep on ROWMAJOR records n={n} m={m}: per-step K {eK:.2e} k {ek:.2e}")
    assert eK < 2e-5 and ek < 5e-5
    assert bool((K[5] == -3.0).all()) and bool((k[5] == -3.0).all())
    if (n, m) in ((12, 4), (4, 1)):                      # the generic (pivoting) kernel exists in the stock library for these
        Kg, kg, _ = ops.riccati_sweep(rec, dev32(d["VxN"]), dev32(d["VxxN"]), n, m, _lib.LAYOUT_ROWMAJOR)
        assert per_step_rel(K[live].cpu().numpy().reshape(-1, S, m * n).transpose(1, 0, 2), Kg[live].cpu().numpy().reshape(-1, S, m * n).transpose(1, 0, 2)) < 5e-6


def _indefinite_rowmajor_problem(B=6, S=5, n=12, m=4):
    """A random convex problem whose trajectory 2 has an indefinite l_uu (and a small B) at its last step."""
    rng = np.random.default_rng(9)
    d = _random_lq_problem(rng, B, S, n, m)
    d["luu"][2, S - 1] = np.diag([1.0, -0.8, 1.0, 0.5])          # indefinite at the last step of trajectory 2
    d["B"][2, S - 1] *= 0.01
    return d


def test_tile_sweep_on_rowmajor_records_flags_what_needs_pivoting():
    """An indefinite Q_uu + reg I: flagged ILLCOND by the tile sweep; ops.riccati_sweep(repair=True) sends exactly the flagged
    trajectories through the pivoting kernel ON THE SAME RECORDS (no repacking) and matches the fp64 oracle there."""
    _lib, models, ops = _ops()
    n, m = 12, 4
    B, S = 6, 5
    d = _indefinite_rowmajor_problem(B, S, n, m)
    k_o, K_o = o_ilqr.riccati_sweep_batched(d)
    rec = dev32(_rowmajor_records(d, n, m))
    K, k, status = ops.riccati_sweep(rec, dev32(d["VxN"]), dev32(d["VxxN"]), n, m, _lib.LAYOUT_ROWMAJOR_TILE)
    assert int(status[2]) & _lib.TRAJ_ILLCOND and int((status != 0).sum()) == 1
    K, k, status = ops.riccati_sweep(rec, dev32(d["VxN"]), dev32(d["VxxN"]), n, m, _lib.LAYOUT_ROWMAJOR_TILE, repair=True)
    assert int(status.abs().sum()) == 0
    assert per_step_rel(K[2].cpu().numpy(), K_o[2]) < 2e-5
