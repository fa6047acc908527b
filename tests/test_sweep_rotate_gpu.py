"""The stand-alone fused sweep (Euler quadrotor) runs each refill batch of 25 steps — its epoch, E = 25 — under one of two
sets of s_setprio levels, chosen per wave from the hardware wave slot and the number of the batch (sweep_tile16_body.h, ROTATE).
Both bodies are the same steps, so nothing may change: the gains must equal the record path's bit for bit and stay inside the
fp64 oracle's bound of tests/test_kernels_gpu.py (5e-6 relative Frobenius per trajectory) at every edge of an epoch and of a
refill, where a wrong epoch loop would drop or repeat a step: N = 1, E - 1, E, E + 1, 2 E, 2 E + 1 (= 1, 24, 25, 26, 50, 51),
B = 1, 2, 9, t_start > 0, the hybrid iteration's in-place tail of one step, and one launch of B = 4096, N = 50, which fills every
wave slot of every SIMD.  The status words of a singular and of a non-finite trajectory come out as the record path's.
A launch of at most 1024 trajectories — a wave per SIMD, nothing to arbitrate — takes the kernel without the second body
(sweep_tile16.hip, ROTATE_ABOVE_B), so every case also runs at B = 1033: just above that threshold, odd, and with a last
workgroup of one wave."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E = 25                       # steps per epoch = FUSED_BATCH
HORIZONS = [1, E - 1, E, E + 1, 2 * E, 2 * E + 1]
assert sorted(set(HORIZONS + [24, 25, 26, 50, 51])) == HORIZONS      # the issue's list, for E = 25
BATCHES = [1, 2, 9, 1033]    # 1033 > ROTATE_ABOVE_B = 1024: the two-bodied kernel
ORACLE_BOUND = 5e-6          # tests/test_kernels_gpu.py::test_fused_linearize_sweep_kernels_against_the_fp64_oracle


def _dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _records_then_sweep(md, x, u, t_start, reg=None):
    from quattro_ilqr_amd import _lib, ops
    kw = {} if reg is None else {"reg": reg}
    rec, VxN, VxxN, _ = ops.linearize(md, x, u, t_start=t_start, layout=_lib.LAYOUT_TILE16C)
    return ops.riccati_sweep(rec, VxN, VxxN, 12, 4, _lib.LAYOUT_TILE16C, **kw)


def _assert_fused_equals_records(md, x, u, t_start):
    from quattro_ilqr_amd import ops
    Kc, kc, sc = _records_then_sweep(md, x, u, t_start)
    Kz, kz, sz = ops.linearize_sweep(md, x, u, t_start=t_start)
    torch.cuda.synchronize()
    B, N = u.shape[0], u.shape[1]
    assert Kz.shape == (B, N - t_start, 4, 12) and kz.shape == (B, N - t_start, 4)
    assert torch.equal(_bits(Kz), _bits(Kc)), (N, B, t_start)
    assert torch.equal(_bits(kz), _bits(kc)), (N, B, t_start)
    assert torch.equal(sz, sc), (N, B, t_start)
    return Kz, kz, sz


def _starts(N):
    # whole horizon; one step short; a partial first batch on either side of an epoch edge; the last step alone
    return sorted({0, min(1, N - 1), max(N - E - 1, 0), max(N - E, 0), max(N - E + 1, 0), N // 2, N - 1})


def _nominal(md, B, N, seed):
    """A rolled-out nominal (x from the device's own simulate, so that the oracle and the kernel linearise the same points)."""
    from quattro_ilqr_amd import ops
    rng = np.random.default_rng(seed)
    x0 = np.asarray(md.x_ref) + rng.uniform(-1, 1, (B, 12)) * 0.3
    u = _dev32(2.4525 + 0.3 * rng.standard_normal((B, N, 4)))
    x, _ = ops.simulate(md, _dev32(x0), u)
    return x, u


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("N", HORIZONS)
def test_fused_gains_equal_the_record_path_at_epoch_and_refill_edges(N, B):
    from quattro_ilqr_amd import models, ops
    md = models.quadrotor_model()
    assert ops.model_fuses_sweep(md)
    rng = np.random.default_rng(77 * N + B)
    x = _dev32(np.asarray(md.x_ref) + 0.4 * rng.standard_normal((B, N + 1, 12)))
    u = _dev32(2.4525 + 1.5 * rng.standard_normal((B, N, 4)))          # some controls negative: barrier terms live
    for t_start in _starts(N):
        _assert_fused_equals_records(md, x, u, t_start)


@pytest.mark.parametrize("B", [9, 1033])
@pytest.mark.parametrize("N", HORIZONS)
def test_fused_gains_against_the_fp64_oracle_at_epoch_and_refill_edges(N, B):
    from oracle import ilqr as o_ilqr
    from oracle import linearize as o_lin
    from oracle import models as o_models
    from quattro_ilqr_amd import models, ops
    md = models.quadrotor_model()
    spec = o_models.quadrotor_spec()
    x, u = _nominal(md, B, N, 500 + N)
    x64, u64 = x.double().cpu().numpy(), u.double().cpu().numpy()
    worst = 0.0
    for t_start in sorted({0, max(N - E - 1, 0), N - 1}):
        K, k, st = ops.linearize_sweep(md, x, u, t_start=t_start)
        assert int(st.abs().sum()) == 0
        kr, Kr = o_ilqr.riccati_sweep_batched(o_lin.linearize_analytic(spec, x64, u64, t_start=t_start))
        Kh, kh = K.double().cpu().numpy(), k.double().cpu().numpy()
        for b in range(B):
            eK = np.linalg.norm(Kh[b] - Kr[b]) / np.linalg.norm(Kr[b])
            ek = np.linalg.norm(kh[b] - kr[b]) / np.linalg.norm(kr[b])
            worst = max(worst, eK, ek)
            assert eK < ORACLE_BOUND and ek < ORACLE_BOUND, (N, t_start, b, eK, ek)
    print(f"fused sweep vs fp64 oracle, N = {N}, B = {B}: worst relative Frobenius error {worst:.2e} (bound {ORACLE_BOUND:.0e})")


@pytest.mark.parametrize("B", [9, 1033])
@pytest.mark.parametrize("N", [E, E + 1, 2 * E])
def test_in_place_tail_of_one_step(N, B):
    """The hybrid iteration's call: full gain stacks, only the last W = 1 step swept and written at its own row."""
    from quattro_ilqr_amd import models, ops
    md = models.quadrotor_model()
    x, u = _nominal(md, B, N, 900 + N)
    Ks, ks, ss = _assert_fused_equals_records(md, x, u, N - 1)
    K = torch.full((B, N, 4, 12), 7.0, dtype=torch.float32, device=DEV)
    k = torch.full((B, N, 4), 7.0, dtype=torch.float32, device=DEV)
    _, _, st = ops.linearize_sweep(md, x, u, t_start=N - 1, K=K, k=k, in_place=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(K[:, N - 1:]), _bits(Ks)) and torch.equal(_bits(k[:, N - 1:]), _bits(ks))
    assert bool((K[:, :N - 1] == 7.0).all()) and bool((k[:, :N - 1] == 7.0).all())      # the rows below are the caller's
    assert torch.equal(st, ss)


def test_full_launch_every_wave_slot():
    """B = 4096, N = 50: four waves on every SIMD, so every slot id and both bodies run in both batches."""
    from quattro_ilqr_amd import models
    md = models.quadrotor_model()
    B, N = 4096, 50
    x, u = _nominal(md, B, N, 4096)
    _, _, st = _assert_fused_equals_records(md, x, u, 0)
    assert int(st.abs().sum()) == 0


@pytest.mark.parametrize("B", [9, 1033])
def test_status_of_singular_and_non_finite_trajectories(B):
    """Status words as before, whichever body ran the step that raises them.  Singular: r[2] = 0, Qf = 0, no barrier, reg = 0 makes
    pivot 2 of the LAST step +0 (Q_uu = diag(2 r) there).  Non-finite: a NaN or infinite state in the nominal of three trajectories, in
    the first and in the second batch and at the refill edge."""
    from quattro_ilqr_amd import _lib, models, ops
    base = models.quadrotor_model().with_(qf=(0.0,) * 12, barrier_alpha=0.0)
    rng = np.random.default_rng(5)
    for N in (1, E + 1, 2 * E):
        x = _dev32(np.asarray(base.x_ref) + 0.1 * rng.standard_normal((B, N + 1, 12)))
        u = _dev32(2.4525 + 0.1 * rng.standard_normal((B, N, 4)))
        md = base.with_(r=(0.01, 0.01, 0.0, 0.01))
        _, _, sz = ops.linearize_sweep(md, x, u, reg=0.0)
        _, _, sc = _records_then_sweep(md, x, u, 0, reg=0.0)
        torch.cuda.synchronize()
        words = sz.cpu().numpy().tolist()
        assert all(w & _lib.TRAJ_SINGULAR for w in words), (N, words)
        assert words == sc.cpu().numpy().tolist(), N
    md = models.quadrotor_model()
    N = 2 * E
    xh = np.asarray(md.x_ref) + 0.2 * rng.standard_normal((B, N + 1, 12))
    xh[1, N - 3, 4] = np.nan          # first batch swept (steps 49 .. 25)
    xh[4, 7, 0] = np.nan              # second batch
    xh[8, E, 7] = np.inf              # the step at the refill edge
    x = _dev32(xh)
    u = _dev32(2.4525 + 0.1 * rng.standard_normal((B, N, 4)))
    _, _, sz = ops.linearize_sweep(md, x, u)
    _, _, sc = _records_then_sweep(md, x, u, 0)
    torch.cuda.synchronize()
    words = sz.cpu().numpy().tolist()
    assert [bool(w & _lib.TRAJ_NONFINITE) for w in words] == [b in (1, 4, 8) for b in range(B)], words
    assert words == sc.cpu().numpy().tolist()
