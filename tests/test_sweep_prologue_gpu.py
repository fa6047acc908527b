"""What the fused linearise + sweep kernel does before its first step (sweep_tile16_body.h, round 9): the first refill batch's
(x, u), the terminal state and the lane's entries of the argument block are requested first thing, the trajectory's `active`
flag is tested behind those requests, and the lane's entry of Qf for V_xx(N) is ONE load from a clamped index plus three selects.

ops.linearize_sweep, Euler quadrotor, N = 1, 24, 25, 26, 50, 51 (the refill batch of 25 steps and its edges), t_start = 0, N - 1
and 25 where it exists, B = 1, 2, 3 (a workgroup holds two trajectories) and B = 1030 (the instantiation for launches that fill the
chip), with `active` = None, all on, mixed and all off:
  * K, k and status equal, bit for bit, those of ops.linearize + ops.riccati_sweep -- the records path, which shares fill_const /
    fill_state with the fused refill and takes V_x(N), V_xx(N) from the linearisation kernel;
  * rows of inactive trajectories keep the poison they were preset to.
The cost weights are not the defaults: Q and Qf have twelve distinct diagonal entries each, so that an entry taken from the wrong
index cannot hide behind an equal neighbour."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NS = (1, 24, 25, 26, 50, 51)
POISON, POISON_ST = -777.25, 0x5A5A
Q = (10.0, 11.0, 50.0, 1.0, 1.25, 1.5, 9.0, 12.0, 40.0, 0.75, 1.75, 2.0)
QF = (100.0, 110.0, 500.0, 10.0, 12.5, 15.0, 90.0, 120.0, 400.0, 7.5, 17.5, 20.0)


def _ops():
    from quattro_ilqr_amd import _lib, models, ops
    return _lib, models, ops


def _dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _model():
    _, models, ops = _ops()
    md = models.quadrotor_model(integrator="euler").with_(q=Q, qf=QF)
    assert ops.model_fuses_sweep(md)
    return md


def _nominal(B, N, seed):
    rng = np.random.default_rng(seed)
    ref = np.zeros(12)
    ref[2] = 0.5
    x = ref + 0.2 * rng.standard_normal((B, N + 1, 12))
    u = rng.uniform(2.05, 4.0, (B, N, 4))
    return _dev32(x), _dev32(u)


def _t_starts(N):
    return sorted({0, N - 1} | ({25} if 25 < N else set()))


def _masks(B):
    out = [None, [1] * B, [0] * B]
    for m in ([b % 2 for b in range(B)], [(b + 1) % 2 for b in range(B)]):
        if m not in out:
            out.append(m)
    return out


def _check(md, x, u, t_start, masks):
    _lib, _, ops = _ops()
    B, N = u.shape[0], u.shape[1]
    S = N - t_start
    rec, VxN, VxxN, _ = ops.linearize(md, x, u, t_start=t_start, layout=_lib.LAYOUT_TILE16C)
    Kr, kr, sr = ops.riccati_sweep(rec, VxN, VxxN, 12, 4, _lib.LAYOUT_TILE16C)
    assert int(sr.abs().sum()) == 0, (B, N, t_start, sr)
    for mask in masks:
        K = torch.full((B, S, 4, 12), POISON, dtype=torch.float32, device=DEV)
        k = torch.full((B, S, 4), POISON, dtype=torch.float32, device=DEV)
        st = torch.full((B,), POISON_ST, dtype=torch.int32, device=DEV)
        act = None if mask is None else torch.as_tensor(np.asarray(mask, dtype=np.int32), device=DEV)
        ops.linearize_sweep(md, x, u, t_start=t_start, K=K, k=k, status=st, active=act)
        torch.cuda.synchronize()
        on = torch.ones(B, dtype=torch.bool, device=DEV) if act is None else act != 0
        tag = (B, N, t_start, "none" if mask is None else (mask if B < 8 else "mixed"))
        assert _same(K[on], Kr[on]) and _same(k[on], kr[on]) and torch.equal(st[on], sr[on]), tag
        assert bool((K[~on] == POISON).all()) and bool((k[~on] == POISON).all()) and bool((st[~on] == POISON_ST).all()), tag
        if act is not None:
            assert torch.equal(act, torch.as_tensor(np.asarray(mask, dtype=np.int32), device=DEV)), tag      # (flags are read only)


@pytest.mark.parametrize("N", NS)
def test_fused_sweep_against_the_records_path(N):
    md = _model()
    for B in (1, 2, 3):
        x, u = _nominal(B, N, 100 * N + B)
        for t_start in _t_starts(N):
            _check(md, x, u, t_start, _masks(B))


def test_fused_sweep_against_the_records_path_where_the_launch_fills_the_chip():
    """B = 1030 > 1024 SIMDs: sweep_tile16_kernel<MODE_FUSED, ROTATE = true>, the headline's instantiation; every third trajectory off"""
    md = _model()
    B = 1030
    for N, t_start in ((26, 0), (51, 25)):
        x, u = _nominal(B, N, 7 * N)
        _check(md, x, u, t_start, [None, [0 if b % 3 == 1 else 1 for b in range(B)]])
