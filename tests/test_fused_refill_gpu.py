"""The fused linearise + sweep kernel (Euler quadrotor) refills an LDS stage of 25 records at a time, two lanes per step,
over a constant image of the stage that it writes once per sweep.  Its gains must equal, bit for bit, those of the separate
linearisation into compact (TILE16C) records followed by the record sweep — around every edge of a refill: horizons of
one step, one stage less one, one stage, one stage and one, two stages less one, two, two and one, three; t_start > 0
(a partial first batch); one, two and 4096 trajectories."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _fused_vs_records(md, x, u, t_start):
    from quattro_ilqr_amd import _lib, ops
    rec, VxN, VxxN, _ = ops.linearize(md, x, u, t_start=t_start, layout=_lib.LAYOUT_TILE16C)
    Kc, kc, sc = ops.riccati_sweep(rec, VxN, VxxN, 12, 4, _lib.LAYOUT_TILE16C)
    Kz, kz, sz = ops.linearize_sweep(md, x, u, t_start=t_start)
    torch.cuda.synchronize()
    B, N = u.shape[0], u.shape[1]
    assert Kz.shape == (B, N - t_start, 4, 12) and kz.shape == (B, N - t_start, 4)
    assert torch.equal(_bits(Kz), _bits(Kc)), (N, B, t_start)
    assert torch.equal(_bits(kz), _bits(kc)), (N, B, t_start)
    assert torch.equal(sz, sc), (N, B, t_start)


@pytest.mark.parametrize("B", [1, 2, 4096])
@pytest.mark.parametrize("N", [1, 24, 25, 26, 49, 50, 51, 75])
def test_fused_refill_equals_compact_records_then_sweep(N, B):
    from quattro_ilqr_amd import models, ops
    md = models.quadrotor_model()
    assert ops.model_fuses_sweep(md)
    rng = np.random.default_rng(1000 * N + B)
    x = _dev32(np.asarray(md.x_ref) + 0.4 * rng.standard_normal((B, N + 1, 12)))
    u = _dev32(2.4525 + 1.5 * rng.standard_normal((B, N, 4)))          # some controls negative: barrier terms live
    for t_start in sorted({0, min(1, N - 1), N // 2, N - 1}):
        _fused_vs_records(md, x, u, t_start)


def test_fused_refill_with_large_angles():
    """Euler angles beyond qt_sincos's fast reduction (|angle| > 2048) on some steps: the wave-uniform slow path is taken
    while the two lanes of a step evaluate different angles."""
    from quattro_ilqr_amd import models
    md = models.quadrotor_model()
    rng = np.random.default_rng(7)
    B, N = 3, 50
    xh = np.asarray(md.x_ref) + 0.4 * rng.standard_normal((B, N + 1, 12))
    xh[0, 3::7, 6] = 3000.0 + rng.standard_normal(len(range(3, N + 1, 7)))      # phi
    xh[1, 5::9, 8] = -2.5e4 * (1.0 + rng.random(len(range(5, N + 1, 9))))       # psi
    xh[2, ::11, 7] = 1.0e5                                                       # theta
    u = _dev32(2.4525 + 0.5 * rng.standard_normal((B, N, 4)))
    _fused_vs_records(md, _dev32(xh), u, 0)
    _fused_vs_records(md, _dev32(xh), u, 13)
