"""The tile sweep keeps three things off the vector ALU: the zero-pivot test behind QUATTRO_TRAJ_SINGULAR (scalar work on the pivot's
bit pattern), the LDS addresses of the fused mode's record loads (per-lane byte addresses stepped by a per-lane stride) and the
quotients of model parameters the Euler quadrotor's records are built from (divided once on the host for shared parameters).  None
of them may move a result:
  1. the status rule on hand-built records whose pivots are known without emulating anything, TILE16 and TILE16C, and one fused
     launch with a zero control weight;
  2. fused sweep against compact records + record sweep, bit for bit, with parameters whose quotients are inexact in fp32, over
     every residue of the three-fold unrolled step loop inside a full and a partial LDS batch;
  3. host quotients against device quotients inside the persistent kernel: a shared-parameter solve against a per-trajectory one
     whose rows all equal the shared set."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# quotients dt / mass, (Iy - Iz) / Ix, ..., arm / Ix, ..., kyaw / Iz all inexact in fp32
INEXACT_PHYS = (0.731, 0.0123, 0.0217, 0.0391, 0.171, 9.81, 0.0137)      # mass, Ix, Iy, Iz, arm, gravity, k_yaw
INEXACT_DT = 0.013


def _dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inexact_model():
    from quattro_ilqr_amd import models
    return models.quadrotor_model(dt=INEXACT_DT).with_(phys=INEXACT_PHYS)


# ------------------------------------------------------------------------------------------------ 1. the status rule
# n = 12, m = 4, reg = 0, A = B = 0, l_ux = 0, l_x = l_u = 0, l_xx = 2 I, V_xx(N) = V_x(N) = 0: Q_uu of every step is exactly the
# step's diagonal l_uu, the multipliers are zero, and pivot a of step t is l_uu[t][a][a] (or NaN once an earlier pivot has
# poisoned the value function).  One launch, B = 10, N = 4; steps are swept 3, 2, 1, 0: the three positions of the unrolled loop and
# its remainder.
STATUS_B, STATUS_N, TYPED_STEP = 10, 4, 2
HEALTHY = (1.0, 2.0, 3.0, 4.0)
#            row, step,       pivot, value
BAD_PIVOTS = ((1, TYPED_STEP, 0, 0.0),          # +0
              (2, TYPED_STEP, 2, -0.0),         # -0
              (3, TYPED_STEP, 3, 1e-40),        # a denormal: a pivot like any other (its reciprocal overflows: NONFINITE, not SINGULAR)
              (4, TYPED_STEP, 1, -1.0),         # negative: not singular (ILLCOND where pivots are checked)
              (5, TYPED_STEP, 0, float("nan")),  # NaN: not singular; the steps after it see NaN pivots only
              (6, 0, 0, 0.0), (7, 1, 1, 0.0), (8, 2, 2, 0.0), (9, 3, 3, 0.0))      # a single +0 at step 0, 1, 2, 3
SINGULAR_ROWS = (1, 2, 6, 7, 8, 9)              # exactly the rows with a pivot that is +0 or -0 (row 0 is healthy)
# The status words libquattro_hip.so returned for these inputs at the parent of the commit that moved the zero-pivot test to the
# scalar unit (v_min3_f32 on |pivot|, `!(pivmin > 0)` at the end), run once on an MI355X: NONFINITE = 1, SINGULAR = 2, ILLCOND = 4.
PARENT_STATUS_TILE16 = (0, 7, 7, 5, 4, 5, 7, 7, 7, 7)
PARENT_STATUS_TILE16C = (0, 3, 3, 1, 0, 1, 3, 3, 3, 3)


def status_rule_inputs():
    """-> (TILE16 records, TILE16C record buffer, VxN, VxxN) on the device."""
    from quattro_ilqr_amd import _lib, ops
    B, N = STATUS_B, STATUS_N
    luu = np.zeros((B, N, 4, 4), dtype=np.float32)
    for a in range(4):
        luu[:, :, a, a] = HEALTHY[a]
    for row, step, piv, val in BAD_PIVOTS:
        luu[row, step, piv, piv] = np.float32(val)
    assert np.signbit(luu[2, TYPED_STEP, 2, 2]) and luu[3, TYPED_STEP, 3, 3] > 0 and luu[3, TYPED_STEP, 3, 3] < np.finfo(np.float32).tiny
    lxx = np.tile(2.0 * np.eye(12, dtype=np.float32), (B, N, 1, 1))
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=DEV)
    rec16, _ = ops.pack_derivs(z(B, N, 12, 12), z(B, N, 12, 4), z(B, N, 12), z(B, N, 4), _dev32(lxx), _dev32(luu), z(B, N, 4, 12),
                               layout=_lib.LAYOUT_TILE16)
    # TILE16C by hand: the header is a TILE16 record of the constants (F = 0, l_xx = 2 I, l_ux = 0); a step's compact record holds
    # the F entries of the dynamic lanes (zero), l_uu row-major and l_z (zero)
    header, _ = ops.pack_derivs(z(1, 1, 12, 12), z(1, 1, 12, 4), z(1, 1, 12), z(1, 1, 4), _dev32(lxx[:1, :1]), z(1, 1, 4, 4),
                                z(1, 1, 4, 12), layout=_lib.LAYOUT_TILE16)
    stride = ops.record_stride(12, 4, _lib.LAYOUT_TILE16C)
    assert ops.record_header(12, 4, _lib.LAYOUT_TILE16C) == header.numel() and stride == 76
    compact = np.zeros((B, N, stride), dtype=np.float32)
    compact[:, :, 44:60] = luu.reshape(B, N, 16)
    rec16c = torch.cat([header.reshape(-1), _dev32(compact).reshape(-1)]).contiguous()
    return rec16, rec16c, z(B, 12), z(B, 12, 12)


@pytest.fixture(scope="module")
def status_words():
    from quattro_ilqr_amd import _lib, ops
    rec16, rec16c, VxN, VxxN = status_rule_inputs()
    _, _, s16 = ops.riccati_sweep(rec16, VxN, VxxN, 12, 4, _lib.LAYOUT_TILE16, reg=0.0)
    _, _, s16c = ops.riccati_sweep(rec16c, VxN, VxxN, 12, 4, _lib.LAYOUT_TILE16C, reg=0.0)
    torch.cuda.synchronize()
    out = {"TILE16": s16.cpu().numpy().tolist(), "TILE16C": s16c.cpu().numpy().tolist()}
    print("[sweep status words]", out)
    return out


@pytest.mark.parametrize("layout", ["TILE16", "TILE16C"])
def test_singular_bit_exactly_where_a_pivot_is_zero(status_words, layout):
    from quattro_ilqr_amd import _lib
    got = [b for b, w in enumerate(status_words[layout]) if w & _lib.TRAJ_SINGULAR]
    assert got == list(SINGULAR_ROWS), status_words[layout]


@pytest.mark.parametrize("layout,parent", [("TILE16", PARENT_STATUS_TILE16), ("TILE16C", PARENT_STATUS_TILE16C)])
def test_status_words_equal_the_parent_commits(status_words, layout, parent):
    assert status_words[layout] == list(parent)


def test_fused_sweep_reports_a_zero_control_weight():
    """Quadrotor with r[2] = 0, Qf = 0, no barrier, reg = 0, N = 1: Q_uu = l_uu + B^T V_xx(N) B = diag(2 r), so pivot 2 is +0.  The
    model constructors take such parameters.  The fused launch raises SINGULAR, returns the status word of the record path, and
    the same problem with r[2] = 0.01 is clean."""
    from quattro_ilqr_amd import _lib, models, ops
    base = models.quadrotor_model().with_(qf=(0.0,) * 12, barrier_alpha=0.0)
    rng = np.random.default_rng(3)
    x = _dev32(np.asarray(base.x_ref) + 0.1 * rng.standard_normal((2, 2, 12)))
    u = _dev32(2.4525 + 0.1 * rng.standard_normal((2, 1, 4)))
    for r2, singular in ((0.0, True), (0.01, False)):
        md = base.with_(r=(0.01, 0.01, r2, 0.01))
        _, _, sz = ops.linearize_sweep(md, x, u, reg=0.0)
        rec, VxN, VxxN, _ = ops.linearize(md, x, u, layout=_lib.LAYOUT_TILE16C)
        _, _, sc = ops.riccati_sweep(rec, VxN, VxxN, 12, 4, _lib.LAYOUT_TILE16C, reg=0.0)
        torch.cuda.synchronize()
        words = sz.cpu().numpy().tolist()
        assert [bool(w & _lib.TRAJ_SINGULAR) for w in words] == [singular] * 2, (r2, words)
        assert words == sc.cpu().numpy().tolist(), r2
        if not singular:
            assert words == [0, 0]


# ------------------------------------------------------------------------------------------------ 2. fused against records
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 6, 7, 26, 27, 28])
def test_fused_equals_records_with_inexact_quotients(N):
    """K, k and status of ops.linearize_sweep against ops.linearize (TILE16C) + ops.riccati_sweep, byte for byte: the record
    kernels divide on the device, the fused kernel takes the host's quotients and addresses its LDS records by stepped byte
    addresses.  N covers every residue of the unrolled-by-three step loop inside one LDS batch (25 steps) and across a refill;
    t_start 0 and 2 (where the horizon has that many steps), 1 and 3 trajectories."""
    from quattro_ilqr_amd import _lib, ops
    md = _inexact_model()
    assert ops.model_fuses_sweep(md)
    for B in (1, 3):
        rng = np.random.default_rng(100 * N + B)
        x = _dev32(np.asarray(md.x_ref) + 0.4 * rng.standard_normal((B, N + 1, 12)))
        u = _dev32(2.4525 * 0.731 + 1.5 * rng.standard_normal((B, N, 4)))       # some controls negative: barrier terms live
        for t_start in (0, 2):
            if t_start >= N:
                continue
            rec, VxN, VxxN, _ = ops.linearize(md, x, u, t_start=t_start, layout=_lib.LAYOUT_TILE16C)
            Kc, kc, sc = ops.riccati_sweep(rec, VxN, VxxN, 12, 4, _lib.LAYOUT_TILE16C)
            Kz, kz, sz = ops.linearize_sweep(md, x, u, t_start=t_start)
            torch.cuda.synchronize()
            assert Kz.shape == (B, N - t_start, 4, 12) and bool(torch.isfinite(Kz).all())
            assert torch.equal(_bits(Kz), _bits(Kc)), (N, B, t_start)
            assert torch.equal(_bits(kz), _bits(kc)), (N, B, t_start)
            assert torch.equal(sz, sc), (N, B, t_start)


# ------------------------------------------------------------------------------------------------ 3. persistent kernel
def test_shared_parameter_solve_equals_per_trajectory_rows_of_the_same_set():
    """B = 3, N = 5, two iterations: the shared-parameter persistent kernel reads the host's quotients from its argument block, the
    per-trajectory one divides each row's parameters on the device.  u, x, K, k and cost agree byte for byte."""
    import quattro_ilqr_amd as q
    md = _inexact_model()
    B, N = 3, 5
    rng = np.random.default_rng(17)
    x0 = np.asarray(md.x_ref) + rng.uniform(-1, 1, (B, 12)) * np.array([0.5, 0.5, 0.01, 0, 0, 0, 0.2, 0.2, 0.5, 0, 0, 0])
    u0 = 2.4525 * 0.731 + 0.1 * rng.standard_normal((B, N, 4))
    rows = np.tile(np.asarray(md.phys, dtype=np.float32), (B, 1))
    kw = dict(max_iter=2, tol=1e-12, device=DEV, tf_window=0)
    shared = {k_: v.clone() for k_, v in q.QuattroILQR(md, N, **kw).solve(x0, u0).items()}
    rowed = q.QuattroILQR(md, N, **kw).solve(x0, u0, model_phys=rows)
    assert int(shared["iters"].max()) == 2 and torch.equal(shared["iters"], rowed["iters"])
    for key in ("u", "x", "K", "k", "cost"):
        assert bool(torch.isfinite(shared[key]).all()), key
        assert torch.equal(_bits(shared[key]), _bits(rowed[key])), key
