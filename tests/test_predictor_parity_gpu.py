"""GPU parity of the fused predictor (csrc/tf_stream.hip behind quattro_tf_forward_* / quattro_tf_gains_*) on the cases of
tests/predictor_cases.py, through TransformerILQR.load_arrays / predict_batch / predict_gains only.

Compared per case and operand type: whole-tensor relative Frobenius error, worst target token, worst output channel, each
against the fp64 oracle on operand-rounded weights and each bounded by 2 x the CPU-measured operand-rounding noise of that
case (predictor_cases.bound).  tests/test_predictor_cases_cpu.py shows that every mutant of predictor_cases.MUTANTS exceeds
such a bound by a stated multiple, so a kernel or packer with one of those mistakes fails here.
"""
import functools

import numpy as np
import pytest

import predictor_cases as pc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _tf(name, precision):
    from quattro_ilqr_amd import TransformerILQR
    cs = pc.case(name)
    tf = TransformerILQR(cs.n, cs.c, device=DEV, precision=precision).load_arrays(cs.w, cs.norm, cs.hp)
    assert tf.fused_kernel_covers()
    return tf


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _report(tag, q, bd):
    print(f"{tag}: " + ", ".join(f"{k} {q[k]:.2e} (bound {bd[k]:.2e})" for k in pc.QUANTITIES))


@pytest.mark.parametrize("precision", pc.PRECISIONS)
@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_kernel_within_twice_the_operand_noise(name, precision):
    cs = pc.case(name)
    x, p = cs.inputs(0)
    got = _tf(name, precision).predict_batch(_dev(x), _dev(p)).double().cpu().numpy()
    want = pc.reference(name, precision)
    assert got.shape == want.shape == (pc.B, cs.T, cs.c)
    assert np.isfinite(got).all()
    q, bd = pc.quantities(got, want), pc.bound(name, precision)
    _report(f"{name} {precision}", q, bd)
    for k in pc.QUANTITIES:
        assert q[k] <= bd[k], (k, q, bd)


def _many_inputs(cs, count):
    xs, ps = zip(*(cs.inputs(d) for d in range((count + pc.B - 1) // pc.B)))
    return _dev(np.concatenate(xs)[:count]), _dev(np.concatenate(ps)[:count])


@pytest.mark.parametrize("precision", pc.PRECISIONS)
@pytest.mark.parametrize("name", pc.WAVE_COUNT_CASES)
def test_no_state_crosses_between_sequences(name, precision):
    """Every row of a batch of 1, 2 or 257 is bit-identical to the same sequence run alone; gains mode writes the same bits;
    a sequence of NaN leaves every other row untouched."""
    cs, tf = pc.case(name), _tf(name, precision)
    n, m = pc.GAIN_DIMS[name]
    big = 257
    x, p = _many_inputs(cs, big)
    alone = torch.cat([tf.predict_batch(x[i:i + 1].contiguous(), p[i:i + 1].contiguous()) for i in range(big)])
    assert bool(torch.isfinite(alone).all())
    N = cs.ns - 1
    assert cs.T <= N
    for Bt in (1, 2, big):
        xb, pb = x[:Bt].contiguous(), p[:Bt].contiguous()
        out = tf.predict_batch(xb, pb)
        assert torch.equal(out, alone[:Bt]), Bt
        K = torch.full((Bt, N, m, n), 7.0, device=DEV)
        k = torch.full((Bt, N, m), 7.0, device=DEV)
        tf.predict_gains(xb, pb, K, k)
        rows = out.view(Bt, cs.T, m, 1 + n)
        assert torch.equal(k[:, :cs.T], rows[..., 0]) and torch.equal(K[:, :cs.T], rows[..., 1:]), Bt
        assert bool((K[:, cs.T:] == 7.0).all()) and bool((k[:, cs.T:] == 7.0).all())
        if Bt > 1:
            bad = Bt // 2
            xn = xb.clone()
            xn[bad] = float("nan")
            outn = tf.predict_batch(xn, pb)
            keep = torch.arange(Bt, device=DEV) != bad
            assert torch.equal(outn[keep], out[keep]), Bt
            assert bool(torch.isnan(outn[bad]).any())


@pytest.mark.parametrize("precision", pc.PRECISIONS)
def test_shifted_mean_equals_feeding_the_difference(precision):
    """predict_gains(x, ..., x_shift=s) normalises with x_mean + s: the prediction for x - s, within the case's bound."""
    name = "L81"
    cs, tf = pc.case(name), _tf(name, precision)
    n, m = pc.GAIN_DIMS[name]
    x, p = cs.inputs(0)
    g = np.random.default_rng(11)
    shift = (cs.norm["x_std"] * g.standard_normal(n)).astype(np.float32).astype(np.float64)
    assert np.abs(shift / cs.norm["x_std"]).min() > 1e-3
    raw = (x + shift).astype(np.float32).astype(np.float64)
    N = cs.ns - 1
    K = torch.zeros((pc.B, N, m, n), device=DEV)
    k = torch.zeros((pc.B, N, m), device=DEV)
    tf.predict_gains(_dev(raw), _dev(p), K, k, x_shift=shift)
    got = torch.cat([k[:, :cs.T, :, None], K[:, :cs.T]], dim=-1).reshape(pc.B, cs.T, cs.c).double().cpu().numpy()
    want = pc.evaluate(pc.rounded(name, precision), cs.norm, raw - shift, p)
    q, bd = pc.quantities(got, want), pc.bound(name, precision)
    _report(f"{name} {precision} shifted mean", q, bd)
    for kq in pc.QUANTITIES:
        assert q[kq] <= bd[kq], (kq, q, bd)
    # and the shift is not ignored: against the prediction for the unshifted x the distance is far outside the bound
    assert pc.quantities(got, pc.evaluate(pc.rounded(name, precision), cs.norm, raw, p))["fro"] > 10 * bd["fro"]
