"""GPU parity of the device training step (csrc/tf_train.hip behind quattro_tf_train_step_f32 / quattro_tf_adam_f32, through
train_hip.HipTrainer only) on the cases of tests/train_cases.py.

Compared per case: the loss, the prediction and, for every parameter block, whole-block, worst-row and worst-column distances
to the float64 restatement of `training.forward`, each bounded by MARGIN = 4 x the floor two fp32 CPU evaluations of the same
restatement leave (train_cases.bound).  tests/test_train_cases_cpu.py shows that every mutant of train_cases.MUTANTS exceeds such
a bound at least five-fold on the case built for it, so a kernel with one of those mistakes fails here.  Every test prints the
measured distance as a multiple of the floor (DESIGN.md §4.6 keeps the table).
"""
import numpy as np
import pytest

import train_cases as tc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _trainer(cs, dropout=0.0):
    from quattro_ilqr_amd import train_hip
    tr = train_hip.HipTrainer(*cs.shape, dropout, cs.pe, DEV)
    tr.load_state_dict({k: torch.as_tensor(v) for k, v in cs.params.items()})
    return tr


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _step(tr, batch, seed=0):
    """One forward_backward on the device: dict(loss, pred, grads) in float64, like train_cases.evaluate."""
    x, u, y = (_dev(a) for a in batch)
    loss, pred = tr.forward_backward(x, u, y, seed=seed, training=True, want_pred=True)
    flat = tr.grads.double().cpu()
    assert bool(torch.isfinite(flat).all()) and bool(torch.isfinite(pred).all())
    return dict(loss=float(loss.item()), pred=pred.double().cpu().numpy(),
                grads={k: tr.view(flat, k).numpy().copy() for k in tr.shapes})


def _within(tag, got, ref, fl):
    bd = tc.bound_of(fl)
    q = tc.compare(got, ref)
    scale = {k: v / tc.MARGIN for k, v in bd.items()}                  # the floor, zero floors replaced as in the bound
    key, r = tc.worst_ratio(q, scale)
    print(f"RATIO {tag}: worst distance / floor {r:.2f} at {key} ({q[key]:.2e}); loss {q['loss'] / scale['loss']:.2f}, "
          f"pred {max(q[k] / scale[k] for k in q if k.startswith('pred:')):.2f}")
    over = {k: (q[k], bd[k]) for k in q if not q[k] <= bd[k]}
    assert not over, (tag, over)


def _padding_is_zero(tr):
    member = torch.zeros(tr.n_params, dtype=torch.bool, device=DEV)
    for name in tr.shapes:
        tr.view(member, name).fill_(True)
    assert int(member.sum()) == sum(int(np.prod(s)) for _, _, s in tr.shapes.values()) <= tr.n_params
    assert bool((tr.grads[~member] == 0).all())


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_step_within_four_times_the_fp32_floor(name):
    cs = tc.case(name)
    tr = _trainer(cs)
    got = _step(tr, cs.batch())
    assert got["pred"].shape == (cs.B, cs.T, cs.c)
    _within(name, got, tc.reference(name), tc.floor(name))
    _padding_is_zero(tr)                    # the floats between blocks stay exactly zero (Adam would otherwise move them)


# ------------------------------------------------------------------------------------------------ 2. dropout
@pytest.mark.parametrize("name,p,seed", tc.DROPOUT_CASES)
def test_dropout_step_differentiates_the_network_it_evaluated(name, p, seed):
    """The masks the kernels hash on the fly, dumped through quattro_tf_train_dropout_mask_f32, go into the float64 reference and
    into the floor; they are the hash of train_cases.hashed_mask bit for bit, have the keep rate p says, and the high word of
    the seed starts another stream (independent streams differ in 2 p (1 - p) of the elements: 18 % at p = 0.1)."""
    cs = tc.case(name)
    tr = _trainer(cs, dropout=p)
    flat, other = {}, {}
    for s, n in cs.mask_sizes().items():
        flat[s] = tr.dropout_mask(seed, p, s, n).cpu().numpy()
        other[s] = tr.dropout_mask(seed + (1 << 32), p, s, n).cpu().numpy()
        kept = float((flat[s] > 0).mean())
        assert abs(kept - (1 - p)) < 0.02, (s, kept)
        assert float(flat[s].max()) == pytest.approx(1.0 / (1.0 - p), rel=1e-6) and float(flat[s].min()) == 0.0
        assert float((flat[s] != other[s]).mean()) > 0.10, s
        assert np.array_equal(flat[s], tc.hashed_mask(seed, p, s, n)), s
    masks = cs.shape_masks(flat)
    draws = tc.n_draws(name)
    refs = [tc.evaluate(cs.params, cs.pe, *cs.batch(d), cs.H, masks=masks) for d in range(draws)]
    got = _step(tr, cs.batch(), seed=seed)
    _within(f"{name} p={p} seed={seed:#x}", got, refs[0], tc.floor_of(cs, draws, masks=masks, refs=refs))
    _padding_is_zero(tr)
    # the masks matter, the two seeds give two networks, and evaluation ignores the rate
    assert tc.compare(got, tc.reference(name))["pred:fro"] > 1e-2
    l2 = float(tr.forward_backward(*(_dev(a) for a in cs.batch()), seed=seed + (1 << 32), training=True).item())
    assert l2 != got["loss"]
    l_eval, pred_eval = tr.evaluate(*(_dev(a) for a in cs.batch()))
    ev = dict(loss=float(l_eval.item()), pred=pred_eval.double().cpu().numpy())
    ref, bd = tc.reference(name), tc.bound(name)
    assert abs(ev["loss"] - ref["loss"]) <= bd["loss"] * abs(ref["loss"])
    q = tc.pc.quantities(ev["pred"], ref["pred"])
    assert all(q[k] <= bd[f"pred:{k}"] for k in q), q


# ------------------------------------------------------------------------------------------------ 3. state
def test_consecutive_steps_and_an_evaluation_between_them():
    name = "L65"
    cs = tc.case(name)
    tr = _trainer(cs)
    fl = tc.floor(name)
    _within(f"{name} first call", _step(tr, cs.batch(0)), tc.reference(name, 0), fl)
    before = tr.grads.clone()
    tr.evaluate(*(_dev(a) for a in cs.batch(1)))
    assert torch.equal(tr.grads, before)                               # an evaluation leaves the gradients alone
    _within(f"{name} second call", _step(tr, cs.batch(1)), tc.reference(name, 1), fl)
    _within(f"{name} third call", _step(tr, cs.batch(0)), tc.reference(name, 0), fl)


def test_small_batch_after_a_large_one_reads_nothing_stale_from_the_workspace():
    """HipTrainer keeps the largest workspace: after the batch of 41 a batch of 2 runs over the large batch's LayerNorm partial
    sums, softmax statistics and rows beyond its own."""
    big, small = tc.case("splitcap"), tc.case("splitcap_b2")
    tr = _trainer(big)
    _within("splitcap before splitcap_b2", _step(tr, big.batch()), tc.reference("splitcap"), tc.floor("splitcap"))
    ws = tr._ws.data_ptr()
    got = _step(tr, small.batch())
    assert tr._ws.data_ptr() == ws and tr._ws_batch == big.B           # the same buffer, not a new one
    _within("splitcap_b2 after splitcap", got, tc.reference("splitcap_b2"), tc.floor("splitcap_b2"))
    fresh = _step(_trainer(small), small.batch())
    assert np.array_equal(got["pred"], fresh["pred"])
    _padding_is_zero(tr)


# ------------------------------------------------------------------------------------------------ 4. Adam
@pytest.mark.parametrize("t", tc.ADAM_T)
def test_adam_update_and_both_moments_elementwise(t):
    """Δp, m and v of one step against float64 NumPy Adam on gradients whose magnitudes are log-uniform over 1e-10 .. 1 (so that
    eps = 1e-8 decides some updates) at step numbers up to 1e5; entries with g = m = v = 0 keep p bit-unchanged."""
    tr = _trainer(tc.case("L32"))
    n = tr.n_params
    prob = tc.adam_problem(n, t)
    p, g, m, v, dead = prob
    for dst, src in ((tr.params, p), (tr.grads, g), (tr.m, m), (tr.v, v)):
        dst.copy_(torch.as_tensor(src))
    tr.t, tr.lr = t - 1, 1e-3
    tr.adam_step()
    assert tr.t == t
    got = tuple(a.cpu().numpy() for a in (tr.params, tr.m, tr.v))
    assert all(np.isfinite(a).all() for a in got)
    assert np.array_equal(got[0][dead], p[dead]) and not got[1][dead].any() and not got[2][dead].any()
    fl = tc.adam_floor(prob, t)
    q = tc.adam_compare(got, tc.adam_step(p, g, m, v, t), prob, t)
    print(f"RATIO adam t={t}: " + ", ".join(f"{k} {q[k] / fl[k]:.2f} ({q[k]:.1e})" for k in tc.ADAM_QUANTITIES))
    for k in tc.ADAM_QUANTITIES:
        assert fl[k] > 0 and q[k] <= tc.MARGIN * fl[k], (k, q[k], fl[k])
