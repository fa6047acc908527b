"""The predictor cases of tests/predictor_cases.py on the CPU, all fp64 (no GPU marker):

  1. the two optional arguments of oracle.transformer.forward leave the default evaluation bit-identical and do what they say;
  2. the case set covers the shapes at which csrc/tf_stream.hip takes another path;
  3. teeth: every mutant moves one of the three compared quantities by >= 10 x its fp16 bound somewhere, every case has a mask
     mutant and a bias mutant that bite, every mutant reaches >= 3 x a bf16 bound or is listed as fp16-only, none is idle;
  4. dropping K's bias is NOT a mistake (the softmax cancels it): the kernel may omit it;
  5. why this file exists: most of the mutants passed the assertion the suite had (whole-tensor rel_fro < 1.5e-2 on
     TransformerILQR.random_init models).
"""
import numpy as np
import pytest

import predictor_cases as pc
from conftest import rel_fro
from oracle import transformer as o_tf

TEETH_FP16, TEETH_BF16 = 10.0, 3.0
# mutants that no bf16 bound separates by 3 x: name -> the largest (shift / bf16 bound) over the cases, as measured.  The bf16
# parity test cannot be relied on for them; the fp16 one (>= 10 x, checked below) can.
FP16_ONLY = {"layernorm_variance_over_d_minus_1": 2.8}


def _ratios(mutant, precision):
    return {name: r for name in pc.CASE_NAMES if (r := pc.mutant_ratio(name, mutant, precision)) is not None}


# ------------------------------------------------------------------------------------------------ 1. the oracle's new arguments
def test_oracle_defaults_are_untouched_and_the_explicit_causal_mask_is_the_default():
    cs = pc.case("L61_straddle")
    x, p = cs.inputs()
    xn, pn = pc._normalise(cs.norm, x, p)
    a = o_tf.forward(cs.w, xn, pn, pc.NHEAD)
    assert np.array_equal(a, o_tf.forward(cs.w, xn, pn, pc.NHEAD, operand=None, mask=None))
    assert np.array_equal(a, o_tf.forward(cs.w, xn, pn, pc.NHEAD, mask=pc.causal_mask(cs.L)))
    one = o_tf.predict(cs.w, cs.norm, x[0], p[0], pc.NHEAD, cs.P)
    assert np.array_equal(one, o_tf.predict(cs.w, cs.norm, x[0], p[0], pc.NHEAD, cs.P, operand=None, mask=None))
    assert np.array_equal(one, pc.evaluate(cs.w, cs.norm, x[:1], p[:1])[0])
    with pytest.raises(ValueError):
        o_tf.forward(cs.w, xn, pn, pc.NHEAD, mask=pc.causal_mask(cs.L + 1))
    with pytest.raises(ValueError):
        o_tf.forward(cs.w, xn, pn, pc.NHEAD, operand="fp8")
    with pytest.raises(ValueError):
        o_tf.forward(cs.w, xn, pn, pc.NHEAD, dtype=np.float32, operand="fp16")


def test_operand_rounding_is_round_to_nearest_even_of_the_named_type():
    torch = pytest.importorskip("torch")
    g = np.random.default_rng(0)
    a = np.concatenate([g.standard_normal(4096) * 10.0 ** g.integers(-6, 5, 4096),
                        [0.0, -0.0, 1.0, 1.00390625, 1.01171875, 65504.0, 6e-8, 1e-40]]).astype(np.float32)   # ties, subnormals
    for name, t in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        want = torch.as_tensor(a).to(t).double().numpy()
        assert np.array_equal(o_tf.round_operand(a, name), want), name
    assert o_tf.round_operand(a, None) is a


@pytest.mark.parametrize("precision", pc.PRECISIONS)
def test_operand_noise_has_the_size_of_the_format(precision):
    """The noise model is neither silent nor wild: between 1/30 and 30 unit roundoffs of the operand type on a plain case,
    and the fp16 one sits well below the bf16 one everywhere."""
    u = 2.0 ** -9 if precision == "bf16" else 2.0 ** -12
    nz = pc.noise("L81", precision)
    assert u / 30 < nz["fro"] < 30 * u, nz
    for name in pc.CASE_NAMES:
        nb, nf = pc.noise(name, "bf16"), pc.noise(name, "fp16")
        assert all(nf[k] < 0.5 * nb[k] for k in pc.QUANTITIES), name
        assert all(nf[q] > 0 and nf["token"] >= nf["fro"] for q in pc.QUANTITIES), name


# ------------------------------------------------------------------------------------------------ 2. coverage of the case set
def test_case_set_covers_the_kernel_paths():
    cases = [pc.case(n) for n in pc.CASE_NAMES]
    rnd = [pc.case(n) for n in pc.SHAPES]
    Ls = {c.L for c in cases}
    assert {21, 61, 81, 101, 128, 32, 33} <= Ls
    assert {(c.L + 31) // 32 for c in rnd} == {1, 2, 3, 4}
    targets = lambda c: set(range(c.L - c.T, c.L))
    assert any({32, 64, 96} <= targets(c) for c in rnd)
    assert any(c.ns < 32 * k < c.ns + c.P for c in rnd for k in (1, 2, 3))              # a prompt across a tile edge
    assert any((c.L - c.T) % 32 == 0 for c in rnd)                                        # targets start on a tile
    assert {64, 1024} <= {c.ff for c in rnd} and any(c.ff > 512 for c in rnd)
    assert {64, 33, 5} <= {c.c for c in rnd}
    assert {1, 16} <= {c.n for c in rnd} and {1, 3} <= {c.layers for c in rnd}
    for c in cases:                                                                        # what fused_kernel_covers admits
        assert c.hp["d_model"] == 128 and c.hp["nhead"] == 4 and c.ff % 64 == 0 and 64 <= c.ff <= 1024
        assert c.c <= 64 and c.n <= 16 and c.L <= min(128, c.hp["max_seq_len"])
    for name in pc.WAVE_COUNT_CASES:
        n, m = pc.GAIN_DIMS[name]
        assert pc.case(name).n == n and pc.case(name).c == m * (1 + n)
    assert [(pc.case(n).L + 31) // 32 for n in pc.WAVE_COUNT_CASES] == [1, 2, 3, 4]


def test_random_cases_are_sharpened_and_non_trivially_normalised():
    for name in pc.SHAPES:
        cs = pc.case(name)
        for k in ("x_mean", "u_mean"):
            assert np.abs(cs.norm[k]).max() > 0.1
        for k in ("x_std", "u_std"):
            assert np.abs(cs.norm[k] - 1).max() > 0.05 and cs.norm[k].min() >= 0.5
        assert 0.2 < cs.w["transformer_decoder.layers.0.linear1.bias"].std() < 0.4
        assert 0.4 < cs.w["target_embedding"].std() < 0.6
        # peaked attention: the visible logits of a query spread over several units (uniform attention: a fraction of one)
        assert pc.layer0_logits(cs).std() > 2.0, name
    hard = pc.case("L61_hard_softmax")
    assert np.abs(pc.layer0_logits(hard)).max() > pc.HARD_LOGIT                        # exp() of it overflows fp32
    x, p = hard.inputs()
    assert np.isfinite(pc.evaluate(hard.w, hard.norm, x, p)).all()


def test_shipped_cases_use_the_recorded_rows():
    from conftest import load_golden
    for name, (model, rows) in pc.SHIPPED.items():
        g = load_golden(f"{rows}_{model}.npz")
        x, p = pc.case(name).inputs(0)
        assert np.array_equal(x[:2], g["x_err"][:2].astype(np.float32))
        assert np.array_equal(p[:2], g["prompt"][:2].astype(np.float32))
    # the oracle on the unrounded checkpoint reproduces the reference module's recorded fp32 output
    g = load_golden("tf_cartpole.npz")
    cs = pc.case("shipped_cartpole")
    x, p = cs.inputs(0)
    assert rel_fro(pc.evaluate(cs.w, cs.norm, x, p), g["pred_fp32"][:3]) < 1e-5


# ------------------------------------------------------------------------------------------------ 3. teeth
@pytest.mark.parametrize("mutant", list(pc.MUTANTS))
def test_every_mutant_bites_at_fp16_and_at_bf16_or_is_listed(mutant):
    r16, rb = _ratios(mutant, "fp16"), _ratios(mutant, "bf16")
    assert r16, f"{mutant} applies to no case"
    print(f"{mutant}: shift / bound, fp16 " + ", ".join(f"{n} {r:.1f}" for n, r in r16.items()))
    print(f"{mutant}: shift / bound, bf16 " + ", ".join(f"{n} {r:.1f}" for n, r in rb.items()))
    assert max(r16.values()) >= TEETH_FP16, r16
    if mutant in FP16_ONLY:
        # listed with its measured ratio: the list is neither stale nor an excuse
        assert max(rb.values()) < TEETH_BF16 and max(rb.values()) == pytest.approx(FP16_ONLY[mutant], rel=0.1), rb
    else:
        assert max(rb.values()) >= TEETH_BF16, rb


def test_no_mutant_is_idle():
    """A mutant that changed nothing anywhere would pass for 'caught' in no test at all: each moves the fp64 oracle by far more
    than round-off in at least one case."""
    for mutant in pc.MUTANTS:
        moved = [pc.mutant_shift(pc.case(n), mutant) for n in pc.CASE_NAMES]
        moved = [q for q in moved if q is not None]
        assert moved and max(q["fro"] for q in moved) > 1e-6, mutant
    assert set(FP16_ONLY) <= set(pc.MUTANTS)


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_every_case_has_a_mask_and_a_bias_mutant_that_bite(name):
    for kind in ("mask", "bias"):
        r = {m: pc.mutant_ratio(name, m, "fp16") for m, (k, _) in pc.MUTANTS.items() if k == kind}
        r = {m: v for m, v in r.items() if v is not None}
        print(f"{name}: {kind} mutants, shift / fp16 bound: " + ", ".join(f"{m} {v:.1f}" for m, v in r.items()))
        assert r and max(r.values()) >= TEETH_FP16, (kind, r)


# ------------------------------------------------------------------------------------------------ 4. what is not a mistake
@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_dropping_the_k_bias_changes_nothing(name):
    q = pc.k_bias_dropped(pc.case(name))
    assert max(q.values()) <= 1e-12, q


# ------------------------------------------------------------------------------------------------ 5. the old assertion
OLD_BOUND = 1.5e-2
OLD_SHAPES = [     # test_transformer_gpu.py::test_every_kernel_instantiation_against_the_oracle
    dict(n=4, c=5, ns=11, P=2, T=8, ff=64, layers=1),
    dict(n=4, c=5, ns=31, P=5, T=25, ff=192, layers=2),
    dict(n=12, c=52, ns=51, P=5, T=25, ff=320, layers=2),
    dict(n=12, c=52, ns=51, P=1, T=49, ff=1024, layers=1),
    dict(n=12, c=52, ns=64, P=32, T=32, ff=512, layers=3),
]


def test_the_whole_tensor_bound_on_unsharpened_models_let_most_mutants_through():
    """On models of TransformerILQR.random_init's distribution (near-uniform attention, biases of std 0.02, identity
    normalisation) at the five shapes the suite had: which mutants stay below rel_fro 1.5e-2 at EVERY shape, i.e. would have
    passed the only assertion there was."""
    invisible = []
    for mutant in pc.MUTANTS:
        worst = 0.0
        for i, sh in enumerate(OLD_SHAPES):
            w, norm, hp = pc.random_model(seed=7, sharp=False, **sh)
            cs = pc.Case(f"old{i}", w, norm, hp, sh["ns"], seed=5)
            q = pc.mutant_shift(cs, mutant, "bf16")
            if q is not None:
                worst = max(worst, q["fro"])
        passed = worst < OLD_BOUND
        print(f"{mutant:40s} worst whole-tensor rel_fro on the old models {worst:.2e}: "
              f"{'PASSED the old assertion' if passed else 'caught'}")
        if passed:
            invisible.append(mutant)
    assert len(invisible) >= 4, invisible
