"""The training-step cases of tests/train_cases.py on the CPU (no GPU marker):

  1. the restatement is `training.forward`: values and every gradient, with and without explicit dropout factors, in float64;
     predictor_cases.random_model with its new keywords at their defaults draws the models it always drew;
  2. the case set reaches the regimes of csrc/tf_train.hip it was built for (launch arithmetic restated, not trusted);
  3. the bounds: none is zero, and MARGIN x floor(fro) of every block of every dropout-free case is at most 2e-5, ten times
     tighter than the per-block rel_fro < 2e-4 the suite had;
  4. teeth: every mutant moves a compared quantity of the case built for it to >= 5 x its bound, and leaves the neighbouring
     case it must not touch exactly unchanged;
  5. the record of what the old assertion (rel_fro < 2e-4 per block, `training.init_params` models, the seven old shapes) let
     through;
  6. Adam: the fp64 NumPy step is torch.optim.Adam, both Adam mutants exceed 5 x the bound of the GPU test and what the old Adam
     test made of them;
  7. shapes beyond the kernels' limits are refused by the library, which loads without a device.
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import predictor_cases as pc
import train_cases as tc


# ------------------------------------------------------------------------------------------------ 1. the restatement
def _autograd_of_training_forward(cs, draw=0, masks=None):
    from quattro_ilqr_amd import training
    x, u, y = (torch.as_tensor(a, dtype=torch.float64) for a in cs.batch(draw))
    W = {k: torch.as_tensor(v, dtype=torch.float64).requires_grad_(True) for k, v in cs.params.items()}
    buffers = {"pos_encoder.pe": torch.as_tensor(cs.pe, dtype=torch.float64)[None]}
    if masks is None:
        pred = training.forward(W, buffers, x, u, cs.H)
    else:
        pred = tc.forward_with_masks(W, buffers, x, u, cs.H, {s: m.reshape(-1) for s, m in masks.items()})
    loss = F.mse_loss(pred, y)
    loss.backward()
    return dict(loss=float(loss.detach()), pred=pred.detach().numpy(), grads={k: v.grad.numpy() for k, v in W.items()})


@pytest.mark.parametrize("name", ["L33", "L97", "hd1", "hd3", "d480", "n33_c65"])
def test_restatement_is_training_forward_with_its_autograd_gradients(name):
    cs = tc.case(name)
    q = tc.compare(tc.reference(name), _autograd_of_training_forward(cs))
    assert max(q.values()) < 1e-12, tc.worst_ratio(q, dict.fromkeys(q, 1.0))
    micro = tc.evaluate(cs.params, cs.pe, *cs.batch(), cs.H, micro=True)         # the second evaluation is the same function
    q = tc.compare(micro, tc.reference(name))
    assert max(q.values()) < 1e-12, tc.worst_ratio(q, dict.fromkeys(q, 1.0))


def test_restatement_with_explicit_dropout_factors_is_the_masked_forward():
    cs = tc.case("L33")
    masks = cs.shape_masks(tc.hashed_masks(cs, 1234567, 0.1))
    got = tc.evaluate(cs.params, cs.pe, *cs.batch(), cs.H, masks=masks)
    q = tc.compare(got, _autograd_of_training_forward(cs, masks=masks))
    assert max(q.values()) < 1e-12, q
    assert tc.compare(got, tc.reference("L33"))["pred:fro"] > 0.05                 # and the factors are not ignored
    ones = {s: torch.ones_like(m) for s, m in masks.items()}
    same = tc.evaluate(cs.params, cs.pe, *cs.batch(), cs.H, masks=ones)
    assert max(tc.compare(same, tc.reference("L33")).values()) < 1e-13
    q = tc.compare(tc.evaluate(cs.params, cs.pe, *cs.batch(), cs.H, masks=masks, micro=True), got)
    assert max(q.values()) < 1e-12, q


def test_hashed_masks_have_the_rate_and_independent_streams():
    for p in (0.1, 0.5):
        a, b = tc.hashed_mask(1234567, p, 0, 50000), tc.hashed_mask(1234567 + (1 << 32), p, 0, 50000)
        assert abs(float((a > 0).mean()) - (1 - p)) < 0.01
        assert set(np.unique(a)) == {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(p))}
        assert abs(float((a != b).mean()) - 2 * p * (1 - p)) < 0.01                # the high word of the seed starts another stream
        assert abs(float((a != tc.hashed_mask(1234567, p, 1, 50000)).mean()) - 2 * p * (1 - p)) < 0.01


# digests of (w, norm, hp) of predictor_cases.case(name) before random_model took d_model / nhead
_PREDICTOR_DIGESTS = {
    "L21_ff64_c5": "874651ef83985592", "L61_straddle": "d3495b9bd8c59b08", "L81": "4c2e608fd6f42fce",
    "L101_ff1024": "a324fa261f9ae510", "L128_3layers": "ee468f416ed1c51d", "L32_n1": "5edb553693901141",
    "L33_n16": "c9d121d83de7967b", "L104_tile_rows": "82bbd12a73b27678", "L64_c64": "983ae8d1a9a6d6c0",
    "L47_c33": "d61589f8fdbbaf82", "L61_hard_softmax": "043aa8be36ead9d1",
}


def _digest(w, norm, hp):
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k]).tobytes())
        h.update(str(w[k].dtype).encode())
    for k in sorted(norm):
        h.update(k.encode())
        h.update(np.ascontiguousarray(norm[k]).tobytes())
    h.update(repr(sorted(hp.items())).encode())
    return h.hexdigest()[:16]


def test_random_model_draws_the_predictor_cases_bit_for_bit():
    assert set(_PREDICTOR_DIGESTS) == set(pc.SHAPES)
    for name, want in _PREDICTOR_DIGESTS.items():
        cs = pc.case(name)
        assert _digest(cs.w, cs.norm, cs.hp) == want, name
    w, norm, hp = pc.random_model(seed=7, sharp=False, n=4, c=5, ns=11, P=2, T=8, ff=64, layers=1)
    assert _digest(w, norm, hp) == "2d11b6a90b72548b"
    # and the new keywords do what they say
    w, _, hp = pc.random_model(4, 5, 20, 4, 9, 64, 1, seed=1, d_model=480, nhead=15)
    assert w["transformer_decoder.layers.0.self_attn.in_proj_weight"].shape == (1440, 480) and hp["nhead"] == 15
    assert w["pos_encoder.pe"].shape == (1, 128, 480) and w["target_embedding"].shape == (9, 480)


# ------------------------------------------------------------------------------------------------ 2. the regimes
def test_case_set_reaches_the_regimes_it_names():
    C = {n: tc.case(n) for n in tc.CASE_NAMES}
    assert [C[n].L for n in ("L32", "L33", "L64", "L65", "L96", "L97", "L128_hd8")] == [32, 33, 64, 65, 96, 97, 128]
    assert (C["hd1"].hd, C["hd3"].hd, C["L128_hd8"].hd) == (1, 3, 8) and (C["hd1"].H, C["hd3"].H) == (64, 32)
    assert C["L33"].M == 99 and C["L33"].M % 4 and C["L33"].M % 16
    assert (C["d512"].d + 63) // 64 == 8 == (C["d480"].d + 63) // 64 and C["d480"].d % 64 == 32 and C["d512"].d % 64 == 0
    assert (C["n33_c65"].n, C["n33_c65"].c) == (33, 65)
    s = C["splitcap"]
    assert s.M == 5248 and (s.ff // 64) * (s.d // 64) == 32 and 1024 // 32 < (s.M + 127) // 128 == 41
    assert tc.gemm_split(s.ff, s.d, s.M) == (28, 192) and s.M - 27 * 192 == 64
    assert tc.ln_reduce_split(s.M) == (328, 6) and 328 - 54 * 6 == 4 and 55 * 6 >= 328
    assert tc.MUTANTS["split_tail_dropped"](s) == dict(w1_rows=(5184, 5248))
    assert tc.MUTANTS["ln_reduce_partial_slice_dropped"](s) == dict(norm2_rows=(16 * 324, 5248))
    # none of it ran before: at the old shapes the cap was never active, no slice was short of kchunk rounding and per was 1
    for name, (shape, B) in tc.OLD_SHAPES.items():
        n, c, d, H, layers, ff, NS, P, T = shape
        M = B * (NS + P + T)
        for rows_out, cols_out in ((ff, d), (d, ff), (3 * d, d), (d, d)):
            tiles = ((rows_out + 63) // 64) * ((cols_out + 63) // 64)
            assert 1024 // tiles >= (M + 127) // 128 and tc.gemm_split(rows_out, cols_out, M)[0] <= 6
        assert tc.ln_reduce_split(M)[1] == 1
    assert tc.layer0_logit_max(C["hard_softmax"]) > tc.HARD_LOGIT
    assert C["hard_softmax"].shape == C["L65"].shape
    for name in tc.CASES:
        cs = C[name]
        assert 0.2 < cs.params["transformer_decoder.layers.0.linear1.bias"].std() < 0.4, name
        assert 0.4 < cs.params["target_embedding"].std() < 0.6
        assert tc.layer0_logit_max(cs) > 3.0, name                                  # peaked attention
        assert cs.pe.shape[0] >= cs.L and cs.pe.shape[1] == cs.d
    for name in tc.SHIPPED:
        cs = C[name]
        x, u, y = cs.batch()
        assert cs.B == 6 and x.shape == (6, cs.NS, cs.n) and u.shape == (6, cs.P, cs.c) and y.shape == (6, cs.T, cs.c)
        assert cs._pool[2] is not None and np.isfinite(y).all() and y.std() > 0     # the recorded gains fit both checkpoints
    assert C["shipped_quadrotor"].shape == (12, 52, 128, 4, 3, 512, 51, 1, 49)
    for name, p, seed in tc.DROPOUT_CASES:
        assert name in tc.CASES and 0 < p < 1
    assert any(seed >> 32 for _, _, seed in tc.DROPOUT_CASES)


# ------------------------------------------------------------------------------------------------ 3. the bounds
@pytest.mark.parametrize("name", tc.CASE_NAMES + tuple(tc.AUX))
def test_no_bound_is_zero_and_every_block_is_bounded_ten_times_tighter_than_before(name):
    fl, bd = tc.floor(name), tc.bound(name)
    assert set(bd) == set(fl) and all(v > 0 and np.isfinite(v) for v in bd.values())
    assert all(bd[k] >= tc.MARGIN * fl[k] for k in fl)
    fro = {k: bd[k] for k in bd if k.endswith(":fro") and not k.startswith("pred:")}
    assert len(fro) == 7 + 12 * tc.case(name).layers
    k = max(fro, key=fro.get)
    print(f"{name}: largest MARGIN x floor(fro) {fro[k]:.2e} ({k}); loss {bd['loss']:.1e}, pred {bd['pred:fro']:.1e}, "
          f"largest row bound {max(v for j, v in bd.items() if j.endswith(':row')):.1e}")
    assert fro[k] <= tc.FRO_CEILING, (k, fro[k])
    assert bd["loss"] < 2e-6 and bd["pred:fro"] < 1e-5


def test_a_zero_floor_borrows_the_smallest_floor_of_its_quantity():
    fl = {"loss": 0.0, "a:fro": 0.0, "b:fro": 3e-7, "c:fro": 2e-7, "a:row": 1e-6, "b:row": 0.0, "pred:fro": 5e-7}
    bd = tc.bound_of(fl)
    assert bd["a:fro"] == tc.MARGIN * 2e-7 and bd["b:row"] == tc.MARGIN * 1e-6 and bd["loss"] == tc.MARGIN * 2.0 ** -24
    assert tc.MARGIN == 4.0


# ------------------------------------------------------------------------------------------------ 4. teeth
def _exactly_equal(a, b):
    return (a["loss"] == b["loss"] and np.array_equal(a["pred"], b["pred"])
            and all(np.array_equal(a["grads"][k], b["grads"][k]) for k in b["grads"]))


@pytest.mark.parametrize("mutant", [m for m, (who, _) in tc.CAUGHT_BY.items() if who not in ("any", "dropout")])
def test_mutant_is_caught_by_the_case_built_for_it(mutant):
    caught_by, untouched = tc.CAUGHT_BY[mutant]
    for name in caught_by:
        key, r = tc.mutant_ratio(name, mutant)
        print(f"{mutant} on {name}: {r:.3g} x bound at {key}")
        assert r >= tc.TEETH, (name, key, r)
    for name in untouched:
        got = tc.mutant_eval(tc.case(name), mutant)
        assert got is not None and _exactly_equal(got, tc.reference(name)), name


@pytest.mark.parametrize("mutant", [m for m, (who, _) in tc.CAUGHT_BY.items() if who == "any"])
def test_mutant_that_any_case_can_catch(mutant):
    r = {name: tc.mutant_ratio(name, mutant) for name in tc.CASE_NAMES}
    print(f"{mutant}: shift / bound " + ", ".join(f"{n} {v[1]:.3g} ({v[0]})" for n, v in r.items()))
    caught = [n for n, v in r.items() if v[1] >= tc.TEETH]
    print(f"{mutant}: caught by {len(caught)} of {len(r)} cases")
    assert caught, r


_MASKED = {}


def _masked_bound(name, p, seed):
    if (name, p, seed) not in _MASKED:
        cs = tc.case(name)
        masks = cs.shape_masks(tc.hashed_masks(cs, seed, p))
        ref = tc.evaluate(cs.params, cs.pe, *cs.batch(), cs.H, masks=masks)
        _MASKED[name, p, seed] = (masks, ref, tc.bound_of(tc.floor_of(cs, tc.n_draws(name), masks=masks)))
    return _MASKED[name, p, seed]


@pytest.mark.parametrize("name,p,seed", tc.DROPOUT_CASES)
def test_dropout_cases_catch_d_formed_without_the_attention_mask(name, p, seed):
    cs = tc.case(name)
    masks, ref, bd = _masked_bound(name, p, seed)
    assert all(v > 0 for v in bd.values())
    key, r = tc.worst_ratio(tc.compare(tc.mutant_eval(cs, "d_from_undropped_p", masks=masks), ref), bd)
    print(f"d_from_undropped_p on {name} at p = {p}: {r:.3g} x bound at {key}")
    assert r >= tc.TEETH, (key, r)
    # without dropout O is P V and the mutant is no mistake: exactly unchanged
    assert _exactly_equal(tc.mutant_eval(cs, "d_from_undropped_p"), tc.reference(name))
    # the other attention mutants bite under dropout too
    for mutant in ("bwd_diag_masked",):
        key, r = tc.worst_ratio(tc.compare(tc.mutant_eval(cs, mutant, masks=masks), ref), bd)
        assert r >= tc.TEETH, (mutant, key, r)


# ------------------------------------------------------------------------------------------------ 5. the old assertion
def test_what_the_per_block_rel_fro_2e_4_on_init_params_models_let_through():
    """Every mutant on the seven old shapes with the old `_setup` models (test_train_hip_gpu.py), float64 against float64: a
    mutant whose every block stays below rel_fro 2e-4 at every shape would have passed the assertion the suite had; one that
    cannot be made at any old shape was never run at all.  d_from_undropped_p goes through the old dropout test's two shapes
    (p = 0.1, B = 4).  As measured: see the printed record (DESIGN.md §4.6 keeps a copy)."""
    passed, unreachable = [], []
    for mutant in tc.MUTANTS:
        worst, reached = 0.0, False
        shapes = ("quadrotor", "small") if mutant == "d_from_undropped_p" else tuple(tc.OLD_SHAPES)
        for name in shapes:
            cs = tc.old_case(name, seed=5 if mutant == "d_from_undropped_p" else 3)
            masks = None
            if mutant == "d_from_undropped_p":
                x, u, y = (a[:4] for a in cs.batch())
                cs.B, cs.M = 4, 4 * cs.L
                cs.batch = lambda draw=0, b=(x, u, y): b
                masks = cs.shape_masks(tc.hashed_masks(cs, 1234567, 0.1))
            got = tc.mutant_eval(cs, mutant, masks=masks)
            if got is None:
                continue
            reached = True
            ref = tc.evaluate(cs.params, cs.pe, *cs.batch(), cs.H, masks=masks)
            q = tc.compare(got, ref)
            worst = max([worst] + [v for k, v in q.items() if k.endswith(":fro") and not k.startswith("pred:")])
        if not reached:
            unreachable.append(mutant)
            print(f"{mutant:36s} cannot be made at any old shape: that code never ran")
        else:
            print(f"{mutant:36s} worst per-block rel_fro on the old models {worst:.2e}: "
                  f"{'PASSED the old assertion' if worst < tc.OLD_BOUND else 'caught'}")
            if worst < tc.OLD_BOUND:
                passed.append(mutant)
    assert "ln_eps_1e-6" in passed, passed
    # n <= 12, c <= 52, d <= 128 and one block per LayerNorm reduction slice at every old shape
    assert set(unreachable) == {"ln_reduce_partial_slice_dropped", "stage_tail_dropped", "last_output_column_dropped",
                                "ln_last_lane_elements_dropped"}, unreachable


# ------------------------------------------------------------------------------------------------ 6. Adam
def test_numpy_adam_is_torch_optim_adam():
    r = np.random.default_rng(0)
    p0 = r.standard_normal(500)
    p, m, v = p0.copy(), np.zeros(500), np.zeros(500)
    ref = torch.as_tensor(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-3)
    for t in range(1, 8):
        g = r.standard_normal(500) * 10.0 ** r.uniform(-10, 0, 500)
        ref.grad = torch.as_tensor(g.copy())
        opt.step()
        p, m, v = tc.adam_step(p, g, m, v, t, abi=False)
        assert np.abs(p - ref.detach().numpy()).max() < 1e-15 * t, t


def test_adam_mutants_exceed_the_bound_of_the_gpu_test_and_what_the_old_test_made_of_them():
    """Both mutants are far outside MARGIN x floor on the gradients of the GPU test (|g| down to 1e-10, where eps = 1e-8 matters;
    t up to 1e5).  The old test (randn x 10^(step - 2), five steps, lr 2e-3, rel_fro of the parameters < 1e-6) was expected to
    let them through; restated here in float64 it does NOT: as measured, eps_inside_sqrt moves a block's parameters by 5e-3 (a
    standard-normal gradient times 0.01 has entries below 1e-4, where eps under the root changes the update by tens of per
    cent) and no_second_bias_correction by more (at t <= 5 the correction is a factor of 14 to 31 on the update).  What the
    old test left open is m and v themselves, t beyond 5 and gradients that are small everywhere."""
    n = 20000
    worst = dict.fromkeys(tc.ADAM_MUTANTS, 0.0)
    for t in tc.ADAM_T:
        prob = tc.adam_problem(n, t)
        p, g, m, v, dead = prob
        assert dead.sum() > n // 20 and (p[: n // 2][~dead[: n // 2]] == 0).all()
        assert np.abs(g[~dead]).min() < 1e-9 and np.abs(g).max() > 0.1
        fl = tc.adam_floor(prob, t)
        assert all(0 < fl[k] < 1e-6 for k in tc.ADAM_QUANTITIES), fl
        ref = tc.adam_step(p, g, m, v, t)
        for mutant in tc.ADAM_MUTANTS:
            q = tc.adam_compare(tc.adam_step(p, g, m, v, t, mutant=mutant), ref, prob, t)
            r = max(q[k] / (tc.MARGIN * fl[k]) for k in tc.ADAM_QUANTITIES)
            print(f"{mutant} at t = {t}: {r:.3g} x bound")
            worst[mutant] = max(worst[mutant], r)
    assert all(r >= tc.TEETH for r in worst.values()), worst
    # the old test
    cs = tc.old_case("small", seed=9)
    gen = torch.Generator().manual_seed(0)
    state = {mu: {k: (v.astype(np.float64), np.zeros(v.shape), np.zeros(v.shape)) for k, v in cs.params.items()}
             for mu in (None,) + tc.ADAM_MUTANTS}
    for step in range(5):
        for k in cs.params:
            g = torch.randn(cs.params[k].shape, generator=gen).numpy().astype(np.float64) * 10.0 ** (step - 2)
            for mu, st in state.items():
                st[k] = tc.adam_step(*((st[k][0], g) + st[k][1:]), step + 1, lr=2e-3, mutant=mu)
    old = {mu: max(np.linalg.norm(state[mu][k][0] - state[None][k][0]) / np.linalg.norm(state[None][k][0]) for k in cs.params)
           for mu in tc.ADAM_MUTANTS}
    print("old Adam test, worst per-block rel_fro of the parameters:", old)
    assert 1e-6 < old["eps_inside_sqrt"] < old["no_second_bias_correction"]


# ------------------------------------------------------------------------------------------------ 7. limits
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    from quattro_ilqr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    return _lib.load()


def test_every_case_has_kernels_and_shapes_beyond_the_limits_are_refused(lib):
    from quattro_ilqr_amd import _lib, train_hip
    for name in tc.CASE_NAMES:
        assert train_hip.supported(*tc.case(name).shape), name
    beyond = {"L = 129": (4, 5, 64, 2, 1, 64, 100, 4, 25), "head dimension 33": (4, 5, 66, 2, 1, 64, 20, 4, 9),
              "d_model = 576": (4, 5, 576, 18, 1, 64, 20, 4, 9)}
    for what, shape in beyond.items():
        n, c, d, H, layers, ff, NS, P, T = shape
        assert d % H == 0
        assert not train_hip.supported(*shape), what
        with pytest.raises(NotImplementedError):
            train_hip.HipTrainer(*shape, 0.0, np.zeros((NS + P + T, d), dtype=np.float32), "cpu")
        desc = train_hip._desc(*shape, 0.0)
        assert lib.quattro_tf_train_step_f32(ctypes.byref(desc), None, None, None, 0, None, None, None, None, 2, 0, 1, None,
                                             None, None) == _lib.ERR_UNSUPPORTED, what
        assert lib.quattro_tf_train_workspace_bytes(ctypes.byref(desc), 2) == 0
    # the limits themselves are inside
    for shape in ((4, 5, 64, 2, 1, 64, 100, 4, 24), (4, 5, 64, 2, 1, 64, 20, 4, 9), (4, 5, 512, 16, 1, 64, 20, 4, 9)):
        assert train_hip.supported(*shape)
