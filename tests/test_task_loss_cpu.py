"""The tracking loss of the gain predictor, what needs no GPU (tests/task_loss_cases.py holds the cases, the NumPy restatements of
quattro_tf_gains_unpack_f32 / quattro_tf_gains_pack_grad_f32 and their mutants):
   1. the three new entries are declared, bound and exported;
   2. every ValueError / NotImplementedError of fit(loss="tracking") comes before anything touches a device;
   3. datagen.nominal_controls on a hand-built log;
   4. fit() and fit(loss="mse") are the same path;
   5. the inputs of the GPU parity cases are well-posed: in fp64 every trajectory's cost under the predicted gains is finite and below
      10 x the cost of its logged gains, and the pack flags nothing (the cap on excluded trajectories in every parity case is zero);
   6. the fp64 chain's d_pred is the derivative of the loss: central differences through unpack, 3 directions in pred_norm.
      Measured worst relative difference (h = 1e-6; all case names, both integrators, alpha 1 and 0.5): cart-pole 5.2e-8, quadrotor
      6.3e-9; asserted: 10 x that (task_loss_cases.FD_BOUND);
   7. teeth: every mutant moves d_pred, in the measure the GPU test asserts, to >= 10 x the GPU bound (2.2e-6 cart-pole, 2.7e-6
      quadrotor) on its named case (task_loss_cases.TEETH, rk4).  Measured:
          prompt layout [k | K.flat]                         6.9e15   quadrotor
          u_std left out of the gradient                     4.4e1    quadrotor
          u_mean left out of unpack                          3.1e1    quadrotor
          alpha not applied to the k slot                    9.8e-1   quadrotor, alpha 0.5
          rows t >= Tn given a gradient                      inf      quadrotor_T8 (a row that must be +0.0 is not)
          logged rows t >= Tn overwritten by the prediction  2.1e-2   cartpole (T = 5 < N = 7)
          scale of trajectory b + 1                          3.1e1    quadrotor
          division by B T c                                  9.9e-1   quadrotor
   8. the fp32 restatement of the pack stands within the pack's own rounding allowance of the fp64 pack, and flags what it should.
"""
import ctypes
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import task_loss_cases as tl

torch = pytest.importorskip("torch")

ENTRIES = ("quattro_tf_train_backward_f32", "quattro_tf_gains_unpack_f32", "quattro_tf_gains_pack_grad_f32")
CASES = [(name, integ) for name in tl.NAMES for integ in tl.gc.INTEGRATORS]


# ------------------------------------------------------------------------------------------------ 1. ABI
def test_the_three_entries_are_declared_bound_and_exported():
    from quattro_ilqr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    want = {
        ENTRIES[0]: [ctypes.POINTER(_lib.TfTrainDesc), P, P, P, ctypes.c_size_t, P, P, P, I, ctypes.c_uint64, I, P],
        ENTRIES[1]: [P, P, P, P, P, P, F, I, I, I, I, I, P, P, P],
        ENTRIES[2]: [P, P, P, P, P, F, F, P, P, F, I, I, I, I, I, P, P, P, P, P],
    }
    for name in ENTRIES:
        assert name in entry.declared_symbols() and name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name] == (ctypes.c_int, want[name])
        assert getattr(lib, name).argtypes == want[name] and getattr(lib, name).restype is ctypes.c_int
        assert hasattr(raw, name)
    # the backward takes the step's arguments without the target, the positional table, the loss and the prediction
    step = _lib.SIGNATURES["quattro_tf_train_step_f32"][1]
    assert want[ENTRIES[0]] == step[:7] + [P] + step[9:12] + [P]


# ------------------------------------------------------------------------------------------------ 2. errors before the device
def _toy(E=6, N=12, n=4, m=1, seed=0):
    r = np.random.default_rng(seed)
    return dict(x_seq=r.standard_normal((E, N + 1, n)).astype(np.float32), k_seq=r.standard_normal((E, N, m)).astype(np.float32),
                K_seq=r.standard_normal((E, N, m, n)).astype(np.float32)), r.standard_normal((E, N, m)).astype(np.float32)


def _tf(n=4, c=5, device="cuda:0"):
    import quattro_ilqr_amd as q
    return q.TransformerILQR(n, c, prompt_len=3, d_model=32, nhead=4, num_decoder_layers=1, dim_feedforward=64, dropout=0.0,
                             max_seq_len=40, device=device)


def test_fit_tracking_refuses_bad_arguments_before_anything_touches_a_device(monkeypatch):
    """The predictor sits on "cuda:0"; whatever reached a device would fail in another way (no GPU here) or, on a GPU box, trip the
    guard that replaces torch.as_tensor's device path."""
    import quattro_ilqr_amd as q
    from quattro_ilqr_amd import training
    real = torch.as_tensor

    def guarded(*a, **kw):
        assert kw.get("device") in (None, "cpu"), "a tensor was sent to a device"
        return real(*a, **kw)

    monkeypatch.setattr(torch, "as_tensor", guarded)
    md = q.models.cartpole_model()
    data, u_nom = _toy()
    fit = lambda tf=None, data=data, **kw: training.fit(_tf() if tf is None else tf, data, num_epochs=1, loss="tracking", **kw)
    with pytest.raises(ValueError, match="loss must be"):
        training.fit(_tf(), data, loss="cost")
    with pytest.raises(ValueError, match="needs task"):
        fit()
    with pytest.raises(ValueError, match="needs task"):
        fit(task=dict(u_nom=u_nom))
    with pytest.raises(ValueError, match="u_nom"):
        fit(task=dict(model=md))
    with pytest.raises(ValueError, match="u_nom"):
        fit(task=dict(model=md, u_nom=u_nom[:, :, 0]))
    with pytest.raises(ValueError, match="u_nom"):
        fit(task=dict(model=md, u_nom=u_nom[:4]))
    with pytest.raises(ValueError, match=r"N \+ 1"):
        fit(task=dict(model=md, u_nom=u_nom[:, :11]))                                  # x_seq.shape[1] != N + 1
    with pytest.raises(ValueError, match="K_seq"):
        fit(data=dict(data, K_seq=data["K_seq"][:, :11]), task=dict(model=md, u_nom=u_nom))
    with pytest.raises(ValueError, match="x0"):
        fit(task=dict(model=md, u_nom=u_nom, x0=np.zeros((6, 3))))
    with pytest.raises(ValueError, match="x_nom"):
        fit(task=dict(model=md, u_nom=u_nom, x_nom=data["x_seq"][:, :12]))
    with pytest.raises(ValueError, match=r"m \(1 \+ n\)"):
        fit(tf=_tf(c=8), task=dict(model=md, u_nom=u_nom))                             # control_dim != m (1 + n)
    with pytest.raises(ValueError, match="x_seq, k_seq and K_seq"):
        fit(data=(data["x_seq"], np.zeros((6, 12, 5), dtype=np.float32)), task=dict(model=md, u_nom=u_nom))
    with pytest.raises(ValueError, match="test_u_nom"):
        training.fit(_tf(), data, data, num_epochs=1, loss="tracking", task=dict(model=md, u_nom=u_nom))
    with pytest.raises(ValueError, match="backend"):
        fit(task=dict(model=md, u_nom=u_nom), backend="cuda")
    monkeypatch.setattr(training, "_dist_world", lambda distributed: (0, 2))
    with pytest.raises(NotImplementedError, match="one process"):
        fit(task=dict(model=md, u_nom=u_nom))
    monkeypatch.setattr(training, "_dist_world", lambda distributed: (0, 1))
    with pytest.raises(NotImplementedError, match="GPU"):
        fit(tf=_tf(device="cpu"), task=dict(model=md, u_nom=u_nom))


# ------------------------------------------------------------------------------------------------ 3. nominal controls
def test_nominal_controls_of_a_hand_built_log():
    from quattro_ilqr_amd import datagen
    N, n, m = 3, 2, 1
    traj = np.array([0, 0, 0, 1, 2, 2], dtype=np.int32)
    it = np.array([0, 1, 2, 0, 0, 1], dtype=np.int32)
    E = traj.size
    u_seq = (10.0 * np.arange(E)[:, None, None] + np.arange(N)[None, :, None] + np.zeros((E, N, m))).astype(np.float32)
    found = np.array([True, False, True, True, True, True])
    u_seq[1] = u_seq[0]                                # no accepted step at (trajectory 0, iteration 1): the controls stay
    z = lambda *s: np.zeros(s, dtype=np.float32)
    log = datagen.IterationLog(traj=traj, iteration=it, x_seq=z(E, N + 1, n), u_seq=u_seq, current_cost=np.zeros(E), k_seq=z(E, N, m),
                               K_seq=z(E, N, m, n), alpha=np.ones(E), new_x_seq=z(E, N + 1, n), new_u_seq=z(E, N, m),
                               new_cost=np.zeros(E), found_update=found)
    before = u_seq.copy()
    got = datagen.nominal_controls(log)
    assert got.shape == (E, N, m) and got.dtype == u_seq.dtype
    for e in (0, 3, 4):
        assert not got[e].any()                        # iteration 0: zeros, the solver's default
    assert np.array_equal(got[1], u_seq[0]) and np.array_equal(got[2], u_seq[1]) and np.array_equal(got[2], u_seq[0])
    assert np.array_equal(got[5], u_seq[4])
    u_init = (100.0 + np.arange(3)[:, None, None] + np.zeros((3, N, m))).astype(np.float32)
    got = datagen.nominal_controls(log, u_init)
    for e, tr in ((0, 0), (3, 1), (4, 2)):
        assert np.array_equal(got[e], u_init[tr])      # a first logged iteration 0 with a given u_init
    assert np.array_equal(got[1], u_seq[0]) and np.array_equal(got[5], u_seq[4])
    assert np.array_equal(log.u_seq, before)           # a pure function
    with pytest.raises(ValueError, match="predecessor"):
        datagen.nominal_controls(log.select(np.array([0, 2, 3])))
    with pytest.raises(ValueError, match="u_init"):
        datagen.nominal_controls(log, u_init[:, :2])
    with pytest.raises(ValueError, match="no row in u_init"):
        datagen.nominal_controls(log, u_init[:2])


# ------------------------------------------------------------------------------------------------ 4. the MSE path
def test_fit_with_its_defaults_and_fit_loss_mse_are_the_same_path(monkeypatch):
    from quattro_ilqr_amd import datagen, training
    from test_training_cpu import _toy_logs
    x, k, K = _toy_logs(24, 12, 4, 1, 0)
    data = datagen.create_dataset(x, k, K, 3)
    monkeypatch.setattr(training, "_fit_tracking", lambda *a, **kw: pytest.fail("the tracking path was taken"))
    a = _tf(device="cpu").fit(data, num_epochs=2, batch_size=8)
    b = _tf(device="cpu").fit(data, num_epochs=2, batch_size=8, loss="mse", task=None, init=None)
    assert a.train_loss_history == b.train_loss_history and a.fit_backend == b.fit_backend == "torch"
    assert all(np.array_equal(a._w[name], b._w[name]) for name in a._w)
    assert not hasattr(a, "diverged_history")
    # init= starts from the given state dict: zero epochs return it unchanged
    c = _tf(device="cpu").fit(data, num_epochs=0, init={name: w for name, w in a._w.items()})
    assert all(np.array_equal(a._w[name], c._w[name]) for name in a._w)
    with pytest.raises(ValueError, match="init"):
        _tf(device="cpu").fit(data, num_epochs=0, init={})
    # a loaded predictor as init keeps its normaliser as well; a state dict has the normaliser refitted to the data
    a._norm["u_std"] = a._norm["u_std"] * 2.0
    d = _tf(device="cpu").fit(data, num_epochs=0, init=a)
    assert np.array_equal(d._norm["u_std"], a._norm["u_std"]) and not np.array_equal(c._norm["u_std"], a._norm["u_std"])
    assert all(np.array_equal(a._w[name], d._w[name]) for name in a._w)


# ------------------------------------------------------------------------------------------------ 5. well-posed inputs
@pytest.mark.parametrize("name,integ", CASES)
def test_parity_inputs_stay_in_the_measured_regime(name, integ):
    cs = tl.case(name, integ)
    assert cs.pred_norm.shape == (cs.B, cs.T, cs.c) and cs.c == cs.m * (1 + cs.n) and cs.Tn == min(cs.T, cs.N)
    logged = tl.logged_cost(cs)
    assert np.all(np.isfinite(logged)) and np.all(logged > 0)
    for alpha in tl.ALPHAS:
        ch = tl.chain64(cs, alpha=alpha, scale=tl.scale_of(cs))
        ratio = ch["cost"] / logged
        print(f"[task loss inputs {name} {integ} alpha {alpha}] cost / logged-gains cost {np.round(ratio, 3)}  loss {ch['loss']:.6f}")
        assert np.all(np.isfinite(ch["cost"])) and np.all(ratio < tl.COST_CAP)
        assert not ch["diverged"].any() and np.all(np.isfinite(ch["d_pred"]))
        assert ch["loss"] == pytest.approx(float(np.sum(tl.scale_of(cs).astype(np.float64) * ch["cost"]) / cs.B), rel=1e-14)


# ------------------------------------------------------------------------------------------------ 6. finite differences
@pytest.mark.parametrize("name,integ", CASES)
def test_fp64_chain_is_the_derivative_of_the_loss_through_unpack(name, integ):
    cs = tl.case(name, integ)
    for alpha in tl.ALPHAS:
        e = tl.fd_error(cs, alpha)
        print(f"[task loss fd {name} {integ} alpha {alpha}] {e:.1e} (bound {tl.FD_BOUND[cs.model]:.1e})")
        assert e < tl.FD_BOUND[cs.model]


# ------------------------------------------------------------------------------------------------ 7. teeth
@pytest.mark.parametrize("mutant", tl.MUTANTS)
def test_every_mutant_stands_ten_bounds_away(mutant):
    assert set(tl.TEETH) == set(tl.MUTANTS)
    name, alpha = tl.TEETH[mutant]
    bound = tl.gpu_bound(tl.SHAPES[name][0])
    e = tl.mutant_error(name, mutant)
    print(f"[task loss teeth] {mutant}: {e:.1e} on {name}, alpha {alpha} (10 x bound {10 * bound:.1e})")
    assert e >= 10.0 * bound


# ------------------------------------------------------------------------------------------------ 8. the fp32 restatement
@pytest.mark.parametrize("name", tl.NAMES)
def test_fp32_pack_restatement_against_the_fp64_pack(name):
    cs = tl.case(name, "rk4")
    scale = tl.scale_of(cs)
    for alpha in tl.ALPHAS:
        ch = tl.chain64(cs, alpha=alpha, scale=scale)
        ref = ch["ref"]
        got = tl.pack(ref["grad_K"].astype(np.float32), ref["grad_u_nom"].astype(np.float32), ch["cost"], scale, cs.u_std, alpha, cs.T)
        assert got["d_pred"].dtype == np.float32 and not got["diverged"].any()
        # the inputs' rounding to fp32 (2^-24) and the pack's own roundings
        assert tl.d_pred_errors(cs, got["d_pred"], ch, alpha, scale) < tl.PACK_ROUNDINGS + 2.0 ** -24
        assert got["loss"] == pytest.approx(ch["loss"], rel=1e-14)
        # the MSE term: mse_kernel's gradient on top, the fp64 mean square in the loss
        mse = tl.pack(ref["grad_K"].astype(np.float32), ref["grad_u_nom"].astype(np.float32), ch["cost"], scale, cs.u_std, alpha, cs.T,
                      pred=cs.pred_norm, target=cs.target_norm, mse_weight=0.25)
        err = (cs.pred_norm - cs.target_norm).astype(np.float64)               # the fp32 difference, as mse_kernel forms it
        assert mse["loss"] == pytest.approx(ch["loss"] + 0.25 * float(np.mean(err ** 2)), rel=1e-12)
        assert np.allclose(mse["d_pred"] - got["d_pred"], 0.25 * 2.0 * err / err.size, rtol=1e-5, atol=1e-9)
    # a NaN cost and an infinite gradient element: flagged, zeroed, left out; the others unchanged
    gK, gu, cost = ref["grad_K"].astype(np.float32), ref["grad_u_nom"].astype(np.float32), ch["cost"].copy()
    clean = tl.pack(gK, gu, cost, scale, cs.u_std, 1.0, cs.T)
    cost[1] = np.nan
    gK[3, cs.N - 1, 0, 0] = np.inf
    bad = tl.pack(gK, gu, cost, scale, cs.u_std, 1.0, cs.T)
    assert bad["diverged"].tolist() == [0, 1, 0, 1, 0]
    assert not bad["d_pred"][[1, 3]].any() and not np.signbit(bad["d_pred"][[1, 3]]).any()
    assert np.array_equal(bad["d_pred"][[0, 2, 4]], clean["d_pred"][[0, 2, 4]])
    assert bad["loss"] == pytest.approx(clean["terms"][0] + clean["terms"][2] + clean["terms"][4], rel=1e-15)
