"""The tracking loss of the gain predictor on the GPU (quattro_tf_train_backward_f32, quattro_tf_gains_unpack_f32,
quattro_tf_gains_pack_grad_f32; train_hip.HipTrainer.forward / backward / tracking_step, training.tracking_loss, fit(loss="tracking")):
   1. the backward entry started from the MSE's own gradient against the step: the prediction bit for bit, the gradients within
      train_cases' MARGIN x floor, and bit for bit where the step itself repeats bit for bit;
   2. the backward entry from a gradient that is not an MSE's, against the fp64 restatement of (pred * d_pred).sum(), the floor by
      train_cases' procedure for that scalar, MARGIN unchanged;
   3. unpack against the NumPy fp32 restatement, bit for bit, with guard rows on both sides of each output;
   4. the loss gradient: d_pred of the pack about the device's own run against policy_cases.reference in fp64, bound
      policy_cases.gpu_bound + 2e-7; loss against the fp64 sum of the device's costs at 1e-12; and d_pred, flags and terms against the
      NumPy fp32 restatement bit for bit;
   5. divergence flags, without diverging anything;
   6. tracking_step against the same chain made from the public pieces;
   7. direction of descent: the central difference of the forward-only loss along the gradient agrees with |g| to 5 %, device path
      and torch path;
   8. fit(loss="tracking", backend="hip", init=...) end to end.
Cases, restatements, measures, mutants: tests/task_loss_cases.py, tests/test_task_loss_cpu.py."""
import numpy as np
import pytest

import param_cases as pc
import task_loss_cases as tl
import train_cases as tc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 1234.5


def _pkg():
    import quattro_ilqr_amd as q
    return q


def dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _trainer(tcs, dropout=0.0):
    from quattro_ilqr_amd import train_hip
    tr = train_hip.HipTrainer(*tcs.shape, dropout, tcs.pe, DEV)
    tr.load_state_dict({k: torch.as_tensor(v) for k, v in tcs.params.items()})
    return tr


def _grads(tr):
    flat = tr.grads.double().cpu()
    assert bool(torch.isfinite(flat).all())
    return {k: tr.view(flat, k).numpy().copy() for k in tr.shapes}


def _task(cs, alpha=1.0, scale=None, mse_weight=0.0):
    from quattro_ilqr_amd import train_hip
    md = pc.device_model(_pkg().models, cs.model, tl.SET, cs.integ)
    return train_hip.TrackingTask(md, dev32(cs.x_nom), dev32(cs.u_nom), dev32(cs.K_log), dev32(cs.k_log), dev32(cs.u_mean), dev32(cs.u_std),
                                  dev32(cs.x0), alpha=alpha, scale=None if scale is None else dev32(scale), mse_weight=mse_weight)


# ------------------------------------------------------------------------------------------------ 1. backward entry against the step
@pytest.mark.parametrize("name,p,seed", [("L33", 0.0, 0), ("L65", 0.0, 0), tc.DROPOUT_CASES[2]])
def test_backward_from_the_mse_gradient_is_the_step(name, p, seed):
    assert tc.DROPOUT_CASES[2][:2] == ("L33", 0.1)
    cs = tc.case(name)
    tr = _trainer(cs, dropout=p)
    x, u, y = (dev32(a) for a in cs.batch())
    steps = []
    for _ in range(2):
        loss, pred_step = tr.forward_backward(x, u, y, seed=seed, training=True, want_pred=True)
        steps.append((tr.grads.clone(), pred_step.clone(), float(loss.item())))
    tr.grads.fill_(float("nan"))                                           # the entry overwrites, as the step does
    pred = tr.forward(x, u, seed=seed, training=True)
    assert torch.equal(pred, steps[0][1]) and torch.equal(pred, steps[1][1])
    inv = torch.tensor(1.0, dtype=torch.float32, device=DEV) / torch.tensor(float(y.numel()), dtype=torch.float32, device=DEV)
    d_pred = ((2.0 * (pred - y)) * inv).contiguous()                       # mse_kernel: 2.0f * e * inv, inv = 1.0f / (float)n
    tr.backward(d_pred, x, u, seed=seed, training=True)
    got = dict(pred=pred.double().cpu().numpy(), grads=_grads(tr))
    tr.grads.copy_(steps[0][0])
    ref = dict(loss=steps[0][2], pred=steps[0][1].double().cpu().numpy(), grads=_grads(tr))
    if p > 0.0:
        masks = cs.shape_masks(tc.hashed_masks(cs, seed, p))
        fl = tc.floor_of(cs, tc.n_draws(name), masks=masks)
    else:
        fl = tc.floor(name)
    tl.within(f"backward vs step {name} p={p}", tl.grad_compare(got, ref), {k: v for k, v in fl.items() if k != "loss"})
    repeats = torch.equal(steps[0][0], steps[1][0])
    print(f"[backward vs step {name} p={p}] the step repeats bit for bit: {repeats}")
    if repeats:
        tr.backward(d_pred, x, u, seed=seed, training=True)
        assert torch.equal(tr.grads, steps[0][0])


# ------------------------------------------------------------------------------------------------ 2. any gradient
@pytest.mark.parametrize("name", ["L33", "L65"])
def test_backward_from_a_gradient_that_is_not_an_mse(name):
    cs = tc.case(name)
    d_pred = np.random.default_rng(3).standard_normal((cs.B, cs.T, cs.c)).astype(np.float32)
    fl, refs = tl.floor_linear(cs, d_pred, tc.n_draws(name))
    tr = _trainer(cs)
    x, u, _ = (dev32(a) for a in cs.batch())
    pred = tr.forward(x, u, seed=0, training=True)
    tr.backward(dev32(d_pred), x, u, seed=0, training=True)
    got = dict(pred=pred.double().cpu().numpy(), grads=_grads(tr))
    tl.within(f"backward, random d_pred, {name}", tl.grad_compare(got, refs[0]), fl)
    # the gradient is linear in d_pred: the MSE's gradient buffer of an earlier step is not read
    tr.forward_backward(x, u, dev32(cs.batch()[2]), seed=0, training=True)
    tr.forward(x, u, seed=0, training=True)
    tr.backward(dev32(d_pred), x, u, seed=0, training=True)
    tl.within(f"backward after a step, {name}", tl.grad_compare(dict(pred=got["pred"], grads=_grads(tr)), refs[0]), fl)


# ------------------------------------------------------------------------------------------------ 3. unpack
def _guarded(shape):
    """A sentinel-filled buffer with one guard row on each side of the (B, ...) block handed to the entry."""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[1:-1]


@pytest.mark.parametrize("B", [tl.B_CASE, 1])
@pytest.mark.parametrize("name", tl.NAMES)
def test_unpack_is_the_numpy_restatement_bit_for_bit(name, B):
    from quattro_ilqr_amd import train_hip
    cs = tl.case(name, "rk4", B)
    assert (cs.T < cs.N, cs.T == cs.N, cs.T > cs.N) == {"cartpole": (1, 0, 0), "quadrotor": (0, 1, 0), "quadrotor_T8": (0, 0, 1)}[name]
    for alpha in tl.ALPHAS:
        Kbuf, K = _guarded(cs.K_log.shape)
        ubuf, u_ff = _guarded(cs.u_nom.shape)
        assert K.is_contiguous() and u_ff.is_contiguous()
        train_hip.gains_unpack(dev32(cs.pred_norm), _task(cs, alpha), K, u_ff)
        K_ref, u_ref = tl.unpack(cs.pred_norm, cs.u_mean, cs.u_std, cs.K_log, cs.k_log, cs.u_nom, alpha)
        assert np.array_equal(K.cpu().numpy(), K_ref) and np.array_equal(u_ff.cpu().numpy(), u_ref)
        assert np.array_equal(K.cpu().numpy()[:, cs.Tn:], cs.K_log[:, cs.Tn:])                 # the logged rows, copied through
        for buf in (Kbuf, ubuf):
            assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all())
        # the layout mutant of the restatement is visible at this level too (with m = 1 the two layouts coincide)
        assert cs.m == 1 or not np.array_equal(tl.unpack(cs.pred_norm, cs.u_mean, cs.u_std, cs.K_log, cs.k_log, cs.u_nom, alpha,
                                            mutant="prompt layout")[0], K_ref)


# ------------------------------------------------------------------------------------------------ 4. loss gradient
def _device_chain(cs, task, pred, target=None):
    """unpack, ops.track, ops.score, ops.track_gradient, pack on the device -> dict of host arrays."""
    from quattro_ilqr_amd import train_hip
    q = _pkg()
    K, u_ff = train_hip.gains_unpack(pred, task)
    x, u = q.ops.track(task.model, task.x0, task.x_nom, u_ff, K, cs.N)
    cost, _ = q.ops.score(task.model, x, u, terminal=True, want_stage=False)
    g = q.ops.track_gradient(task.model, x, u, task.x_nom, K, want=("K",))
    out = train_hip.gains_pack_grad(g["grad_K"], g["grad_u_nom"], cost, task, cs.T, pred, target)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    host.update(K=K.cpu().numpy(), x=x.cpu().numpy(), u=u.cpu().numpy(), cost=cost.cpu().numpy(), grad_K=g["grad_K"].cpu().numpy(),
                grad_u_nom=g["grad_u_nom"].cpu().numpy())
    return host


@pytest.mark.parametrize("integ", tl.gc.INTEGRATORS)
@pytest.mark.parametrize("name", tl.NAMES)
def test_loss_gradient_against_the_fp64_reference_about_the_device_run(name, integ):
    bad = []
    for B in (tl.B_CASE, 1):
        cs = tl.case(name, integ, B)
        scale = tl.scale_of(cs)
        bound = tl.gpu_bound(cs.model)
        for alpha in tl.ALPHAS:
            got = _device_chain(cs, _task(cs, alpha, scale), dev32(cs.pred_norm))
            assert not got["diverged"].any() and np.all(np.isfinite(got["cost"]))
            d, ref = tl.reference_about(cs, got["x"], got["u"], got["K"])
            about = dict(d=d, ref=ref, x=got["x"].astype(np.float64), K=got["K"].astype(np.float64))
            e = tl.d_pred_errors(cs, got["d_pred"], about, alpha, scale)
            want = float(sum(np.float64(scale[b]) * got["cost"][b] / B for b in range(B)))
            e_loss = abs(float(got["loss"]) - want) / abs(want)
            print(f"[task loss gradient {name} {integ} B={B} alpha={alpha}] d_pred {e:.2e} (bound {bound:.2e})  loss {e_loss:.1e}")
            if not e < bound:
                bad.append((B, alpha, e))
            assert e_loss < 1e-12
            # every output is the NumPy restatement on the device's own inputs, bit for bit
            rs = tl.pack(got["grad_K"], got["grad_u_nom"], got["cost"], scale, cs.u_std, alpha, cs.T)
            assert np.array_equal(got["d_pred"], rs["d_pred"]) and not np.signbit(got["d_pred"][:, cs.Tn:]).any()
            assert np.array_equal(got["terms"], rs["terms"]) and float(got["loss"]) == rs["loss"]
    assert not bad, (bound, bad)


def test_pack_with_the_mse_term_is_the_numpy_restatement_bit_for_bit():
    cs = tl.case("quadrotor_T8", "rk4")
    scale = tl.scale_of(cs)
    got = _device_chain(cs, _task(cs, 0.5, scale, mse_weight=0.25), dev32(cs.pred_norm), dev32(cs.target_norm))
    rs = tl.pack(got["grad_K"], got["grad_u_nom"], got["cost"], scale, cs.u_std, 0.5, cs.T, pred=cs.pred_norm, target=cs.target_norm,
                 mse_weight=0.25)
    assert np.array_equal(got["d_pred"], rs["d_pred"]) and got["d_pred"][:, cs.Tn:].any()      # the unused row has an MSE gradient
    assert float(got["loss"]) == pytest.approx(rs["loss"], rel=1e-14) and np.allclose(got["terms"], rs["terms"], rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------------------ 5. divergence
def test_pack_flags_a_nan_cost_and_an_infinite_gradient_element_and_leaves_the_rest():
    from quattro_ilqr_amd import train_hip
    cs = tl.case("quadrotor", "rk4")
    task = _task(cs, 1.0, tl.scale_of(cs))
    base = _device_chain(cs, task, dev32(cs.pred_norm))
    gK, gu, cost = dev32(base["grad_K"]), dev32(base["grad_u_nom"]), torch.as_tensor(base["cost"], device=DEV)
    cost[1] = float("nan")
    gK[3, cs.N - 1, cs.m - 1, cs.n - 1] = float("inf")                        # the last element the wave looks at
    out = {k: v.cpu().numpy() for k, v in train_hip.gains_pack_grad(gK, gu, cost, task, cs.T).items()}
    assert out["diverged"].tolist() == [0, 1, 0, 1, 0] and base["diverged"].tolist() == [0] * 5
    for b in (1, 3):
        assert not out["d_pred"][b].any() and not np.signbit(out["d_pred"][b]).any() and out["terms"][b] == 0.0
    for b in (0, 2, 4):
        assert np.array_equal(out["d_pred"][b], base["d_pred"][b]) and out["terms"][b] == base["terms"][b]
    assert float(out["loss"]) == (base["terms"][0] + base["terms"][2]) + base["terms"][4]
    # a NaN in grad_u_nom alone, and a non-finite scale
    gK[3, cs.N - 1, cs.m - 1, cs.n - 1] = 0.0
    gu[4, 0, 0] = float("nan")
    task.scale[0] = float("inf")
    out = train_hip.gains_pack_grad(gK, gu, cost, task, cs.T)
    assert out["diverged"].tolist() == [1, 1, 0, 0, 1] and bool(torch.isfinite(out["d_pred"]).all())
    assert float(out["loss"]) == base["terms"][2] + base["terms"][3]


# ------------------------------------------------------------------------------------------------ 6. tracking_step
@pytest.mark.parametrize("name,mse_weight", [("cartpole", 0.0), ("quadrotor", 0.0), ("quadrotor_T8", 0.25)])
def test_tracking_step_is_the_chain_of_its_public_pieces(name, mse_weight):
    from quattro_ilqr_amd import train_hip
    q = _pkg()
    cs = tl.case(name, "rk4")
    task = _task(cs, 1.0, tl.scale_of(cs), mse_weight)
    tr = _trainer(cs.train)
    x, u, y = dev32(cs.x_norm), dev32(cs.prompt_norm), dev32(cs.target_norm)
    chains = []
    for _ in range(2):
        pred = tr.forward(x, u, seed=0, training=True)
        K, u_ff = train_hip.gains_unpack(pred, task)
        xs, us = q.ops.track(task.model, task.x0, task.x_nom, u_ff, K, cs.N)
        cost, _ = q.ops.score(task.model, xs, us, terminal=True, want_stage=False)
        g = q.ops.track_gradient(task.model, xs, us, task.x_nom, K, want=("K",))
        out = train_hip.gains_pack_grad(g["grad_K"], g["grad_u_nom"], cost, task, cs.T, pred, y)
        tr.backward(out["d_pred"], x, u, seed=0, training=True)
        chains.append((tr.grads.clone(), out["loss"].clone(), out["d_pred"].clone()))
    tr.grads.fill_(float("nan"))
    loss, diverged = tr.tracking_step(x, u, task, seed=0, training=True, target_norm=y if mse_weight else None)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and diverged.dtype == torch.int32 and diverged.tolist() == [0] * cs.B
    assert float(loss) == float(chains[0][1]) and np.isfinite(float(loss))
    # the CPU's fp64 chain from the CPU's fp32 prediction: the same number to fp32 accuracy of the run
    want = tl.chain64(cs, scale=tl.scale_of(cs))["loss"] + mse_weight * float(np.mean((cs.pred_norm - cs.target_norm).astype(np.float64) ** 2))
    print(f"[tracking_step {name}] loss {float(loss):.9f}, fp64 chain {want:.9f}")
    assert float(loss) == pytest.approx(want, rel=1e-4)
    repeats = torch.equal(chains[0][0], chains[1][0])
    print(f"[tracking_step {name}] the chain repeats bit for bit: {repeats}")
    got = dict(pred=cs.pred_norm, grads=_grads(tr))
    if repeats:
        assert torch.equal(tr.grads, chains[0][0])
    d_pred = chains[0][2].cpu().numpy()
    fl, refs = tl.floor_linear(cs.train, d_pred, 1)
    tr.grads.copy_(chains[0][0])
    tl.within(f"tracking_step vs chain {name}", tl.grad_compare(got, dict(refs[0], pred=cs.pred_norm, grads=_grads(tr))), fl)
    # a second call at the same batch size reuses the buffers
    before = {k: v.data_ptr() for k, v in tr._task_bufs[(cs.B, cs.N)].items()}
    loss2, _ = tr.tracking_step(x, u, task, seed=0, training=True, target_norm=y if mse_weight else None)
    assert {k: v.data_ptr() for k, v in tr._task_bufs[(cs.B, cs.N)].items()} == before and float(loss2) == float(chains[0][1])


# ------------------------------------------------------------------------------------------------ 7. direction of descent
def test_gradient_is_the_slope_of_the_forward_only_loss_device_and_torch_paths():
    """h from tests/task_loss_cases.descent_step (fp64 chain on the CPU, along the fp64 gradient): the central difference's truncation
    error is below 0.5 % of |g| and the fp32 loss noise 2 x 2^-23 x loss / h below 1 % of |g| -- asserted here; measured: h = 3e-3,
    truncation 0.11 %, noise 0.02 %.  Both paths must then agree with their own |g| to 5 %."""
    from quattro_ilqr_amd import training
    cs = tl.case(*tl.DESCENT_CASE)
    st = tl.descent_step()
    assert st["truncation"] < tl.TRUNCATION_CAP and st["noise"] < tl.NOISE_CAP
    h = st["h"]
    scale = tl.scale_of(cs)
    task = _task(cs, 1.0, scale)
    x, u = dev32(cs.x_norm), dev32(cs.prompt_norm)
    # --- device path
    tr = _trainer(cs.train)
    p0 = tr.params.clone()
    loss0, _ = tr.tracking_step(x, u, task, seed=0, training=False)
    g = tr.grads.double().clone()
    gnorm = float(g.norm())

    def loss_at(step):
        tr.params.copy_((p0.double() + step * g / gnorm).float())
        cost = training._tracked_cost(tr.forward(x, u, 0, False), task)
        return float((cost * task.scale.double()).sum() / cs.B)

    fd = (loss_at(h) - loss_at(-h)) / (2.0 * h)
    print(f"[descent, device] |g| {gnorm:.6f} (fp64 chain {st['gnorm']:.6f})  central difference {fd:.6f}  h {h}  loss {float(loss0):.6f}")
    assert abs(fd - gnorm) <= tl.DESCENT_TOL * gnorm and abs(gnorm - st["gnorm"]) <= tl.DESCENT_TOL * st["gnorm"]
    # --- torch path: training.forward under autograd, training.tracking_loss
    names = sorted(cs.train.params)
    params = {k: dev32(cs.train.params[k]).requires_grad_(True) for k in names}
    buffers = {"pos_encoder.pe": dev32(cs.train.pe)[None]}
    norm = dict(u_mean=dev32(cs.u_mean), u_std=dev32(cs.u_std))
    args = (norm, task.x_nom, task.u_nom, task.K_log, task.k_log, task.x0, 1.0, task.scale)
    loss_t = training.tracking_loss(task.model, training.forward(params, buffers, x, u, tl.NHEAD), *args)
    assert loss_t.dtype == torch.float64 and float(loss_t.detach()) == pytest.approx(float(loss0), rel=1e-4)
    loss_t.backward()
    gt = torch.cat([params[k].grad.double().flatten() for k in names])
    gtn = float(gt.norm())

    def loss_torch(step):
        with torch.no_grad():
            at, moved = 0, {}
            for k in names:
                v = params[k]
                moved[k] = (v.double() + step * gt[at:at + v.numel()].view(v.shape) / gtn).float()
                at += v.numel()
            return float(training.tracking_loss(task.model, training.forward(moved, buffers, x, u, tl.NHEAD), *args))

    fdt = (loss_torch(h) - loss_torch(-h)) / (2.0 * h)
    print(f"[descent, torch] |g| {gtn:.6f}  central difference {fdt:.6f}")
    assert abs(fdt - gtn) <= tl.DESCENT_TOL * gtn and abs(gtn - gnorm) <= tl.DESCENT_TOL * gnorm


# ------------------------------------------------------------------------------------------------ 8. fit
def test_fit_tracking_on_a_collected_cartpole_log():
    q = _pkg()
    from quattro_ilqr_amd import datagen
    md = q.cartpole_model()
    N, P = 12, 3
    rng = np.random.default_rng(3)
    x0 = np.zeros((6, 4))
    x0[:, 0], x0[:, 2] = rng.uniform(-0.5, 0.5, 6), rng.uniform(-0.5, 0.5, 6)
    full = datagen.collect(q.QuattroILQR(md, N, max_iter=3, tol=1e-9, device=DEV), x0)
    assert len(full) >= 12
    log = full.select(np.arange(12))
    u_nom = datagen.nominal_controls(full)[:12]
    make = lambda: q.TransformerILQR(md.n, md.m * (1 + md.n), prompt_len=P, d_model=32, nhead=4, num_decoder_layers=1, dim_feedforward=64,
                                     dropout=0.0, max_seq_len=40, device=DEV)
    pre = make().fit(log, num_epochs=30, batch_size=4, backend="hip")                     # imitation first: tracking is a fine-tuning loss
    init = {k: v for k, v in pre._w.items() if k != "pos_encoder.pe"}
    tf = make().fit(log, log, num_epochs=2, batch_size=5, backend="hip", loss="tracking", init=init,
                    task=dict(model=md, u_nom=u_nom, test_u_nom=u_nom))
    assert tf.fit_backend == "hip" and tf.target_len == N + 1 - P
    assert len(tf.train_loss_history) == len(tf.test_loss_history) == 2 and tf.diverged_history == [0, 0]
    assert np.all(np.isfinite(tf.train_loss_history)) and np.all(np.isfinite(tf.test_loss_history))
    print(f"[fit tracking] train {tf.train_loss_history} test {tf.test_loss_history}")
    assert any(not np.array_equal(tf._w[k], pre._w[k]) for k in init)
    xe = torch.as_tensor(log.x_seq, dtype=torch.float32, device=DEV).contiguous()
    prompt = torch.randn((12, P, md.m * (1 + md.n)), device=DEV)
    out = tf.predict_batch(xe, prompt)
    assert tuple(out.shape) == (12, tf.target_len, md.m * (1 + md.n)) and bool(torch.isfinite(out).all())
