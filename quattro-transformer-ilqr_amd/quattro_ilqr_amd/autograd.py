"""The trajectory cost as a differentiable torch function: a loss through the device model without leaving the device.

trajectory_cost(model, x0, u) is J(x0, u) = sum_t L(x_t, u_t) + Lf(x_N) with x_{t+1} = f(x_t, u_t), rolled out and summed by the
library's kernels (ops.simulate / ops.track + ops.score); its backward pass is ONE adjoint sweep (ops.cost_gradient) on the saved
rollout.  torch only carries the tensors: the arithmetic of the forward and backward pass is the library's, apart from the scaling
of the gradient by the incoming one (one torch multiplication per output) and, under model_phys, two zero-filled placeholders that
ops.track asks for (x_nom and K: not read with the feedback off).  The placeholders of the LAST shape and device are kept, so that a
loop over one problem does not fill them again: (B, N, m, n) floats of device memory for K, 39 MB for the quadrotor at B = 4096,
N = 50.  autograd.release_placeholders() gives them back.

The rows -- model_phys, weights, targets -- are differentiable too where they are passed as torch tensors that require a gradient:
the backward pass then adds ONE ops.cost_param_gradient launch on the costate of the adjoint sweep (system identification, weight
tuning, goal optimisation; the built-in models and user models compiled with param_grad=True).  Without such a tensor nothing changes: the same launches, the same bits.

tracking_cost(model, x0, x_nom, u_nom, K) is the cost of the run the gain law u = u_nom + K (x - x_nom) produces on a plant (ops.track
+ ops.score); its backward pass is ONE ops.track_gradient launch: gradients for the gains, the nominal, the start and the disturbance,
and through one ops.cost_param_gradient launch on the closed-loop costate for the plant's parameters, the weights and the targets.
"""
import numpy as np
import torch

from . import ops


_PLACEHOLDERS = {}


def _placeholders(B, N, n, m, device):
    """x_nom (B, N+1, n) and K (B, N, m, n) of zeros for ops.track with the feedback off: never read, never written."""
    key = (B, N, n, m, str(device))
    if key not in _PLACEHOLDERS:
        _PLACEHOLDERS.clear()                      # one entry: another shape replaces the last one
        _PLACEHOLDERS[key] = (torch.zeros((B, N + 1, n), dtype=torch.float32, device=device),
                              torch.zeros((B, N, m, n), dtype=torch.float32, device=device))
    return _PLACEHOLDERS[key]


def release_placeholders():
    """Drop the zero tensors kept for trajectory_cost(..., model_phys=...) (the next such call makes them again)."""
    _PLACEHOLDERS.clear()


def _forward(model, x0, u, targets, weights, model_phys):
    """-> (x (B, N+1, n) float32, cost (B,) float64): the rollout of u from x0 and its cost, under the rows."""
    if targets is None and weights is None and model_phys is None:
        return ops.simulate(model, x0, u)
    if model_phys is None:
        x, _ = ops.simulate(model, x0, u)
    else:
        # the open-loop rollout under per-trajectory parameters: the tracked plant steps with the feedback off (x_nom and K are
        # then not looked at; they only have to be there)
        Bt, N, m = u.shape
        x_nom, K = _placeholders(Bt, N, model.n, m, u.device)
        x, _ = ops.track(model, x0, x_nom, u, K, N, plant_phys=model_phys, feedback=False)
    total, _ = ops.score(model, x, u, targets=targets, weights=weights, model_phys=model_phys, terminal=True, want_stage=False)
    return x, total


class _TrajectoryCost(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, u, model, targets, weights, model_phys):
        x0d, ud = x0.detach().contiguous(), u.detach().contiguous()
        x, cost = _forward(model, x0d, ud, targets, weights, model_phys)
        ctx.save_for_backward(x, ud)
        ctx.call = (model, targets, weights, model_phys)
        return cost

    @staticmethod
    def backward(ctx, grad_cost):
        x, u = ctx.saved_tensors
        model, targets, weights, model_phys = ctx.call
        want_x0 = ctx.needs_input_grad[0]
        g = ops.cost_gradient(model, x, u, targets=targets, weights=weights, model_phys=model_phys, want_x0=want_x0)
        w = grad_cost.to(torch.float32)
        grad_u = g["grad_u"] * w[:, None, None] if ctx.needs_input_grad[1] else None
        grad_x0 = g["grad_x0"] * w[:, None] if want_x0 else None
        return grad_x0, grad_u, None, None, None, None


def _row_grad(g, like, pad_cols=None):
    """A gradient in the layout ops.cost_param_gradient returns -> the shape, dtype and device `like` of the tensor that was passed
    as the row.  pad_cols: for a row passed in the C ABI's padded form, (width, column index of every entry of g); the padding is zero."""
    shape, dtype, device = like
    if pad_cols is not None and shape[-1] == pad_cols[0] and g.shape[-1] != pad_cols[0]:
        full = torch.zeros((g.shape[0], pad_cols[0]), dtype=g.dtype, device=g.device)
        full[:, pad_cols[1]] = g
        g = full
    return g.reshape(shape).to(device=device, dtype=dtype)


class _TrajectoryCostRows(torch.autograd.Function):
    """_TrajectoryCost with the rows as inputs of the function: the same forward pass; the backward pass adds one
    ops.cost_param_gradient launch for the rows that ask for a gradient (and skips the adjoint sweep when nothing needs it)."""

    @staticmethod
    def forward(ctx, x0, u, row_phys, row_weights, row_targets, model, targets, weights, model_phys):
        x0d, ud = x0.detach().contiguous(), u.detach().contiguous()
        x, cost = _forward(model, x0d, ud, targets, weights, model_phys)
        ctx.save_for_backward(x, ud)
        ctx.call = (model, targets, weights, model_phys)
        ctx.like = tuple(None if r is None else (tuple(r.shape), r.dtype, r.device) for r in (row_phys, row_weights, row_targets))
        return cost

    @staticmethod
    def backward(ctx, grad_cost):
        x, u = ctx.saved_tensors
        model, targets, weights, model_phys = ctx.call
        want_x0, want_u, want_phys, want_w, want_t = ctx.needs_input_grad[:5]
        like_phys, like_w, like_t = ctx.like
        n, m = model.n, model.m
        g = None
        if want_x0 or want_u or want_phys:
            g = ops.cost_gradient(model, x, u, targets=targets, weights=weights, model_phys=model_phys, want_x0=want_x0,
                                  want_costate=want_phys)
        w = grad_cost.to(torch.float32)
        grad_u = g["grad_u"] * w[:, None, None] if want_u else None
        grad_x0 = g["grad_x0"] * w[:, None] if want_x0 else None
        want = tuple(name for name, on in (("phys", want_phys), ("weights", want_w), ("targets", want_t)) if on)
        pg = ops.cost_param_gradient(model, x, u, targets=targets, weights=weights, model_phys=model_phys, want=want,
                                     costate=g["costate"] if want_phys else None) if want else {}
        w64 = grad_cost.to(torch.float64)
        grad_phys = grad_w = grad_t = None
        if want_phys:
            grad_phys = _row_grad(pg["grad_phys"] * w64[:, None], like_phys, (8, list(range(len(model.phys)))))
        if want_w:
            MX = ops._lib.MAX_NX
            cols = list(range(n)) + list(range(MX, MX + n)) + list(range(2 * MX, 2 * MX + m))
            grad_w = _row_grad(pg["grad_weights"] * w64[:, None], like_w, (ops.COST_ROW_FLOATS, cols))
        if want_t:
            grad_t = _row_grad(pg["grad_targets"] * w64[:, None, None], like_t)
        return grad_x0, grad_u, grad_phys, grad_w, grad_t, None, None, None, None


def _wants_grad(row):
    return isinstance(row, torch.Tensor) and row.requires_grad


def trajectory_cost(model, x0, u, targets=None, weights=None, model_phys=None):
    """J(x0, u) per trajectory: x0 (B, n), u (B, N, m), float32 device tensors -> cost (B,) float64, differentiable with respect to
    x0 and u, and with respect to the rows or the model's parameters where a row is a torch tensor that requires a gradient
    (torch.autograd.Function).
      forward   without rows: ops.simulate, whose cost is returned.  With rows: the rollout under model_phys
                (ops.track(..., feedback=False, plant_phys=model_phys)) when that row is given, otherwise ops.simulate; the cost is
                ops.score(..., terminal=True) under the same rows
      backward  one ops.cost_gradient launch on the saved x, u under the same rows, scaled per trajectory by the incoming gradient
                (cast to float32: the gradients are float32 like x0 and u); for rows that require a gradient one
                ops.cost_param_gradient launch more, on the costate of the first (which is skipped when neither x0, u nor model_phys
                needs it)
    targets, weights, model_phys: per-trajectory rows in the forms ops.score and ops.cost_gradient take.  A torch tensor among them
    with requires_grad -- model_phys (B, len(phys)), weights (B, 2n + m), targets (B, R, n) or (B, n), or the padded device forms
    of the C ABI -- receives dJ/d(row) in its own shape, dtype and device: ops.cost_param_gradient's fp64 result times the incoming
    gradient, cast; padding entries are zero.  Anything else (a dict of weights, arrays, tensors without requires_grad) is a constant
    of the function, and then the function makes the launches and returns the bits it always has.  The row gradients run for
    the built-in models and for a user model compiled with compile_model(..., param_grad=True), whose own costs and dynamics are
    then differentiated (NotImplementedError from the backward pass of any other user-compiled model).  dt and the barrier are not
    differentiated.  Second derivatives are not available either (the backward pass is not itself differentiable)."""
    # the rows are converted once, so that forward and backward see the same device arrays
    rows_in = (model_phys, None if isinstance(weights, dict) else weights, targets)
    Bt = int(u.shape[0]) if hasattr(u, "shape") and len(u.shape) == 3 else 0
    if Bt > 0:
        ops.check_phys_rows(model, model_phys, Bt, "model_phys")
        ops.check_ref_rows(model, targets, Bt, name="targets")
        ops.check_cost_rows(model, weights, Bt, name="weights")
        if u.is_cuda:
            with torch.no_grad():
                model_phys = ops.model_phys_tensor(model, model_phys, Bt, u.device)
                targets = ops.x_ref_rows_tensor(model, targets, Bt, u.device, name="targets")
                weights = ops.cost_rows_tensor(model, weights, Bt, u.device, name="weights")
    if not any(_wants_grad(r) for r in rows_in):
        return _TrajectoryCost.apply(x0, u, model, targets, weights, model_phys)
    detach = lambda t: t.detach() if isinstance(t, torch.Tensor) else t
    rows_in = tuple(r if _wants_grad(r) else None for r in rows_in)
    return _TrajectoryCostRows.apply(x0, u, *rows_in, model, detach(targets), detach(weights), detach(model_phys))


class _TrackingCost(torch.autograd.Function):
    """tracking_cost: ops.track + ops.score forward, one ops.track_gradient launch backward, and one ops.cost_param_gradient launch
    more on the closed-loop costate where a row asks for a gradient."""

    @staticmethod
    def forward(ctx, x0, x_nom, u_nom, K, disturbance, row_phys, row_weights, row_targets, model, steps, plant, plant_phys, targets,
                weights, terminal, feedback):
        c = lambda t: t.detach().contiguous()
        x_nomd, Kd = c(x_nom), c(K)
        dist = None if disturbance is None else c(disturbance)
        x, u = ops.track(model, c(x0), x_nomd, c(u_nom), Kd, steps, plant=plant, plant_phys=plant_phys, feedback=feedback,
                         disturbance=dist)
        cost, _ = ops.score(model, x, u, targets=targets, weights=weights, model_phys=plant_phys, terminal=terminal, ref_hold=1,
                            want_stage=False)
        ctx.save_for_backward(x, u, x_nomd, Kd)
        ctx.call = (model, plant, plant_phys, targets, weights, terminal, feedback)
        ctx.like = tuple(None if r is None else (tuple(r.shape), r.dtype, r.device) for r in (row_phys, row_weights, row_targets))
        return cost

    @staticmethod
    def backward(ctx, grad_cost):
        x, u, x_nom, K = ctx.saved_tensors
        model, plant, plant_phys, targets, weights, terminal, feedback = ctx.call
        want_x0, want_xn, want_un, want_K, want_d, want_phys, want_w, want_t = ctx.needs_input_grad[:8]
        like_phys, like_w, like_t = ctx.like
        n, m = model.n, model.m
        want = tuple(name for name, on in (("K", want_K and feedback), ("x_nom", want_xn and feedback), ("x0", want_x0)) if on)
        g = ops.track_gradient(model, x, u, x_nom if feedback else None, K if feedback else None, plant=plant, plant_phys=plant_phys,
                               targets=targets, weights=weights, terminal=terminal, want=want, want_costate=want_d or want_phys)
        w = grad_cost.to(torch.float32)
        grad_x0 = g["grad_x0"] * w[:, None] if want_x0 else None
        grad_xn = g["grad_x_nom"] * w[:, None, None] if "x_nom" in want else None
        grad_un = None
        if want_un:
            grad_un = g["grad_u_nom"] * w[:, None, None]
            if grad_un.shape[1] < K.shape[1]:       # feedback off: the entry was not told N, and the rows past `steps` are zero
                grad_un = torch.cat([grad_un, grad_un.new_zeros((grad_un.shape[0], K.shape[1] - grad_un.shape[1], m))], dim=1)
        grad_K = g["grad_K"] * w[:, None, None, None] if "K" in want else None
        grad_d = (g["costate"][:, 1:] * w[:, None, None]).transpose(0, 1).contiguous() if want_d else None
        rows = tuple(name for name, on in (("phys", want_phys), ("weights", want_w), ("targets", want_t)) if on)
        grad_phys = grad_w = grad_t = None
        if rows:
            # the rows' gradient of the tracked cost: the open-loop kernel on the realised run (N = steps), under the plant's integrator
            # and parameters, with the CLOSED-LOOP costate as the multiplier
            pm = model if plant is None else model.with_(integrator=plant.integrator, phys=tuple(plant.phys))
            pg = ops.cost_param_gradient(pm, x, u, targets=targets, weights=weights, model_phys=plant_phys, want=rows,
                                         costate=g["costate"] if want_phys else None)
            w64 = grad_cost.to(torch.float64)
            if want_phys:
                grad_phys = _row_grad(pg["grad_phys"] * w64[:, None], like_phys, (8, list(range(len(model.phys)))))
            if want_w:
                MX = ops._lib.MAX_NX
                cols = list(range(n)) + list(range(MX, MX + n)) + list(range(2 * MX, 2 * MX + m))
                grad_w = _row_grad(pg["grad_weights"] * w64[:, None], like_w, (ops.COST_ROW_FLOATS, cols))
            if want_t:
                grad_t = _row_grad(pg["grad_targets"] * w64[:, None, None], like_t)
        return (grad_x0, grad_xn, grad_un, grad_K, grad_d, grad_phys, grad_w, grad_t) + (None,) * 8


def tracking_cost(model, x0, x_nom, u_nom, K, steps=None, plant=None, plant_phys=None, disturbance=None, targets=None, weights=None,
                  terminal=True, feedback=True):
    """The cost of a tracked closed-loop run, per trajectory: x0 (B, n), x_nom (B, N+1, n), u_nom (B, N, m), K (B, N, m, n), float32
    device tensors -> cost (B,) float64, differentiable with respect to x0, x_nom, u_nom, K and disturbance (steps, B, n).
      forward   ops.track(model, x0, x_nom, u_nom, K, steps, plant=, plant_phys=, feedback=, disturbance=) -- `steps` <= N plant steps
                (None: N) of u = u_nom[t] + K[t] (x - x_nom[t]) -- followed by ops.score(..., terminal=terminal, ref_hold=1,
                model_phys=plant_phys) on the realised run under targets and weights
      backward  ONE ops.track_gradient launch on the saved run, scaled per trajectory by the incoming gradient (cast to float32); rows
                of x_nom, u_nom and K past `steps` receive zero; the disturbance's gradient is the closed-loop costate[:, 1:]
    A feed-forward k or a line-search step alpha is a torch expression in front of u_nom and K (u_nom + alpha * k, alpha * K): torch's
    chain rule covers it.  With feedback=False the cost does not depend on x_nom and K, which receive no gradient.
    plant_phys, weights, targets that are torch tensors requiring a gradient receive dJ/d(row) as in trajectory_cost: one
    ops.cost_param_gradient launch more, on the closed-loop costate, under the plant's integrator (the built-in models and user models
    compiled with param_grad=True; NotImplementedError from the backward pass of any other user-compiled model).  That kernel always
    includes the terminal slot, so terminal=False together with such a row raises NotImplementedError here.  Without such a tensor no
    extra launch is made.  A plant with parameters of its own and no plant_phys rows: a user model's cost that reads P is scored with
    the model's parameters but differentiated with the plant's (the built-in costs read none)."""
    if not hasattr(u_nom, "shape") or len(u_nom.shape) != 3:
        raise ValueError(f"u_nom must have shape (B, N, m) (got {tuple(np.shape(u_nom))})")
    Bt, N = int(u_nom.shape[0]), int(u_nom.shape[1])
    steps = N if steps is None else int(steps)
    if not 1 <= steps <= N:
        raise ValueError("steps must be in 1..N")
    rows_in = (plant_phys, None if isinstance(weights, dict) else weights, targets)
    if any(_wants_grad(r) for r in rows_in) and not terminal:
        raise NotImplementedError("tracking_cost(terminal=False) cannot differentiate plant_phys, weights or targets: "
                                  "ops.cost_param_gradient always includes the terminal slot")
    if disturbance is not None and tuple(disturbance.shape) != (steps, Bt, model.n):
        raise ValueError(f"disturbance must have shape {(steps, Bt, model.n)} (got {tuple(disturbance.shape)})")
    ops.check_plant(model, plant)
    ops.check_phys_rows(model, plant_phys, Bt, "plant_phys")
    ops.check_ref_rows(model, targets, Bt, name="targets")
    ops.check_cost_rows(model, weights, Bt, name="weights")
    if u_nom.is_cuda:
        with torch.no_grad():
            plant_phys = ops.plant_phys_tensor(model, plant_phys, Bt, u_nom.device)
            targets = ops.x_ref_rows_tensor(model, targets, Bt, u_nom.device, name="targets")
            weights = ops.cost_rows_tensor(model, weights, Bt, u_nom.device, name="weights")
    detach = lambda t: t.detach() if isinstance(t, torch.Tensor) else t
    rows_in = tuple(r if _wants_grad(r) else None for r in rows_in)
    return _TrackingCost.apply(x0, x_nom, u_nom, K, disturbance, *rows_in, model, steps, plant, detach(plant_phys), detach(targets),
                               detach(weights), bool(terminal), bool(feedback))
