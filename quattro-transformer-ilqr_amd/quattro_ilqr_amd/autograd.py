"""The trajectory cost as a differentiable torch function: a loss through the device model without leaving the device.

trajectory_cost(model, x0, u) is J(x0, u) = sum_t L(x_t, u_t) + Lf(x_N) with x_{t+1} = f(x_t, u_t), rolled out and summed by the
library's kernels (ops.simulate / ops.track + ops.score); its backward pass is ONE adjoint sweep (ops.cost_gradient) on the saved
rollout.  torch only carries the tensors: the arithmetic of the forward and backward pass is the library's, apart from the scaling
of the gradient by the incoming one (one torch multiplication per output) and, under model_phys, two zero-filled placeholders that
ops.track asks for (x_nom and K: not read with the feedback off).  The placeholders of the LAST shape and device are kept, so that a
loop over one problem does not fill them again: (B, N, m, n) floats of device memory for K, 39 MB for the quadrotor at B = 4096,
N = 50.  autograd.release_placeholders() gives them back.
"""
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


def trajectory_cost(model, x0, u, targets=None, weights=None, model_phys=None):
    """J(x0, u) per trajectory: x0 (B, n), u (B, N, m), float32 device tensors -> cost (B,) float64, differentiable with respect to
    x0 and u (torch.autograd.Function).
      forward   without rows: ops.simulate, whose cost is returned.  With rows: the rollout under model_phys
                (ops.track(..., feedback=False, plant_phys=model_phys)) when that row is given, otherwise ops.simulate; the cost is
                ops.score(..., terminal=True) under the same rows
      backward  one ops.cost_gradient launch on the saved x, u under the same rows, scaled per trajectory by the incoming gradient
                (cast to float32: the gradients are float32 like x0 and u)
    targets, weights, model_phys: per-trajectory rows in the forms ops.score and ops.cost_gradient take.  NOTHING is differentiable
    with respect to the rows or the model's parameters: they are constants of the function, and a tensor passed for them receives
    no gradient.  Second derivatives are not available either (the backward pass is not itself differentiable)."""
    # the rows are converted once, so that forward and backward see the same device arrays
    Bt = int(u.shape[0]) if hasattr(u, "shape") and len(u.shape) == 3 else 0
    if Bt > 0:
        ops.check_phys_rows(model, model_phys, Bt, "model_phys")
        ops.check_ref_rows(model, targets, Bt, name="targets")
        ops.check_cost_rows(model, weights, Bt, name="weights")
        if u.is_cuda:
            model_phys = ops.model_phys_tensor(model, model_phys, Bt, u.device)
            targets = ops.x_ref_rows_tensor(model, targets, Bt, u.device, name="targets")
            weights = ops.cost_rows_tensor(model, weights, Bt, u.device, name="weights")
    return _TrajectoryCost.apply(x0, u, model, targets, weights, model_phys)
