"""Device training step of the gain predictor over the C ABI (`quattro_tf_train_step_f32`, `quattro_tf_adam_f32`).

What `training.fit(..., backend="hip")` runs per mini-batch instead of torch autograd: the hand-written forward with
saved activations, the MSE loss, the backward and the Adam update of csrc/tf_train.hip.  torch is plumbing here — it
owns the flat parameter / gradient / moment arrays and the workspace.  Mirrors the loop body of
quattro_ilqr_tf/transformer_ilqr.py:150-172.

The flat parameter array holds every block of the reference module's state dict in its own shape and layout
(`state_dict()` / `load_state_dict()` slice it by the reference names), so weights trained here go straight into
checkpoints, the HIP inference kernel and the torch restatement in `training.forward`.

Besides the MSE step, `HipTrainer.forward` / `backward` are its two halves with any gradient of the prediction between them
(`quattro_tf_train_backward_f32`), and `tracking_step` puts the closed-loop cost of the predicted gains there (TrackingTask,
`quattro_tf_gains_unpack_f32`, ops.track / score / track_gradient, `quattro_tf_gains_pack_grad_f32`): what
`training.fit(..., loss="tracking", backend="hip")` runs per mini-batch.
"""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from ._lib import check
from .ops import _ptr, _stream


def _desc(state_dim, control_dim, d_model, nhead, n_layers, d_ff, n_state_tok, prompt_len, target_len, dropout):
    d = _lib.TfTrainDesc()
    d.state_dim, d.control_dim, d.d_model, d.nhead, d.n_layers, d.d_ff = state_dim, control_dim, d_model, nhead, n_layers, d_ff
    d.n_state_tok, d.prompt_len, d.target_len, d.dropout = n_state_tok, prompt_len, target_len, float(dropout)
    return d


def supported(state_dim, control_dim, d_model, nhead, n_layers, d_ff, n_state_tok, prompt_len, target_len, dropout=0.0):
    """True when the device training step has kernels for this shape (head dimension <= 32, d_model <= 512, sequence of
    at most 128 tokens)."""
    d = _desc(state_dim, control_dim, d_model, nhead, n_layers, d_ff, n_state_tok, prompt_len, target_len, dropout)
    return _lib.load().quattro_tf_train_param_count(ctypes.byref(d)) > 0


class TrackingTask:
    """What the tracking loss of one mini-batch is taken about: per entry b the nominal the gains were logged for, x_nom (B, N+1, n),
    u_nom (B, N, m), the logged gains K_log (B, N, m, n), k_log (B, N, m) (the rows the predictor does not cover, t >= min(T, N)),
    the start x0 (B, n) of the tracked run (None: x_nom[:, 0]), the normaliser's u_mean, u_std (c,) and the line-search step `alpha`
    of the feed-forward.  scale (B,) or None weighs each trajectory's cost; loss = task_weight * mean_b(scale_b cost_b)
    + mse_weight * MSE(pred, target).  All tensors float32, contiguous, on the trainer's device; `model` is the DeviceModel that
    is both the controller's and the plant's."""

    def __init__(self, model, x_nom, u_nom, K_log, k_log, u_mean, u_std, x0=None, alpha=1.0, scale=None, task_weight=1.0,
                 mse_weight=0.0):
        self.model, self.x_nom, self.u_nom, self.K_log, self.k_log = model, x_nom, u_nom, K_log, k_log
        self.x0 = x_nom[:, 0].contiguous() if x0 is None else x0
        self.u_mean, self.u_std, self.scale = u_mean, u_std, scale
        self.alpha, self.task_weight, self.mse_weight = float(alpha), float(task_weight), float(mse_weight)

    def select(self, idx):
        """The task of the entries idx (an index tensor or a slice)."""
        pick = lambda t: None if t is None else t[idx].contiguous()
        return TrackingTask(self.model, pick(self.x_nom), pick(self.u_nom), pick(self.K_log), pick(self.k_log), self.u_mean,
                            self.u_std, pick(self.x0), self.alpha, pick(self.scale), self.task_weight, self.mse_weight)

    def check(self, B, T, c, device):
        """ValueError unless every tensor has the shape a batch of B predictions (B, T, c) needs.  -> N"""
        md = self.model
        n, m = md.n, md.m
        if c != m * (1 + n):
            raise ValueError(f"control_dim {c} is not m (1 + n) for a model with n = {n}, m = {m}")
        if self.u_nom.dim() != 3:
            raise ValueError(f"u_nom must have shape (B, N, {m}) (got {tuple(self.u_nom.shape)})")
        N = int(self.u_nom.shape[1])
        f32 = torch.float32
        for t, shape, nm in ((self.x_nom, (B, N + 1, n), "x_nom"), (self.u_nom, (B, N, m), "u_nom"), (self.K_log, (B, N, m, n), "K_log"),
                             (self.k_log, (B, N, m), "k_log"), (self.x0, (B, n), "x0"), (self.u_mean, (c,), "u_mean"),
                             (self.u_std, (c,), "u_std"), (self.scale, (B,), "scale")):
            if t is None and nm == "scale":
                continue
            if tuple(t.shape) != shape or t.dtype != f32 or t.device.type != torch.device(device).type or not t.is_contiguous():
                raise ValueError(f"{nm} must be a contiguous float32 tensor of shape {shape} on {device} (got {tuple(t.shape)}, "
                                 f"{t.dtype}, {t.device})")
        return N


def gains_unpack(pred_norm, task, K_out=None, u_ff=None):
    """quattro_tf_gains_unpack_f32: the normalised prediction (B, T, c) -> (K (B, N, m, n), u_ff = u_nom + alpha k (B, N, m)), the rows
    t >= min(T, N) from the task's logged gains."""
    B, T, c = (int(v) for v in pred_norm.shape)
    N = task.check(B, T, c, pred_norm.device)
    ops._req(pred_norm, (B, T, c), torch.float32, "pred_norm")
    K_out = torch.empty_like(task.K_log) if K_out is None else K_out
    u_ff = torch.empty_like(task.u_nom) if u_ff is None else u_ff
    check(_lib.load().quattro_tf_gains_unpack_f32(_ptr(pred_norm), _ptr(task.u_mean), _ptr(task.u_std), _ptr(task.K_log),
                                                  _ptr(task.k_log), _ptr(task.u_nom), task.alpha, B, T, N, task.model.n,
                                                  task.model.m, _ptr(K_out), _ptr(u_ff), _stream()), "quattro_tf_gains_unpack_f32")
    return K_out, u_ff


def gains_pack_grad(grad_K, grad_u_nom, cost, task, T, pred_norm=None, target_norm=None, out=None):
    """quattro_tf_gains_pack_grad_f32: the tracked cost's gradients -> dict(d_pred (B, T, c) float32, diverged (B,) int32, terms (B,)
    float64, loss () float64) of loss = task_weight mean_b(scale_b cost_b) + mse_weight MSE over the trajectories kept.  out: a dict
    of those four to write into."""
    B, N, m, n = (int(v) for v in grad_K.shape)
    c, dev = m * (1 + n), grad_K.device
    f32 = torch.float32
    ops._req(grad_K, (B, N, m, n), f32, "grad_K"); ops._req(grad_u_nom, (B, N, m), f32, "grad_u_nom")
    ops._req(cost, (B,), torch.float64, "cost")
    if task.scale is not None:
        ops._req(task.scale, (B,), f32, "scale")
    ops._req(task.u_std, (c,), f32, "u_std")
    mse_w = task.mse_weight
    if mse_w != 0.0:
        if pred_norm is None or target_norm is None:
            raise ValueError("mse_weight != 0 needs pred_norm and target_norm")
        ops._req(pred_norm, (B, T, c), f32, "pred_norm"); ops._req(target_norm, (B, T, c), f32, "target_norm")
    if out is None:
        out = dict(d_pred=torch.empty((B, T, c), dtype=f32, device=dev), diverged=torch.empty((B,), dtype=torch.int32, device=dev),
                   terms=torch.empty((B,), dtype=torch.float64, device=dev), loss=torch.empty((), dtype=torch.float64, device=dev))
    check(_lib.load().quattro_tf_gains_pack_grad_f32(
        _ptr(grad_K), _ptr(grad_u_nom), _ptr(cost), _ptr(task.scale), _ptr(task.u_std), task.alpha, task.task_weight,
        _ptr(pred_norm) if mse_w != 0.0 else None, _ptr(target_norm) if mse_w != 0.0 else None, mse_w, B, int(T), N, n, m,
        _ptr(out["d_pred"]), _ptr(out["diverged"]), _ptr(out["terms"]), _ptr(out["loss"]), _stream()), "quattro_tf_gains_pack_grad_f32")
    return out


class HipTrainer:
    """Flat fp32 parameters + Adam state on `device`, and the per-mini-batch step."""

    def __init__(self, state_dim, control_dim, d_model, nhead, n_layers, d_ff, n_state_tok, prompt_len, target_len,
                 dropout, pe, device, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.lib = _lib.load()
        self.desc = _desc(state_dim, control_dim, d_model, nhead, n_layers, d_ff, n_state_tok, prompt_len, target_len,
                          dropout)
        self.n_params = int(self.lib.quattro_tf_train_param_count(ctypes.byref(self.desc)))
        if self.n_params == 0:
            raise NotImplementedError("quattro_tf_train_step_f32 has no kernels for this predictor shape")
        self.device = torch.device(device)
        self.L = n_state_tok + prompt_len + target_len
        self.shapes = self._shapes()
        self.offsets = {}
        for name, (which, layer, shape) in self.shapes.items():
            off = int(self.lib.quattro_tf_train_param_offset(ctypes.byref(self.desc), which, layer))
            if off < 0:
                raise RuntimeError(f"no offset for {name}")
            self.offsets[name] = off
        z = lambda: torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
        self.params, self.grads, self.m, self.v = z(), z(), z(), z()
        pe = torch.as_tensor(np.asarray(pe, dtype=np.float32)).reshape(-1, d_model)
        if pe.shape[0] < self.L:
            raise ValueError("positional table shorter than the sequence")
        self.pe = pe[: self.L].contiguous().to(self.device)
        self.lr, self.betas, self.eps, self.t = float(lr), betas, float(eps), 0
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._ws, self._ws_batch = None, 0
        self._task_bufs = {}      # batch size -> the buffers tracking_step writes

    def _shapes(self):
        D = self.desc
        d, ff, c, n, T = D.d_model, D.d_ff, D.control_dim, D.state_dim, D.target_len
        glob = [(T, d), (d, n), (d,), (d, c), (d,), (c, d), (c,)]
        lay = [(3 * d, d), (3 * d,), (d, d), (d,), (ff, d), (ff,), (d, ff), (d,), (d,), (d,), (d,), (d,)]
        out = {}
        for i, (nm, sh) in enumerate(zip(_lib.TF_TRAIN_GLOBAL, glob)):
            out[nm] = (i, 0, sh)
        for l in range(D.n_layers):
            for i, (nm, sh) in enumerate(zip(_lib.TF_TRAIN_LAYER, lay)):
                out[f"transformer_decoder.layers.{l}.{nm}"] = (len(glob) + i, l, sh)
        return out

    # ------------------------------------------------------------------ state dict <-> flat array
    def view(self, flat, name):
        _, _, shape = self.shapes[name]
        off = self.offsets[name]
        return flat[off: off + int(np.prod(shape))].view(*shape)

    def load_state_dict(self, sd):
        for name in self.shapes:
            self.view(self.params, name).copy_(torch.as_tensor(sd[name], dtype=torch.float32).detach().to(self.device))
        return self

    def state_dict(self, flat=None):
        flat = self.params if flat is None else flat
        return {name: self.view(flat, name).clone() for name in self.shapes}

    # ------------------------------------------------------------------ steps
    def _workspace(self, batch):
        if self._ws is None or batch > self._ws_batch:
            nbytes = int(self.lib.quattro_tf_train_workspace_bytes(ctypes.byref(self.desc), batch))
            if nbytes == 0:
                raise NotImplementedError("quattro_tf_train_workspace_bytes: unsupported shape")
            self._ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
            self._ws_batch = batch
        base = self._ws.data_ptr()
        aligned = (base + 255) // 256 * 256
        return ctypes.c_void_p(aligned), self._ws.numel() - (aligned - base)

    def _check_batch(self, x_norm, prompt_norm, target_norm):
        D = self.desc
        B = x_norm.shape[0]
        for t, shape, nm in ((x_norm, (B, D.n_state_tok, D.state_dim), "x_norm"),
                             (prompt_norm, (B, D.prompt_len, D.control_dim), "prompt_norm"),
                             (target_norm, (B, D.target_len, D.control_dim), "target_norm")):
            if t is None:
                continue
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"{nm} must be a contiguous float32 GPU tensor of shape {shape} (got {tuple(t.shape)}, "
                                 f"{t.dtype}, {t.device})")
        return B

    def forward_backward(self, x_norm, prompt_norm, target_norm, seed=0, training=True, want_pred=False):
        """Loss and gradients of one mini-batch (gradients land in self.grads).  Returns the loss as a device scalar
        tensor (and the normalised prediction when asked)."""
        B = self._check_batch(x_norm, prompt_norm, target_norm)
        ws, ws_bytes = self._workspace(B)
        pred = (torch.empty((B, self.desc.target_len, self.desc.control_dim), dtype=torch.float32, device=self.device)
                if want_pred else None)
        check(self.lib.quattro_tf_train_step_f32(ctypes.byref(self.desc), _ptr(self.params), _ptr(self.grads), ws, ws_bytes,
                                                 _ptr(x_norm), _ptr(prompt_norm), _ptr(target_norm), _ptr(self.pe), B,
                                                 ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), 1 if training else 0,
                                                 _ptr(self.loss), _ptr(pred), _stream()), "quattro_tf_train_step_f32")
        return (self.loss, pred) if want_pred else self.loss

    def forward(self, x_norm, prompt_norm, seed=0, training=True, out=None):
        """The step's forward half alone (quattro_tf_train_step_f32 with grads = NULL): -> the normalised prediction (B, T, c).  The
        saved activations stay in the workspace for `backward`."""
        B = self._check_batch(x_norm, prompt_norm, None)
        ws, ws_bytes = self._workspace(B)
        pred = (torch.empty((B, self.desc.target_len, self.desc.control_dim), dtype=torch.float32, device=self.device)
                if out is None else out)
        check(self.lib.quattro_tf_train_step_f32(ctypes.byref(self.desc), _ptr(self.params), None, ws, ws_bytes, _ptr(x_norm),
                                                 _ptr(prompt_norm), None, _ptr(self.pe), B,
                                                 ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), 1 if training else 0, None, _ptr(pred),
                                                 _stream()), "quattro_tf_train_step_f32")
        return pred

    def backward(self, d_pred, x_norm, prompt_norm, seed=0, training=True):
        """The step's backward half from a given gradient d_pred (B, T, c) of any scalar with respect to the prediction `forward`
        returned for the same inputs, seed and training flag (quattro_tf_train_backward_f32).  The gradients land in self.grads."""
        B = self._check_batch(x_norm, prompt_norm, d_pred)
        if self._ws is None or B > self._ws_batch:
            raise RuntimeError("backward() before forward(): the workspace holds no activations of this mini-batch")
        ws, ws_bytes = self._workspace(B)
        check(self.lib.quattro_tf_train_backward_f32(ctypes.byref(self.desc), _ptr(self.params), _ptr(self.grads), ws, ws_bytes,
                                                     _ptr(x_norm), _ptr(prompt_norm), _ptr(d_pred), B,
                                                     ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), 1 if training else 0, _stream()),
              "quattro_tf_train_backward_f32")
        return self.grads

    def tracking_step(self, x_norm, prompt_norm, task, seed=0, training=True, target_norm=None):
        """Loss and gradients of one mini-batch under the tracking loss (TrackingTask): forward, quattro_tf_gains_unpack_f32,
        ops.track from task.x0 over the whole horizon, ops.score, ops.track_gradient(want=("K",)), quattro_tf_gains_pack_grad_f32,
        backward.  -> (loss, diverged): a float64 device scalar and the int32 flags (B,) of the trajectories left out; the gradients
        land in self.grads.  Everything is enqueued on the current stream: no host synchronisation, and after the first call at a
        batch size the buffers of this class are reused (the outputs of ops.* come from torch's caching allocator).  target_norm
        (B, T, c) is read only with task.mse_weight != 0."""
        B = self._check_batch(x_norm, prompt_norm, target_norm)
        D = self.desc
        T, c = D.target_len, D.control_dim
        N = task.check(B, T, c, self.device)
        if task.mse_weight != 0.0 and target_norm is None:
            raise ValueError("task.mse_weight != 0 needs target_norm")
        buf = self._task_bufs.get((B, N))
        if buf is None:
            f32, dev = torch.float32, self.device
            buf = self._task_bufs[(B, N)] = dict(
                pred=torch.empty((B, T, c), dtype=f32, device=dev), K=torch.empty((B, N, task.model.m, task.model.n), dtype=f32, device=dev),
                u_ff=torch.empty((B, N, task.model.m), dtype=f32, device=dev), d_pred=torch.empty((B, T, c), dtype=f32, device=dev),
                diverged=torch.empty((B,), dtype=torch.int32, device=dev), terms=torch.empty((B,), dtype=torch.float64, device=dev),
                loss=torch.empty((), dtype=torch.float64, device=dev))
        md = task.model
        pred = self.forward(x_norm, prompt_norm, seed, training, out=buf["pred"])
        K, u_ff = gains_unpack(pred, task, buf["K"], buf["u_ff"])
        x, u = ops.track(md, task.x0, task.x_nom, u_ff, K, N)
        cost, _ = ops.score(md, x, u, terminal=True, want_stage=False)
        g = ops.track_gradient(md, x, u, task.x_nom, K, want=("K",))
        gains_pack_grad(g["grad_K"], g["grad_u_nom"], cost, task, T, pred, target_norm, out=buf)
        self.backward(buf["d_pred"], x_norm, prompt_norm, seed, training)
        return buf["loss"], buf["diverged"]

    EVAL_CHUNK = 1024      # sequences per forward-only call: bounds the workspace (~2.8 MB per sequence of the shipped predictor:
                           # saved activations + gradient temporaries are carved even when no gradient is asked for) and keeps
                           # the attention grids (dim3(H, batch)) inside gridDim.y <= 65535

    def evaluate(self, x_norm, prompt_norm, target_norm=None):
        """Forward without dropout: (loss or None, normalised prediction).  Any batch size: evaluated in chunks of
        EVAL_CHUNK sequences, the loss as the sequence-weighted mean of the chunks' means (= the mean over the whole set)."""
        B = self._check_batch(x_norm, prompt_norm, target_norm)
        pred = torch.empty((B, self.desc.target_len, self.desc.control_dim), dtype=torch.float32, device=self.device)
        total = None
        for lo in range(0, B, self.EVAL_CHUNK):
            hi = min(B, lo + self.EVAL_CHUNK)
            ws, ws_bytes = self._workspace(hi - lo)
            tgt = None if target_norm is None else target_norm[lo:hi]
            check(self.lib.quattro_tf_train_step_f32(ctypes.byref(self.desc), _ptr(self.params), None, ws, ws_bytes,
                                                     _ptr(x_norm[lo:hi]), _ptr(prompt_norm[lo:hi]), _ptr(tgt), _ptr(self.pe),
                                                     hi - lo, ctypes.c_uint64(0), 0, _ptr(self.loss) if tgt is not None else None,
                                                     _ptr(pred[lo:hi]), _stream()), "quattro_tf_train_step_f32")
            if tgt is not None:
                part = self.loss * ((hi - lo) / B)
                total = part if total is None else total + part
        if total is not None and B > self.EVAL_CHUNK:
            return total, pred
        return (self.loss if target_norm is not None else None), pred

    def adam_step(self):
        self.t += 1
        check(self.lib.quattro_tf_adam_f32(_ptr(self.params), _ptr(self.grads), _ptr(self.m), _ptr(self.v), self.n_params,
                                           self.lr, self.betas[0], self.betas[1], self.eps, self.t, _stream()),
              "quattro_tf_adam_f32")

    def dropout_mask(self, seed, p, site, n):
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        check(self.lib.quattro_tf_train_dropout_mask_f32(ctypes.c_uint64(int(seed) & (2 ** 64 - 1)), float(p), int(site), n,
                                                         _ptr(out), _stream()), "quattro_tf_train_dropout_mask_f32")
        return out
