"""Batched iLQR on the GPU (QuattroILQR) and the reference-compatible single-trajectory class (iLQR_TF).

Reference mirrored: quattro_ilqr_tf/quattro_ilqr_tf.py (class iLQR_TF :50, optimize :424-591).  The reference solves one
trajectory per instance in NumPy; here B independent trajectories advance together, each with its own line-search
result and stop flag kept ON THE DEVICE (no host round trip inside an iteration):

    simulate (once)  ->  repeat:  linearize -> riccati_sweep [-> transformer gains] -> fused line search/commit

An accepted forward pass IS the next iteration's nominal rollout (the reference recomputes it with simulate(),
:429/:485, from the same u and the same f, so the numbers are identical); only the very first rollout is explicit.
"""
import time

import numpy as np
import torch

from . import _lib, ops
from .models import DeviceModel

ALPHAS = ops.ALPHAS


def _pack_prompt(k_seg, K_seg):
    """[k (m) | K.reshape(m*n)] per prompt row — quattro_ilqr_tf.py:498-502 (NOT the unpack layout)."""
    return torch.cat([k_seg, K_seg.reshape(K_seg.shape[0], K_seg.shape[1], -1)], dim=-1)


def _unpack_prediction(pred, m, n):
    """(B, T, m(1+n)) -> k (B,T,m) = [...,0], K (B,T,m,n) = [...,1:] of the (T, m, 1+n) view — :510-514."""
    v = pred.reshape(pred.shape[0], pred.shape[1], m, 1 + n)
    return v[..., 0].contiguous(), v[..., 1:].contiguous()


class QuattroILQR:
    """Batched solver façade (BASELINE north_star: `QuattroILQR.solve()`).

    model      : DeviceModel (quattro_ilqr_amd.models)
    horizon    : N
    tf         : optional predictor with `.predict_batch(x_err (B,N+1,n), prompt (B,P,c)) -> (B,T,c)` on device and
                 `.prompt_len`; hybrid mode = gains for t < N-P from the predictor, the last P steps from the sweep.
    """

    def __init__(self, model, horizon, max_iter=100, tol=1e-3, tf=None, tf_window=10, alphas=ALPHAS, reg=ops.QUU_REG,
                 device="cuda:0", state_offset=None, check_every=4, use_graph=False, device_loop=True):
        if not isinstance(model, DeviceModel):
            raise TypeError("model must be a quattro_ilqr_amd.models.DeviceModel")
        self.model, self.horizon = model, int(horizon)
        self.max_iter, self.tol = int(max_iter), float(tol)
        self.alphas, self.reg = tuple(alphas), float(reg)
        self.device = torch.device(device)
        self.tf = tf
        if tf is not None and hasattr(tf, "prompt_len"):
            tf_window = tf.prompt_len                    # quattro_ilqr_tf.py:118-119
        if tf_window >= horizon:
            raise ValueError("tf_window must be less than the horizon.")   # :96-97
        self.tf_window = int(tf_window)
        n = model.n
        self.state_offset = np.zeros(n) if state_offset is None else np.asarray(state_offset, dtype=np.float64)
        self.layout = ops.model_layout(model)
        self.check_every = max(1, int(check_every))
        # use_graph: one iLQR iteration (4-8 launches) is captured once per batch size into a hipGraph and replayed;
        # small batches (cart-pole B = 1024: ~75 us of kernels per iteration) are otherwise bound by host launch time
        self.use_graph = bool(use_graph)
        # device_loop: pure-mode solves run as ONE C call (quattro_ilqr_solve_f32) with no host synchronisation at all —
        # one persistent launch where the model has such a kernel (ops.model_has_device_loop), max_iter enqueued
        # iterations otherwise (taken only when that costs less than it saves: see solve()).  False = the host-driven loop
        # (one call per iteration, a convergence check every `check_every` iterations); results are bit-identical.
        self.device_loop = device_loop if device_loop == "always" else bool(device_loop)
        self._model_lib = _lib.load_for(self.model)      # a user model's kernels live in a library of its own
        self._graph = None
        self._B = None
        self._tf_mean = None             # hybrid mode: the predictor's normalisation mean shifted by x_ref - state_offset,
                                         # in a fixed-address device buffer (captured graphs hold its address)

    def _wants_device_loop(self):
        """device_loop=True: the persistent kernel where it is the model's fastest form; "always": wherever one exists (a
        user-compiled model's is slower than its enqueued iterations, but runs without any host involvement)."""
        if self.device_loop == "always":
            return ops.model_can_device_loop(self.model)
        return bool(self.device_loop) and ops.model_has_device_loop(self.model)

    # ---------------------------------------------------------------------------------------- buffers
    def _alloc(self, B):
        if self._B == B:
            return
        n, m, N, dev = self.model.n, self.model.m, self.horizon, self.device
        f32 = torch.float32
        self.t_start = 0 if self.tf is None else N - self.tf_window
        S = N - self.t_start
        # Everything a solve reads from or hands back to the host lives in ONE device block
        #   [x | cost | u | x0 | iters | alpha_idx | status | active]   (every part 16-byte aligned)
        # so that host inputs go up as one copy of [u | x0], a single-trajectory caller (the iLQR_TF drop-in) gets its whole
        # result with one download, and "the same problem again" is one device copy of the tail [u | x0 | per-solve state]
        # (self.restart_block); the tensors below are typed views of it.
        parts = (("x", B * (N + 1) * n * 4), ("cost", B * 8), ("u", B * N * m * 4), ("x0", B * n * 4), ("iters", B * 4),
                 ("alpha_idx", B * 4), ("status", B * 4), ("active", B * 4))
        off, pos = {}, 0
        for name, nbytes in parts:
            off[name] = (pos, nbytes)
            pos += (nbytes + 15) // 16 * 16
        self._state = torch.zeros((pos,), dtype=torch.uint8, device=dev)
        self._state_off = off
        part = lambda name, dt, shape: self._state[off[name][0]:off[name][0] + off[name][1]].view(dt).view(shape)
        self.u = part("u", f32, (B, N, m))
        self._x0 = part("x0", f32, (B, n))
        self.x = part("x", f32, (B, N + 1, n))
        # record buffer + terminal pair: only for models whose sweep does not linearise its own trajectory (ADVICE r2:
        # the fused models never touch them; 62 MB at B = 4096)
        self.rec = self.VxN = self.VxxN = None
        if not ops.model_fuses_sweep(self.model):
            self._alloc_records(B, S)
        # K and k are views of ONE flat buffer [K | k]: a sharded run gathers both with a single collective straight
        # out of the memory the sweep writes (parallel.GainGather), with no repacking copy
        nK = B * N * m * n
        self.gains_flat = torch.zeros((nK + B * N * m,), dtype=f32, device=dev)
        self.K = self.gains_flat[:nK].view(B, N, m, n)
        self.k = self.gains_flat[nK:].view(B, N, m)
        if self.tf is not None:
            self.K_seg = torch.zeros((B, S, m, n), dtype=f32, device=dev)
            self.k_seg = torch.zeros((B, S, m), dtype=f32, device=dev)
        self.cost = part("cost", torch.float64, (B,))
        self.iters = part("iters", torch.int32, (B,))
        self.alpha_idx = part("alpha_idx", torch.int32, (B,))
        self.status = part("status", torch.int32, (B,))
        self.active = part("active", torch.int32, (B,))
        self.alpha_idx.fill_(-1)
        self.active.fill_(1)
        # the per-solve state as one block and its initial contents: reset = ONE device copy instead of four fills
        self._ints = self._state[off["iters"][0]:]
        self._ints_init = self._ints.clone()
        self.restart_block = self._state[off["u"][0]:]                  # [u | x0 | iters | alpha_idx | status | active]
        self._state_host = None                                         # pinned mirror of the block (download_state)
        self._x_ref_t = torch.zeros((n,), dtype=f32, device=dev)       # hybrid mode: x_ref and state offset, fixed addresses
        self._offset_t = torch.zeros((n,), dtype=f32, device=dev)
        self._alphas_t = torch.tensor(self.alphas + (float("nan"),), dtype=f32, device=dev)
        self._ws = None
        # hybrid mode: the solver OWNS its line-search scratch (a captured graph holds the address; a cache shared with
        # other solvers could hand the memory to someone else between replays) and the shifted normalisation mean
        self._ls_scratch = None
        self._tf_mean = None
        if self.tf is not None:
            self._ls_scratch = torch.empty((ops.linesearch_scratch_bytes(self.model, B, N),), dtype=torch.uint8, device=dev)
            if hasattr(self.tf, "shifted_mean"):
                self._tf_mean = torch.zeros((n,), dtype=f32, device=dev)
        # fused linearise+sweep of the RK4 quadrotor: the wave's coefficient scratch (owned here: fixed address for graphs)
        need = ops.linearize_sweep_scratch_bytes(self.model, B, N, self.t_start) if ops.model_fuses_sweep(self.model) else 0
        self._sweep_scratch = torch.empty((need,), dtype=torch.uint8, device=dev) if need else None
        self._pin_in = None                                             # pinned staging of the [u | x0] prefix, see _upload
        self._pin_done = None
        self._graph = None
        self._graph_log = None
        self._log = None
        self._ref_key = None
        self._solve_call = None
        self._B = B

    def _alloc_records(self, B, S):
        n, m, dev = self.model.n, self.model.m, self.device
        self.rec = ops.alloc_records(n, m, self.layout, B, S, dev, _lib.load_for(self.model))
        self.VxN = torch.empty((B, n), dtype=torch.float32, device=dev)
        self.VxxN = torch.empty((B, n, n), dtype=torch.float32, device=dev)

    def ensure_records(self):
        """Record buffer + terminal pair for callers that run linearize / riccati_sweep as separate launches on the
        solver's buffers although the model fuses them (A/B timing scripts, bench.py --no-fused-sweep)."""
        if self.rec is None:
            self._alloc_records(self._B, self.horizon - self.t_start)

    def _upload(self, x0, u_init, guard=True):
        """x0 -> self._x0 and u_init (None = zeros) -> self.u.  Host inputs go through ONE pinned staging buffer that mirrors
        the [u | x0] prefix of the state block and ONE async copy, with no torch CPU kernel on the way (see below: that, not
        the H2D copy, was what made a 20-iteration solve fed from NumPy take 27 ms instead of 5 ms)."""
        on_dev = lambda t: isinstance(t, torch.Tensor) and t.device.type == "cuda"
        (u_off, u_len), (x_off, x_len) = self._state_off["u"], self._state_off["x0"]
        lo, hi = None, None
        if self._pin_in is None and not (on_dev(x0) and on_dev(u_init)):
            # (mirrors bytes [u_off, x_off + x_len) of the state block)
            self._pin_in = torch.zeros((x_off + x_len - u_off,), dtype=torch.uint8, pin_memory=True)
            self._pin_np = self._pin_in.numpy()
            self._pin_u = self._pin_np[:u_len].view(np.float32).reshape(tuple(self.u.shape))
            self._pin_x0 = self._pin_np[x_off - u_off:x_off - u_off + x_len].view(np.float32).reshape(tuple(self._x0.shape))
        if guard and self._pin_done is not None and not (on_dev(x0) and on_dev(u_init)):
            self._pin_done.synchronize()                                # the previous upload has left the staging buffer
        # dtype conversion by NumPy straight into the pinned buffer: a torch CPU copy of > 32 k elements runs on the
        # intra-op thread pool, and waking 64 OpenMP threads inside a 16-core CPU quota stalled this line for 25-60 ms
        to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        if on_dev(u_init):
            self.u.copy_(u_init.reshape(self.u.shape))
        else:
            if u_init is None:
                self._pin_u[...] = 0.0
            else:
                self._pin_u[...] = to_np(u_init).reshape(self._pin_u.shape)
            lo, hi = u_off, u_off + u_len
        if on_dev(x0):
            self._x0.copy_(x0.reshape(self._x0.shape))
        else:
            self._pin_x0[...] = to_np(x0).reshape(self._pin_x0.shape)
            lo, hi = (x_off if lo is None else lo), x_off + x_len
        if lo is not None:
            self._state[lo:hi].copy_(self._pin_in[lo - u_off:hi - u_off], non_blocking=True)
            if guard:      # (a caller that synchronises the stream before its next upload needs no event: download_state)
                if self._pin_done is None:
                    self._pin_done = torch.cuda.Event()
                self._pin_done.record()

    def download_state(self, log=None, log_rows=0):
        """The whole state block (u, x0, x, cost, iters, alpha_idx, status, active) in ONE device-to-host copy; returns
        NumPy views of a pinned mirror (valid until the next call).  Synchronises the stream.  With `log` (an ops.SolveLog of
        a single-trajectory solve) its first `log_rows` records ride along before the same synchronisation (a caller that
        guessed the iteration count right needs no second download): read them with log.staged(count)."""
        if self._state_host is None:
            self._state_host = torch.empty_like(self._state, device="cpu").pin_memory()
            raw = self._state_host.numpy()
            B, N, n, m = self._B, self.horizon, self.model.n, self.model.m
            o = self._state_off
            v = lambda name, dt, shape: raw[o[name][0]:o[name][0] + o[name][1]].view(dt).reshape(shape)
            self._state_np = dict(u=v("u", np.float32, (B, N, m)), x=v("x", np.float32, (B, N + 1, n)),
                                  cost=v("cost", np.float64, (B,)), iters=v("iters", np.int32, (B,)),
                                  alpha_idx=v("alpha_idx", np.int32, (B,)), status=v("status", np.int32, (B,)),
                                  active=v("active", np.int32, (B,)))
            self._stream_obj = torch.cuda.current_stream(self.device)
        self._state_host.copy_(self._state, non_blocking=True)
        if log is not None and log_rows > 0:
            log.stage(0, log_rows)
        self._stream_obj.synchronize()
        return self._state_np

    # ---------------------------------------------------------------------------------------- one iteration
    def backward(self, x_ref_t=None):
        """linearize + sweep (+ transformer) -> self.K, self.k for every active trajectory."""
        n, m = self.model.n, self.model.m
        fused = ops.model_fuses_sweep(self.model)      # the sweep linearises its own trajectory: one launch, no records
        if not fused:
            ops.linearize(self.model, self.x, self.u, t_start=self.t_start, layout=self.layout, rec=self.rec,
                          VxN=self.VxN, VxxN=self.VxxN)
        if self.tf is None:
            if fused:
                ops.linearize_sweep(self.model, self.x, self.u, 0, self.reg, K=self.K, k=self.k, status=self.status,
                                    active=self.active, scratch=self._sweep_scratch)
            else:
                ops.riccati_sweep(self.rec, self.VxN, self.VxxN, n, m, self.layout, self.reg, K=self.K, k=self.k,
                                  status=self.status, active=self.active, lib=self._model_lib)
            return
        S = self.horizon - self.t_start
        T = self.tf.target_len
        if T + S < self.horizon:
            raise IndexError(f"gain stack has {T} predicted + {S} swept steps for horizon {self.horizon}")
        N = self.horizon
        if fused and hasattr(self.tf, "predict_gains") and T + S == N:
            # The whole hybrid backward pass as TWO launches and no torch kernel: the tail sweep writes rows N - S .. N - 1 of
            # the full stacks in place, the predictor reads its prompt [k | K.flat] from those rows (:498-502) and fills the
            # rows below (:510-518); stopped trajectories are skipped by both.
            ops.linearize_sweep(self.model, self.x, self.u, self.t_start, self.reg, K=self.K, k=self.k, status=self.status,
                                active=self.active, scratch=self._sweep_scratch, in_place=True)
            self._log_phase(_lib.LOG_PHASE_BACKWARD_DONE)
            if self._tf_mean is not None:
                self.tf.predict_gains(self.x, None, self.K, self.k, self.active, x_mean=self._tf_mean)
            else:
                self.tf.predict_gains(self.x - x_ref_t + self._offset_t, None, self.K, self.k, self.active)
            return
        if fused:
            ops.linearize_sweep(self.model, self.x, self.u, self.t_start, self.reg, K=self.K_seg, k=self.k_seg,
                                status=self.status, active=self.active, scratch=self._sweep_scratch)
        else:
            ops.riccati_sweep(self.rec, self.VxN, self.VxxN, n, m, self.layout, self.reg, K=self.K_seg, k=self.k_seg,
                              status=self.status, active=self.active, lib=self._model_lib)
        self._log_phase(_lib.LOG_PHASE_BACKWARD_DONE)
        prompt = _pack_prompt(self.k_seg, self.K_seg)                     # (B, P, c)
        live = self.active.bool()                                         # no data-dependent shapes: graph-capturable
        if hasattr(self.tf, "predict_gains"):
            # the kernel unpacks its prediction into K / k itself (rows t < N - S ... and any it writes past that are
            # overwritten by the swept tail below); a stack LONGER than the horizon (a predictor fitted on N+1-row state
            # sequences, transformer_ilqr.py:106) is legal in the reference: forward_pass only indexes t < horizon (:379)
            # x_err = x - x_ref + state_offset (:504/:532) is formed inside the kernel: it normalises with a shifted mean
            if self._tf_mean is not None:
                self.tf.predict_gains(self.x, prompt, self.K, self.k, self.active, x_mean=self._tf_mean)
            else:
                self.tf.predict_gains(self.x - x_ref_t + self._offset_t, prompt, self.K, self.k, self.active)
            Tn = min(T, N)
            keep = min(S, N - Tn)                                         # swept rows that land inside the horizon
            if keep > 0:
                self.k[:, Tn:Tn + keep] = torch.where(live[:, None, None], self.k_seg[:, :keep], self.k[:, Tn:Tn + keep])   # :517-518 / :542-543
                self.K[:, Tn:Tn + keep] = torch.where(live[:, None, None, None], self.K_seg[:, :keep], self.K[:, Tn:Tn + keep])
            return
        x_err = self.x - x_ref_t + self._offset_t                          # :504/:532
        pred = self.tf.predict_batch(x_err, prompt)                        # (B, T, c): duck-typed predictors
        pk, pK = _unpack_prediction(pred, m, n)
        self.k.copy_(torch.where(live[:, None, None], torch.cat([pk, self.k_seg], dim=1)[:, :N], self.k))
        self.K.copy_(torch.where(live[:, None, None, None], torch.cat([pK, self.K_seg], dim=1)[:, :N], self.K))

    def _log_phase(self, phase):
        """Hybrid / host-driven loops: one small launch per phase fills the device log ring (no host involvement)."""
        if self._log is not None:
            ops.solve_log_record(self.model, self._log, phase, self.x, self.u, self.K, self.k, self.cost, self.alpha_idx,
                                 self.active, self.iters)

    def iterate(self, x_ref_t=None):
        if self.tf is None:
            # pure mode: the fused C driver (one host call, three launches); rec/VxN/VxxN live in its workspace
            if self._ws is None:
                self._ws = ops.workspace(self.model, self._B, self.horizon, self.device)
            self._log_phase(_lib.LOG_PHASE_BEGIN)
            ops.ilqr_iterate(self.model, self.x, self.u, self.K, self.k, self.cost, self.tol, self._ws, self.alphas,
                             self.reg, alpha_idx=self.alpha_idx, active=self.active, iters=self.iters,
                             status=self.status)
            self._log_phase(_lib.LOG_PHASE_END)
            return
        self._log_phase(_lib.LOG_PHASE_BEGIN)
        self.backward(x_ref_t)
        self._log_phase(_lib.LOG_PHASE_GAINS_DONE)
        ops.linesearch(self.model, self.x, self.u, self.K, self.k, self.cost, self.tol, self.alphas,
                       alpha_idx=self.alpha_idx, active=self.active, iters=self.iters, scratch=self._ls_scratch)
        self._log_phase(_lib.LOG_PHASE_END)

    def _iterate_maybe_graph(self, x_ref_t):
        if not self.use_graph:
            return self.iterate(x_ref_t)
        if self._graph is not None and self._graph_log is not self._log:
            self._graph = None                       # the captured launches include (or lack) the log ring's: capture again
        if self._graph is None:
            if self.tf is None:                                                       # allocate outside the capture
                self._ws = ops.workspace(self.model, self._B, self.horizon, self.device)
            elif hasattr(self.tf, "prepare"):
                # token-bias table upload + C struct: no host-to-device copy may happen inside the capture
                self.tf.prepare(self.horizon + 1, x_mean=self._tf_mean)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            # No automatic garbage collection while the stream captures: a collection that happens to run between two of
            # the captured launches may destroy objects that own device resources (graphs, events, tensors of earlier
            # solvers), and a runtime call that is illegal during capture inside a destructor aborts the process (seen once
            # in ~200 runs of the suite).  torch.cuda.graph() itself collects once BEFORE the capture begins.
            import gc
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(g):        # the ops launch on torch's current (capture) stream
                    self.iterate(x_ref_t)
            finally:
                if gc_was_on:
                    gc.enable()
            self._graph = g                      # NOTE: capturing does not execute; the first replay runs iteration 1
            self._graph_log = self._log
        self._graph.replay()

    # ---------------------------------------------------------------------------------------- solve
    def _any_active(self):
        """Host check of the stop flags (the only synchronisation of a host-driven loop)."""
        if self._B <= 64:
            if getattr(self, "_active_host", None) is None or self._active_host.shape[0] != self._B:
                self._active_host = torch.empty((self._B,), dtype=torch.int32).pin_memory()
            self._active_host.copy_(self.active, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            return bool(self._active_host.numpy().any())
        return int(self.active.sum().item()) != 0

    def _require_device_loop(self, what):
        """Per-trajectory rows (`what`: the keyword) run in the device-resident loop alone: NotImplementedError for every mode that
        has none, before anything touches the device."""
        why = None
        if self.tf is not None:
            why = "a predictor (tf) makes the solve a host-driven hybrid loop"
        elif self.use_graph:
            why = "use_graph=True replays host-enqueued iterations"
        elif not self.device_loop:
            why = "device_loop=False is the host-driven loop"
        elif not ops.model_can_device_loop(self.model):
            why = f"model {self.model.name} ({self.model.integrator}) has no persistent kernel"
        if why is not None:
            raise NotImplementedError(f"{what} runs only in the device-resident loop: {why}")

    def _check_model_phys(self, model_phys, B):
        """_require_device_loop, then ValueError for a wrong shape; both before anything touches the device."""
        self._require_device_loop("model_phys")
        ops.check_phys_rows(self.model, model_phys, B, "model_phys")

    def _check_targets(self, targets, B):
        """The same for reference rows."""
        self._require_device_loop("targets")
        ops.check_ref_rows(self.model, targets, B)

    def _check_weights(self, weights, B):
        """The same for per-trajectory cost weights."""
        self._require_device_loop("weights")
        if not ops.model_can_cost_rows(self.model):
            raise NotImplementedError(f"weights runs only in the device-resident loop: model {self.model.name} "
                                      f"({self.model.integrator}) has no persistent kernel that takes cost rows")
        ops.check_cost_rows(self.model, weights, B)

    def solve(self, x0, u_init=None, x_ref=None, max_iter=None, fixed_iters=False, log=None, want_alpha=True,
              upload_guard=True, model_phys=None, targets=None, weights=None, want_grad=False):
        """x0 (B,n), u_init (B,N,m) (zeros if None).  Returns a dict of device tensors:
        K (B,N,m,n), k (B,N,m), x (B,N+1,n), u (B,N,m), cost (B,) fp64, iters (B,), alpha (B,) last accepted step
        (-1: none), status (B,).  fixed_iters=True runs exactly max_iter iterations (benchmarking: stop flags off).
        log: an ops.SolveLog ring the DEVICE fills with one record per trajectory and iteration (the reference's log dict
        and timing samples) — by the persistent kernel between its phases, or by one small launch per phase of a hybrid
        iteration; no host involvement either way.
        model_phys (B, len(model.phys)), or the (B, 8) float32 device tensor of ops.model_phys_tensor: trajectory b is solved with
        row b in place of model.phys (a user model's free parameters likewise) — what B solvers, each built on
        model.with_(phys=row b), return for their one trajectory, bit for bit.  Always the model's persistent kernel (a user
        model's too, as with device_loop="always"); NotImplementedError with a predictor, use_graph=True, device_loop=False or
        a model without such a kernel, ValueError for a wrong shape, both before anything touches the device.  A later call
        without it is the plain solve.
        targets (B, R, n), or (B, n) for R = 1, or the device tensor of ops.x_ref_rows_tensor: per-trajectory, per-step state
        targets.  The cost of trajectory b at horizon step t (t = N: the terminal cost) is taken against row min(t, R - 1) of its
        rows in place of model.x_ref: R = 1 gives every trajectory a goal of its own, R = N + 1 a reference trajectory over the
        horizon, anything between holds its last row.  Weights, barrier, dt and integrator stay the model's.  The same kernel rule,
        refusals and order as model_phys, with which it combines.  Out of scope: iLQR_TF, ShardedILQR, datagen, hybrid mode.
        x_ref: pure mode ignores it — the cost keeps model.x_ref — and hybrid mode feeds it to the predictor's input only
        (x - x_ref + state_offset); a target for the COST is `targets`.
        weights: per-trajectory cost weights — a dict with any of the keys "q", "qf", "r" (each (B, n) / (B, n) / (B, m), or one
        vector that is broadcast over the batch; a missing key keeps the model's values), a plain (B, 2n + m) array in the order
        [q | qf | r], or the device tensor of ops.cost_rows_tensor.  Trajectory b is solved with row b in place of model.q, qf
        and r: what B solvers, each built on model.with_(q=..., qf=..., r=...), return for their one trajectory, bit for bit.  The
        barrier, x_ref (unless targets), dt, integrator and phys (unless model_phys) stay the model's; the values are used as
        given, and a row that makes Q_uu singular shows in that trajectory's status alone.  The same kernel rule, refusals and
        order as model_phys, with which and with targets it combines.  The cart-pole and user-compiled models take weights; the
        built-in quadrotor's persistent kernel has no such form yet and refuses like a model without a kernel
        (NotImplementedError).  Out of scope: per-step weights, ShardedILQR.
        want_grad=True: one ops.cost_gradient launch after the solve, on the returned x, u under this call's model_phys, targets
        and weights, adds "grad_u" (B,N,m) = dJ/du and "grad_norm" (B,) = max |grad_u| per trajectory (computed on the device): a
        first-order optimality measure, which tells a stationary point from a stalled line search (alpha = -1 says only that no
        step was found).  Works in every mode, since it only reads x, u.  Without the keyword nothing new is launched and the
        dict is what it always was; the stop test does not use the gradient.
        QuattroILQR.tube(cov0=, noise=) after a solve: the first-order covariance tube around the returned plan.
        QuattroILQR.fly(observed=, meas_var=) after a solve: the returned plan and gains flown behind a sensor and an estimator."""
        n, m, N, dev = self.model.n, self.model.m, self.horizon, self.device
        if not isinstance(x0, torch.Tensor):
            x0 = np.asarray(x0)
        B = int(np.prod(tuple(x0.shape))) // n
        if model_phys is not None:
            self._check_model_phys(model_phys, B)
        if targets is not None:
            self._check_targets(targets, B)
        if weights is not None:
            self._check_weights(weights, B)
        self._alloc(B)
        self._upload(x0, u_init, guard=upload_guard)
        x0 = self._x0
        self._log = log
        max_iter = self.max_iter if max_iter is None else int(max_iter)
        x_ref_t = None
        rows = dict(model_phys=None, targets=None, weights=None)
        if self.tf is not None:
            xr = np.asarray(self.model.x_ref if x_ref is None else x_ref, dtype=np.float64).reshape(-1)
            off = np.asarray(self.state_offset, dtype=np.float64).reshape(-1)
            key = (xr.tobytes(), off.tobytes())
            if self._ref_key != key:            # (three small host-to-device copies: skipped while the reference stays put)
                self._x_ref_t.copy_(torch.as_tensor(xr.astype(np.float32), device=dev))
                self._offset_t.copy_(torch.as_tensor(off.astype(np.float32), device=dev))
                if self._tf_mean is not None:   # contents change per solve, the address never does (graph-safe)
                    self.tf.shifted_mean(xr - off, out=self._tf_mean)
                self._ref_key = key
            x_ref_t = self._x_ref_t
        if self.tf is None and not self.use_graph and (self._wants_device_loop() or model_phys is not None or targets is not None
                                                           or weights is not None):
            # the whole loop on the device: per-solve state reset, nominal rollout, iterations, per-trajectory stop tests —
            # one launch, no synchronisation
            if self._ws is None:
                self._ws = ops.workspace(self.model, B, N, dev)
            if self._solve_call is None:        # shapes and pointers are fixed for this batch size: checked once
                self._solve_call = ops.PreparedSolve(self.model, self.x, self.u, self.K, self.k, self.cost, self._ws, self.alphas,
                                                     self.reg, x0, self.alpha_idx, self.active, self.iters, self.status)
            # (the rows stay referenced until the next solve: the launch is asynchronous)
            self._model_phys = ops.model_phys_tensor(self.model, model_phys, B, dev)
            self._targets = ops.x_ref_rows_tensor(self.model, targets, B, dev)
            self._weights = ops.cost_rows_tensor(self.model, weights, B, dev)
            self._solve_call(self.tol, max_iter, fixed_iters=fixed_iters, log=log, persistent=self.device_loop == "always",
                             model_phys=self._model_phys, x_ref_rows=self._targets, cost_rows=self._weights)
            rows = dict(model_phys=self._model_phys, targets=self._targets, weights=self._weights)
            max_iter = 0
        else:
            self._ints.copy_(self._ints_init)          # active = 1, iters = 0, alpha_idx = -1, status = 0
            ops.simulate(self.model, x0, self.u, x=self.x, cost=self.cost)
        for it in range(max_iter):
            if fixed_iters:
                self.active.fill_(1)
            self._iterate_maybe_graph(x_ref_t)
            if not fixed_iters and (it + 1) % self.check_every == 0 and it + 1 < max_iter:
                if not self._any_active():                  # the only host sync of the loop
                    break
        self._log = None
        out = dict(K=self.K, k=self.k, x=self.x, u=self.u, cost=self.cost, iters=self.iters, status=self.status)
        if want_alpha:
            alphas_t = self._alphas_t
            out["alpha"] = torch.where(self.alpha_idx >= 0, alphas_t[self.alpha_idx.clamp(min=0).long()],
                                       torch.full_like(alphas_t[:1], -1.0).expand(B))
        if want_grad:
            out["grad_u"] = ops.cost_gradient(self.model, self.x, self.u, want_x0=False, **rows)["grad_u"]
            out["grad_norm"] = out["grad_u"].abs().amax(dim=(1, 2))
        self._solved_rows = rows                        # (what tube() reads the plan under)
        return out

    def tube(self, cov0=None, noise=None):
        """The first-order covariance tube around the plan of the LAST solve when that plan is tracked with its own gains: one
        ops.track_covariance launch on the solve's x, u, K under that call's model_phys (as the plant's rows) and weights, from a
        start of covariance cov0 under a disturbance of covariance noise (the forms ops.track_covariance takes; None: zero).
        -> dict of device tensors "var" (B,N+1,n), "var_u" (B,N,m), "excess" (B,) fp64.  A method of its own rather than a keyword of
        solve(), whose argument list stays what it was: a solve launches nothing new and returns the keys it always did.  The
        built-in models, every mode.  NotImplementedError for a user-compiled model, RuntimeError before the first solve, ValueError
        for a wrong shape, all before anything touches the device."""
        if self.model.model_id == _lib.MODEL_USER:
            raise NotImplementedError("tube: ops.track_covariance runs only for the built-in models")
        rows = getattr(self, "_solved_rows", None)
        if rows is None or self._B is None:
            raise RuntimeError("tube() reads the plan of the last solve: call solve() first")
        ops.check_cov_rows(self.model, cov0, self._B, "cov0")
        ops.check_cov_rows(self.model, noise, self._B, "noise")
        return ops.track_covariance(self.model, self.x, self.u, K=self.K, plant_phys=rows["model_phys"], weights=rows["weights"],
                                    cov0=cov0, noise=noise)

    def fly(self, observed, meas_var, steps=None, xhat0=None, cov0=None, noise=None, meas_noise=None, disturbance=None, plant=None,
            plant_phys=None, want=("xhat", "var", "nis")):
        """The plan of the LAST solve flown behind a sensor: one ops.track_estimate launch from the solve's start x[:, 0] along its
        x, u with its gains K, the control acting on the estimate of an extended Kalman filter that measures the states `observed`
        with variances meas_var.  That call's model_phys rows are the estimator's rows and, unless plant_phys is given, the plant's
        too (as tube() takes them for the covariance).  steps: None = the horizon.  Everything else as ops.track_estimate takes it.
        -> its dict: "x", "u" and what `want` names.  A method of its own rather than a keyword of solve(), whose argument list and
        results stay what they were.  The built-in models.  NotImplementedError for a user-compiled model, RuntimeError before the
        first solve, ValueError for a wrong shape or value, all before anything touches the device."""
        if self.model.model_id == _lib.MODEL_USER:
            raise NotImplementedError("fly: ops.track_estimate runs only for the built-in models")
        rows = getattr(self, "_solved_rows", None)
        if rows is None or self._B is None:
            raise RuntimeError("fly() reads the plan of the last solve: call solve() first")
        obs = ops.check_observed(self.model, observed)
        ops.check_meas_var(meas_var, self._B, len(obs))
        ops.check_cov_rows(self.model, cov0, self._B, "cov0")
        ops.check_cov_rows(self.model, noise, self._B, "noise")
        ops.check_plant(self.model, plant)
        ops.check_phys_rows(self.model, plant_phys, self._B, "plant_phys")
        S, n = self.horizon if steps is None else int(steps), self.model.n
        if not 1 <= S <= self.horizon:
            raise ValueError("steps must be in 1..N")
        for name, t, shape in (("xhat0", xhat0, (self._B, n)), ("meas_noise", meas_noise, (S, self._B, len(obs))),
                               ("disturbance", disturbance, (S, self._B, n))):
            if t is not None and tuple(np.shape(t)) != shape:
                raise ValueError(f"{name} must have shape {shape} (got {tuple(np.shape(t))})")
        return ops.track_estimate(self.model, self.x[:, 0].contiguous(), self.x, self.u, self.K,
                                  S, obs, meas_var, xhat0=xhat0, cov0=cov0, noise=noise,
                                  meas_noise=meas_noise, disturbance=disturbance, plant=plant,
                                  plant_phys=rows["model_phys"] if plant_phys is None else plant_phys, model_phys=rows["model_phys"],
                                  want=want)


# ================================================================================================ iLQR_TF drop-in
def _timed(attr):
    """Append the wall time of the call (device work included: the stream is synchronised first) to a list attribute —
    the reference's measure_time decorator, quattro_ilqr_tf.py:16-26."""
    def deco(fn):
        def wrapper(self, *a, **kw):
            t0 = time.time()
            out = fn(self, *a, **kw)
            torch.cuda.synchronize(self._dev)
            getattr(self, attr).append(time.time() - t0)
            return out
        wrapper.__name__ = fn.__name__
        wrapper.__doc__ = fn.__doc__
        return wrapper
    return deco


def _diag_or_none(M, k):
    M = np.asarray(M, dtype=np.float64)
    if M.shape != (k, k) or np.any(M - np.diag(np.diag(M)) != 0.0):
        return None
    return tuple(float(v) for v in np.diag(M))


def recognise_problem_object(owner):
    """The reference's OWN problem objects — examples/quadrotor/quadrotor_mpc.py:29-66 (QuadrotorMPC) and
    examples/cartpole/cartpole_mpc.py:183-216 (CartPoleMPC), whose bound methods discrete_dynamics / running_cost / final_cost
    they hand to iLQR_TF — carry everything a built-in device model is made of as attributes: Q, R, Qf, x_ref, dt,
    integration_method, the physical constants on `.dynamics` (quadrotor_dynamics.py:40-45: m, Ix, Iy, Iz, arm, g;
    cartpole_dynamics.py:27-30: m_cart, m_pole, length, gravity) and, for the quadrotor, the barrier's alpha / beta.
    -> the DeviceModel those attributes describe, or None if the object does not have that shape.  The caller must still CHECK
    that the callables compute what the model computes (resolve_device_model probes them): attributes are only a claim."""
    from .models import cartpole_model, quadrotor_model
    if owner is None or not all(hasattr(owner, a) for a in ("Q", "R", "Qf", "x_ref", "dt", "integration_method", "dynamics")):
        return None
    try:
        x_ref = np.asarray(owner.x_ref, dtype=np.float64).reshape(-1)
        n, m = x_ref.shape[0], np.asarray(owner.R).shape[0]
        q, r, qf = _diag_or_none(owner.Q, n), _diag_or_none(owner.R, m), _diag_or_none(owner.Qf, n)
        if q is None or r is None or qf is None or owner.integration_method not in ("euler", "rk4"):
            return None
        dyn = owner.dynamics
        if (n, m) == (12, 4) and all(hasattr(dyn, a) for a in ("m", "Ix", "Iy", "Iz", "arm", "g")) and \
                hasattr(owner, "alpha") and hasattr(owner, "beta"):
            base = quadrotor_model(dt=float(owner.dt), integrator=owner.integration_method, x_ref=x_ref)
            return base.with_(q=q, r=r, qf=qf, barrier_alpha=float(owner.alpha), barrier_beta=float(owner.beta),
                              phys=(float(dyn.m), float(dyn.Ix), float(dyn.Iy), float(dyn.Iz), float(dyn.arm), float(dyn.g),
                                    base.phys[6]))          # k_yaw is a literal in the reference (quadrotor_dynamics.py:144)
        if (n, m) == (4, 1) and all(hasattr(dyn, a) for a in ("m_cart", "m_pole", "length", "gravity")):
            base = cartpole_model(dt=float(owner.dt), integrator=owner.integration_method, x_ref=x_ref)
            return base.with_(q=q, r=r, qf=qf, phys=(float(dyn.m_cart), float(dyn.m_pole), float(dyn.length), float(dyn.gravity)))
    except (TypeError, ValueError, AttributeError):
        return None
    return None


def _device_eval(md, xs, us, device):
    """f(x, u), L(x, u), Lf(x) of the device model at P points (xs (P, n), us (P, m)), through the kernels the solver runs."""
    dev = torch.device(device)
    x = torch.as_tensor(np.ascontiguousarray(xs, dtype=np.float32), device=dev)
    u = torch.as_tensor(np.ascontiguousarray(us, dtype=np.float32), device=dev).reshape(-1, 1, md.m)
    traj, _ = ops.simulate(md, x, u)                                            # (P, 2, n): [x, f(x, u)]
    f = traj[:, 1].double().cpu().numpy()
    ref = torch.as_tensor(np.asarray(md.x_ref, dtype=np.float32), device=dev).expand(x.shape[0], md.n)
    L = ops.total_cost(md, torch.stack([x, ref], dim=1).contiguous(), u).cpu().numpy()          # Lf(x_ref) = 0
    zero = md.with_(q=(0.0,) * md.n, r=(0.0,) * md.m, barrier_alpha=0.0)
    Lf = ops.total_cost(zero, torch.stack([ref, x], dim=1).contiguous(), torch.zeros_like(u)).cpu().numpy()
    return f, L, Lf


def probe_callables(md, dynamics, cost, cost_final, device="cuda:0", points=6, seed=20240607):
    """Do the three Python callables compute what device model `md` computes?  Evaluates both at a few seeded points
    (states around x_ref, controls of both signs: the barrier's active side included) and compares at the tolerances of the
    golden families G1 / G2 (fp32 device vs the reference's fp64, 1e-6 relative; 1e-5 used).  -> (ok, worst)."""
    rng = np.random.default_rng(seed)
    xs = np.asarray(md.x_ref, dtype=np.float64) + 0.3 * rng.standard_normal((points, md.n))
    us = rng.uniform(-0.5, 3.0, (points, md.m))
    xs, us = xs.astype(np.float32).astype(np.float64), us.astype(np.float32).astype(np.float64)
    f_d, L_d, Lf_d = _device_eval(md, xs, us, device)
    worst = 0.0
    for i in range(points):
        f_h = np.asarray(dynamics(xs[i].copy(), us[i].copy()), dtype=np.float64).reshape(-1)
        if f_h.shape != (md.n,):
            return False, float("inf")
        worst = max(worst, float(np.max(np.abs(f_h - f_d[i]) / (1.0 + np.abs(f_h)))))
        L_h, Lf_h = float(cost(xs[i].copy(), us[i].copy())), float(cost_final(xs[i].copy()))
        worst = max(worst, abs(L_h - L_d[i]) / (1.0 + abs(L_h)), abs(Lf_h - Lf_d[i]) / (1.0 + abs(Lf_h)))
    return worst <= 1e-5, worst


def resolve_device_model(dynamics, cost, cost_final, model=None, device="cuda:0"):
    """Find the device model behind the callables the reference signature takes.
      1. `model=` given, or a DeviceModel handed over in place of a callable;
      2. callables bound to an object with `device_model()` (the MPC mirrors of quattro_ilqr_amd.mpc);
      3. callables bound to one of the REFERENCE's own problem objects (examples/*/…_mpc.py): recognised by their attribute
         set (recognise_problem_object) and then VERIFIED — the three callables are probed at seeded points against the
         device model's f, L, Lf — so the reference's QuadrotorMPC / CartPoleMPC bind unchanged;
    anything else raises: arbitrary Python cannot run inside a kernel and there is deliberately no CPU path."""
    if model is not None:
        return model if isinstance(model, DeviceModel) or not callable(model) else model()
    for fn in (dynamics, cost, cost_final):
        if isinstance(fn, DeviceModel):           # a (user-compiled) device model handed over in place of the callables
            return fn
        owner = getattr(fn, "__self__", None)
        if owner is not None and hasattr(owner, "device_model"):
            return owner.device_model()
    owners = {id(getattr(fn, "__self__", None)) for fn in (dynamics, cost, cost_final)}
    owner = getattr(dynamics, "__self__", None)
    hint = ("write the problem as a device model with quattro_ilqr_amd.compile_model(...) and pass it as model=, or use "
            "quattro_ilqr_amd.mpc.QuadrotorMPC / CartPoleMPC")
    if owner is not None and len(owners) == 1:
        md = recognise_problem_object(owner)
        if md is not None:
            ok, worst = probe_callables(md, dynamics, cost, cost_final, device)
            if ok:
                return md
            raise NotImplementedError(
                f"the callables belong to an object that looks like the reference's {md.name} problem (Q, R, Qf, x_ref, dt, "
                f"dynamics.*), but they do not compute what the built-in {md.name} device model computes from those attributes "
                f"(worst relative difference {worst:.2e} at the probe points, tolerance 1e-5): {hint}.")
    raise NotImplementedError(
        "iLQR_TF on the GPU needs a device model: pass model=quattro_ilqr_amd.models.<...>_model(...) or callables "
        "bound to an object with .device_model() (quattro_ilqr_amd.mpc.QuadrotorMPC / CartPoleMPC) or to one of the "
        "reference's own QuadrotorMPC / CartPoleMPC objects.  Arbitrary Python callables cannot be evaluated by a HIP kernel, "
        f"and this package has no CPU fallback: {hint}.")


def _owner_fingerprint(owner):
    """What recognise_problem_object reads, as bytes: the verified model is reused while these do not change."""
    b = lambda a: np.asarray(a, dtype=np.float64).tobytes()
    dyn = owner.dynamics
    return (b(owner.Q), b(owner.R), b(owner.Qf), b(owner.x_ref), float(owner.dt), owner.integration_method,
            getattr(owner, "alpha", None), getattr(owner, "beta", None),
            tuple(sorted((k, float(v)) for k, v in vars(dyn).items() if isinstance(v, (int, float)))))


class iLQR_TF:
    """Same constructor, attributes, methods and return conventions as the reference's iLQR_TF
    (quattro_ilqr_tf/quattro_ilqr_tf.py:50-612); every numeric step runs in libquattro_hip.so on `device`.
    NumPy fp64 at the surface, fp32 on the device.  Extra keyword arguments: model, device."""

    def __init__(self, dynamics, cost, cost_final, x0, u_init, horizon, dt=0.01, max_iter=100, tol=1e-3, tf=None,
                 tf_window=10, blend_mode=False, enable_log=True, model=None, device="cuda:0"):
        self.f, self.L, self.Lf = dynamics, cost, cost_final
        self._model_arg = model
        self.x0 = x0
        self.u = u_init
        self.horizon = horizon
        self.dt = dt
        self.total_iter = 0
        self.max_iter = max_iter
        self.tol = tol
        self.state_offset = np.zeros_like(np.asarray(self.x0, dtype=np.float64))
        if tf_window >= horizon:
            raise ValueError("tf_window must be less than the horizon.")
        self.tf_window = tf_window
        self.tf = tf
        self.blend_mode = blend_mode
        self.enable_log = enable_log
        self.logs = []
        self.log_the_optimal_solution = False
        self.backward_pass_time, self.forward_pass_time, self.total_time, self.inference_time = [], [], [], []
        self._dev = torch.device(device)
        self._log_guess = 2
        self._foreign = None                                         # (fingerprint, verified model) of a reference problem object
        self._model()                                                # fail at construction, not at the first solve
        if self.tf is not None:
            if hasattr(self.tf, "prompt_len"):
                self.tf_window = self.tf.prompt_len
            inner = self.tf.predict

            def timed_predict(*a, **kw):
                t0 = time.time()
                out = inner(*a, **kw)
                self.inference_time.append(time.time() - t0)
                return out
            self.tf.predict = timed_predict

    # ------------------------------------------------------------------ helpers
    def _model(self):
        owner = getattr(self.f, "__self__", None)
        if self._model_arg is None and owner is not None and not isinstance(self.f, DeviceModel) and \
                not hasattr(owner, "device_model") and hasattr(owner, "dynamics"):
            # one of the reference's own problem objects: recognised and probed once, again only when an attribute changes
            try:
                fp = _owner_fingerprint(owner)
            except (AttributeError, TypeError, ValueError):
                fp = None
            if fp is not None and self._foreign is not None and self._foreign[0] == fp:
                return self._foreign[1]
            md = resolve_device_model(self.f, self.L, self.Lf, None, self._dev)
            self._foreign = (fp, md)
            return md
        return resolve_device_model(self.f, self.L, self.Lf, self._model_arg, self._dev)

    def _t(self, a, shape):
        return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32)).reshape(shape), device=self._dev)

    def _u_t(self, u_seq, m):
        return self._t(np.array([np.asarray(v, dtype=np.float64).reshape(-1) for v in u_seq]), (1, self.horizon, m))

    # ------------------------------------------------------------------ reference API
    def simulate(self, u_seq):
        md = self._model()
        x, _ = ops.simulate(md, self._t(self.x0, (1, md.n)), self._u_t(u_seq, md.m))
        return x[0].double().cpu().numpy()

    def compute_total_cost(self, x_seq, u_seq):
        md = self._model()
        J = ops.total_cost(md, self._t(x_seq, (1, self.horizon + 1, md.n)), self._u_t(u_seq, md.m))
        return float(J[0].item())

    # ---- the reference's per-point derivative methods (:149-275), on the device: exact derivatives of the built-in
    # model where the reference takes finite differences (eps = 1e-5)
    def _point_derivs(self, x, u):
        md = self._model()
        xs = ops.simulate(md, self._t(x, (1, md.n)), self._t(u, (1, 1, md.m)))[0]      # (1, 2, n): [x, f(x, u)]
        layout = ops.model_layout(md)
        rec, VxN, VxxN, _ = ops.linearize(md, xs, self._t(u, (1, 1, md.m)), layout=layout)
        d = {k: v[0, 0].double().cpu().numpy() for k, v in ops.unpack_derivs(rec, 1, md.n, md.m, layout, lib=_lib.load_for(md)).items()}
        return d

    def _compute_dynamics_jacobians(self, x, u):
        """-> (A (n,n), B (n,m)) of x' = f(x, u) — quattro_ilqr_tf.py:182-204."""
        d = self._point_derivs(x, u)
        return d["A"], d["B"]

    def _compute_cost_derivatives(self, x, u):
        """-> (L, L_x, L_u, L_xx, L_uu, L_xu) with L_xu (n,m) as the reference returns it — :217-275."""
        md = self._model()
        d = self._point_derivs(x, u)
        xx = torch.cat([self._t(x, (1, md.n)), self._t(md.x_ref, (1, md.n))], dim=0).reshape(1, 2, md.n)
        L = float(ops.total_cost(md, xx, self._t(u, (1, 1, md.m)))[0].item())         # L(x,u) + Lf(x_ref) = L(x,u)
        return L, d["lx"], d["lu"], d["lxx"], d["luu"], d["lux"].T.copy()

    def _terminal(self, x):
        md = self._model()
        xs = torch.cat([self._t(x, (1, md.n)), self._t(x, (1, md.n))], dim=0).reshape(1, 2, md.n)
        _, VxN, VxxN, _ = ops.linearize(md, xs, torch.zeros((1, 1, md.m), dtype=torch.float32, device=self._dev),
                                        layout=ops.model_layout(md))
        return VxN[0].double().cpu().numpy(), VxxN[0].double().cpu().numpy()

    def _finite_diff_gradient_final(self, x):
        """grad Lf(x) — :149-157."""
        return self._terminal(x)[0]

    def _finite_diff_hessian_final(self, x):
        """Hessian of Lf at x — :163-174."""
        return self._terminal(x)[1]

    def _backward(self, x_seq, u_seq, start_idx):
        md = self._model()
        x = self._t(x_seq, (1, self.horizon + 1, md.n))
        u = self._u_t(u_seq, md.m)
        if ops.model_fuses_sweep(md):                   # the same kernel the batched solver runs
            K, k, status = ops.linearize_sweep(md, x, u, t_start=start_idx)
        else:
            layout = ops.model_layout(md)
            rec, VxN, VxxN, _ = ops.linearize(md, x, u, t_start=start_idx, layout=layout)
            K, k, status = ops.riccati_sweep(rec, VxN, VxxN, md.n, md.m, layout, repair=True, lib=_lib.load_for(md))
        st = int(status[0].item())
        if st & 2:
            raise np.linalg.LinAlgError("Singular matrix")      # what np.linalg.inv raises in the reference (:306)
        K, k = K[0].double().cpu().numpy(), k[0].double().cpu().numpy()
        return [k[s] for s in range(k.shape[0])], [K[s] for s in range(K.shape[0])]

    @_timed("backward_pass_time")
    def backward_pass(self, x_seq, u_seq):
        return self._backward(x_seq, u_seq, 0)

    @_timed("backward_pass_time")
    def backward_pass_segment(self, x_seq, u_seq, start_idx):
        return self._backward(x_seq, u_seq, start_idx)

    @_timed("forward_pass_time")
    def forward_pass(self, x_seq, u_seq, k_seq, K_seq, alpha=1.0):
        md = self._model()
        N = self.horizon
        if len(k_seq) < N or len(K_seq) < N:
            raise IndexError("list index out of range")          # the reference indexes k_seq[t] for t < horizon
        x = self._t(x_seq, (1, N + 1, md.n))
        x[0, 0] = self._t(self.x0, (md.n,))                        # new_x_seq[0] = self.x0 (:379)
        cost, xn, un = ops.rollout(md, x, self._u_t(u_seq, md.m), self._t(np.array(K_seq)[:N], (1, N, md.m, md.n)),
                                   self._t(np.array(k_seq)[:N], (1, N, md.m)), (float(alpha),), want_traj=True)
        new_u = un[0, 0].double().cpu().numpy()
        return xn[0, 0].double().cpu().numpy(), [new_u[t] for t in range(N)], float(cost[0, 0].item())

    @_timed("forward_pass_time")
    def forward_pass_segment(self, x_seq, u_seq, k_seq_seg, K_seq_seg, start_idx, alpha=1.0):
        """Closed-loop rollout of the tail t in [start_idx, horizon) from x_seq[start_idx] with gains indexed t - start_idx;
        returns (new_x_seq_seg (S+1, n), new_u_seq_seg (list of S), seg_cost) — quattro_ilqr_tf.py:402-421 (never called by
        the reference itself; part of the class surface).  seg_cost follows the reference literally: compute_total_cost
        sums L over the first `horizon` rows it is given, so the reference raises IndexError for a proper tail
        (start_idx > 0) — reproduced here; start_idx == 0 is forward_pass from x_seq[0]."""
        md = self._model()
        N = self.horizon
        S = N - int(start_idx)
        if not 0 <= int(start_idx) < N:
            raise IndexError("list index out of range")
        if len(k_seq_seg) < S or len(K_seq_seg) < S:
            raise IndexError("list index out of range")
        x_tail = np.asarray(x_seq, dtype=np.float64)[start_idx:]
        u_tail = np.array([np.asarray(v, dtype=np.float64).reshape(-1) for v in u_seq])[start_idx:]
        x = self._t(x_tail, (1, S + 1, md.n))
        cost, xn, un = ops.rollout(md, x, self._t(u_tail, (1, S, md.m)), self._t(np.array(K_seq_seg)[:S], (1, S, md.m, md.n)),
                                   self._t(np.array(k_seq_seg)[:S], (1, S, md.m)), (float(alpha),), want_traj=True)
        new_x = xn[0, 0].double().cpu().numpy()
        new_u = un[0, 0].double().cpu().numpy()
        if S < N:
            raise IndexError("list index out of range")          # compute_total_cost indexes u_seq[t] for t < horizon (:140-141)
        return new_x, [new_u[t] for t in range(S)], float(cost[0, 0].item())

    def optimize(self, x_ref, verbose=False):
        """Returns (u_seq: list of (m,) arrays, final_x_seq: (N+1, n) array) and sets self.u, like the reference.

        The whole loop of quattro_ilqr_tf.py:424-591 runs on the device: pure mode = ONE persistent launch
        (quattro_ilqr_solve_logged_f32), hybrid mode with a device predictor = one captured graph per iteration; the
        per-iteration log entries and the samples of the *_time lists come back in one download of the device log ring
        (csrc/solve_log.h).  A foreign predictor that only offers predict() on NumPy arrays is driven from the host,
        iteration by iteration (_optimize_host_loop)."""
        t0 = time.time()
        md = self._model()
        tf = self.tf
        if tf is not None and not (hasattr(tf, "predict_gains") and hasattr(tf, "target_len") and
                                   int(tf.target_len) + int(self.tf_window) == int(self.horizon)):
            out = self._optimize_host_loop(md, x_ref, verbose)
            torch.cuda.synchronize(self._dev)
        else:
            out = self._optimize_device(md, x_ref, verbose)        # (ends with a synchronising download)
        self.total_time.append(time.time() - t0)                   # measure_time("total_time"), quattro_ilqr_tf.py:423
        return out

    def _single(self, md):
        """The single-trajectory batched solver behind optimize(): buffers, workspace, captured graph and log ring live as
        long as the problem (model, horizon, predictor, window) does not change."""
        key = (md, int(self.horizon), id(self.tf), int(self.tf_window), bool(self.enable_log))
        cap = max(1, int(self.max_iter))
        if getattr(self, "_single_key", None) != key:
            use_graph = self.tf is not None and (not hasattr(self.tf, "fused_kernel_covers") or self.tf.fused_kernel_covers())
            self._single_solver = QuattroILQR(md, int(self.horizon), max_iter=int(self.max_iter), tol=float(self.tol),
                                              tf=self.tf, tf_window=int(self.tf_window), device=self._dev, check_every=1,
                                              use_graph=use_graph, device_loop="always")
            self._single_log = None
            self._single_key = key
        if self._single_log is None or self._single_log.capacity < cap:
            self._single_log = ops.SolveLog(md, int(self.horizon), 1, cap, self._dev, traj=bool(self.enable_log),
                                            gains=bool(self.enable_log))
        return self._single_solver, self._single_log

    def _optimize_device(self, md, x_ref, verbose):
        N, n, m = int(self.horizon), md.n, md.m
        sv, log = self._single(md)
        sv.max_iter, sv.tol = int(self.max_iter), float(self.tol)
        sv.state_offset = self.state_offset
        x0 = np.asarray(self.x0, dtype=np.float64).reshape(1, n)
        u0 = np.asarray(self.u, dtype=np.float64).reshape(1, N, m)
        sv.solve(x0, u0, x_ref=x_ref, log=log, want_alpha=False, upload_guard=False)
        # ONE download: the state block (u, x, cost, iters, flags) and, ahead of the synchronisation, as many log records as
        # the previous solve needed (a warm-started control loop repeats itself); a second, exactly sized one only if this
        # solve ran longer
        guess = min(max(2, self._log_guess), log.capacity)
        st = sv.download_state(log, guess)
        n_it = int(st["iters"][0])
        self._log_guess = n_it + 1
        u_fin = st["u"][0].astype(np.float64)
        x_fin = st["x"][0].astype(np.float64)
        hybrid = self.tf is not None
        if n_it > 0:
            rows = log.staged(n_it) if n_it <= guess else log.rows(0, n_it)
            dt = (rows["stamps"][:, 1:].astype(np.int64) - rows["stamps"][:, :-1].astype(np.int64)) * ops.SolveLog.TICK
            self.backward_pass_time.extend(dt[:, 0].tolist())
            if hybrid:
                self.inference_time.extend(dt[:, 1].tolist())
            self.forward_pass_time.extend(dt[:, 2].tolist())
            if self.enable_log or verbose:
                self._append_logs(rows, n_it, u_fin, x_fin, hybrid, verbose)
            self.total_iter = n_it - 1
            if int(st["status"][0]) & _lib.TRAJ_SINGULAR:
                raise np.linalg.LinAlgError("Singular matrix")      # what np.linalg.inv raises in the reference (:306)
        u_seq = list(u_fin)
        self.u = u_seq
        return u_seq, x_fin

    def _append_logs(self, rows, n_it, u_fin, x_fin, hybrid, verbose):
        """Device log records -> the reference's per-iteration dicts (quattro_ilqr_tf.py:453-466 / :565-578)."""
        N, W = int(self.horizon), int(self.tf_window)
        have = self.enable_log
        if have:
            xs, us = rows["x"].astype(np.float64), rows["u"].astype(np.float64)
            Ks, ks = rows["K"].astype(np.float64), rows["k"].astype(np.float64)
        for i in range(n_it):
            ai = int(rows["alpha_idx"][i])
            found = ai >= 0
            alpha = ALPHAS[ai] if found else None
            new_cost = float(rows["cost"][i, 1]) if found else None
            if have:
                if found:      # the accepted candidate is the next iteration's nominal (or the result)
                    new_x = xs[i + 1] if i + 1 < n_it else x_fin
                    new_u = list(us[i + 1] if i + 1 < n_it else u_fin)
                else:
                    new_x, new_u = None, None
                entry = {"iteration": i, "x_seq": xs[i], "u_seq": new_u if found else list(us[i]),
                         "current_cost": float(rows["cost"][i, 0])}
                if hybrid:     # the swept tail of the stack (:493-502): rows N - W .. N - 1
                    entry["k_seq_seg"], entry["K_seq_seg"] = list(ks[i, N - W:]), list(Ks[i, N - W:])
                else:
                    entry["k_seq"], entry["K_seq"] = list(ks[i]), list(Ks[i])
                entry.update({"alpha": alpha, "new_x_seq": new_x, "new_u_seq": new_u, "new_cost": new_cost,
                              "found_update": found})
                self.logs.append(entry)
            if verbose:
                print(f"Iteration {i}, Cost: {new_cost:.4f}, Alpha: {alpha}")

    def _optimize_host_loop(self, md, x_ref, verbose=False):
        """The reference's loop driven from the host, one iteration at a time through the per-step methods: the path for a
        predictor that is not a device predictor (any object with predict(x_seq_err, kK_prompt) on NumPy arrays,
        quattro_ilqr_tf.py:116-122) or whose stack does not tile the horizon exactly."""
        N = self.horizon
        u_seq = [np.asarray(v, dtype=np.float64).reshape(-1) for v in self.u]
        for iteration in range(self.max_iter):
            x_seq = self.simulate(u_seq)
            current_cost = self.compute_total_cost(x_seq, u_seq)
            if self.tf is None:
                k_seq, K_seq = self.backward_pass(x_seq, u_seq)
                full_k, full_K = k_seq, K_seq
                gains_log = dict(k_seq=k_seq, K_seq=K_seq)
            else:
                start_idx = N - self.tf_window
                k_seg, K_seg = self.backward_pass_segment(x_seq, u_seq, start_idx)
                k_arr, K_arr = np.array(k_seg), np.array(K_seg)
                kK_prompt = np.concatenate([k_arr, K_arr.reshape(k_arr.shape[0], -1)], axis=-1)
                x_seq_err = x_seq - x_ref + self.state_offset
                pred = np.asarray(self.tf.predict(x_seq_err, kK_prompt))
                pv = pred.reshape(pred.shape[0], md.m, 1 + md.n)
                full_k = np.concatenate([pv[:, :, 0], k_arr], axis=0)
                full_K = np.concatenate([pv[:, :, 1:], K_arr], axis=0)
                gains_log = dict(k_seq_seg=k_seg, K_seq_seg=K_seg)
            found_update, chosen_alpha, new_x_seq, new_u_seq, new_cost = False, None, None, None, None
            for alpha in ALPHAS:
                cand_x, cand_u, cand_cost = self.forward_pass(x_seq, u_seq, full_k, full_K, alpha)
                if cand_cost <= current_cost:
                    found_update, chosen_alpha = True, alpha
                    new_x_seq, new_u_seq, new_cost = cand_x, cand_u, cand_cost
                    u_seq = cand_u
                    break
            if self.enable_log:
                entry = {"iteration": iteration, "x_seq": x_seq, "u_seq": u_seq, "current_cost": current_cost}
                entry.update(gains_log)
                entry.update({"alpha": chosen_alpha, "new_x_seq": new_x_seq, "new_u_seq": new_u_seq,
                              "new_cost": new_cost, "found_update": found_update})
                self.logs.append(entry)
            self.total_iter = iteration
            if verbose:
                print(f"Iteration {iteration}, Cost: {new_cost:.4f}, Alpha: {chosen_alpha}")
            if (not found_update) or (abs(current_cost - new_cost) < self.tol):
                break
        self.u = u_seq
        return u_seq, self.simulate(u_seq)

    def get_time(self):
        if self.tf is not None:
            return (self.total_time, self.backward_pass_time, self.forward_pass_time, self.inference_time)
        return (self.total_time, self.backward_pass_time, self.forward_pass_time)

    def set_state_offset(self, x_offset):
        self.state_offset = x_offset

    def get_state_offset(self):
        return self.state_offset.copy()
