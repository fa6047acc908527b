"""Receding-horizon wrappers with the reference's interface, solving on the GPU.

Mirrors:
  QuadrotorMPC       <- examples/quadrotor/quadrotor_mpc.py:6-124
  CartPoleMPC        <- examples/cartpole/cartpole_mpc.py:122-359 (every mode: LQR only, iLQR only, iLQR + transformer,
                        and the blending of either with the LQR law)
  ControllerSwitcher <- examples/cartpole/cartpole_mpc.py:10-116
The LQR law is a constant of the problem (infinite-horizon DARE on the upright linearisation); it is host arithmetic,
solved once with scipy and cached, not a kernel.

The `discrete_dynamics` / `running_cost` / `final_cost` methods exist because the reference's callers read them; they
are handles that identify the built-in device model to iLQR_TF (via `device_model()`), and are NOT evaluated by the
solver.  Calling them directly evaluates one point on the GPU through the same kernels.
"""
import numpy as np
import torch

from . import ops
from .models import cartpole_model, quadrotor_model
from .solver import QuattroILQR, iLQR_TF


class _DeviceProblem:
    """Shared plumbing: the three reference callables, evaluated on the device for a single point."""

    _dev = "cuda:0"

    def device_model(self):
        raise NotImplementedError

    def _pt(self, v, d):
        return torch.as_tensor(np.asarray(v, dtype=np.float32).reshape(1, d), device=self._dev)

    def discrete_dynamics(self, x, u):
        md = self.device_model()
        xs, _ = ops.simulate(md, self._pt(x, md.n), self._pt(u, md.m).reshape(1, 1, md.m))
        return xs[0, 1].double().cpu().numpy()

    def running_cost(self, x, u):
        # L(x,u) = total cost of a one-step sequence minus the terminal term of its end state
        md = self.device_model()
        xx = torch.cat([self._pt(x, md.n), self._pt(self.x_ref, md.n)], dim=0).reshape(1, 2, md.n)
        return float(ops.total_cost(md, xx, self._pt(u, md.m).reshape(1, 1, md.m))[0].item())

    def final_cost(self, x):
        md = self.device_model().with_(q=(0.0,) * len(self.x_ref), r=(0.0,) * self.device_model().m, barrier_alpha=0.0)
        xx = torch.cat([self._pt(self.x_ref, md.n), self._pt(x, md.n)], dim=0).reshape(1, 2, md.n)
        return float(ops.total_cost(md, xx, torch.zeros((1, 1, md.m), device=self._dev))[0].item())


class QuadrotorMPC(_DeviceProblem):
    def __init__(self, horizon=30, dt=0.01, integration_method="rk4", transformer_model=None,
                 log_filename="quad_ilqr_log.pkl", device="cuda:0"):
        self.horizon, self.dt, self.integration_method, self.log_filename = horizon, dt, integration_method, log_filename
        self._dev = device
        self.x_ref = np.zeros(12)
        self.x_ref[2] = 0.5
        self.Q = np.diag([10.0, 10.0, 50.0, 1.0, 1.0, 1.0, 10.0, 10.0, 50.0, 1.0, 1.0, 1.0])
        self.R = np.diag([0.01, 0.01, 0.01, 0.01])
        self.Qf = np.diag([100.0, 100.0, 500.0, 10.0, 10.0, 10.0, 100.0, 100.0, 500.0, 10.0, 10.0, 10.0])
        self.alpha, self.beta = 1000.0, 10.0
        self.u_init = [np.zeros(4) for _ in range(horizon)]
        self.transformer_model = transformer_model
        self.ilqr = iLQR_TF(dynamics=self.discrete_dynamics, cost=self.running_cost, cost_final=self.final_cost,
                            x0=self.x_ref, u_init=self.u_init, horizon=horizon, tf=self.transformer_model,
                            device=device)
        offset = self.ilqr.get_state_offset()
        offset[2] = 0.5                                      # quadrotor_mpc.py:64-66
        self.ilqr.set_state_offset(offset)

    def device_model(self):
        # rebuilt only when an attribute it is made of has changed (optimize() asks on every call: the weights stay
        # assignable like the reference's, and an unchanged problem costs a few byte comparisons)
        b = lambda a: np.asarray(a, dtype=np.float64).tobytes()
        key = (self.dt, self.integration_method, b(self.x_ref), b(self.Q), b(self.R), b(self.Qf), self.alpha, self.beta)
        if getattr(self, "_md_key", None) != key:
            self._md = quadrotor_model(dt=self.dt, integrator=self.integration_method, x_ref=self.x_ref).with_(
                q=tuple(np.diag(self.Q)), r=tuple(np.diag(self.R)), qf=tuple(np.diag(self.Qf)),
                barrier_alpha=float(self.alpha), barrier_beta=float(self.beta))
            self._md_key = key
        return self._md

    def control_step(self, x_current):
        self.ilqr.x0 = x_current
        optimal_u_seq, optimal_x_seq = self.ilqr.optimize(x_ref=self.x_ref, verbose=False)
        self.ilqr.u = optimal_u_seq[1:].copy()               # warm start: shift, hold the last input (:121-122)
        self.ilqr.u.append(optimal_u_seq[-1])
        return optimal_x_seq, optimal_u_seq


class ControllerSwitcher:
    """Blending weight between the nonlinear controller (1) and the LQR law (0) from the norm of the state error:
    0 below epsilon_low, 1 above epsilon_high, linear in between.  The error history (3 entries) and the acceleration
    norm exist as in the reference, whose acceleration damping is commented out (cartpole_mpc.py:98-112)."""

    def __init__(self, epsilon_low=0.05, epsilon_high=0.2, epsilon_dd=0.1, gamma=10.0, use_sigmoid=False):
        self.epsilon_low, self.epsilon_high, self.epsilon_dd = epsilon_low, epsilon_high, epsilon_dd
        self.gamma, self.use_sigmoid = gamma, use_sigmoid
        self.error_history = []

    def update_error(self, error):
        self.error_history.append(error)
        if len(self.error_history) > 3:
            self.error_history.pop(0)

    def compute_current_error_norm(self):
        return float(np.linalg.norm(self.error_history[-1])) if self.error_history else 0.0

    def compute_acceleration_norm(self, dt):
        if len(self.error_history) < 3:
            return 0.0
        e0, e1, e2 = self.error_history
        return float(np.linalg.norm((e2 - 2 * e1 + e0) / dt ** 2))

    def get_blending_weight(self, dt):
        e = self.compute_current_error_norm()
        if e <= self.epsilon_low:
            return 0.0
        if e >= self.epsilon_high:
            return 1.0
        return (e - self.epsilon_low) / (self.epsilon_high - self.epsilon_low)


class CartPoleMPC(_DeviceProblem):
    """Modes as in the reference (flags; `lqr_only` wins, then `ilqr_only`; default = iLQR only):
    lqr_only | ilqr_only | ilqr_tf_only | ilqr_tf_blend (| use_transformer, kept for signature compatibility)."""

    def __init__(self, horizon=30, dt=0.01, integration_method="rk4", transformer_model=None,
                 log_filename="ilqr_log.pkl", switcher_params=None, lqr_only=False, ilqr_only=False, ilqr_tf_only=False,
                 ilqr_tf_blend=False, use_transformer=False, device="cuda:0"):
        self.horizon, self.dt, self.integration_method, self.log_filename = horizon, dt, integration_method, log_filename
        self.lqr_only, self.ilqr_only, self.ilqr_tf_only = lqr_only, ilqr_only, ilqr_tf_only
        self.ilqr_tf_blend, self.use_transformer = ilqr_tf_blend, use_transformer
        self._dev = device
        self.x_ref = np.array([0.0, 0.0, 0.0, 0.0])
        self.Q = np.diag([5.0, 0.1, 10.0, 0.1])
        self.R = np.diag([0.001])
        self.Qf = np.diag([50.0, 6.0, 100.0, 0.1])
        self.Q_lqr = np.diag([1.0, 0.1, 10.0, 0.1])
        self.R_lqr = np.diag([0.001])
        self.phys = dict(m_cart=1.0, m_pole=0.1, length=0.15, gravity=9.81)      # cartpole_dynamics.py:14
        self.u_init = [np.array([0.0]) for _ in range(horizon)]
        if not lqr_only:
            tf_model = None if ilqr_only else (transformer_model if (ilqr_tf_only or ilqr_tf_blend) else None)   # :196-205
            self.ilqr = iLQR_TF(dynamics=self.discrete_dynamics, cost=self.running_cost, cost_final=self.final_cost,
                                x0=self.x_ref, u_init=self.u_init, horizon=self.horizon, tf=tf_model, tol=1e-1,
                                device=device)
        else:
            self.ilqr = None
        sp = switcher_params or {}
        self.switcher = ControllerSwitcher(epsilon_low=sp.get("epsilon_low", 0.5), epsilon_high=sp.get("epsilon_high", 1.5),
                                           epsilon_dd=sp.get("epsilon_dd", 0.01), gamma=sp.get("gamma", 10.0),
                                           use_sigmoid=sp.get("use_sigmoid", False))
        self._lqr_gain = None

    def device_model(self):
        b = lambda a: np.asarray(a, dtype=np.float64).tobytes()
        key = (self.dt, self.integration_method, b(self.x_ref), b(self.Q), b(self.R), b(self.Qf))
        if getattr(self, "_md_key", None) != key:
            self._md = cartpole_model(dt=self.dt, integrator=self.integration_method, x_ref=self.x_ref).with_(
                q=tuple(np.diag(self.Q)), r=tuple(np.diag(self.R)), qf=tuple(np.diag(self.Qf)))
            self._md_key = key
        return self._md

    # ------------------------------------------------------------------ LQR law (cartpole_mpc.py:272-301)
    def linearized_dynamics(self, dt):
        """Euler discretisation of the linearisation about the upright equilibrium (cartpole_dynamics.py:110-142)."""
        M, m, l, g = (self.phys[k] for k in ("m_cart", "m_pole", "length", "gravity"))
        A = np.array([[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, -(m * g) / M, 0.0], [0.0, 0.0, 0.0, 1.0],
                      [0.0, 0.0, ((M + m) * g) / (M * l), 0.0]])
        B = np.array([[0.0], [1.0 / M], [0.0], [-1.0 / (M * l)]])
        return np.eye(4) + dt * A, dt * B

    def compute_linear_lqr_control(self, x_current):
        """u = -K (x - x_ref) with the infinite-horizon discrete LQR gain; the gain is a constant and cached."""
        if self._lqr_gain is None:
            from scipy.linalg import inv, solve_discrete_are
            A_d, B_d = self.linearized_dynamics(self.dt)
            P = solve_discrete_are(A_d, B_d, self.Q_lqr, self.R_lqr)
            self._lqr_gain = inv(self.R_lqr + B_d.T @ P @ B_d) @ (B_d.T @ P @ A_d)
        return (-self._lqr_gain @ (np.asarray(x_current, dtype=np.float64) - self.x_ref)).flatten()

    def _ilqr_step(self, x_current):
        self.ilqr.x0 = x_current
        optimal_u_seq, optimal_x_seq = self.ilqr.optimize(x_ref=self.x_ref)
        self.ilqr.u = optimal_u_seq[1:].copy() + [optimal_u_seq[-1]]   # :331
        return optimal_x_seq, optimal_u_seq[0]

    def control_step(self, x_current):
        """(optimal_x_seq or [], u_final).  The LQR branches apply MINUS compute_linear_lqr_control, exactly as the
        reference does (:322, :342, :355)."""
        if self.lqr_only:
            return [], -self.compute_linear_lqr_control(x_current)
        if self.ilqr_only or self.ilqr_tf_only:
            return self._ilqr_step(x_current)
        # everything else — ilqr_tf_blend, and also a controller built with no flag at all — takes the reference's
        # blending branch (:334-359)
        self.switcher.update_error(np.asarray(x_current, dtype=np.float64) - self.x_ref)
        w = self.switcher.get_blending_weight(self.dt)
        if w <= 0.05:
            return [], -self.compute_linear_lqr_control(x_current)
        x_seq, u_primary = self._ilqr_step(x_current)
        if w >= 0.95:
            return x_seq, u_primary
        return x_seq, w * u_primary + (1 - w) * (-self.compute_linear_lqr_control(x_current))


class BatchedMPC:
    """B receding-horizon controllers advancing together on the device: what the reference does with
    one `control_step` per simulator tick and per process (quadrotor_mpc.py:102-124, cartpole_mpc.py:326-332;
    `multiprocessing.Pool` in training_data_collection.py:298-305), here as batched kernels with no host round trip per
    controller: solve -> apply u_0 -> shift the warm start (u[1:] + [u[-1]])."""

    def __init__(self, model, horizon, max_iter=100, tol=1e-3, tf=None, tf_window=10, device="cuda:0",
                 state_offset=None, check_every=4):
        self.model, self.horizon = model, int(horizon)
        self.solver = QuattroILQR(model, horizon, max_iter=max_iter, tol=tol, tf=tf, tf_window=tf_window,
                                  device=device, state_offset=state_offset, check_every=check_every)
        self.device = self.solver.device
        self.u_warm = None                      # (B, N, m) warm start for the next control step

    def control_step(self, x_current, x_ref=None, model_phys=None, targets=None, weights=None):
        """x_current (B, n) -> (x_seq (B,N+1,n), u_seq (B,N,m), iters (B,)) as fresh device tensors; keeps the shifted
        control sequence as the next warm start.  model_phys: per-controller model parameters, as in QuattroILQR.solve.
        targets: per-controller, per-step state targets of THIS solve, as in QuattroILQR.solve (row min(t, R - 1) at horizon step
        t); x_ref: handed to the solver as it is — the predictor's input in hybrid mode, nothing in pure mode; a target for the
        cost is `targets`.  weights: per-controller cost weights of THIS solve, as in QuattroILQR.solve."""
        if model_phys is not None:
            self.solver._check_model_phys(model_phys, int(np.prod(tuple(np.shape(x_current)))) // self.model.n)
        if targets is not None:
            self.solver._check_targets(targets, int(np.prod(tuple(np.shape(x_current)))) // self.model.n)
        if weights is not None:
            self.solver._check_weights(weights, int(np.prod(tuple(np.shape(x_current)))) // self.model.n)
        x_current = torch.as_tensor(x_current, dtype=torch.float32, device=self.device).reshape(-1, self.model.n)
        B = x_current.shape[0]
        if self.u_warm is not None and self.u_warm.shape[0] != B:
            raise ValueError("batch size changed between control steps")
        out = self.solver.solve(x_current, self.u_warm, x_ref=x_ref, model_phys=model_phys, targets=targets, weights=weights)
        u = out["u"]
        self.u_warm = torch.cat([u[:, 1:], u[:, -1:]], dim=1).contiguous()
        return out["x"].clone(), u.clone(), out["iters"].clone()

    def plant_step(self, x, u0):
        """One step of the (same) device dynamics: x (B,n), u0 (B,m) -> x_next (B,n)."""
        xs, _ = ops.simulate(self.model, x.contiguous(), u0.reshape(-1, 1, self.model.m).contiguous())
        return xs[:, 1].contiguous()

    _SCORE_KEYS = ("targets", "weights", "model_phys", "terminal", "ref_hold")

    def _score_args(self, score, B, targets, preview, replan_every):
        """The keywords of the one ops.score call that `score=` of run() asks for, or None; host logic only.  True: the model's own q, r
        (not the run's `weights=` candidates), no terminal term, no model_phys, against the run's own targets if it had any -- row s
        at plant step s under preview, the row of the last replan step without.  A dict overrides any of these."""
        if score is None or score is False:
            return None
        args = dict(targets=targets, weights=None, model_phys=None, terminal=False, ref_hold=1 if preview else int(replan_every))
        if score is not True:
            if not isinstance(score, dict):
                raise ValueError(f"score must be None, True or a dict with keys from {list(self._SCORE_KEYS)} (got {type(score).__name__})")
            unknown = [key for key in score if key not in self._SCORE_KEYS]
            if unknown:
                raise ValueError(f"score has unknown keys {unknown}: the keys are {list(self._SCORE_KEYS)}")
            args.update(score)
        ops.check_ref_rows(self.model, args["targets"], B, name="score['targets']" if args["targets"] is not targets else "targets")
        ops.check_cost_rows(self.model, args["weights"], B, name="score['weights']")
        ops.check_phys_rows(self.model, args["model_phys"], B, "score['model_phys']")
        h = args["ref_hold"]
        if isinstance(h, bool) or int(h) != h or int(h) < 1:
            raise ValueError(f"score['ref_hold'] must be an integer >= 1 (got {h!r})")
        args["ref_hold"], args["terminal"] = int(h), bool(args["terminal"])
        return args

    def _scored(self, out, args):
        """The dict run() returns, with "score" (B,) float64 and "stage_cost" (B, steps + 1) added where asked for: one ops.score call
        on the returned x, u, whichever path made them."""
        if args is not None:
            out["score"], out["stage_cost"] = ops.score(self.model, out["x"].contiguous(), out["u"].contiguous(), **args)
        return out

    def run(self, x0, steps, disturbance=None, device_loop=True, *, plant=None, plant_phys=None, replan_every=1, feedback=False,
            model_phys=None, targets=None, preview=True, weights=None, score=None):
        """Closed loop for `steps` control steps from x0 (B,n); the plant is the device model itself (the reference's
        plant is MuJoCo, out of scope), plus an optional additive state disturbance tensor (steps, B, n).
        Returns dict(x (B,steps+1,n), u (B,steps,m), iters (B,steps)).

        device_loop (default True: where a persistent kernel is the model's fastest form and there is no predictor; "always":
        wherever one exists, i.e. also for a user-compiled model): ALL `steps` control
        steps of all B controllers are ONE launch (quattro_mpc_run_f32) — no host call, synchronisation or tensor
        operation per control step; a controller that converges early goes on to its next control step at once.
        Results are bit-identical to the host-driven loop below.

        A plant of its own and gain feedback between solves (any of the four keywords off its default; `steps` are then PLANT
        steps and `iters` is (B, steps // replan_every)):
          plant         a DeviceModel like the controller's — same name, n, m, dt and, for a user model, library — whose integrator
                        and phys are the plant's; its cost is ignored
          plant_phys    (B, len(model.phys)): controller b's plant takes row b for its phys (B controllers, B plants)
          replan_every  h: a solve every h plant steps; between solves u = u_nom[j] + (feedback ? K[j] (x - x_nom[j]) : 0) on the
                        nominal and gains of the last solve (ops.track), and the warm start shifts by h
          feedback      the gain term above on or off (open-loop hold against feedback hold); it is exactly zero for h = 1
        The same one launch (quattro_mpc_run_plant_f32) where the plain loop has one; the host-driven form — solve, ops.track,
        shift — otherwise, and always with a predictor.  ValueError, before anything touches the device: a plant that is not the
        controller's problem, a plant_phys of the wrong shape, steps % replan_every != 0.

        model_phys (B, len(model.phys)), or the (B, 8) float32 device tensor of ops.model_phys_tensor: controller b PLANS with row
        b in place of model.phys (B controllers that each know their own vehicle, or each hold a different belief about one
        plant).  Its plant is plant_phys[b] if given, else plant.phys if a plant is given, else the same row — the default plant
        is the controller's own model; the other plant keywords work as above.  One launch (quattro_mpc_run_phys_f32), always
        the model's persistent kernel (a user model's too, as with device_loop="always"); NotImplementedError with a predictor,
        device_loop=False or a model without such a kernel, ValueError for a wrong shape, before anything touches the device.

        targets (B, R, n), or (B, n) for R = 1: per-controller, per-step state targets that may MOVE during the run.  Plan c starts
        at plant step s = c * replan_every; horizon step t of its solve (t = N: the terminal cost) takes its cost against row
        min(s + t, R - 1) of controller b's rows with preview=True — tracking along a sliding window of the path: the horizon sees
        where the reference will be; R >= steps + N + 1 covers the run — and against row min(s, R - 1) for every t with
        preview=False: a set-point schedule, known at replan time only and constant inside a solve, as the reference's
        simulator moves mpc_controller.x_ref between control steps.  Past its last row a controller holds that row.  The tracked
        steps between solves follow the plan as above; they have no cost and read no rows.  One launch (quattro_mpc_run_ref_f32);
        the kernel rule, refusals and their order are model_phys's, with which — and with the plant keywords — it combines.

        weights: per-controller cost weights, constant over the run — a dict with any of "q", "qf", "r" (each (B, n) / (B, n) /
        (B, m), or one vector for the whole batch; a missing key keeps the model's), a plain (B, 2n + m) array [q | qf | r], or the
        device tensor of ops.cost_rows_tensor.  Controller b PLANS with row b in place of model.q, qf and r in every solve of the
        run: B candidate weightings of one controller against one plant, or a fleet with different priorities.  The tracked steps
        have no cost.  To compare candidates, score the run under ONE evaluation cost: `score=` below.  One launch
        (quattro_mpc_run_cost_f32); the kernel rule, refusals and their order are model_phys's, with which — and with targets and
        the plant keywords — it combines.  Cart-pole and user-compiled models; the built-in quadrotor's kernel has no such form yet
        (NotImplementedError, like a model without a persistent kernel).

        score (default None: the dict above, nothing else launched): True adds "stage_cost" (B, steps + 1) float32 -- the cost of every
        plant step, slot `steps` zero -- and "score" (B,) float64, their sum in step order, from one ops.score call on the returned x, u
        on every path of run.  They are taken under ONE evaluation cost: the model's own q and r, NOT the candidates of `weights=`, no
        terminal term, no model_phys, against the run's own `targets` if it had any, as the run followed them (row s at plant step s
        with preview=True; the row of the last replan step with preview=False).  A dict with any of targets, weights, model_phys,
        terminal, ref_hold (ops.score's keywords) overrides these: a fleet scored under each controller's own weights, a run scored
        against another path.  Every model, the quadrotor's weights included.  ValueError for anything else, a wrong shape or
        ref_hold < 1, before anything touches the device."""
        h = int(replan_every)
        if model_phys is not None:
            if not device_loop:
                raise NotImplementedError("model_phys runs only in the device-resident loop: device_loop=False is the host-driven loop")
            self.solver._check_model_phys(model_phys, int(np.prod(tuple(np.shape(x0)))) // self.model.n)
        if targets is not None:
            if not device_loop:
                raise NotImplementedError("targets runs only in the device-resident loop: device_loop=False is the host-driven loop")
            self.solver._check_targets(targets, int(np.prod(tuple(np.shape(x0)))) // self.model.n)
        if weights is not None:
            if not device_loop:
                raise NotImplementedError("weights runs only in the device-resident loop: device_loop=False is the host-driven loop")
            self.solver._check_weights(weights, int(np.prod(tuple(np.shape(x0)))) // self.model.n)
        plain = (plant is None and plant_phys is None and h == 1 and not feedback and model_phys is None and targets is None
                 and weights is None)
        if not plain:
            ops.check_plant(self.model, plant)
            if h < 1 or h > self.horizon or steps % h != 0:
                raise ValueError(f"steps ({steps}) must be a multiple of replan_every ({replan_every}) in 1..horizon")
            if plant_phys is not None:
                B0 = int(np.prod(tuple(np.shape(x0)))) // self.model.n
                if tuple(plant_phys.shape) != (B0, len(self.model.phys)):
                    raise ValueError(f"plant_phys must have shape {(B0, len(self.model.phys))} (got {tuple(plant_phys.shape)})")
            if feedback and self.solver.max_iter < 1:
                raise ValueError("feedback needs gains: max_iter >= 1")
        sc = self._score_args(score, int(np.prod(tuple(np.shape(x0)))) // self.model.n, targets, preview, replan_every)
        x = torch.as_tensor(x0, dtype=torch.float32, device=self.device).reshape(-1, self.model.n).contiguous()
        sv = self.solver
        rows = model_phys is not None or targets is not None or weights is not None
        use_kernel = (ops.model_can_device_loop(self.model) if device_loop == "always" or rows
                      else bool(device_loop) and ops.model_has_device_loop(self.model))
        if not plain:
            plant_phys = ops.plant_phys_tensor(self.model, plant_phys, x.shape[0], self.device)
        if use_kernel and sv.tf is None:
            B, N, n, m = x.shape[0], self.horizon, self.model.n, self.model.m
            if self.u_warm is not None and self.u_warm.shape[0] != B:
                raise ValueError("batch size changed between control steps")
            sv._alloc(B)
            if self.u_warm is None:
                sv.u.zero_()
            else:
                sv.u.copy_(self.u_warm)
            if sv._ws is None:
                sv._ws = ops.workspace(self.model, B, N, self.device)
            x_cur = x.clone()
            traj_x = torch.empty((B, steps + 1, n), dtype=torch.float32, device=self.device)
            traj_u = torch.empty((B, steps, m), dtype=torch.float32, device=self.device)
            traj_it = torch.empty((B, steps // h), dtype=torch.int32, device=self.device)
            dist_t = None
            if disturbance is not None:
                dist_t = torch.as_tensor(disturbance, dtype=torch.float32, device=self.device).reshape(steps, B, n).contiguous()
            extra = {} if plain else dict(plant=plant, plant_phys=plant_phys, hold=h, feedback=feedback,
                                          model_phys=ops.model_phys_tensor(self.model, model_phys, B, self.device),
                                          x_ref_rows=ops.x_ref_rows_tensor(self.model, targets, B, self.device),
                                          preview=bool(preview),
                                          cost_rows=ops.cost_rows_tensor(self.model, weights, B, self.device))
            ops.mpc_run(self.model, x_cur, sv.x, sv.u, sv.K, sv.k, sv.cost, sv.tol, sv.max_iter, steps, sv._ws, traj_x,
                        traj_u, traj_it, disturbance=dist_t, alphas=sv.alphas, reg=sv.reg, alpha_idx=sv.alpha_idx,
                        active=sv.active, iters=sv.iters, status=sv.status, **extra)
            self.u_warm = sv.u.clone()
            return self._scored(dict(x=traj_x, u=traj_u, iters=traj_it), sc)
        if not plain:
            B, n = x.shape[0], self.model.n
            if self.u_warm is not None and self.u_warm.shape[0] != B:
                raise ValueError("batch size changed between control steps")
            dist_t = None
            if disturbance is not None:
                dist_t = torch.as_tensor(disturbance, dtype=torch.float32, device=self.device).reshape(steps, B, n).contiguous()
            xs, us, its = [x[:, None]], [], []
            for c in range(steps // h):
                out = sv.solve(x, self.u_warm)
                xt, ut = ops.track(self.model, x, out["x"], out["u"], out["K"], h, plant=plant, plant_phys=plant_phys,
                                   feedback=feedback, disturbance=None if dist_t is None else dist_t[c * h:(c + 1) * h])
                u = out["u"]
                self.u_warm = torch.cat([u[:, h:]] + [u[:, -1:]] * h, dim=1).contiguous()
                x = xt[:, -1].contiguous()
                xs.append(xt[:, 1:]); us.append(ut); its.append(out["iters"].clone())
            return self._scored(dict(x=torch.cat(xs, dim=1), u=torch.cat(us, dim=1), iters=torch.stack(its, dim=1)), sc)
        xs, us, its = [x], [], []
        for s in range(steps):
            _, u_seq, iters = self.control_step(x)
            x = self.plant_step(x, u_seq[:, 0])
            if disturbance is not None:
                x = (x + disturbance[s]).contiguous()
            xs.append(x); us.append(u_seq[:, 0]); its.append(iters)
        return self._scored(dict(x=torch.stack(xs, dim=1), u=torch.stack(us, dim=1), iters=torch.stack(its, dim=1)), sc)
