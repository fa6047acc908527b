"""Tensor-level operators over the C ABI.  torch is plumbing here: it owns device memory and the stream; every
computation is a kernel of libquattro_hip.so.  All tensors must be contiguous CUDA(=HIP) tensors on one device.

Shape checks happen here, on the host, before anything is launched: a hand-written kernel that is handed a
buffer smaller than its grid assumes faults the GPU.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check

ALPHAS = (1.0, 0.5, 0.25, 0.1, 0.05, 0.01)      # reference line search, quattro_ilqr_tf.py:440,552
QUU_REG = 1e-6                                    # quattro_ilqr_tf.py:304


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _req(t, shape, dtype, name):
    if t is None:
        raise ValueError(f"{name} is required")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (got {t.device})")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype} (got {t.dtype})")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)} (got {tuple(t.shape)})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _alphas(alphas):
    if not 0 < len(alphas) <= _lib.MAX_ALPHAS:
        raise ValueError(f"1..{_lib.MAX_ALPHAS} line-search step sizes supported")
    return (ctypes.c_float * len(alphas))(*alphas), len(alphas)


def record_stride(n, m, layout, lib=None):
    s = (lib or _lib.load()).quattro_record_stride(n, m, layout)
    if s == 0:
        raise NotImplementedError(f"no record layout {layout} for (n, m) = ({n}, {m})")
    return s


def record_header(n, m, layout, lib=None):
    return (lib or _lib.load()).quattro_record_header(n, m, layout)


def preferred_layout(n, m, lib=None):
    return (lib or _lib.load()).quattro_preferred_layout(n, m)


def model_layout(model):
    """The layout linearize + sweep are fastest with for this model (TILE16C for the Euler quadrotor: constants of the
    problem live once in a header record, 304 B per step through HBM instead of 1,664 B)."""
    p = model.c_params()
    lay = _lib.load_for(model).quattro_model_layout(ctypes.byref(p))
    if lay < 0:
        raise NotImplementedError(f"no device kernels for model {model.name}")
    return lay


def alloc_records(n, m, layout, B, S, device, lib=None):
    """Record buffer for B x S steps: (B, S, stride) for the plain layouts, a flat header + B*S*stride buffer for TILE16C.
    `lib` (here and below): the library of a user model (its (n, m) exist only there); None = libquattro_hip.so."""
    stride, header = record_stride(n, m, layout, lib), record_header(n, m, layout, lib)
    if header == 0:
        return torch.empty((B, S, stride), dtype=torch.float32, device=device)
    return torch.empty((header + B * S * stride,), dtype=torch.float32, device=device)


def _check_records(rec, n, m, layout, B, S=None, lib=None):
    """-> S.  Shape / size check of a record buffer against (B, S) for either kind of layout."""
    stride, header = record_stride(n, m, layout, lib), record_header(n, m, layout, lib)
    if rec.dtype != torch.float32 or not rec.is_contiguous() or rec.device.type != "cuda":
        raise ValueError("rec must be a contiguous float32 tensor on the GPU")
    body = rec.numel() - header
    if S is None:
        S = body // (B * stride) if B > 0 else 0
    if S <= 0 or body != B * S * stride:
        raise ValueError(f"rec holds {rec.numel()} floats, expected {header} + {B} x {S} x {stride}")
    return S


def pack_derivs(A, Bm, lx, lu, lxx, luu, lux, layout=None, lib=None):
    """Separate row-major blocks (B, S, ...) -> records (B, S, stride)."""
    Bt, S, n, _ = A.shape
    m = Bm.shape[3]
    layout = preferred_layout(n, m, lib) if layout is None else layout
    stride = record_stride(n, m, layout, lib)
    f32 = torch.float32
    _req(A, (Bt, S, n, n), f32, "A"); _req(Bm, (Bt, S, n, m), f32, "B"); _req(lx, (Bt, S, n), f32, "lx")
    _req(lu, (Bt, S, m), f32, "lu"); _req(lxx, (Bt, S, n, n), f32, "lxx"); _req(luu, (Bt, S, m, m), f32, "luu")
    _req(lux, (Bt, S, m, n), f32, "lux")
    rec = torch.zeros((Bt, S, stride), dtype=f32, device=A.device)
    check((lib or _lib.load()).quattro_pack_derivs_f32(_ptr(A), _ptr(Bm), _ptr(lx), _ptr(lu), _ptr(lxx), _ptr(luu), _ptr(lux),
                                              Bt, S, n, m, layout, _ptr(rec), _stream()), "quattro_pack_derivs_f32")
    return rec, layout


def unpack_derivs(rec, B, n, m, layout, lib=None):
    """Records (any layout) -> dict of row-major blocks A (B,S,n,n), B (B,S,n,m), lx, lu, lxx, luu, lux — the arrays the
    reference's _compute_dynamics_jacobians / _compute_cost_derivatives return, for every (b, t) of the buffer."""
    S = _check_records(rec, n, m, layout, B, lib=lib)
    f32, dev = torch.float32, rec.device
    out = dict(A=torch.empty((B, S, n, n), dtype=f32, device=dev), B=torch.empty((B, S, n, m), dtype=f32, device=dev),
               lx=torch.empty((B, S, n), dtype=f32, device=dev), lu=torch.empty((B, S, m), dtype=f32, device=dev),
               lxx=torch.empty((B, S, n, n), dtype=f32, device=dev), luu=torch.empty((B, S, m, m), dtype=f32, device=dev),
               lux=torch.empty((B, S, m, n), dtype=f32, device=dev))
    check((lib or _lib.load()).quattro_unpack_derivs_f32(_ptr(rec), B, S, n, m, layout, _ptr(out["A"]), _ptr(out["B"]),
                                                _ptr(out["lx"]), _ptr(out["lu"]), _ptr(out["lxx"]), _ptr(out["luu"]),
                                                _ptr(out["lux"]), _stream()), "quattro_unpack_derivs_f32")
    return out


def riccati_sweep(rec, VxN, VxxN, n, m, layout, reg=QUU_REG, K=None, k=None, status=None, active=None, repair=False,
                  lib=None):
    """Backward sweep over the S steps held in `rec`.  Returns K (B,S,m,n), k (B,S,m), status (B,).

    repair=True (one host synchronisation): trajectories the quadrotor-shaped kernel flags TRAJ_ILLCOND — an indefinite or
    badly scaled Q_uu + reg I, which it eliminates without pivoting — are swept again by the generic kernel, which pivots
    like the reference's np.linalg.inv (quattro_ilqr_tf.py:306); their bit is cleared when the second sweep is clean."""
    Bt = VxN.shape[0]
    f32 = torch.float32
    S = _check_records(rec, n, m, layout, Bt, lib=lib)
    _req(VxN, (Bt, n), f32, "VxN"); _req(VxxN, (Bt, n, n), f32, "VxxN")
    K = torch.empty((Bt, S, m, n), dtype=f32, device=rec.device) if K is None else _req(K, (Bt, S, m, n), f32, "K")
    k = torch.empty((Bt, S, m), dtype=f32, device=rec.device) if k is None else _req(k, (Bt, S, m), f32, "k")
    status = (torch.zeros((Bt,), dtype=torch.int32, device=rec.device) if status is None
              else _req(status, (Bt,), torch.int32, "status"))
    if active is not None:
        _req(active, (Bt,), torch.int32, "active")
    # N and t_start only enter the kernel as S = N - t_start
    check((lib or _lib.load()).quattro_riccati_sweep_f32(_ptr(rec), _ptr(VxN), _ptr(VxxN), Bt, S, 0, n, m, layout, reg,
                                                _ptr(K), _ptr(k), _ptr(status), _ptr(active), _stream()),
          "quattro_riccati_sweep_f32")
    if repair and layout == _lib.LAYOUT_ROWMAJOR_TILE:   # the same records through the pivoting kernel: no repacking
        flagged = torch.nonzero((status & _lib.TRAJ_ILLCOND) != 0).reshape(-1)
        if flagged.numel() > 0:
            stride = record_stride(n, m, layout, lib)
            rec2 = rec.reshape(Bt, S, stride).index_select(0, flagged).contiguous()
            K2, k2, st2 = riccati_sweep(rec2, VxN.index_select(0, flagged).contiguous(),
                                        VxxN.index_select(0, flagged).contiguous(), n, m, _lib.LAYOUT_ROWMAJOR, reg, lib=lib)
            K.index_copy_(0, flagged, K2)
            k.index_copy_(0, flagged, k2)
            status.index_copy_(0, flagged, st2)
    if repair and layout == _lib.LAYOUT_TILE16:          # (TILE16C / TILE16R come from the built-in convex cost: never flagged)
        flagged = torch.nonzero((status & _lib.TRAJ_ILLCOND) != 0).reshape(-1)
        if flagged.numel() > 0:
            blocks = unpack_derivs(rec, Bt, n, m, layout)
            sel = {name: t.index_select(0, flagged).contiguous() for name, t in blocks.items()}
            rec2, lay2 = pack_derivs(sel["A"], sel["B"], sel["lx"], sel["lu"], sel["lxx"], sel["luu"], sel["lux"],
                                     layout=_lib.LAYOUT_ROWMAJOR)
            K2, k2, st2 = riccati_sweep(rec2, VxN.index_select(0, flagged).contiguous(),
                                        VxxN.index_select(0, flagged).contiguous(), n, m, lay2, reg)
            K.index_copy_(0, flagged, K2)
            k.index_copy_(0, flagged, k2)
            status.index_copy_(0, flagged, st2)
    return K, k, status


def linearize(model, x, u, t_start=0, layout=None, rec=None, VxN=None, VxxN=None):
    """Records for t in [t_start, N) and the terminal pair, about the nominal (x, u)."""
    Bt, N, m = u.shape
    n = x.shape[2]
    if (n, m) != (model.n, model.m):
        raise ValueError(f"trajectory dims ({n}, {m}) do not match model {model.name} ({model.n}, {model.m})")
    if not 0 <= t_start < N:
        raise ValueError("t_start must be in [0, N)")
    layout = model_layout(model) if layout is None else layout
    f32 = torch.float32
    _req(x, (Bt, N + 1, n), f32, "x"); _req(u, (Bt, N, m), f32, "u")
    S = N - t_start
    lib = _lib.load_for(model)
    if rec is None:
        rec = alloc_records(n, m, layout, Bt, S, x.device, lib)
    else:
        _check_records(rec, n, m, layout, Bt, S, lib)
    VxN = torch.empty((Bt, n), dtype=f32, device=x.device) if VxN is None else _req(VxN, (Bt, n), f32, "VxN")
    VxxN = torch.empty((Bt, n, n), dtype=f32, device=x.device) if VxxN is None else _req(VxxN, (Bt, n, n), f32, "VxxN")
    p = model.c_params()
    check(lib.quattro_linearize_f32(ctypes.byref(p), _ptr(x), _ptr(u), Bt, N, t_start, layout, _ptr(rec),
                                            _ptr(VxN), _ptr(VxxN), None, _stream()), "quattro_linearize_f32")
    return rec, VxN, VxxN, layout


def model_fuses_sweep(model):
    """True where linearize_sweep() — the sweep kernel linearising its own trajectory — is the model's fastest backward pass."""
    p = model.c_params()
    return _lib.load_for(model).quattro_model_fuses_sweep(ctypes.byref(p)) == 1


def model_can_fuse_sweep(model):
    """True where linearize_sweep() works at all (also the RK4 quadrotor, whose record path is faster as separate launches)."""
    p = model.c_params()
    return _lib.load_for(model).quattro_model_fuses_sweep(ctypes.byref(p)) > 0


def linearize_sweep_scratch_bytes(model, B, N, t_start=0):
    """Device scratch linearize_sweep needs for this model (0 except for the RK4 quadrotor: 528 B per step)."""
    p = model.c_params()
    return int(_lib.load_for(model).quattro_linearize_sweep_scratch_bytes(ctypes.byref(p), B, N, t_start))


def linearize_sweep(model, x, u, t_start=0, reg=QUU_REG, K=None, k=None, status=None, active=None, scratch=None,
                    in_place=False):
    """Linearisation + backward sweep in one launch, no record buffer (Euler quadrotor: bit-identical to linearize +
    riccati_sweep).  Returns K (B,S,m,n), k (B,S,m), status (B,) for the S = N - t_start steps from t_start.
    in_place=True: K (B,N,m,n) and k (B,N,m) are the FULL gain stacks and the swept steps are written at rows t_start .. N-1
    (quattro_linearize_sweep_rows_f32): what a hybrid iteration wants — the predictor fills the rows below.
    `scratch`: uint8 device buffer of >= linearize_sweep_scratch_bytes(...) where that is not 0 (allocated here if None)."""
    Bt, N, m = u.shape
    n = x.shape[2]
    if (n, m) != (model.n, model.m):
        raise ValueError(f"trajectory dims ({n}, {m}) do not match model {model.name} ({model.n}, {model.m})")
    if not 0 <= t_start < N:
        raise ValueError("t_start must be in [0, N)")
    f32 = torch.float32
    _req(x, (Bt, N + 1, n), f32, "x"); _req(u, (Bt, N, m), f32, "u")
    S = N if in_place else N - t_start
    if in_place and (K is None or k is None):
        raise ValueError("in_place needs the full gain stacks K (B,N,m,n) and k (B,N,m)")
    K = torch.empty((Bt, S, m, n), dtype=f32, device=x.device) if K is None else _req(K, (Bt, S, m, n), f32, "K")
    k = torch.empty((Bt, S, m), dtype=f32, device=x.device) if k is None else _req(k, (Bt, S, m), f32, "k")
    status = (torch.zeros((Bt,), dtype=torch.int32, device=x.device) if status is None
              else _req(status, (Bt,), torch.int32, "status"))
    if active is not None:
        _req(active, (Bt,), torch.int32, "active")
    p = model.c_params()
    need = linearize_sweep_scratch_bytes(model, Bt, N, t_start)
    if need and scratch is None:
        scratch = torch.empty((need,), dtype=torch.uint8, device=x.device)
    nbytes = 0 if scratch is None else scratch.numel() * scratch.element_size()
    check(_lib.load_for(model).quattro_linearize_sweep_rows_f32(ctypes.byref(p), _ptr(x), _ptr(u), Bt, N, t_start, reg, _ptr(K),
                                                                _ptr(k), N if in_place else 0, _ptr(status), _ptr(active),
                                                                _ptr(scratch), nbytes, _stream()),
          "quattro_linearize_sweep_rows_f32")
    return K, k, status


def simulate(model, x0, u, x=None, cost=None):
    """Open-loop rollout from x0 (B,n) under u (B,N,m): x (B,N+1,n), cost (B,) fp64."""
    Bt, N, m = u.shape
    n = model.n
    f32 = torch.float32
    _req(x0, (Bt, n), f32, "x0"); _req(u, (Bt, N, model.m), f32, "u")
    x = torch.empty((Bt, N + 1, n), dtype=f32, device=u.device) if x is None else _req(x, (Bt, N + 1, n), f32, "x")
    cost = torch.empty((Bt,), dtype=torch.float64, device=u.device) if cost is None else _req(cost, (Bt,), torch.float64, "cost")
    p = model.c_params()
    check(_lib.load_for(model).quattro_simulate_f32(ctypes.byref(p), _ptr(x0), _ptr(u), Bt, N, _ptr(x), _ptr(cost), _stream()),
          "quattro_simulate_f32")
    return x, cost


def total_cost(model, x, u):
    """sum_t L(x_t,u_t) + Lf(x_N) for given sequences: cost (B,) fp64."""
    Bt, N, m = u.shape
    f32 = torch.float32
    _req(x, (Bt, N + 1, model.n), f32, "x"); _req(u, (Bt, N, model.m), f32, "u")
    cost = torch.empty((Bt,), dtype=torch.float64, device=u.device)
    p = model.c_params()
    check(_lib.load_for(model).quattro_total_cost_f32(ctypes.byref(p), _ptr(x), _ptr(u), Bt, N, _ptr(cost), _stream()),
          "quattro_total_cost_f32")
    return cost


def rollout(model, x_nom, u_nom, K, k, alphas=ALPHAS, want_traj=False, active=None):
    """Closed-loop forward passes for every alpha: cost (n_alpha, B) fp64 [, x_new (n_alpha,B,N+1,n), u_new]."""
    Bt, N, m = u_nom.shape
    n = model.n
    f32 = torch.float32
    _req(x_nom, (Bt, N + 1, n), f32, "x_nom"); _req(u_nom, (Bt, N, model.m), f32, "u_nom")
    _req(K, (Bt, N, m, n), f32, "K"); _req(k, (Bt, N, m), f32, "k")
    arr, na = _alphas(alphas)
    cost = torch.empty((na, Bt), dtype=torch.float64, device=u_nom.device)
    x_new = torch.empty((na, Bt, N + 1, n), dtype=f32, device=u_nom.device) if want_traj else None
    u_new = torch.empty((na, Bt, N, m), dtype=f32, device=u_nom.device) if want_traj else None
    if active is not None:
        _req(active, (Bt,), torch.int32, "active")
    p = model.c_params()
    check(_lib.load_for(model).quattro_rollout_f32(ctypes.byref(p), _ptr(x_nom), _ptr(u_nom), _ptr(K), _ptr(k), arr, na, Bt, N,
                                          _ptr(x_new), _ptr(u_new), _ptr(cost), _ptr(active), _stream()),
          "quattro_rollout_f32")
    return (cost, x_new, u_new) if want_traj else cost


def linesearch_scratch_bytes(model, B, N):
    return int(_lib.load_for(model).quattro_linesearch_scratch_bytes(model.n, model.m, B, N))


def linesearch_scratch(model, B, N, device):
    """Fresh device scratch for one fused line search (candidate trajectories).  Not cached: torch's caching allocator
    makes the allocation cheap and stream-ordered, and a module-level cache could free a buffer whose address a
    captured graph (or a launch in flight on another stream) still holds.  Long-lived callers (QuattroILQR) own
    their scratch and pass it as `scratch=`."""
    return torch.empty((linesearch_scratch_bytes(model, B, N),), dtype=torch.uint8, device=device)


def linesearch(model, x_nom, u_nom, K, k, cost, tol, alphas=ALPHAS, alpha_idx=None, active=None, iters=None,
               scratch=None):
    """Fused line search; commits the first accepted alpha into x_nom/u_nom/cost IN PLACE.  Returns alpha_idx (B,)."""
    Bt, N, m = u_nom.shape
    n = model.n
    f32 = torch.float32
    _req(x_nom, (Bt, N + 1, n), f32, "x_nom"); _req(u_nom, (Bt, N, model.m), f32, "u_nom")
    _req(K, (Bt, N, m, n), f32, "K"); _req(k, (Bt, N, m), f32, "k"); _req(cost, (Bt,), torch.float64, "cost")
    arr, na = _alphas(alphas)
    alpha_idx = (torch.empty((Bt,), dtype=torch.int32, device=u_nom.device) if alpha_idx is None
                 else _req(alpha_idx, (Bt,), torch.int32, "alpha_idx"))
    if active is not None:
        _req(active, (Bt,), torch.int32, "active")
    if iters is not None:
        _req(iters, (Bt,), torch.int32, "iters")
    if scratch is None:
        scratch = linesearch_scratch(model, Bt, N, u_nom.device)
    p = model.c_params()
    check(_lib.load_for(model).quattro_linesearch_f32(ctypes.byref(p), _ptr(x_nom), _ptr(u_nom), _ptr(K), _ptr(k), arr, na, Bt,
                                             N, float(tol), _ptr(cost), _ptr(alpha_idx), _ptr(active), _ptr(iters),
                                             _ptr(scratch), scratch.numel() * scratch.element_size(), _stream()),
          "quattro_linesearch_f32")
    return alpha_idx


def workspace(model, B, N, device):
    """Device workspace of the fused iteration (records, V_x(N), V_xx(N), candidate trajectories); uint8, 256-aligned
    (torch's caching allocator hands out 512-byte aligned blocks)."""
    p = model.c_params()
    nbytes = _lib.load_for(model).quattro_model_workspace_bytes(ctypes.byref(p), B, N)
    if nbytes == 0:
        raise NotImplementedError(f"no device kernel for n={model.n}, m={model.m}")
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def ilqr_iterate(model, x_nom, u_nom, K, k, cost, tol, workspace, alphas=ALPHAS, reg=QUU_REG, alpha_idx=None,
                 active=None, iters=None, status=None):
    """One whole pure-iLQR iteration (linearize + sweep + line search/commit) from ONE C call; everything in place."""
    Bt, N, m = u_nom.shape
    n = model.n
    f32, i32 = torch.float32, torch.int32
    _req(x_nom, (Bt, N + 1, n), f32, "x_nom"); _req(u_nom, (Bt, N, model.m), f32, "u_nom")
    _req(K, (Bt, N, m, n), f32, "K"); _req(k, (Bt, N, m), f32, "k"); _req(cost, (Bt,), torch.float64, "cost")
    _req(alpha_idx, (Bt,), i32, "alpha_idx"); _req(active, (Bt,), i32, "active")
    if iters is not None:
        _req(iters, (Bt,), i32, "iters")
    if status is not None:
        _req(status, (Bt,), i32, "status")
    arr, na = _alphas(alphas)
    p = model.c_params()
    check(_lib.load_for(model).quattro_ilqr_iterate_f32(ctypes.byref(p), _ptr(x_nom), _ptr(u_nom), Bt, N, float(reg), arr, na,
                                               float(tol), _ptr(K), _ptr(k), _ptr(cost), _ptr(alpha_idx), _ptr(active),
                                               _ptr(iters), _ptr(status), _ptr(workspace),
                                               workspace.numel() * workspace.element_size(), _stream()),
          "quattro_ilqr_iterate_f32")
    return alpha_idx


def model_has_device_loop(model):
    """True where the whole solve (and the MPC loop around it) as ONE persistent launch is the model's fastest form
    (csrc/solve_quad.hip, csrc/solve_cartpole.hip)."""
    p = model.c_params()
    return _lib.load_for(model).quattro_model_has_device_loop(ctypes.byref(p)) == 1


def model_can_device_loop(model):
    """True where a persistent kernel exists at all — also a user-compiled model's (csrc/solve_user.hip: one wave per
    trajectory through the generic device bodies; no host involvement, but slower than enqueued iterations)."""
    p = model.c_params()
    return _lib.load_for(model).quattro_model_has_device_loop(ctypes.byref(p)) > 0


class SolveLog:
    """Device-side per-iteration log ring of a solve (include/quattro_hip.h: quattro_solve_log) and its decoding.

    One record per (trajectory, iteration): a 64-byte header (four s_memrealtime stamps, cost before / after, accepted step,
    iteration number) followed by x_seq, u_seq (traj=True) and K, k (gains=True) — the contents of the reference's log dict
    (quattro_ilqr_tf.py:453-466) and the samples of its *_time lists (:16-42).  Iteration i of trajectory b is record
    b * capacity + (i % capacity); `rows(b, count)` downloads and decodes the first `count` of them."""

    TICK = 1e-8            # s_memrealtime counts at 100 MHz

    def __init__(self, model, N, B, capacity, device, traj=True, gains=True):
        self.lib = _lib.load_for(model)
        self.n, self.m, self.N, self.B, self.capacity = model.n, model.m, int(N), int(B), int(capacity)
        self.flags = (_lib.LOG_TRAJ if traj else 0) | (_lib.LOG_GAINS if gains else 0)
        self.rec_bytes = int(self.lib.quattro_solve_log_record_bytes(self.n, self.m, self.N, self.flags))
        off = lambda f: int(self.lib.quattro_solve_log_offset(self.n, self.m, self.N, self.flags, f))
        self.off = dict(x=off(_lib.LOG_FIELD_X), u=off(_lib.LOG_FIELD_U), K=off(_lib.LOG_FIELD_K), k=off(_lib.LOG_FIELD_KFF))
        if self.rec_bytes < _lib.LOG_HEADER_BYTES or self.capacity <= 0:
            raise ValueError("bad log geometry")
        self.buf = torch.zeros((self.B * self.capacity * self.rec_bytes,), dtype=torch.uint8, device=device)
        self.c = _lib.SolveLogC(self.buf.data_ptr(), self.capacity, self.flags)
        self._pin = None

    def byref(self):
        return ctypes.byref(self.c)

    def decode(self, raw, count):
        """raw: uint8 array of `count` consecutive records -> dict of arrays (first axis = record)."""
        rec = np.asarray(raw, dtype=np.uint8).reshape(count, self.rec_bytes)
        n, m, N = self.n, self.m, self.N
        take = lambda a, b, dt: np.ascontiguousarray(rec[:, a:b]).view(dt)
        out = dict(stamps=take(0, 32, np.uint64), cost=take(32, 48, np.float64), alpha_idx=take(48, 52, np.int32)[:, 0],
                   iteration=take(52, 56, np.int32)[:, 0])
        if self.flags & _lib.LOG_TRAJ:
            out["x"] = take(self.off["x"], self.off["x"] + 4 * (N + 1) * n, np.float32).reshape(count, N + 1, n)
            out["u"] = take(self.off["u"], self.off["u"] + 4 * N * m, np.float32).reshape(count, N, m)
        if self.flags & _lib.LOG_GAINS:
            out["K"] = take(self.off["K"], self.off["K"] + 4 * N * m * n, np.float32).reshape(count, N, m, n)
            out["k"] = take(self.off["k"], self.off["k"] + 4 * N * m, np.float32).reshape(count, N, m)
        return out

    def stage(self, b, count):
        """Enqueue the download of the first `count` records of trajectory b into a pinned buffer (no synchronisation)."""
        count = min(int(count), self.capacity)
        if self._pin is None or self._pin.shape[0] < count * self.rec_bytes:
            self._pin = torch.empty((max(count, 4) * self.rec_bytes,), dtype=torch.uint8).pin_memory()
        a = b * self.capacity * self.rec_bytes
        self._pin[:count * self.rec_bytes].copy_(self.buf[a:a + count * self.rec_bytes], non_blocking=True)
        self._staged = (b, count)

    def staged(self, count):
        """Decode `count` records of the last stage() (the stream must have been synchronised since)."""
        b, have = self._staged
        if count > have:
            raise ValueError("more records asked for than were staged")
        return self.decode(self._pin.numpy()[:count * self.rec_bytes], count)

    def rows(self, b, count):
        """Download and decode the first `count` (<= capacity) records of trajectory b (synchronises the stream)."""
        count = min(int(count), self.capacity)
        if count <= 0:
            return self.decode(np.zeros((0,), dtype=np.uint8), 0)
        a = b * self.capacity * self.rec_bytes
        return self.decode(self.buf[a:a + count * self.rec_bytes].cpu().numpy(), count)


def solve_log_record(model, log, phase, x_nom, u_nom, K, k, cost, alpha_idx, active, iters, force=False):
    """One phase of the log of a loop the caller enqueues kernel by kernel (quattro_solve_log_record_f32)."""
    Bt, N, m = u_nom.shape
    check(_lib.load_for(model).quattro_solve_log_record_f32(log.byref(), int(phase), _ptr(x_nom), _ptr(u_nom), _ptr(K), _ptr(k),
                                                            _ptr(cost), _ptr(alpha_idx), _ptr(active), _ptr(iters), Bt, N,
                                                            model.n, m, int(bool(force)), _stream()),
          "quattro_solve_log_record_f32")


def ilqr_solve(model, x_nom, u_nom, K, k, cost, tol, max_iter, workspace, alphas=ALPHAS, reg=QUU_REG, x0=None,
               alpha_idx=None, active=None, iters=None, status=None, fixed_iters=False, reset=False, log=None,
               persistent=False, enqueue=False, model_phys=None, x_ref_rows=None, cost_rows=None):
    """The whole solve from ONE C call with no host involvement: up to max_iter iterations, every trajectory stopping on
    its own test; x0 given = roll the nominal out from it first.  Everything in place (quattro_ilqr_solve_phys_f32).
    reset: the call sets active / iters / alpha_idx / status itself; log: a SolveLog ring filled by the device;
    persistent: take a persistent kernel that exists but is not the model's fastest form (a user model's); enqueue: never
    the persistent kernel.
    model_phys (B, len(model.phys)), or the (B, 8) float32 device tensor of model_phys_tensor: trajectory b is solved with row b
    for the model's phys (always the model's persistent kernel; NotImplementedError where there is none, ValueError together
    with enqueue).  None: the solve with model.phys for every trajectory.
    x_ref_rows (B, R, n) or (B, n), or the device tensor of x_ref_rows_tensor: the cost of trajectory b at horizon step t (t = N: the
    terminal cost) is taken against row min(t, R - 1) of its rows in place of model.x_ref (quattro_ilqr_solve_ref_f32; the same
    kernel rule and refusals as model_phys).  None: model.x_ref for every trajectory and step.
    cost_rows: per-trajectory cost weights in any form cost_rows_tensor takes, or its (B, 40) device tensor: trajectory b is solved
    with row b for model.q, qf and r (quattro_ilqr_solve_cost_f32; the same kernel rule and refusals as model_phys).  None: the
    model's weights for every trajectory."""
    Bt, N, m = u_nom.shape
    model_phys = model_phys_tensor(model, model_phys, Bt, u_nom.device)
    x_ref_rows = x_ref_rows_tensor(model, x_ref_rows, Bt, u_nom.device, name="x_ref_rows")
    cost_rows = cost_rows_tensor(model, cost_rows, Bt, u_nom.device, name="cost_rows")
    n = model.n
    f32, i32 = torch.float32, torch.int32
    _req(x_nom, (Bt, N + 1, n), f32, "x_nom"); _req(u_nom, (Bt, N, model.m), f32, "u_nom")
    _req(K, (Bt, N, m, n), f32, "K"); _req(k, (Bt, N, m), f32, "k"); _req(cost, (Bt,), torch.float64, "cost")
    _req(alpha_idx, (Bt,), i32, "alpha_idx"); _req(active, (Bt,), i32, "active"); _req(iters, (Bt,), i32, "iters")
    if status is not None:
        _req(status, (Bt,), i32, "status")
    flags = (_lib.SOLVE_FIXED_ITERS if fixed_iters else 0) | (_lib.SOLVE_RESET if reset else 0) | \
        (_lib.SOLVE_PERSISTENT if persistent else 0) | (_lib.SOLVE_ENQUEUE if enqueue else 0)
    if x0 is not None:
        _req(x0, (Bt, n), f32, "x0")
        flags |= _lib.SOLVE_SIMULATE
    if log is not None and (log.B != Bt or log.N != N or (log.n, log.m) != (n, m)):
        raise ValueError("log ring was built for another problem size")
    arr, na = _alphas(alphas)
    p = model.c_params()
    args = (ctypes.byref(p), _ptr(x0), _ptr(x_nom), _ptr(u_nom), Bt, N, float(reg), arr, na, float(tol), int(max_iter), flags,
            _ptr(K), _ptr(k), _ptr(cost), _ptr(alpha_idx), _ptr(active), _ptr(iters), _ptr(status), _ptr(workspace),
            workspace.numel() * workspace.element_size(), None if log is None else log.byref())
    _solve_call(_lib.load_for(model), args, model_phys, x_ref_rows, _stream(), cost_rows)


def _solve_call(lib, args, model_phys, x_ref_rows, stream, cost_rows=None):
    """The one C call of a solve: the cost entry with weights, else the ref entry with rows, else the phys entry (whose NULL rows
    forward inside the library)."""
    if cost_rows is not None:
        check(lib.quattro_ilqr_solve_cost_f32(*args, _ptr(model_phys), _ptr(x_ref_rows),
                                              0 if x_ref_rows is None else x_ref_rows.shape[1], _ptr(cost_rows), stream),
              "quattro_ilqr_solve_cost_f32")
    elif x_ref_rows is not None:
        check(lib.quattro_ilqr_solve_ref_f32(*args, _ptr(model_phys), _ptr(x_ref_rows), x_ref_rows.shape[1], stream),
              "quattro_ilqr_solve_ref_f32")
    else:
        check(lib.quattro_ilqr_solve_phys_f32(*args, _ptr(model_phys), stream), "quattro_ilqr_solve_phys_f32")


class PreparedSolve:
    """ilqr_solve with everything that does not change between solves of one QuattroILQR checked and converted ONCE: shapes,
    dtypes, device pointers, the alpha array, the parameter struct.  A call is then one ctypes call (single-trajectory
    solves are a few tens of microseconds of device time: a dozen shape checks per call were a third of the host's share)."""

    def __init__(self, model, x_nom, u_nom, K, k, cost, workspace, alphas, reg, x0, alpha_idx, active, iters, status):
        Bt, N, m = u_nom.shape
        n = model.n
        f32, i32 = torch.float32, torch.int32
        _req(x_nom, (Bt, N + 1, n), f32, "x_nom"); _req(u_nom, (Bt, N, model.m), f32, "u_nom")
        _req(K, (Bt, N, m, n), f32, "K"); _req(k, (Bt, N, m), f32, "k"); _req(cost, (Bt,), torch.float64, "cost")
        _req(alpha_idx, (Bt,), i32, "alpha_idx"); _req(active, (Bt,), i32, "active"); _req(iters, (Bt,), i32, "iters")
        _req(status, (Bt,), i32, "status"); _req(x0, (Bt, n), f32, "x0")
        self.keep = (x_nom, u_nom, K, k, cost, workspace, x0, alpha_idx, active, iters, status)     # the pointers stay valid
        self.arr, self.na = _alphas(alphas)
        self.p = model.c_params()
        self.lib = _lib.load_for(model)
        self.model = model
        self.dims = (Bt, N, n, m)
        self.head = (ctypes.byref(self.p), _ptr(x0), _ptr(x_nom), _ptr(u_nom), Bt, N, float(reg), self.arr, self.na)
        self.tail = (_ptr(K), _ptr(k), _ptr(cost), _ptr(alpha_idx), _ptr(active), _ptr(iters), _ptr(status), _ptr(workspace),
                     workspace.numel() * workspace.element_size())

    def __call__(self, tol, max_iter, fixed_iters=False, log=None, persistent=False, stream=None, model_phys=None,
                 x_ref_rows=None, cost_rows=None):
        """model_phys, x_ref_rows, cost_rows: per-trajectory phys rows, reference rows and cost weights (ilqr_solve).  Nothing of
        them is prepared or kept: the rows are THIS call's argument, so a later call without them is the plain solve."""
        flags = _lib.SOLVE_SIMULATE | _lib.SOLVE_RESET | (_lib.SOLVE_FIXED_ITERS if fixed_iters else 0) | \
            (_lib.SOLVE_PERSISTENT if persistent else 0)
        if log is not None and (log.B, log.N, log.n, log.m) != self.dims:
            raise ValueError("log ring was built for another problem size")
        model_phys = model_phys_tensor(self.model, model_phys, self.dims[0], self.keep[0].device)
        x_ref_rows = x_ref_rows_tensor(self.model, x_ref_rows, self.dims[0], self.keep[0].device, name="x_ref_rows")
        cost_rows = cost_rows_tensor(self.model, cost_rows, self.dims[0], self.keep[0].device, name="cost_rows")
        _solve_call(self.lib, (*self.head, float(tol), int(max_iter), flags, *self.tail, None if log is None else log.byref()),
                    model_phys, x_ref_rows, _stream() if stream is None else stream, cost_rows)


def check_plant(model, plant):
    """A plant is the controller's own problem with other physical parameters and, if wanted, another integrator: the same name,
    n, m, dt and, for a user model, the same library.  ValueError otherwise; host logic only."""
    if plant is None:
        return
    same = (getattr(plant, "name", None) == model.name and getattr(plant, "model_id", None) == model.model_id
            and (plant.n, plant.m) == (model.n, model.m) and float(plant.dt) == float(model.dt)
            and getattr(plant, "lib_path", "") == getattr(model, "lib_path", ""))
    if not same:
        raise ValueError("plant must be the controller's model (name, n, m, dt and library) with its own phys / integrator")


def check_phys_rows(model, rows, B, name):
    """Per-controller physical parameters, a plant's or a model's: None, (B, len(model.phys)), or the (B, 8) float32 device tensor the
    C ABI takes.  ValueError otherwise; host logic only.  -> True where the rows need no conversion (None or such a tensor)."""
    if rows is None or (isinstance(rows, torch.Tensor) and tuple(rows.shape) == (B, 8) and rows.is_cuda
                        and rows.dtype == torch.float32 and rows.is_contiguous()):
        return True
    shape = tuple(np.shape(rows))
    if shape != (B, len(model.phys)):
        raise ValueError(f"{name} must have shape {(B, len(model.phys))} (got {shape})")
    return False


def plant_phys_tensor(model, plant_phys, B, device, name="plant_phys"):
    """(B, len(model.phys)) rows -> the (B, 8) float32 device array the C ABI takes: the one conversion of both kinds of rows (a
    plant's, a model's).  Such an array is passed through as it is, None stays None; the shape is checked (check_phys_rows) before
    anything touches the device."""
    if check_phys_rows(model, plant_phys, B, name):
        return plant_phys
    out = torch.zeros((B, 8), dtype=torch.float32, device=device)
    out[:, :len(model.phys)] = torch.as_tensor(plant_phys, dtype=torch.float32, device=device)
    return out


def model_phys_tensor(model, model_phys, B, device):
    """Per-trajectory model parameters: plant_phys_tensor under the name the errors use."""
    return plant_phys_tensor(model, model_phys, B, device, name="model_phys")


def check_ref_rows(model, rows, B, name="targets", device=None):
    """Reference rows: None, (B, R, n) with R >= 1, or (B, n) for R = 1.  ValueError otherwise, under the keyword's `name`; host logic
    only.  -> True where the rows need no conversion: None, or a contiguous (B, R, n) float32 tensor on `device` (any CUDA device
    if None) whose first element is 16-byte aligned, as the C ABI asks (a slice of a larger tensor may not be)."""
    if rows is None:
        return True
    shape = tuple(np.shape(rows))
    if not ((len(shape) == 2 and shape == (B, model.n)) or (len(shape) == 3 and shape[0] == B and shape[1] >= 1 and shape[2] == model.n)):
        raise ValueError(f"{name} must have shape {(B, 'R', model.n)} with R >= 1, or {(B, model.n)} (got {shape})")
    return (isinstance(rows, torch.Tensor) and len(shape) == 3 and rows.is_cuda and rows.dtype == torch.float32
            and rows.is_contiguous() and rows.data_ptr() % 16 == 0
            and (device is None or rows.device == torch.device(device)))


def x_ref_rows_tensor(model, rows, B, device, name="targets"):
    """Reference rows (B, R, n), or (B, n) as R = 1 -> the contiguous, 16-byte aligned (B, R, n) float32 array on `device` that the
    C ABI takes (x_ref_rows, include/quattro_hip.h).  Such an array is passed through as it is, None stays None; the shape is
    checked (check_ref_rows) before anything touches the device."""
    if check_ref_rows(model, rows, B, name, device):
        return rows
    t = torch.as_tensor(rows, dtype=torch.float32, device=device).reshape(B, -1, model.n).contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


COST_ROW_FLOATS = 2 * _lib.MAX_NX + _lib.MAX_NU      # QUATTRO_COST_ROW_FLOATS: q at float 0, qf at float MAX_NX, r at float 2 MAX_NX
_COST_KEYS = ("q", "qf", "r")


def model_can_cost_rows(model):
    """Whether the model's persistent kernel has a form that reads per-trajectory cost weights: the cart-pole's and a user model's
    have, the built-in quadrotor's has not (the C entries answer QUATTRO_ERR_UNSUPPORTED for it before any launch)."""
    return model_can_device_loop(model) and model.model_id != _lib.MODEL_QUADROTOR


def check_cost_rows(model, weights, B, name="weights", device=None):
    """Per-trajectory cost weights: None; a dict with any of the keys "q", "qf", "r", each (B, n) / (B, n) / (B, m) or one vector
    that is broadcast over the batch (a missing key takes the model's own values); a plain (B, 2n + m) array in the order
    [q | qf | r]; or the (B, 40) float32 device tensor the C ABI takes.  ValueError otherwise, under the keyword's `name`; host
    logic only, the values are not looked at.  -> True where the rows need no conversion (None or such a tensor)."""
    if weights is None:
        return True
    n, m = model.n, model.m
    if isinstance(weights, dict):
        unknown = [key for key in weights if key not in _COST_KEYS]
        if unknown:
            raise ValueError(f"{name} has unknown keys {unknown}: the keys are {list(_COST_KEYS)}")
        for key in weights:
            d = m if key == "r" else n
            shape = tuple(np.shape(weights[key]))
            if shape != (B, d) and shape != (d,):
                raise ValueError(f"{name}[{key!r}] must have shape {(B, d)} or {(d,)} (got {shape})")
        return False
    shape = tuple(np.shape(weights))
    if (isinstance(weights, torch.Tensor) and shape == (B, COST_ROW_FLOATS) and weights.is_cuda and weights.dtype == torch.float32
            and weights.is_contiguous() and weights.data_ptr() % 16 == 0
            and (device is None or weights.device == torch.device(device))):
        return True
    if shape != (B, 2 * n + m):
        raise ValueError(f"{name} must be a dict with keys from {list(_COST_KEYS)} or have shape {(B, 2 * n + m)} (got {shape})")
    return False


def cost_rows_tensor(model, weights, B, device, name="weights"):
    """Per-trajectory cost weights in any form check_cost_rows takes -> the (B, 40) float32 array on `device` that the C ABI takes
    (cost_rows, include/quattro_hip.h: q at float 0, qf at float 16, r at float 32; the entries beyond n / m are zero and ignored).
    Such an array is passed through as it is, None stays None; the one check and the one conversion of the rows, before anything
    touches the device."""
    if check_cost_rows(model, weights, B, name, device):
        return weights
    n, m = model.n, model.m
    parts = {"q": np.asarray(model.q, dtype=np.float32), "qf": np.asarray(model.qf, dtype=np.float32),
             "r": np.asarray(model.r, dtype=np.float32)}
    if isinstance(weights, dict):
        for key, v in weights.items():
            parts[key] = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    else:
        w = weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else np.asarray(weights)
        parts = {"q": w[:, :n], "qf": w[:, n:2 * n], "r": w[:, 2 * n:]}
    rows = np.zeros((B, COST_ROW_FLOATS), dtype=np.float32)
    for key, at, d in (("q", 0, n), ("qf", _lib.MAX_NX, n), ("r", 2 * _lib.MAX_NX, m)):
        rows[:, at:at + d] = np.broadcast_to(np.asarray(parts[key], dtype=np.float32), (B, d))
    t = torch.as_tensor(rows, device=device)
    return t if t.data_ptr() % 16 == 0 else t.clone()


def score(model, x, u, targets=None, weights=None, model_phys=None, terminal=False, ref_hold=1, want_stage=True):
    """Per-step costs and their fp64 totals of sequences x (B, S+1, n), u (B, S, m), which need not satisfy the dynamics, on the
    device (quattro_score_f32): -> (total (B,) float64, stage (B, S+1) float32, or None with want_stage=False).
    stage[b, s] = L(x_s, u_s) for s < S; stage[b, S] = Lf(x_S) with terminal=True, else +0; total[b] is the fp64 sum of stage[b, :]
    in step order (with terminal=True and no rows: ops.total_cost, bit for bit).  Each trajectory under rows of its own, in the
    forms the solves and runs take, every model (the built-in quadrotor's weights too: model_can_cost_rows guards solves and runs):
      targets     as x_ref_rows_tensor takes them: step s is scored against row min((s // ref_hold) * ref_hold, R - 1) of trajectory b
                  -- ref_hold=1 is "row s", what a run with preview=True was planned against at plant step s; ref_hold=h is the
                  set-point schedule of preview=False with replan_every=h; past the last row the last row holds
      weights     as cost_rows_tensor takes them: q, r (and qf for the terminal slot) of row b
      model_phys  as model_phys_tensor takes them: phys of row b (read by a user model's cost only)
    None: the model's own x_ref / q, qf, r / phys.  ValueError for a wrong shape or ref_hold < 1, before anything touches the device."""
    if len(np.shape(x)) != 3 or len(np.shape(u)) != 3:
        raise ValueError(f"x must have shape (B, S + 1, n) and u (B, S, m) (got {tuple(np.shape(x))} and {tuple(np.shape(u))})")
    Bt, S, m = (int(v) for v in u.shape)
    if Bt < 1 or S < 1 or m != model.m or tuple(x.shape) != (Bt, S + 1, model.n):
        raise ValueError(f"x must have shape (B, S + 1, {model.n}) and u (B, S, {model.m}) with B, S >= 1 "
                         f"(got {tuple(x.shape)} and {tuple(u.shape)})")
    check_phys_rows(model, model_phys, Bt, "model_phys")
    check_ref_rows(model, targets, Bt, name="targets")
    check_cost_rows(model, weights, Bt, name="weights")
    if isinstance(ref_hold, bool) or int(ref_hold) != ref_hold or int(ref_hold) < 1:
        raise ValueError(f"ref_hold must be an integer >= 1 (got {ref_hold!r})")
    f32 = torch.float32
    _req(x, (Bt, S + 1, model.n), f32, "x"); _req(u, (Bt, S, model.m), f32, "u")
    model_phys = model_phys_tensor(model, model_phys, Bt, u.device)
    rows = x_ref_rows_tensor(model, targets, Bt, u.device, name="targets")
    cost_rows = cost_rows_tensor(model, weights, Bt, u.device, name="weights")
    stage = torch.empty((Bt, S + 1), dtype=f32, device=u.device) if want_stage else None
    total = torch.empty((Bt,), dtype=torch.float64, device=u.device)
    p = model.c_params()
    check(_lib.load_for(model).quattro_score_f32(ctypes.byref(p), _ptr(x), _ptr(u), Bt, S, _ptr(model_phys), _ptr(rows),
                                                 0 if rows is None else rows.shape[1], int(ref_hold), _ptr(cost_rows),
                                                 _lib.SCORE_TERMINAL if terminal else 0, _ptr(stage), _ptr(total), _stream()),
          "quattro_score_f32")
    return total, stage


def cost_gradient(model, x, u, targets=None, weights=None, model_phys=None, want_x0=True, want_costate=False):
    """Gradient of the trajectory cost J(x0, u) = sum_t L(x_t, u_t) + Lf(x_N), x_{t+1} = f(x_t, u_t), by the adjoint sweep on the
    device (quattro_cost_gradient_f32) about x (B, N+1, n), u (B, N, m): -> dict with "grad_u" (B, N, m) = dJ/du, and "grad_x0"
    (B, n) = dJ/dx0 with want_x0, "costate" (B, N+1, n) with want_costate (costate[:, 0] is grad_x0), all float32.  x is meant to
    be the rollout of u (ops.simulate, or ops.track(..., feedback=False, plant_phys=model_phys) under model_phys); as for
    ops.linearize this is not checked.  Each trajectory under rows of its own, in the forms the solves and ops.score take, every
    model (the built-in quadrotor's weights too):
      targets     as x_ref_rows_tensor takes them: horizon step t against row min(t, R - 1) of trajectory b, t = N the terminal term
      weights     as cost_rows_tensor takes them: q, qf, r of row b
      model_phys  as model_phys_tensor takes them: phys of row b, in the dynamics and in a user model's cost
    None: the model's own x_ref / q, qf, r / phys.  Nothing is differentiated with respect to rows or model parameters.  ValueError
    for a wrong shape, before anything touches the device."""
    if len(np.shape(x)) != 3 or len(np.shape(u)) != 3:
        raise ValueError(f"x must have shape (B, N + 1, n) and u (B, N, m) (got {tuple(np.shape(x))} and {tuple(np.shape(u))})")
    Bt, N, m = (int(v) for v in u.shape)
    if Bt < 1 or N < 1 or m != model.m or tuple(x.shape) != (Bt, N + 1, model.n):
        raise ValueError(f"x must have shape (B, N + 1, {model.n}) and u (B, N, {model.m}) with B, N >= 1 "
                         f"(got {tuple(x.shape)} and {tuple(u.shape)})")
    check_phys_rows(model, model_phys, Bt, "model_phys")
    check_ref_rows(model, targets, Bt, name="targets")
    check_cost_rows(model, weights, Bt, name="weights")
    f32 = torch.float32
    _req(x, (Bt, N + 1, model.n), f32, "x"); _req(u, (Bt, N, model.m), f32, "u")
    model_phys = model_phys_tensor(model, model_phys, Bt, u.device)
    rows = x_ref_rows_tensor(model, targets, Bt, u.device, name="targets")
    cost_rows = cost_rows_tensor(model, weights, Bt, u.device, name="weights")
    out = {"grad_u": torch.empty((Bt, N, model.m), dtype=f32, device=u.device)}
    if want_x0:
        out["grad_x0"] = torch.empty((Bt, model.n), dtype=f32, device=u.device)
    if want_costate:
        out["costate"] = torch.empty((Bt, N + 1, model.n), dtype=f32, device=u.device)
    p = model.c_params()
    check(_lib.load_for(model).quattro_cost_gradient_f32(ctypes.byref(p), _ptr(x), _ptr(u), Bt, N, _ptr(model_phys), _ptr(rows),
                                                         0 if rows is None else rows.shape[1], _ptr(cost_rows),
                                                         _ptr(out["grad_u"]), _ptr(out.get("grad_x0")), _ptr(out.get("costate")),
                                                         _stream()),
          "quattro_cost_gradient_f32")
    return out


PARAM_GRADIENT_WANTS = ("phys", "weights", "targets")


def cost_param_gradient(model, x, u, targets=None, weights=None, model_phys=None, want=PARAM_GRADIENT_WANTS, costate=None):
    """Gradient of the trajectory cost of ops.cost_gradient with respect to what a trajectory's rows hold, on the device
    (quattro_cost_param_gradient_f32) about x (B, N+1, n), u (B, N, m): -> dict of float64 device tensors, by `want`:
      "phys"     "grad_phys" (B, len(model.phys)): sum_t lambda_{t+1}^T df/dtheta_k (x_t, u_t), f the whole integrator step at
                 trajectory b's own parameters
      "weights"  "grad_weights" (B, 2n + m) in the order [q | qf | r]: sum_t (x_t - ref_t)^2, (x_N - ref_N)^2, sum_t u_t^2
      "targets"  "grad_targets" (B, R, n): row rho collects -2 q (x_t - ref_rho) of the steps that read it (min(t, R - 1) = rho) and
                 -2 qf (x_N - ref_rho) where the terminal term reads it; R = 1 without targets (the gradient with respect to a
                 per-trajectory copy of model.x_ref); rows past the horizon are zero
    targets, weights, model_phys: the rows the gradient is taken about, in the forms ops.cost_gradient takes; None: the model's own
    values.  costate (B, N+1, n) float32: ops.cost_gradient(..., want_costate=True)["costate"] under the same rows, used as it is;
    None with "phys" wanted: that call is made first (two launches).  The barrier and dt are not differentiated.  The built-in
    models, and a user model compiled with compile_model(..., param_grad=True): its costs are arbitrary, so every entry is then the
    derivative of the whole cost -- "phys" adds dL/dtheta_k and dLf/dtheta_k of a cost that reads P, each weight collects its partial
    of both L and Lf, each target row those of the slots that read it (for a default cost these are the forms above).
    NotImplementedError for any other user-compiled model.  ValueError for a wrong shape or an unknown entry of `want`, before
    anything touches the device."""
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in want if w not in PARAM_GRADIENT_WANTS]
    if unknown or not want:
        raise ValueError(f"want must name at least one of {list(PARAM_GRADIENT_WANTS)} (got {list(want)})")
    if len(np.shape(x)) != 3 or len(np.shape(u)) != 3:
        raise ValueError(f"x must have shape (B, N + 1, n) and u (B, N, m) (got {tuple(np.shape(x))} and {tuple(np.shape(u))})")
    Bt, N, m = (int(v) for v in u.shape)
    if Bt < 1 or N < 1 or m != model.m or tuple(x.shape) != (Bt, N + 1, model.n):
        raise ValueError(f"x must have shape (B, N + 1, {model.n}) and u (B, N, {model.m}) with B, N >= 1 "
                         f"(got {tuple(x.shape)} and {tuple(u.shape)})")
    check_phys_rows(model, model_phys, Bt, "model_phys")
    check_ref_rows(model, targets, Bt, name="targets")
    check_cost_rows(model, weights, Bt, name="weights")
    if costate is not None and tuple(np.shape(costate)) != (Bt, N + 1, model.n):
        raise ValueError(f"costate must have shape {(Bt, N + 1, model.n)} (got {tuple(np.shape(costate))})")
    if model.model_id == _lib.MODEL_USER and not getattr(model, "param_grad", False):
        raise NotImplementedError("cost_param_gradient runs only for the built-in models and for user models compiled with "
                                  "compile_model(..., param_grad=True): without it a user-compiled model reads its parameters as float")
    f32, f64 = torch.float32, torch.float64
    _req(x, (Bt, N + 1, model.n), f32, "x"); _req(u, (Bt, N, model.m), f32, "u")
    n, dev = model.n, u.device
    model_phys = model_phys_tensor(model, model_phys, Bt, dev)
    rows = x_ref_rows_tensor(model, targets, Bt, dev, name="targets")
    cost_rows = cost_rows_tensor(model, weights, Bt, dev, name="weights")
    if "phys" in want:
        if costate is None:
            costate = cost_gradient(model, x, u, targets=rows, weights=cost_rows, model_phys=model_phys, want_x0=False,
                                    want_costate=True)["costate"]
        _req(costate, (Bt, N + 1, n), f32, "costate")
    R = 1 if rows is None else int(rows.shape[1])
    g_phys = torch.empty((Bt, 8), dtype=f64, device=dev) if "phys" in want else None
    g_cost = torch.empty((Bt, COST_ROW_FLOATS), dtype=f64, device=dev) if "weights" in want else None
    g_ref = torch.empty((Bt, R, n), dtype=f64, device=dev) if "targets" in want else None
    p = model.c_params()
    check(_lib.load_for(model).quattro_cost_param_gradient_f32(ctypes.byref(p), _ptr(x), _ptr(u), Bt, N,
                                                               _ptr(costate) if "phys" in want else None, _ptr(model_phys),
                                                               _ptr(rows), 0 if rows is None else R, _ptr(cost_rows), _ptr(g_phys),
                                                               _ptr(g_cost), _ptr(g_ref), _stream()),
          "quattro_cost_param_gradient_f32")
    out = {}
    if g_phys is not None:
        out["grad_phys"] = g_phys[:, :len(model.phys)].contiguous()
    if g_cost is not None:
        out["grad_weights"] = torch.cat([g_cost[:, :n], g_cost[:, _lib.MAX_NX:_lib.MAX_NX + n],
                                         g_cost[:, 2 * _lib.MAX_NX:2 * _lib.MAX_NX + m]], dim=1)
    if g_ref is not None:
        out["grad_targets"] = g_ref
    return out


def track(model, x0, x_nom, u_nom, K, steps, plant=None, plant_phys=None, feedback=True, disturbance=None):
    """`steps` <= N plant steps from x0 (B,n) along the first rows of a nominal with its gains (quattro_track_f32):
    u = u_nom[j] + (feedback ? K[j] (x - x_nom[j]) : 0), x <- f_plant(x, u) + disturbance[j].  plant: a DeviceModel like `model`
    with the plant's integrator and phys (None = the model itself); plant_phys (B, len(model.phys)): per-controller phys.
    -> x (B,steps+1,n), u (B,steps,m)."""
    Bt, N, m = u_nom.shape
    n = model.n
    f32 = torch.float32
    steps = int(steps)
    if not 1 <= steps <= N:
        raise ValueError("steps must be in 1..N")
    _req(x0, (Bt, n), f32, "x0"); _req(x_nom, (Bt, N + 1, n), f32, "x_nom"); _req(u_nom, (Bt, N, model.m), f32, "u_nom")
    _req(K, (Bt, N, m, n), f32, "K")
    if disturbance is not None:
        _req(disturbance, (steps, Bt, n), f32, "disturbance")
    check_plant(model, plant)
    pp = None if plant is None else plant.c_params()
    pphys = plant_phys_tensor(model, plant_phys, Bt, u_nom.device)
    x = torch.empty((Bt, steps + 1, n), dtype=f32, device=u_nom.device)
    u = torch.empty((Bt, steps, m), dtype=f32, device=u_nom.device)
    p = model.c_params()
    pref = None if pp is None else ctypes.byref(pp)
    check(_lib.load_for(model).quattro_track_f32(ctypes.byref(p), pref, _ptr(pphys), _ptr(x0), _ptr(x_nom), _ptr(u_nom), _ptr(K),
                                                 int(bool(feedback)), Bt, N, steps, _ptr(disturbance), _ptr(x), _ptr(u), _stream()),
          "quattro_track_f32")
    return x, u


TRACK_GRADIENT_WANTS = ("K", "x_nom", "x0")


def track_gradient(model, x, u, x_nom=None, K=None, plant=None, plant_phys=None, targets=None, weights=None, terminal=True,
                   want=TRACK_GRADIENT_WANTS, want_costate=False):
    """Gradient of the tracked closed-loop cost on the device (quattro_track_gradient_f32): S steps of ops.track,
    u_t = u_nom_t + K_t (x_t - x_nom_t), x_{t+1} = f_plant(x_t, u_t) + d_t, scored by ops.score(..., ref_hold=1, terminal=terminal),
    about the realised x (B, S+1, n), u (B, S, m) that ops.track returned.  x_nom (B, N+1, n), K (B, N, m, n), N >= S: the arrays
    that call was given; K None: the feedback was off (x_nom is then not looked at, and "grad_K" and "grad_x_nom" are not returned:
    the cost does not depend on either).
    -> dict of float32 device tensors: "grad_u_nom" (B, N, m) always, and by `want`: "K" -> "grad_K" (B, N, m, n) = g_t (x_t - x_nom_t)^T,
    "x_nom" -> "grad_x_nom" (B, N+1, n) = -K_t^T g_t, "x0" -> "grad_x0" (B, n); want_costate: "costate" (B, S+1, n), the closed-loop
    costate (costate[:, t+1] is the gradient with respect to the disturbance of step t, and the multiplier ops.cost_param_gradient
    takes for the plant-parameter gradient of the tracked cost).  Rows t >= S of the full-shape outputs are +0.0.  With K None and
    N taken as S, "grad_u_nom" is ops.cost_gradient's "grad_u".
    plant / plant_phys: as ops.track takes them; the struct the entry is given carries the model's cost fields and the plant's
    integrator and phys (which a user model's cost bodies then see too).  targets, weights: as ops.cost_gradient takes them.
    ValueError for a wrong shape or an unknown entry of `want`, before anything touches the device."""
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in want if w not in TRACK_GRADIENT_WANTS]
    if unknown:
        raise ValueError(f"want may name {list(TRACK_GRADIENT_WANTS)} (got {list(want)})")
    if len(np.shape(x)) != 3 or len(np.shape(u)) != 3:
        raise ValueError(f"x must have shape (B, S + 1, n) and u (B, S, m) (got {tuple(np.shape(x))} and {tuple(np.shape(u))})")
    Bt, S, m = (int(v) for v in u.shape)
    n = model.n
    if Bt < 1 or S < 1 or m != model.m or tuple(x.shape) != (Bt, S + 1, n):
        raise ValueError(f"x must have shape (B, S + 1, {n}) and u (B, S, {model.m}) with B, S >= 1 "
                         f"(got {tuple(x.shape)} and {tuple(u.shape)})")
    if K is None:
        want = tuple(w for w in want if w == "x0")          # nothing depends on K or x_nom
        N = S
    else:
        kshape = tuple(np.shape(K))
        if len(kshape) != 4 or kshape[0] != Bt or kshape[1] < S or kshape[2:] != (m, n):
            raise ValueError(f"K must have shape ({Bt}, N, {m}, {n}) with N >= {S} (got {kshape})")
        N = int(kshape[1])
        if x_nom is None or tuple(np.shape(x_nom)) != (Bt, N + 1, n):
            raise ValueError(f"x_nom must have shape {(Bt, N + 1, n)} (got {None if x_nom is None else tuple(np.shape(x_nom))})")
    check_plant(model, plant)
    check_phys_rows(model, plant_phys, Bt, "plant_phys")
    check_ref_rows(model, targets, Bt, name="targets")
    check_cost_rows(model, weights, Bt, name="weights")
    f32 = torch.float32
    _req(x, (Bt, S + 1, n), f32, "x"); _req(u, (Bt, S, m), f32, "u")
    if K is not None:
        _req(K, (Bt, N, m, n), f32, "K"); _req(x_nom, (Bt, N + 1, n), f32, "x_nom")
    dev = u.device
    pphys = plant_phys_tensor(model, plant_phys, Bt, dev)
    rows = x_ref_rows_tensor(model, targets, Bt, dev, name="targets")
    cost_rows = cost_rows_tensor(model, weights, Bt, dev, name="weights")
    out = {"grad_u_nom": torch.empty((Bt, N, m), dtype=f32, device=dev)}
    if "K" in want:
        out["grad_K"] = torch.empty((Bt, N, m, n), dtype=f32, device=dev)
    if "x_nom" in want:
        out["grad_x_nom"] = torch.empty((Bt, N + 1, n), dtype=f32, device=dev)
    if "x0" in want:
        out["grad_x0"] = torch.empty((Bt, n), dtype=f32, device=dev)
    if want_costate:
        out["costate"] = torch.empty((Bt, S + 1, n), dtype=f32, device=dev)
    # the cost fields of the model, the integrator and phys of the plant
    p = (model if plant is None else model.with_(integrator=plant.integrator, phys=tuple(plant.phys))).c_params()
    check(_lib.load_for(model).quattro_track_gradient_f32(
        ctypes.byref(p), _ptr(x), _ptr(u), Bt, N, S, _ptr(x_nom) if K is not None else None, _ptr(K), _ptr(pphys), _ptr(rows),
        0 if rows is None else rows.shape[1], _ptr(cost_rows), _lib.SCORE_TERMINAL if terminal else 0, _ptr(out["grad_u_nom"]),
        _ptr(out.get("grad_K")), _ptr(out.get("grad_x_nom")), _ptr(out.get("grad_x0")), _ptr(out.get("costate")), _stream()),
        "quattro_track_gradient_f32")
    return out


TRACK_COVARIANCE_WANTS = ("cov", "var", "var_u", "excess")


def check_cov_rows(model, v, B, name):
    """A covariance per trajectory: None; a diagonal (n,) or (B, n); or a matrix (n, n) or (B, n, n) -- a 2-D (n, n) is the one
    matrix for every trajectory, also where B = n.  A torch tensor must be floating point.  ValueError otherwise, under the keyword's
    `name`; host logic only, the values are not looked at."""
    if v is None:
        return
    n = model.n
    shape = tuple(np.shape(v))
    if shape not in ((n,), (B, n), (n, n), (B, n, n)):
        raise ValueError(f"{name} must be a diagonal of shape {(n,)} or {(B, n)} or a matrix of shape {(n, n)} or {(B, n, n)} "
                         f"(got {shape})")
    if isinstance(v, torch.Tensor) and not v.is_floating_point():
        raise ValueError(f"{name} must be floating point (got {v.dtype})")


def cov_rows_tensor(model, v, B, device, name="cov0"):
    """A covariance in any form check_cov_rows takes -> the contiguous [B][n][n] float32 array on `device` that the C ABI takes,
    expanded with torch ops on the device.  None stays None."""
    check_cov_rows(model, v, B, name)
    if v is None:
        return None
    n = model.n
    t = torch.as_tensor(v if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float32)).to(device=device, dtype=torch.float32)
    if tuple(t.shape) in ((n,), (B, n)) and tuple(t.shape) != (n, n):
        t = torch.diag_embed(t)
    return t.expand(B, n, n).contiguous()


def track_covariance(model, x, u, K=None, plant=None, plant_phys=None, weights=None, cov0=None, noise=None, terminal=True,
                     want=("var", "var_u", "excess")):
    """First-order covariance of a tracked closed-loop run on the device (quattro_track_covariance_f32): how far the run of
    ops.track spreads under noise.  About the realised x (B, S+1, n), u (B, S, m) that ops.track returned under the gains
    K (B, N, m, n), N >= S, with A_t, B_t the PLANT's step Jacobians at (x_t, u_t) (its integrator, its per-trajectory plant_phys row):
        Acl_t       = A_t + B_t K_t                        (K None: Acl_t = A_t, the open loop)
        Sigma_0     = cov0[b]                              (None: 0)
        Sigma_{t+1} = Acl_t Sigma_t Acl_t^T + W[b]         (W = noise, None: 0: the covariance of ops.track's additive disturbance
                                                            d_t, which enters after the plant step)
        var_u_t     = diag(K_t Sigma_t K_t^T)              (t < S; K None: 0)
        excess      = sum_{t<S} [ sum_i q_i Sigma_t[i][i] + 1/2 sum_a l_uu,t[a][a] var_u_t[a] ] + [terminal] sum_i qf_i Sigma_S[i][i]
    excess is the second-order estimate of E[J] - J(realised run) under ops.score's cost: l_uu is 2 r_a plus the second derivative of
    the control barrier at u_t, and q, qf, r are the trajectory's row of `weights` where given (as ops.score takes them, the built-in
    quadrotor's too).  Targets do not enter: the Hessians do not depend on them.
    -> dict of device tensors, by `want`: "cov" (B, S+1, n, n) = Sigma_t, "var" (B, S+1, n) its diagonal (the same bits), "var_u"
    (B, N, m) (rows t >= S are +0.0; N = S with K None), all float32; "excess" (B,) float64, summed in step order.
    cov0, noise: a diagonal (n,) or (B, n), or a matrix (n, n) or (B, n, n); a 2-D (n, n) is one matrix for every trajectory.  They
    are expanded on the device.  That they are symmetric and positive semi-definite is the CALLER's responsibility: neither is
    checked, and the recursion reads Sigma as symmetric (the returned "cov" is symmetric to round-off only).
    plant / plant_phys: as ops.track takes them.  The built-in models only: NotImplementedError for a user-compiled model, before its
    library is loaded.  ValueError for a wrong shape or dtype or an unknown or empty `want`, before anything touches the device."""
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in want if w not in TRACK_COVARIANCE_WANTS]
    if unknown or not want:
        raise ValueError(f"want must name at least one of {list(TRACK_COVARIANCE_WANTS)} (got {list(want)})")
    if len(np.shape(x)) != 3 or len(np.shape(u)) != 3:
        raise ValueError(f"x must have shape (B, S + 1, n) and u (B, S, m) (got {tuple(np.shape(x))} and {tuple(np.shape(u))})")
    Bt, S, m = (int(v) for v in u.shape)
    n = model.n
    if Bt < 1 or S < 1 or m != model.m or tuple(x.shape) != (Bt, S + 1, n):
        raise ValueError(f"x must have shape (B, S + 1, {n}) and u (B, S, {model.m}) with B, S >= 1 "
                         f"(got {tuple(x.shape)} and {tuple(u.shape)})")
    N = S
    if K is not None:
        kshape = tuple(np.shape(K))
        if len(kshape) != 4 or kshape[0] != Bt or kshape[1] < S or kshape[2:] != (m, n):
            raise ValueError(f"K must have shape ({Bt}, N, {m}, {n}) with N >= {S} (got {kshape})")
        N = int(kshape[1])
    check_plant(model, plant)
    check_phys_rows(model, plant_phys, Bt, "plant_phys")
    check_cost_rows(model, weights, Bt, name="weights")
    check_cov_rows(model, cov0, Bt, "cov0")
    check_cov_rows(model, noise, Bt, "noise")
    if model.model_id == _lib.MODEL_USER:
        raise NotImplementedError("track_covariance runs only for the built-in models")
    f32 = torch.float32
    _req(x, (Bt, S + 1, n), f32, "x"); _req(u, (Bt, S, m), f32, "u")
    if K is not None:
        _req(K, (Bt, N, m, n), f32, "K")
    dev = u.device
    pphys = plant_phys_tensor(model, plant_phys, Bt, dev)
    cost_rows = cost_rows_tensor(model, weights, Bt, dev, name="weights")
    c0 = cov_rows_tensor(model, cov0, Bt, dev, "cov0")
    w = cov_rows_tensor(model, noise, Bt, dev, "noise")
    out = {}
    if "cov" in want:
        out["cov"] = torch.empty((Bt, S + 1, n, n), dtype=f32, device=dev)
    if "var" in want:
        out["var"] = torch.empty((Bt, S + 1, n), dtype=f32, device=dev)
    if "var_u" in want:
        out["var_u"] = torch.empty((Bt, N, m), dtype=f32, device=dev)
    if "excess" in want:
        out["excess"] = torch.empty((Bt,), dtype=torch.float64, device=dev)
    # the cost fields of the model, the integrator and phys of the plant
    p = (model if plant is None else model.with_(integrator=plant.integrator, phys=tuple(plant.phys))).c_params()
    check(_lib.load_for(model).quattro_track_covariance_f32(
        ctypes.byref(p), _ptr(x), _ptr(u), Bt, N, S, _ptr(K), _ptr(pphys), _ptr(cost_rows), _ptr(c0), _ptr(w),
        _lib.SCORE_TERMINAL if terminal else 0, _ptr(out.get("cov")), _ptr(out.get("var")), _ptr(out.get("var_u")),
        _ptr(out.get("excess")), _stream()), "quattro_track_covariance_f32")
    return out


TRACK_ESTIMATE_WANTS = ("xhat", "var", "cov", "nis")


def check_observed(model, observed):
    """The observed state indices of a selection sensor -> a tuple of ints: 1 <= p_y <= n of them, in 0 .. n - 1, ascending and
    distinct.  ValueError otherwise; host logic only."""
    try:
        arr = np.asarray(observed)
        ok = arr.ndim == 1 and 1 <= arr.size <= model.n and np.issubdtype(arr.dtype, np.integer)
    except Exception:
        ok = False
    if not ok:
        raise ValueError(f"observed must be 1..{model.n} integer state indices (got {observed!r})")
    obs = tuple(int(v) for v in arr)
    if obs[0] < 0 or obs[-1] >= model.n or any(b <= a for a, b in zip(obs, obs[1:])):
        raise ValueError(f"observed must be ascending, distinct indices in 0..{model.n - 1} (got {obs})")
    return obs


def check_meas_var(meas_var, B, p_y):
    """The measurement variances of a selection sensor, (p_y,) for every trajectory or (B, p_y) -- a 2-D (B, p_y) is per trajectory,
    also where B = 1 -- every one of them finite and > 0 (the VALUES are looked at, on the host).  -> float32 numpy array.
    ValueError otherwise."""
    if isinstance(meas_var, torch.Tensor):
        if not meas_var.is_floating_point():
            raise ValueError(f"meas_var must be floating point (got {meas_var.dtype})")
        meas_var = meas_var.detach().cpu().numpy()
    try:
        arr = np.asarray(meas_var, dtype=np.float64)
    except Exception:
        raise ValueError(f"meas_var must be numbers of shape {(p_y,)} or {(B, p_y)}") from None
    if arr.shape not in ((p_y,), (B, p_y)):
        raise ValueError(f"meas_var must have shape {(p_y,)} or {(B, p_y)} (got {arr.shape})")
    with np.errstate(over="ignore", under="ignore"):
        a32 = arr.astype(np.float32)
    if not (np.all(np.isfinite(arr)) and np.all(arr > 0.0) and np.all(a32 > 0.0) and np.all(np.isfinite(a32))):
        raise ValueError("meas_var must be finite and > 0 (in float32 too): a noiseless sensor makes the innovation variance singular")
    return np.ascontiguousarray(arr, dtype=np.float32)


def track_estimate(model, x0, x_nom, u_nom, K, steps, observed, meas_var, xhat0=None, cov0=None, noise=None, meas_noise=None,
                   disturbance=None, plant=None, plant_phys=None, model_phys=None, want=("xhat", "var", "nis")):
    """Output feedback on the device (quattro_track_estimate_f32): `steps` <= N steps of ops.track's gain law acting on the ESTIMATE
    of an extended Kalman filter that runs inside the same launch, behind a sensor that measures the states `observed`.  Per
    trajectory b, with f_plant the plant's step (plant / plant_phys as ops.track takes them) and f_model the estimator's (the model's
    integrator and phys, or row b of model_phys):
        x_0 = x0[b],  xh = xhat0[b] (None: x0[b]),  P = cov0[b] (None: 0);  for t = 0 .. steps - 1:
        measure   y_i = x_t[observed[i]] + meas_noise[t, b, i]                  (None: 0)
        update    for i in order, j = observed[i]:  g = P[:, j],  s = P[j][j] + meas_var[b][i],  e = y_i - xh[j],
                  nis_t += e^2 / s,  xh += g e / s,  P -= g g^T / s
        control   u_t = u_nom_t + K_t (xh - x_nom_t)                            (xh AFTER the update)
        plant     x_{t+1} = f_plant(x_t, u_t) + disturbance[t, b]               (None: 0)
        predict   A = df_model/dx at (xh, u_t),  xh <- f_model(xh, u_t),  P <- A P A^T + noise[b]      (None: 0)
    A selection sensor with independent noise: the scalar updates in sequence are exactly the batch Kalman update.
    x0 (B, n), x_nom (B, N+1, n), u_nom (B, N, m), K (B, N, m, n): float32 device tensors, as ops.track takes them.  observed: 1..n
    state indices, ascending and distinct, shared by the batch.  meas_var: (p_y,) or (B, p_y), finite and > 0 (checked on the host).
    xhat0 (B, n) float32 device tensor.  cov0, noise: the forms ops.track_covariance takes (check_cov_rows); symmetric positive
    semi-definite is the CALLER's responsibility, and P is read as symmetric.  meas_noise (steps, B, p_y), disturbance (steps, B, n):
    float32 device tensors, the realised noises.
    -> dict of float32 device tensors: "x" (B, steps+1, n) and "u" (B, steps, m) always, and by `want`: "xhat" (B, steps+1, n) (row
    t < steps the updated estimate the control of step t used, row `steps` the last prediction), "var" (B, steps+1, n) the diagonal
    of the same P (the same bits as "cov"), "cov" (B, steps+1, n, n) (symmetric to round-off only), "nis" (B, steps) the normalised
    innovation squared, whose mean sits near p_y for a consistent filter.
    The plant's step and the estimator's are one statement of the dynamics: a perfectly informed estimator (xhat0 None, no
    meas_noise, the plant equal to the model) returns xhat[:, :steps] == x[:, :steps] bit for bit and nis of +0.0.
    The built-in models only: NotImplementedError for a user-compiled model, before its library is loaded.  ValueError for a wrong
    shape, dtype or value, or an unknown entry of `want`, before anything touches the device."""
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in want if w not in TRACK_ESTIMATE_WANTS]
    if unknown:
        raise ValueError(f"want may name {list(TRACK_ESTIMATE_WANTS)} (got {list(want)})")
    if len(np.shape(u_nom)) != 3:
        raise ValueError(f"u_nom must have shape (B, N, m) (got {tuple(np.shape(u_nom))})")
    Bt, N, m = (int(v) for v in u_nom.shape)
    n = model.n
    if Bt < 1 or N < 1 or m != model.m:
        raise ValueError(f"u_nom must have shape (B, N, {model.m}) with B, N >= 1 (got {tuple(u_nom.shape)})")
    steps = int(steps)
    if not 1 <= steps <= N:
        raise ValueError("steps must be in 1..N")
    for name, t, shape in (("x0", x0, (Bt, n)), ("x_nom", x_nom, (Bt, N + 1, n)), ("K", K, (Bt, N, m, n))):
        if tuple(np.shape(t)) != shape:
            raise ValueError(f"{name} must have shape {shape} (got {tuple(np.shape(t))})")
    obs = check_observed(model, observed)
    p_y = len(obs)
    mv = check_meas_var(meas_var, Bt, p_y)
    for name, t, shape in (("xhat0", xhat0, (Bt, n)), ("meas_noise", meas_noise, (steps, Bt, p_y)),
                           ("disturbance", disturbance, (steps, Bt, n))):
        if t is not None and tuple(np.shape(t)) != shape:
            raise ValueError(f"{name} must have shape {shape} (got {tuple(np.shape(t))})")
    check_cov_rows(model, cov0, Bt, "cov0")
    check_cov_rows(model, noise, Bt, "noise")
    check_plant(model, plant)
    check_phys_rows(model, plant_phys, Bt, "plant_phys")
    check_phys_rows(model, model_phys, Bt, "model_phys")
    if model.model_id == _lib.MODEL_USER:
        raise NotImplementedError("track_estimate runs only for the built-in models")
    f32 = torch.float32
    _req(x0, (Bt, n), f32, "x0"); _req(x_nom, (Bt, N + 1, n), f32, "x_nom"); _req(u_nom, (Bt, N, m), f32, "u_nom")
    _req(K, (Bt, N, m, n), f32, "K")
    if xhat0 is not None:
        _req(xhat0, (Bt, n), f32, "xhat0")
    if meas_noise is not None:
        _req(meas_noise, (steps, Bt, p_y), f32, "meas_noise")
    if disturbance is not None:
        _req(disturbance, (steps, Bt, n), f32, "disturbance")
    dev = u_nom.device
    pphys = plant_phys_tensor(model, plant_phys, Bt, dev)
    mphys = model_phys_tensor(model, model_phys, Bt, dev)
    c0 = cov_rows_tensor(model, cov0, Bt, dev, "cov0")
    w = cov_rows_tensor(model, noise, Bt, dev, "noise")
    mvt = torch.as_tensor(mv, device=dev)
    out = {"x": torch.empty((Bt, steps + 1, n), dtype=f32, device=dev), "u": torch.empty((Bt, steps, m), dtype=f32, device=dev)}
    if "xhat" in want:
        out["xhat"] = torch.empty((Bt, steps + 1, n), dtype=f32, device=dev)
    if "var" in want:
        out["var"] = torch.empty((Bt, steps + 1, n), dtype=f32, device=dev)
    if "cov" in want:
        out["cov"] = torch.empty((Bt, steps + 1, n, n), dtype=f32, device=dev)
    if "nis" in want:
        out["nis"] = torch.empty((Bt, steps), dtype=f32, device=dev)
    p = model.c_params()
    pp = None if plant is None else plant.c_params()
    obs_c = (ctypes.c_int32 * p_y)(*obs)
    check(_lib.load_for(model).quattro_track_estimate_f32(
        ctypes.byref(p), None if pp is None else ctypes.byref(pp), _ptr(x0), _ptr(x_nom), _ptr(u_nom), _ptr(K), Bt, N, steps, obs_c,
        p_y, _ptr(mvt), 1 if mv.ndim == 2 else 0, _ptr(xhat0), _ptr(c0), _ptr(w), _ptr(meas_noise), _ptr(disturbance), _ptr(pphys),
        _ptr(mphys), _ptr(out["x"]), _ptr(out["u"]), _ptr(out.get("xhat")), _ptr(out.get("var")), _ptr(out.get("cov")),
        _ptr(out.get("nis")), _stream()), "quattro_track_estimate_f32")
    return out


ESTIMATE_LOG_FILTER_WANTS = ("xhat", "var", "cov", "innov", "innov_var", "nis", "loglik")
ESTIMATE_LOG_SMOOTH_WANTS = ("xs", "var_s", "cov_s")


def estimate_log(model, y, u, observed, meas_var, xhat0, cov0=None, noise=None, model_phys=None, smooth=False,
                 want=("xhat", "var", "nis", "loglik")):
    """A LOGGED run filtered and smoothed on the device (quattro_estimate_log_f32): ops.track_estimate's extended Kalman filter over
    sensor readings and controls that are inputs, its log-likelihood, and the fixed-interval smoother.  Nothing here steps a plant or
    forms a control.  Per trajectory b, f the model's step (its integrator and phys, or row b of model_phys), S the number of logged
    controls; a NaN in y is "no reading of that sensor at that step" (dropouts, slow sensors, a log without a final reading):
        xh = xhat0[b],  P = cov0[b] (None: 0);  for t = 0 .. S:
        update    for i in order, j = observed[i], only where y_t[i] is not NaN:  g = P[:, j],  s = P[j][j] + meas_var[b][i],
                  e = y_t[i] - xh[j],  innov[t][i] = e,  innov_var[t][i] = s,  nis_t += e^2 / s,  xh += g e / s,  P -= g g^T / s
                  (a missing reading: innov = innov_var = NaN, xh and P untouched bit for bit, nothing added to nis_t)
        record    xhat[t] = xh,  cov[t] = P,  var[t] = diag P                   (the posterior of step t)
        predict   (t < S)  A_t = df/dx at (xh, u_t),  xh <- f(xh, u_t),  P <- A_t P A_t^T + noise[b]      (None: 0)
        loglik[b] = -1/2 sum_t sum_i (ln(2 pi s) + e^2 / s) over the readings that exist, summed in fp64 in step and sensor order
    smooth=True adds the modified Bryson-Frazier smoother (in exact arithmetic the extended Rauch-Tung-Striebel smoother about the
    filter's linearisation points), r and Lambda zero after the last step, for t = S .. 0:
        xs[t] = xhat[t] + cov[t] r,   cov_s[t] = cov[t] - cov[t] Lambda cov[t],   var_s[t] = its diagonal
        for i in REVERSE order, the readings that exist, k = g / s of that update:  q = Lambda k,  c = k^T q,
                  rj = r[j] + e / s - k^T r,  Lambda[j][:] -= q^T,  Lambda[:, j] -= q,  Lambda[j][j] += c + 1 / s,  r[j] = rj
        (t > 0)   r <- A_{t-1}^T r,  Lambda <- A_{t-1}^T Lambda A_{t-1}
    y: (S+1, p_y) for one log shared by every hypothesis, or (B, S+1, p_y); u: (S, m) or (B, S, m); float32 device tensors.  B comes
    from whichever is 3-D, else from xhat0 (B, n), which is required: a log has no true state to default to.  observed, meas_var: as
    ops.track_estimate takes them (check_observed, check_meas_var).  cov0, noise: check_cov_rows' forms; symmetric positive
    semi-definite is the CALLER's responsibility, and P is read as symmetric.  model_phys: rows as ops.track_estimate takes them.
    -> dict of device tensors, by `want`: "xhat", "var" (B, S+1, n), "cov" (B, S+1, n, n), "innov", "innov_var" (B, S+1, p_y), "nis"
    (B, S+1) float32; "loglik" (B,) float64; with smooth=True also "xs", "var_s" (B, S+1, n), "cov_s" (B, S+1, n, n), of which "xs"
    and "var_s" are added to the default `want`.  var / var_s are the diagonals of cov / cov_s (the same bits); the filter's outputs do
    not depend on whether the smoother runs.  The workspace is a torch allocation sized by quattro_estimate_log_workspace_bytes.
    The built-in models only: NotImplementedError for a user-compiled model, before its library is loaded.  ValueError for a wrong
    shape, dtype or value, an unknown or empty `want`, or a smoothed entry of `want` without smooth=True, before anything touches the
    device."""
    smooth = bool(smooth)
    default = want is estimate_log.__defaults__[-1]
    want = (want,) if isinstance(want, str) else tuple(want)
    if default and smooth:
        want = want + ("xs", "var_s")
    known = ESTIMATE_LOG_FILTER_WANTS + ESTIMATE_LOG_SMOOTH_WANTS
    unknown = [w for w in want if w not in known]
    if unknown or not want:
        raise ValueError(f"want must name at least one of {list(known)} (got {list(want)})")
    if not smooth and any(w in ESTIMATE_LOG_SMOOTH_WANTS for w in want):
        raise ValueError(f"want names {[w for w in want if w in ESTIMATE_LOG_SMOOTH_WANTS]}, which need smooth=True")
    n, m = model.n, model.m
    obs = check_observed(model, observed)
    p_y = len(obs)
    yshape, ushape, hshape = tuple(np.shape(y)), tuple(np.shape(u)), tuple(np.shape(xhat0))
    if len(ushape) not in (2, 3) or ushape[-1] != m or ushape[-2] < 1:
        raise ValueError(f"u must have shape (S, {m}) or (B, S, {m}) with S >= 1 (got {ushape})")
    S = int(ushape[-2])
    if len(yshape) not in (2, 3) or yshape[-2:] != (S + 1, p_y):
        raise ValueError(f"y must have shape ({S + 1}, {p_y}) or (B, {S + 1}, {p_y}) (got {yshape})")
    if len(hshape) != 2 or hshape[1] != n or hshape[0] < 1:
        raise ValueError(f"xhat0 must have shape (B, {n}) with B >= 1 (got {hshape})")
    Bt = int(hshape[0])
    for name, shape in (("y", yshape), ("u", ushape)):
        if len(shape) == 3 and shape[0] != Bt:
            raise ValueError(f"{name} must have {Bt} trajectories, as xhat0 has (got {shape})")
    mv = check_meas_var(meas_var, Bt, p_y)
    check_cov_rows(model, cov0, Bt, "cov0")
    check_cov_rows(model, noise, Bt, "noise")
    check_phys_rows(model, model_phys, Bt, "model_phys")
    if model.model_id == _lib.MODEL_USER:
        raise NotImplementedError("estimate_log runs only for the built-in models")
    f32 = torch.float32
    for name, t in (("y", y), ("u", u), ("xhat0", xhat0)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a float32 device tensor (got {type(t).__name__})")
    _req(y, yshape, f32, "y"); _req(u, ushape, f32, "u"); _req(xhat0, (Bt, n), f32, "xhat0")
    dev = xhat0.device
    mphys = model_phys_tensor(model, model_phys, Bt, dev)
    c0 = cov_rows_tensor(model, cov0, Bt, dev, "cov0")
    w = cov_rows_tensor(model, noise, Bt, dev, "noise")
    mvt = torch.as_tensor(mv, device=dev)
    shapes = dict(xhat=(Bt, S + 1, n), var=(Bt, S + 1, n), cov=(Bt, S + 1, n, n), innov=(Bt, S + 1, p_y), innov_var=(Bt, S + 1, p_y),
                  nis=(Bt, S + 1), xs=(Bt, S + 1, n), var_s=(Bt, S + 1, n), cov_s=(Bt, S + 1, n, n))
    out = {k: torch.empty(shapes[k], dtype=f32, device=dev) for k in known if k in want and k != "loglik"}
    if "loglik" in want:
        out["loglik"] = torch.empty((Bt,), dtype=torch.float64, device=dev)
    p = model.c_params()
    lib = _lib.load_for(model)
    ws_bytes = int(lib.quattro_estimate_log_workspace_bytes(ctypes.byref(p), Bt, S, p_y, int(smooth)))
    ws = torch.empty(((ws_bytes + 15) // 16 * 4,), dtype=f32, device=dev)
    obs_c = (ctypes.c_int32 * p_y)(*obs)
    check(lib.quattro_estimate_log_f32(
        ctypes.byref(p), _ptr(y), 1 if len(yshape) == 3 else 0, _ptr(u), 1 if len(ushape) == 3 else 0, Bt, S, obs_c, p_y, _ptr(mvt),
        1 if mv.ndim == 2 else 0, _ptr(xhat0), _ptr(c0), _ptr(w), _ptr(mphys), _ptr(ws), ws_bytes, _ptr(out.get("xhat")),
        _ptr(out.get("var")), _ptr(out.get("cov")), _ptr(out.get("innov")), _ptr(out.get("innov_var")), _ptr(out.get("nis")),
        _ptr(out.get("loglik")), _ptr(out.get("xs")), _ptr(out.get("var_s")), _ptr(out.get("cov_s")), _stream()),
        "quattro_estimate_log_f32")
    return out


def _mpc_args(model, x_cur, x_nom, u_nom, K, k, cost, tol, max_iter, n_steps, workspace, traj_x, traj_u, traj_iters, disturbance,
              alphas, reg, alpha_idx, active, iters, status):
    """-> (the arguments the three MPC entries share, in the order of quattro_mpc_run_f32 without its stream; what they point to,
    to be kept until the call has returned)."""
    Bt, N, _ = u_nom.shape
    arr, na = _alphas(alphas)
    p = model.c_params()
    return (ctypes.byref(p), _ptr(x_cur), _ptr(x_nom), _ptr(u_nom), Bt, N, float(reg), arr, na, float(tol), int(max_iter),
            int(n_steps), _ptr(traj_x), _ptr(traj_u), _ptr(traj_iters), _ptr(disturbance), _ptr(K), _ptr(k), _ptr(cost),
            _ptr(alpha_idx), _ptr(active), _ptr(iters), _ptr(status), _ptr(workspace),
            workspace.numel() * workspace.element_size()), (p, arr)


def mpc_run(model, x_cur, x_nom, u_nom, K, k, cost, tol, max_iter, n_steps, workspace, traj_x, traj_u, traj_iters,
            disturbance=None, alphas=ALPHAS, reg=QUU_REG, alpha_idx=None, active=None, iters=None, status=None,
            plant=None, plant_phys=None, hold=1, feedback=False, model_phys=None, x_ref_rows=None, preview=True, cost_rows=None):
    """B controllers x n_steps control steps (solve -> apply u_0 -> shift the warm start) in ONE launch
    (quattro_mpc_run_f32); x_cur and u_nom advance in place, the closed-loop record goes to traj_x / traj_u / traj_iters.
    plant / plant_phys / hold / feedback (any of them off its default: quattro_mpc_run_plant_f32): n_steps PLANT steps, a solve
    every `hold` of them and the gain law of track() in between, on a plant of its own; traj_iters is then (B, n_steps / hold).
    model_phys (as in ilqr_solve; quattro_mpc_run_phys_f32, the plant entry's arguments and these rows): controller b plans with
    row b for its model's phys, and its plant is plant_phys[b], else plant.phys, else that same row.
    x_ref_rows (as in ilqr_solve; quattro_mpc_run_ref_f32, the phys entry's arguments, these rows and preview): horizon step t of the
    plan that starts at plant step s takes its cost against row min(s + preview * t, R - 1) of controller b's rows — preview=True
    looks along the rows over the horizon, preview=False holds the row of the replan step for the whole solve.
    cost_rows (as in ilqr_solve; quattro_mpc_run_cost_f32, the ref entry's arguments and these rows): controller b plans with row b
    for its q, qf and r, in every solve of the run."""
    Bt, N, m = u_nom.shape
    n = model.n
    f32, i32 = torch.float32, torch.int32
    hold = int(hold)
    check_phys_rows(model, model_phys, Bt, "model_phys")
    check_ref_rows(model, x_ref_rows, Bt, name="x_ref_rows")
    check_cost_rows(model, cost_rows, Bt, name="cost_rows")
    plain = (plant is None and plant_phys is None and hold == 1 and not feedback and model_phys is None and x_ref_rows is None
             and cost_rows is None)
    if hold < 1 or n_steps % hold != 0:
        raise ValueError("n_steps must be a multiple of hold >= 1")
    _req(x_cur, (Bt, n), f32, "x_cur"); _req(x_nom, (Bt, N + 1, n), f32, "x_nom"); _req(u_nom, (Bt, N, model.m), f32, "u_nom")
    _req(K, (Bt, N, m, n), f32, "K"); _req(k, (Bt, N, m), f32, "k"); _req(cost, (Bt,), torch.float64, "cost")
    _req(alpha_idx, (Bt,), i32, "alpha_idx"); _req(active, (Bt,), i32, "active"); _req(iters, (Bt,), i32, "iters")
    _req(traj_x, (Bt, n_steps + 1, n), f32, "traj_x"); _req(traj_u, (Bt, n_steps, m), f32, "traj_u")
    _req(traj_iters, (Bt, n_steps // hold), i32, "traj_iters")
    if status is not None:
        _req(status, (Bt,), i32, "status")
    if disturbance is not None:
        _req(disturbance, (n_steps, Bt, n), f32, "disturbance")
    head, keep = _mpc_args(model, x_cur, x_nom, u_nom, K, k, cost, tol, max_iter, n_steps, workspace, traj_x, traj_u, traj_iters,
                           disturbance, alphas, reg, alpha_idx, active, iters, status)
    if plain:
        check(_lib.load_for(model).quattro_mpc_run_f32(*head, _stream()), "quattro_mpc_run_f32")
        return
    check_plant(model, plant)
    pp = None if plant is None else plant.c_params()
    pref = None if pp is None else ctypes.byref(pp)
    pphys = plant_phys_tensor(model, plant_phys, Bt, u_nom.device)
    model_phys = model_phys_tensor(model, model_phys, Bt, u_nom.device)
    if cost_rows is not None:
        x_ref_rows = x_ref_rows_tensor(model, x_ref_rows, Bt, u_nom.device, name="x_ref_rows")
        cost_rows = cost_rows_tensor(model, cost_rows, Bt, u_nom.device, name="cost_rows")
        check(_lib.load_for(model).quattro_mpc_run_cost_f32(*head, pref, _ptr(pphys), hold, int(bool(feedback)), _ptr(model_phys),
                                                            _ptr(x_ref_rows), 0 if x_ref_rows is None else x_ref_rows.shape[1],
                                                            int(bool(preview)), _ptr(cost_rows), _stream()),
              "quattro_mpc_run_cost_f32")
        return
    if x_ref_rows is not None:
        x_ref_rows = x_ref_rows_tensor(model, x_ref_rows, Bt, u_nom.device, name="x_ref_rows")
        check(_lib.load_for(model).quattro_mpc_run_ref_f32(*head, pref, _ptr(pphys), hold, int(bool(feedback)), _ptr(model_phys),
                                                           _ptr(x_ref_rows), x_ref_rows.shape[1], int(bool(preview)), _stream()),
              "quattro_mpc_run_ref_f32")
        return
    if model_phys is not None:
        check(_lib.load_for(model).quattro_mpc_run_phys_f32(*head, pref, _ptr(pphys), hold, int(bool(feedback)), _ptr(model_phys),
                                                            _stream()), "quattro_mpc_run_phys_f32")
        return
    check(_lib.load_for(model).quattro_mpc_run_plant_f32(*head, pref, _ptr(pphys), hold, int(bool(feedback)), _stream()),
          "quattro_mpc_run_plant_f32")
