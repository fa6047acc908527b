"""User-supplied device models: any problem the reference's callable interface admits, on the GPU.

The reference's iLQR_TF takes arbitrary Python callables f, L, Lf (quattro_ilqr_tf/quattro_ilqr_tf.py:66-84) and
differentiates them by finite differences (:149-275).  A kernel cannot call Python and this package has no CPU path, so
a problem other than the two shipped ones is written as three short C++ bodies over a scalar type `T` and compiled —
hipcc, gfx950, a few seconds, cached by content — together with the generic kernels of csrc/ (ROWMAJOR records, the
pivoting sweep, one lane per line-search candidate) into a small library that exports the same C ABI
(include/quattro_hip.h) with the problem built in as QUATTRO_MODEL_USER.  Derivatives are exact: forward-mode
differentiation through the whole integrator step and second-order duals for the cost (csrc/dual.h, csrc/user_model.h).

    pendulum = compile_model(
        "pendulum", n=2, m=1, dt=0.02, integrator="rk4", phys=(9.81, 1.0),          # P[0] = g, P[1] = l
        rate="xd[0] = x[1];  xd[1] = -(P[0] / P[1]) * sin(x[0]) + u[0];",
        q=(1.0, 0.1), r=(0.01,), qf=(50.0, 5.0), x_ref=(3.14159, 0.0))             # default diagonal cost
    out = QuattroILQR(pendulum, horizon=50).solve(x0_batch)                          # or iLQR_TF(..., model=pendulum)

Inside the bodies: `x`, `u` (arrays of T), `xd` (rate only, to be filled), `p` (quattro_model_params), `P` = p.phys,
`NX`, `NU`, and sin cos tan sincos exp log sqrt tanh atan pow(x, const) fabs abs fmax fmin square softplus(z, beta) for every T;
`default_stage_cost<T>(p, x, u)` / `default_final_cost<T>(p, x)` are the built-in diagonal forms.  `+ - * /`, unary `-` / `+`
and `+= -= *= /=` take a T or a plain number (int, float or double literal) on either side; so do fmax / fmin
(`fmax(x[0], 0.0f)`; a tie takes the first argument) and the comparisons `< > <= >= == !=`, which look at the value only
(`primal(v)` is that value as a float): a branch differentiates the side that is taken, fabs(0) is +x.  pow(x, e) is
finite at x = 0 wherever the mathematical derivative is (e = 0, 1, 2, ...).  Each of these is checked on the device against
fp64 derivatives at all three instantiations (tests/test_dual_algebra_gpu.py; tests/test_dual_host_cpu.py on the host).
`helpers` is pasted in front (function templates of your own, constants).

compile_model(..., param_grad=True) builds a library whose quattro_cost_param_gradient_f32 (ops.cost_param_gradient, the row gradients
of autograd.trajectory_cost) runs for this model: the three bodies are then also instantiated over a parameter block whose `phys`,
`q`, `qf`, `r` and `x_ref` are dual numbers (csrc/user_param_gradient.hip).  The rule for the bodies of such a model: a local that
holds a parameter or a weight is declared `T` or `auto`, not `float` -- inside the gradient kernel `P[k]`, `p.q[i]`, `p.qf[i]`,
`p.r[a]` and `p.x_ref[i]` have type `T`; `p.dt` and `p.barrier_*` stay `float` and are not differentiated.  A body that breaks the
rule (`const float mass = P[0];`) does not compile with param_grad=True: QuattroError with the compiler's message and the rule.
Without the keyword nothing changes: the same generated text, units and flags as before, and the entry answers
QUATTRO_ERR_UNSUPPORTED.

The reference's `dynamics` argument is a discrete map x_next = f(x, u); here the model is the continuous rate plus the
integrator the reference's own problems use (explicit Euler or RK4 with zero-order hold).  A map that is only available in
discrete form is `integrator="euler", dt=1.0` with `rate` = f(x, u) - x.
"""
import hashlib
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np

from . import _lib
from .models import DeviceModel

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
def _default_cache_dir():
    """In-tree (next to libquattro_hip.so: a model compiled in one container travels with the tree) when the package directory
    can be written, a per-user directory otherwise (an installed, read-only package)."""
    local = os.path.join(_HERE, "_user_models")
    if os.path.isdir(local) and os.access(local, os.W_OK) or (not os.path.exists(local) and os.access(_HERE, os.W_OK)):
        return local
    return os.path.join(os.path.expanduser("~"), ".cache", "quattro_ilqr_amd", "user_models")


CACHE_DIR = os.environ.get("QUATTRO_USER_MODEL_DIR") or _default_cache_dir()
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the translation units that know about models without being tied to one of the built-in kernels; everything else
# (the quadrotor / cart-pole specialisations, the transformer) is resolved from libquattro_hip.so
# (no implicit fma contraction anywhere in a user library: its device-resident loop, solve_user.hip, inlines the same device
#  functions as the stand-alone kernels and must round like them to reproduce the host-driven loop bit for bit)
_UNITS = {u: ["-ffp-contract=off"] for u in ("capi", "linearize", "rollout", "cost_gradient", "sweep_generic", "solve_user")}
_UNITS["solve_user"] = _UNITS["solve_user"] + ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]      # (the tile sweep's accumulators: Makefile)
# the unit of the tracked closed-loop cost's gradient (quattro_track_gradient_f32): in every library like the ones above, named on its
# own because the six entries of _UNITS are held fixed by a test of the plain build list
_TRACK_UNIT = "track_gradient"


def _all_units():
    """Every translation unit of a plain user-model library with its flags."""
    return {**_UNITS, _TRACK_UNIT: ["-ffp-contract=off"]}


# the unit of compile_model(..., param_grad=True) alone (kept out of _UNITS: a plain library is built from the same units as ever)
_PARAM_GRAD_UNIT = "user_param_gradient"
_PARAM_GRAD_RULE = ("param_grad=True: a local that holds a parameter or a weight (P[k], p.q[i], p.qf[i], p.r[a], p.x_ref[i]) must be "
                    "declared T or auto, not float; p.dt and p.barrier_* stay float")
_FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-fno-slp-vectorize"]   # (csrc/Makefile)


@dataclass(frozen=True)
class UserDeviceModel(DeviceModel):
    lib_path: str = ""          # the library that holds this model's kernels (ops load it instead of libquattro_hip.so)
    source: str = ""            # the generated header, for the record
    param_grad: bool = False    # built with param_grad=True: the library's quattro_cost_param_gradient_f32 runs for this model


def _header(name, rate, stage_cost, final_cost, helpers, param_grad=False):
    def body(src, default):
        src = default if src is None else src
        return "\n".join("  " + ln for ln in src.strip().splitlines())
    if param_grad:
        # the same three bodies, generic over the parameter block too: with PB = quattro_model_params these are the functions below
        return f"""// generated by quattro_ilqr_amd.user_model.compile_model(param_grad=True) for model "{name}" (included inside namespace qt_user, csrc/user_model.h)
{helpers.strip()}
template <class T, class PB = quattro_model_params>
__device__ __forceinline__ void rate(const PB& p, const T* x, const T* u, T* xd) {{
  const auto* P = p.phys;
  (void)P;
{body(rate, None)}
}}
template <class T, class PB = quattro_model_params>
__device__ __forceinline__ T stage_cost(const PB& p, const T* x, const T* u) {{
  const auto* P = p.phys;
  (void)P;
{body(stage_cost, "return default_stage_cost<T>(p, x, u);")}
}}
template <class T, class PB = quattro_model_params>
__device__ __forceinline__ T final_cost(const PB& p, const T* x) {{
  const auto* P = p.phys;
  (void)P;
{body(final_cost, "return default_final_cost<T>(p, x);")}
}}
"""
    return f"""// generated by quattro_ilqr_amd.user_model.compile_model for model "{name}" (included inside namespace qt_user, csrc/user_model.h)
{helpers.strip()}
template <class T>
__device__ __forceinline__ void rate(const quattro_model_params& p, const T* x, const T* u, T* xd) {{
  const float* P = p.phys;
  (void)P;
{body(rate, None)}
}}
template <class T>
__device__ __forceinline__ T stage_cost(const quattro_model_params& p, const T* x, const T* u) {{
  const float* P = p.phys;
  (void)P;
{body(stage_cost, "return default_stage_cost<T>(p, x, u);")}
}}
template <class T>
__device__ __forceinline__ T final_cost(const quattro_model_params& p, const T* x) {{
  const float* P = p.phys;
  (void)P;
{body(final_cost, "return default_final_cost<T>(p, x);")}
}}
"""


_TOOLCHAIN = None


def _toolchain_id():
    """What else a compiled library depends on besides its sources: the compiler, the flags of every unit, and the ABI of the
    libquattro_hip.so it links against (a flag change or a rebuilt main library must not reuse a stale model library)."""
    global _TOOLCHAIN
    if _TOOLCHAIN is None:
        try:
            ver = subprocess.run([HIPCC, "--version"], capture_output=True, text=True, timeout=60).stdout
        except (OSError, subprocess.SubprocessError):
            ver = "no hipcc"
        try:
            abi = str(_lib.load().quattro_version())
        except Exception:           # (the main library is missing: build_library says so itself)
            abi = "no main library"
        _TOOLCHAIN = hashlib.sha1(f"{ver}\n{_FLAGS}\n{sorted(_all_units().items())}\n{abi}".encode()).hexdigest()
    return _TOOLCHAIN


def _sources_digest(param_grad=False):
    """Digest of every source a model library is built from, or None when the sources are not there (an installed package that
    ships only built libraries: a cached model library is then found by its header alone)."""
    if not os.path.isdir(CSRC):
        return None
    h = hashlib.sha1()
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".h", ".hip")) and (fn.endswith(".h") or fn[:-4] in _all_units() or (param_grad and fn[:-4] == _PARAM_GRAD_UNIT)):
            with open(os.path.join(CSRC, fn), "rb") as f:
                h.update(fn.encode()); h.update(f.read())
    with open(os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "quattro_hip.h"), "rb") as f:
        h.update(f.read())
    return h.hexdigest()


def _find_by_header(safe, n, m, header_text):
    """A cached library whose generated header is this one (used only when the kernel sources are absent)."""
    want = hashlib.sha1(f"{n},{m}\n{header_text}".encode()).hexdigest()
    if not os.path.isdir(CACHE_DIR):
        return None
    for d in sorted(os.listdir(CACHE_DIR)):
        so, tag = os.path.join(CACHE_DIR, d, "libquattro_user.so"), os.path.join(CACHE_DIR, d, "header.sha1")
        if d.startswith(safe + "_") and os.path.exists(so) and os.path.exists(tag):
            with open(tag) as f:
                if f.read().strip() == want:
                    return so
    return None


def build_library(name, n, m, header_text, verbose=False, param_grad=None):
    """Compile (or find in the cache) the library of one user model -> path of its .so.  param_grad: None, or the number of free
    parameters of a model built with compile_model(..., param_grad=True)."""
    if not (1 <= n <= _lib.MAX_NX and 1 <= m <= _lib.MAX_NU):
        raise ValueError(f"user model dims (n, m) = ({n}, {m}) outside 1..{_lib.MAX_NX} x 1..{_lib.MAX_NU}")
    safe = "".join(c if c.isalnum() or c == "_" else "_" for c in name) or "model"
    digest = _sources_digest(param_grad is not None)
    if digest is None:
        so = _find_by_header(safe, n, m, header_text)
        if so is None:
            raise _lib.QuattroError(f"user model {name!r}: no cached library and no kernel sources at {CSRC} to build one from")
        return so
    units = _all_units()
    defs_pg = []
    if param_grad is not None:
        units[_PARAM_GRAD_UNIT] = ["-ffp-contract=off"]
        defs_pg = ["-DQT_USER_PARAM_GRAD=1", f"-DQT_USER_NP={int(param_grad)}"]
    key = hashlib.sha1(f"{n},{m}\n{header_text}\n{digest}\n{_toolchain_id()}{''.join(defs_pg)}".encode()).hexdigest()[:16]
    out_dir = os.path.join(CACHE_DIR, f"{safe}_{key}")
    so = os.path.join(out_dir, "libquattro_user.so")
    if os.path.exists(so):
        return so
    if not os.path.exists(_lib.LIB_PATH):
        raise _lib.QuattroError(f"{_lib.LIB_NAME} must be built before a user model (python __graft_entry__.py)")
    os.makedirs(out_dir, exist_ok=True)
    # everything is built in a directory private to this process and only the finished library is moved into place (atomic
    # rename): ranks of one job compiling the same model at the same time never see each other's half-written files
    work = os.path.join(out_dir, f".build_{os.getpid()}")
    os.makedirs(work, exist_ok=True)
    hdr = os.path.join(work, "model.h")
    with open(hdr, "w") as f:
        f.write(header_text)
    defs = [f'-DQT_USER_MODEL_HEADER="{hdr}"', f"-DQT_USER_NX={n}", f"-DQT_USER_NU={m}", *defs_pg]

    def compile_unit(unit):
        obj = os.path.join(work, unit + ".o")
        cmd = [HIPCC, *_FLAGS, *defs, *units[unit], "-c", os.path.join(CSRC, unit + ".hip"), "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
        if verbose and r.stderr:
            print(r.stderr)
        if r.returncode != 0:
            rule = f"\n{_PARAM_GRAD_RULE}" if unit == _PARAM_GRAD_UNIT else ""
            raise _lib.QuattroError(f"user model {name!r} does not compile ({unit}.hip):\n{r.stderr[-4000:]}{rule}")
        return obj

    try:
        with ThreadPoolExecutor(max_workers=len(units)) as ex:
            objs = list(ex.map(compile_unit, units))
        tmp = os.path.join(work, "libquattro_user.so")
        rel = os.path.relpath(_HERE, out_dir)
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", tmp, f"-L{_HERE}", "-lquattro_hip",
               f"-Wl,-rpath,$ORIGIN/{rel}", "-Wl,-Bsymbolic"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise _lib.QuattroError(f"user model {name!r} does not link:\n{r.stderr[-4000:]}")
        with open(os.path.join(out_dir, "model.h"), "w") as f:      # for the record (not read again)
            f.write(header_text)
        with open(os.path.join(out_dir, "header.sha1"), "w") as f:  # lets a source-less installation find this library
            f.write(hashlib.sha1(f"{n},{m}\n{header_text}".encode()).hexdigest())
        os.replace(tmp, so)
    finally:
        shutil.rmtree(work, ignore_errors=True)
        if not os.path.exists(so):
            try:
                os.rmdir(out_dir)                    # a failed build leaves nothing behind
            except OSError:
                pass
    return so


def compile_model(name, n, m, rate, stage_cost=None, final_cost=None, *, dt=0.01, integrator="euler", x_ref=None,
                  q=None, r=None, qf=None, phys=(), barrier_alpha=0.0, barrier_beta=1.0, helpers="", verbose=False, param_grad=False):
    """-> UserDeviceModel usable wherever a built-in DeviceModel is (QuattroILQR, iLQR_TF(model=...), BatchedMPC, ops.*).

    rate / stage_cost / final_cost: C++ statement bodies (see the module docstring); stage_cost / final_cost None = the
    diagonal quadratic (+ softplus barrier) of include/quattro_hip.h over q, r, qf, x_ref, barrier_*.  The cost only needs
    Q_uu + reg I invertible along the trajectories solved, as the reference's np.linalg.inv (quattro_ilqr_tf.py:306) does:
    an indefinite block is swept with pivoting (the tile sweep flags it, every loop of the library re-sweeps it).
    param_grad=True: the library also holds the kernel of quattro_cost_param_gradient_f32 for this model (gradients of the trajectory
    cost with respect to phys, q / qf / r and the targets); the bodies must then obey the rule of the module docstring."""
    n, m = int(n), int(m)
    if len(phys) > 8:
        raise ValueError("at most 8 free parameters (phys)")
    param_grad = bool(param_grad)
    text = _header(name, rate, stage_cost, final_cost, helpers, param_grad)
    so = build_library(name, n, m, text, verbose=verbose, param_grad=len(phys) if param_grad else None)
    vec = lambda v, k, fill: tuple(float(fill) for _ in range(k)) if v is None else tuple(float(t) for t in np.asarray(v).reshape(-1))
    md = UserDeviceModel(name=name, model_id=_lib.MODEL_USER, n=n, m=m, dt=float(dt), integrator=integrator,
                         x_ref=vec(x_ref, n, 0.0), q=vec(q, n, 1.0), r=vec(r, m, 1.0), qf=vec(qf, n, 1.0),
                         barrier_alpha=float(barrier_alpha), barrier_beta=float(barrier_beta),
                         phys=tuple(float(v) for v in phys), lib_path=so, source=text, param_grad=param_grad)
    for fld, k in (("x_ref", n), ("q", n), ("qf", n), ("r", m)):
        if len(getattr(md, fld)) != k:
            raise ValueError(f"{fld} must have {k} entries")
    return md


def example_planar_model(integrator="rk4", dt=0.02, param_grad=False):
    """A problem the reference does not ship, used by bench.py and the docs: a planar two-rotor vehicle, state (px, pz, theta,
    vx, vz, omega), controls = the two rotor thrusts, phys = (mass, inertia, arm, gravity), diagonal cost about a hover
    point plus a cross term (so that l_xx is not diagonal)."""
    return compile_model(
        "planar_example", 6, 2, dt=dt, integrator=integrator, phys=(1.0, 0.05, 0.2, 9.81),
        rate="""T s, c;
sincos(x[2], &s, &c);
const T thrust = (u[0] + u[1]) / P[0];
xd[0] = x[3];  xd[1] = x[4];  xd[2] = x[5];
xd[3] = -(thrust * s);
xd[4] = thrust * c - P[3];
xd[5] = (u[0] - u[1]) * (P[2] / P[1]);""",
        stage_cost="return default_stage_cost<T>(p, x, u) + x[0] * x[2] * 0.3f;",
        q=(1.0, 1.0, 1.0, 0.1, 0.1, 0.1), r=(0.01, 0.01), qf=(10.0,) * 6, x_ref=(0.0, 1.0, 0.0, 0.0, 0.0, 0.0),
        param_grad=param_grad)
