"""Probe models for csrc/dual.h: every operator form and every elementary function a user model may call, written ONCE per
row as C++ text and as a Python function over a small math namespace, so that the same row gives

  * the device code (rate / stage cost / final cost bodies of a compile_model library, and a host driver for the CPU test),
  * exact fp64 references: sympy derivatives evaluated in mpmath (SymMath; a kinked function contributes the closed form of
    the branch taken at the point), and a complex-valued version for complex-step Jacobians of a whole integrator step
    (ComplexMath; branches on the real part),
  * an independent fp32 emulation of the textbook derivative formulas (numpy float32), from which the tolerances come.

Layout of a probe library (n states, m = 1): row k owns state slot ia (and ib = ia + 1 when it reads two states) and reads
u[0]; it reads nothing else, so every row is evaluated inside its own domain whatever the other rows do.

    rate:        xd[ia] = g_k(x[ia], x[ib], u[0])            (xd[ib] = 0 for an owned second slot)
    stage cost:  sum_k p.q[ia_k] g_k(...) + p.r[0] h(u[0])
    final cost:  sum_k p.qf[ia_k] g_k(x[ia], x[ib], P[0])    (P[0] = phys[0] stands in for u[0])

q, r, qf, phys, dt and the integrator are runtime parameters: a one-hot q isolates one row without recompiling.  A deselected
term is multiplied by 0, so every row's points must stay inside its domain (0 * NaN would leak).

The seeded random libraries use the overlapping form xd[i] = g_i(x[i], x[(i + 1) % n], u[0]) over total-domain forms only.

Errors are measured as |got - ref| / S, S = max(1, |value|, |gradient entries|, |Hessian entries|) of the reference jet (value,
first, second derivative) of that row at that point: the dual rules mix those entries, so an error relative to one entry
that cancels to something tiny means nothing.  Asserted tolerance: 8 x max(E_row, 2^-23) per row and derivative order, E_row
the worst error of the fp32 emulation on the points tested; the factor 8 is for device math functions that are allowed a few
ulp where the host's are within about 1 ulp.
"""
import os
import sys
from dataclasses import dataclass

import mpmath
import numpy as np
import sympy as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "quattro-transformer-ilqr_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DT = 0.01
WF = 0.75                                                   # phys[0]: what the final cost passes to a row as u[0]
W_ITEM = [0.75, -1.25, 0.5, 2.0, -0.375, 1.5, -2.0, 0.25]   # u[0] of main point p (shared by the rows of an item)
NPTS = len(W_ITEM)
EPS32 = 2.0 ** -23
FACTOR = 8.0
SOFTPLUS_VALUE_TOL = 2e-6                                   # csrc/models_device.h: hardware exp / log in qt_softplus
H_CPP, H_FN = "sin(u[0] * 0.5f)", (lambda M, w: M.sin(w * 0.5))     # the control term h(u[0]) (weight p.r[0]; total and bounded)

A_, B_, W_ = sp.symbols("a b w", real=True)


def f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------ math namespaces
class Sigmoid(sp.Function):
    def fdiff(self, argindex=1):
        return Sigmoid(self.args[0]) * (1 - Sigmoid(self.args[0]))


class Softplus(sp.Function):
    """softplus_beta(z) = log(1 + exp(beta z)) / beta; d/dz = sigmoid(beta z) (beta is a constant)."""

    def fdiff(self, argindex=1):
        if argindex != 1:
            raise ValueError("softplus: beta is a constant")
        return Sigmoid(self.args[1] * self.args[0])


class SymMath:
    """sympy expressions in (a, b, w).  Comparisons and the kinked functions look at the numeric point `at` and return the
    closed form of the branch the device takes there (fabs(0) = +x; a tie in fmax / fmin takes the first argument)."""

    def __init__(self, at):
        self.subs = dict(zip((A_, B_, W_), (sp.Float(float(v), 40) for v in at)))

    def val(self, e):
        return float(sp.sympify(e).evalf(30, subs=self.subs))

    sin, cos, tan, exp, log, sqrt, tanh, atan = (staticmethod(f) for f in (sp.sin, sp.cos, sp.tan, sp.exp, sp.log, sp.sqrt, sp.tanh, sp.atan))

    def sincos(self, x):
        return sp.sin(x), sp.cos(x)

    def pow(self, x, e):
        return x ** sp.nsimplify(e)

    def square(self, x):
        return x * x

    def softplus(self, z, beta):
        return Softplus(z, sp.nsimplify(beta))

    def fabs(self, x):
        return -x if self.val(x) < 0 else x

    def fmax(self, x, y):
        return x if self.val(x) >= self.val(y) else y

    def fmin(self, x, y):
        return x if self.val(x) <= self.val(y) else y

    def lt(self, x, y): return self.val(x) < self.val(y)
    def gt(self, x, y): return self.val(x) > self.val(y)
    def le(self, x, y): return self.val(x) <= self.val(y)
    def ge(self, x, y): return self.val(x) >= self.val(y)
    def eq(self, x, y): return self.val(x) == self.val(y)
    def ne(self, x, y): return self.val(x) != self.val(y)


class ComplexMath:
    """numpy complex128 for complex-step differentiation; every comparison branches on the real part."""
    sin, cos, tan, exp, log, sqrt, tanh, atan = (staticmethod(f) for f in (np.sin, np.cos, np.tan, np.exp, np.log, np.sqrt, np.tanh, np.arctan))

    def sincos(self, x):
        return np.sin(x), np.cos(x)

    def pow(self, x, e):
        return x ** int(e) if float(e).is_integer() else x ** e

    def square(self, x):
        return x * x

    def softplus(self, z, beta):
        bz = beta * z
        return (z + np.log1p(np.exp(-bz)) / beta) if np.real(bz) > 0 else np.log1p(np.exp(bz)) / beta

    def fabs(self, x):
        from test_user_model_gpu import cs_fabs
        return cs_fabs(x)

    def fmax(self, x, y):
        from test_user_model_gpu import cs_fmax
        return cs_fmax(x, y)

    def fmin(self, x, y):
        from test_user_model_gpu import cs_fmin
        return cs_fmin(x, y)

    def lt(self, x, y): return np.real(x) < np.real(y)
    def gt(self, x, y): return np.real(x) > np.real(y)
    def le(self, x, y): return np.real(x) <= np.real(y)
    def ge(self, x, y): return np.real(x) >= np.real(y)
    def eq(self, x, y): return np.real(x) == np.real(y)
    def ne(self, x, y): return np.real(x) != np.real(y)


def _mp_sigmoid(t):
    return 1 / (1 + mpmath.exp(-t))


def _mp_softplus(z, beta):
    bz = beta * z
    return (max(bz, 0) + mpmath.log1p(mpmath.exp(-abs(bz)))) / beta


def _np_sigmoid(t):
    t = np.asarray(t, dtype=np.float32)
    e = np.exp(-np.abs(t))
    return np.where(t >= 0, np.float32(1) / (np.float32(1) + e), e / (np.float32(1) + e)).astype(np.float32)


def _np_softplus(z, beta):
    bz = np.asarray(z, dtype=np.float32) * np.float32(beta)
    return ((np.maximum(bz, np.float32(0)) + np.log1p(np.exp(-np.abs(bz)))) / np.float32(beta)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ rows
@dataclass
class Row:
    name: str
    cpp: str                  # an expression, or a statement body that returns, over {a} {b} {w}
    fn: object                # fn(M, a, b, w) -> the same function through a math namespace
    a: list = None            # NPTS sample values of x[ia]
    b: list = None            # NPTS sample values of x[ib] (rows that read two states)
    ia: int = -1
    ib: int = -1
    k: int = -1

    @property
    def nx(self):
        return 1 if self.b is None else 2

    def point(self, p):
        return (f32(self.a[p]), f32(self.b[p]) if self.b is not None else 0.0, f32(W_ITEM[p]))

    def z_index(self, n):
        """Where (a, b, w) sit in z = (x, u) of an n-state library."""
        return (self.ia, self.ib if self.ib >= 0 else None, n)

    def helper(self):
        text = self.cpp.strip()
        if "return" not in text:
            text = f"return {text};"
        text = text.replace("{a}", f"x[{self.ia}]").replace("{b}", f"x[{self.ib}]").replace("{w}", "u[0]")
        body = "\n".join("  " + ln.strip() for ln in text.splitlines())
        return (f"template <class T>\n__device__ __forceinline__ T g{self.k}(const T* x, const T* u) {{   // {self.name}\n"
                f"{body}\n}}")


def _compound(M, a, b, w):
    g = a
    g = g + b
    g = g * w
    g = g - a * 0.5
    g = g / (b * b + 1.0)
    g = g + 1.5
    g = g - 2
    g = g * 3.0
    g = g / 4.0
    return g


def _sincos_mix(M, a, b, w):
    s, c = M.sincos(a)
    return s * b + c * w


_POS = [0.25, 1.7, 3.0, 0.4, 2.2, 0.9, 1.2, 4.0]
_ANY = [0.3, -0.9, 1.6, -2.2, 0.05, 2.8, -0.5, 1.1]
_ANY2 = [1.0, -2.0, 0.2, 3.0, -0.8, 2.4, -3.1, 0.6]

LIB_A = [
    Row("div", "{a} / {b}", lambda M, a, b, w: a / b,
        [1.5, -0.7, 0.3, 2.2, -1.9, 0.05, 1.0, -0.25], [0.8, -1.3, 2.5, 0.6, -0.5, 1.7, -2.4, 3.0]),
    Row("sin_over_cos", "sin({a}) / (cos({b}) + 2.0f)", lambda M, a, b, w: M.sin(a) / (M.cos(b) + 2.0),
        [0.3, -1.1, 2.0, 3.5, -2.7, 0.9, 5.0, -0.4], _ANY2),
    Row("pow3_u", "pow({a}, 3) * {w}", lambda M, a, b, w: M.pow(a, 3) * w, [1.2, -0.8, 0.4, -2.0, 1.7, -0.3, 2.3, 0.9]),
    Row("fmax2", "fmax({a}, {b})", lambda M, a, b, w: M.fmax(a, b),
        [1.5, -0.7, 0.3, 2.2, -1.9, 0.05, 1.0, -0.25], [0.8, -1.3, 2.5, 0.6, -0.5, 1.7, -2.4, 3.0]),
    Row("fmin2", "fmin({a}, {b})", lambda M, a, b, w: M.fmin(a, b),
        [1.5, -0.7, 0.3, 2.2, -1.9, 0.05, 1.0, -0.25], [0.8, -1.3, 2.5, 0.6, -0.5, 1.7, -2.4, 3.0]),
    Row("sqrt_norm", "sqrt({a} * {a} + {w} * {w} + 1.0f)", lambda M, a, b, w: M.sqrt(a * a + w * w + 1.0), _ANY),
    Row("tanh_atan", "tanh({a}) * atan({w})", lambda M, a, b, w: M.tanh(a) * M.atan(w), _ANY),
    Row("tan_u", "tan({a}) * {w}", lambda M, a, b, w: M.tan(a) * w, [0.4, -0.9, 1.1, -0.2, 0.7, -1.15, 0.05, 1.2]),
    Row("log_u", "log({a}) * {w}", lambda M, a, b, w: M.log(a) * w, [0.5, 1.7, 3.0, 0.3, 2.2, 0.9, 1.2, 4.0]),
    Row("exp_half", "exp({a} * 0.5f)", lambda M, a, b, w: M.exp(a * 0.5), _ANY),
    Row("cos_x", "cos({a}) * {a}", lambda M, a, b, w: M.cos(a) * a, _ANY2),
    Row("sqrt1", "sqrt({a})", lambda M, a, b, w: M.sqrt(a), _POS),
]

LIB_B = [
    Row("softplus2", "softplus({a}, 2.0f)", lambda M, a, b, w: M.softplus(a, 2.0), [0.3, -0.9, 1.6, -2.2, 0.05, 2.8, -0.5, 4.0]),
    Row("softplus40", "softplus({a} - {w}, 40.0f)", lambda M, a, b, w: M.softplus(a - w, 40.0),
        [wv + d for wv, d in zip(W_ITEM, [0.01, -0.02, 0.05, -0.1, 0.3, -0.5, 0.002, 1.0])]),
    Row("branch_gt", "({a} > 0.0f ? {a} * {a} * {b} : sin({a}) + {b})",
        lambda M, a, b, w: a * a * b if M.gt(a, 0.0) else M.sin(a) + b, [0.5, -0.7, 1.3, -1.9, 0.2, -0.3, 2.0, -1.0], _ANY2),
    Row("branch_primal", "(primal({a}) < primal({b}) ? {a} * {b} : {a} - {b})",
        lambda M, a, b, w: a * b if M.lt(a, b) else a - b,
        [1.5, -0.7, 0.3, 2.2, -1.9, 0.05, 1.0, -0.25], [0.8, -1.3, 2.5, 0.6, -0.5, 1.7, -2.4, 3.0]),
    Row("compound", """T g = {a};
g += {b};
g *= {w};
g -= {a} * 0.5f;
g /= ({b} * {b} + 1.0f);
g += 1.5f;
g -= 2;
g *= 3.0;
g /= 4.0f;
return g;""", _compound, _ANY, _ANY2),
    Row("literals", "(1 - {a}) * (2.0 / {b})", lambda M, a, b, w: (1 - a) * (2.0 / b),
        _ANY, [0.8, -1.3, 2.5, 0.6, -0.5, 1.7, -2.4, 3.0]),
    Row("neg_pos", "(-{a}) * (+{a}) + (-{w}) * {a}", lambda M, a, b, w: (-a) * (+a) + (-w) * a, _ANY),
    Row("fabs_u", "fabs({a}) * {w}", lambda M, a, b, w: M.fabs(a) * w, [0.3, -0.9, 1.6, -2.2, 0.2, 2.8, -0.5, 1.1]),
    Row("abs_shift", "abs({a} - 0.5f) * {a}", lambda M, a, b, w: M.fabs(a - 0.5) * a, [0.2, -0.9, 1.6, -2.2, 0.05, 2.8, 0.8, 1.1]),
    Row("square_u", "square({a} + {w})", lambda M, a, b, w: M.square(a + w), _ANY),
    Row("cmp_forms", "({a} <= {b} ? {a} * {a} : {b} * {a}) + ({a} >= 0.5f ? {a} * {b} : {a}) + (0.25f < {b} ? {b} : {b} * {b})",
        lambda M, a, b, w: ((a * a if M.le(a, b) else b * a) + (a * b if M.ge(a, 0.5) else a) + (b if M.lt(0.25, b) else b * b)),
        [1.0, -0.7, 0.1, 2.0, 0.9, -1.2, 0.2, 1.5], [2.0, -1.5, 0.8, 0.6, -0.3, 1.4, -0.9, 1.1]),
]

LIB_C = [
    Row("sincos_mix", "T s, c;\nsincos({a}, &s, &c);\nreturn s * {b} + c * {w};", _sincos_mix,
        [0.3, -1.1, 2.0, 3.5, -2.7, 0.9, 5.0, -0.4], _ANY2),
    Row("pow0", "pow({a}, 0.0f)", lambda M, a, b, w: M.pow(a, 0) + 0 * a, _ANY),
    Row("pow1", "pow({a}, 1.0f)", lambda M, a, b, w: M.pow(a, 1), _ANY),
    Row("pow2", "pow({a}, 2.0f)", lambda M, a, b, w: M.pow(a, 2), _ANY),
    Row("pow_frac", "pow({a}, 2.5f)", lambda M, a, b, w: M.pow(a, 2.5), _POS),
    Row("scalar_forms", "({a} + 2) * 0.5 - 3.0f / ({a} * {a} + 1) + (0.25f - {a}) * {a} + 2 * {a} + {a} / 4 + (1.5 + {a}) * ({a} - 1)",
        lambda M, a, b, w: (a + 2) * 0.5 - 3.0 / (a * a + 1) + (0.25 - a) * a + 2 * a + a / 4 + (1.5 + a) * (a - 1), _ANY),
]

# the natural mixed spellings: a library that does not build is the compile-conformance failure
LIB_M = [
    Row("fmax_a0", "fmax({a}, 0.0f)", lambda M, a, b, w: M.fmax(a, 0.0 * a), _ANY),
    Row("fmin_1a", "fmin(1.0f, {a})", lambda M, a, b, w: M.fmin(1.0 + 0.0 * a, a), [0.3, -0.9, 1.6, -2.2, 0.05, 2.8, -0.5, 1.3]),
    Row("eq_branch", "({a} == {b} ? {a} * 2.0f : {a} * {b})", lambda M, a, b, w: a * 2.0 if M.eq(a, b) else a * b,
        [1.5, -0.7, 0.3, 2.2, -1.9, 0.05, 1.0, -0.25], [0.8, -1.3, 2.5, 0.6, -0.5, 1.7, -2.4, 3.0]),
    Row("ne_branch", "({a} != {b} ? {a} + {b} * {b} : {a} * 3.0f)", lambda M, a, b, w: a + b * b if M.ne(a, b) else a * 3.0,
        [1.5, -0.7, 0.3, 2.2, -1.9, 0.05, 1.0, -0.25], [0.8, -1.3, 2.5, 0.6, -0.5, 1.7, -2.4, 3.0]),
    Row("fmin_a2_u", "fmin({a}, 2) * {w}", lambda M, a, b, w: M.fmin(a, 2.0 + 0.0 * a) * w, [0.3, -0.9, 1.6, -2.2, 0.05, 2.8, -0.5, 1.1]),
]


# ------------------------------------------------------------------------------------------------ seeded random expressions
_LEAVES = ("a", "b", "w", 0.5, 1.5, -0.75, 2.0)
_OPS = ("add", "sub", "mul", "neg", "sin", "cos", "tanh", "atan", "exp_q", "sqrt1", "log1", "div1", "pow2", "pow3", "square",
        "softplus")
_ARITY = dict(add=2, sub=2, mul=2, div1=2)


class _Rng:
    """A fixed 64-bit LCG (Knuth's MMIX constants): the expressions do not depend on any library's generator."""

    def __init__(self, seed):
        self.s = (seed * 2654435761 + 12345) % (1 << 64)

    def below(self, n):
        self.s = (self.s * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        return (self.s >> 33) % n


def random_tree(rng, depth):
    """Depth <= 4 over total-domain forms only: sqrt(e e + 1), log(e e + 1), e1 / (e2 e2 + 1), integer pow."""
    if depth == 0 or rng.below(8) == 0:
        return _LEAVES[rng.below(len(_LEAVES))]
    op = _OPS[rng.below(len(_OPS))]
    return (op,) + tuple(random_tree(rng, depth - 1) for _ in range(_ARITY.get(op, 1)))


def tree_cpp(t):
    if isinstance(t, str):
        return "{" + t + "}"
    if isinstance(t, float):
        return f"T({t!r}f)"
    op, s = t[0], [tree_cpp(c) for c in t[1:]]
    return {"add": lambda: f"({s[0]} + {s[1]})", "sub": lambda: f"({s[0]} - {s[1]})", "mul": lambda: f"({s[0]} * {s[1]})",
            "neg": lambda: f"(-{s[0]})", "exp_q": lambda: f"exp({s[0]} * 0.25f)", "sqrt1": lambda: f"sqrt({s[0]} * {s[0]} + 1.0f)",
            "log1": lambda: f"log({s[0]} * {s[0]} + 1.0f)", "div1": lambda: f"({s[0]} / ({s[1]} * {s[1]} + 1.0f))",
            "pow2": lambda: f"pow({s[0]}, 2.0f)", "pow3": lambda: f"pow({s[0]}, 3)", "square": lambda: f"square({s[0]})",
            "softplus": lambda: f"softplus({s[0]}, 2.0f)"}.get(op, lambda: f"{op}({s[0]})")()


def tree_eval(t, M, a, b, w):
    if isinstance(t, str):
        return {"a": a, "b": b, "w": w}[t]
    if isinstance(t, float):
        return t + 0 * a
    op, s = t[0], [tree_eval(c, M, a, b, w) for c in t[1:]]
    return {"add": lambda: s[0] + s[1], "sub": lambda: s[0] - s[1], "mul": lambda: s[0] * s[1], "neg": lambda: -s[0],
            "exp_q": lambda: M.exp(s[0] * 0.25), "sqrt1": lambda: M.sqrt(s[0] * s[0] + 1.0), "log1": lambda: M.log(s[0] * s[0] + 1.0),
            "div1": lambda: s[0] / (s[1] * s[1] + 1.0), "pow2": lambda: M.pow(s[0], 2), "pow3": lambda: M.pow(s[0], 3),
            "square": lambda: M.square(s[0]), "softplus": lambda: M.softplus(s[0], 2.0)}.get(op, lambda: getattr(M, op)(s[0]))()


RANDOM_SEEDS = (2, 3)       # chosen on the CPU: every reference jet finite, scale below RANDOM_SCALE_MAX (the GPU test asserts it)
RANDOM_SCALE_MAX = 1e4


def random_rows(seed, n=16):
    rng = _Rng(seed)
    xs = [[f32((rng.below(3001) - 1500) / 1000.0) for _ in range(n)] for _ in range(NPTS)]       # x of item p, in [-1.5, 1.5]
    rows = []
    for i in range(n):
        tree = random_tree(rng, 4)
        rows.append(Row(f"rand{seed}_{i}", tree_cpp(tree), (lambda M, a, b, w, t=tree: tree_eval(t, M, a, b, w)),
                        [xs[p][i] for p in range(NPTS)], [xs[p][(i + 1) % n] for p in range(NPTS)]))
    return rows


# ------------------------------------------------------------------------------------------------ libraries
class Lib:
    def __init__(self, name, rows, n=None, overlap=False):
        self.name, self.rows, self.overlap = name, rows, overlap
        slot = 0
        for k, r in enumerate(rows):
            r.k = k
            if overlap:
                r.ia, r.ib = k, (k + 1) % len(rows)
            else:
                r.ia, r.ib = slot, (slot + 1 if r.nx == 2 else -1)
                slot += r.nx
        self.n = len(rows) if overlap else slot
        assert n is None or n == self.n, (name, self.n)
        self.m = 1

    def row(self, name):
        return next(r for r in self.rows if r.name == name)

    def helpers(self):
        return "\n".join(r.helper() for r in self.rows)

    def bodies(self):
        rate = [f"xd[{r.ia}] = g{r.k}(x, u);" for r in self.rows]
        if not self.overlap:
            rate += [f"xd[{r.ib}] = T(0.0f);" for r in self.rows if r.nx == 2]
        stage = [f"T c = {H_CPP} * p.r[0];"] + [f"c = c + g{r.k}(x, u) * p.q[{r.ia}];" for r in self.rows] + ["return c;"]
        final = (["const T uf[1] = {T(P[0])};", "T c(0.0f);"] + [f"c = c + g{r.k}(x, uf) * p.qf[{r.ia}];" for r in self.rows]
                 + ["return c;"])
        return "\n".join(rate), "\n".join(stage), "\n".join(final)

    def model(self, integrator="euler", dt=DT):
        """The compiled library (cached by content: the bodies and (n, m) only; everything else is a runtime parameter)."""
        import quattro_ilqr_amd as q
        rate, stage, final = self.bodies()
        return q.compile_model(self.name, self.n, self.m, rate=rate, stage_cost=stage, final_cost=final, helpers=self.helpers(),
                               dt=dt, integrator=integrator, phys=(WF,), q=np.zeros(self.n), r=np.zeros(1), qf=np.zeros(self.n))

    def select(self, md, row=None, final=False, **kw):
        """md with the one-hot weight of `row` in q (or qf), or of the control term h (row None: r = 1)."""
        w = [0.0] * self.n
        if row is not None:
            w[row.ia] = 1.0
        if final:
            return md.with_(q=(0.0,) * self.n, r=(0.0,), qf=tuple(w), **kw)
        return md.with_(q=tuple(w), r=(0.0 if row is not None else 1.0,), qf=(0.0,) * self.n, **kw)

    def states(self):
        """x (NPTS, n) float32 and u (NPTS, 1) float32 of the main points: item p holds point p of every row."""
        x = np.zeros((NPTS, self.n), dtype=np.float32)
        for r in self.rows:
            for p in range(NPTS):
                a, b, _ = r.point(p)
                x[p, r.ia] = a
                if r.nx == 2 and not self.overlap:
                    x[p, r.ib] = b
        return x, np.asarray(W_ITEM, dtype=np.float32).reshape(NPTS, 1)

    def rate_fn(self, M):
        """Python callable rate(x, u) through the math namespace M (for complex-step Jacobians of an integrator step)."""
        def rate(x, u):
            xd = np.zeros(self.n, dtype=np.result_type(x, u))
            for r in self.rows:
                xd[r.ia] = r.fn(M, x[r.ia], x[r.ib] if r.ib >= 0 else 0.0, u[0])
            return xd
        return rate


def step_fn(rate, integrator, dt):
    def f(x, u):
        if integrator == "euler":
            return x + dt * rate(x, u)
        k1 = rate(x, u); k2 = rate(x + 0.5 * dt * k1, u); k3 = rate(x + 0.5 * dt * k2, u); k4 = rate(x + dt * k3, u)
        return x + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    return f


def probe_libs():
    return [Lib("dual_probe_a", LIB_A, 16), Lib("dual_probe_b", LIB_B, 16), Lib("dual_probe_c", LIB_C, 7),
            Lib("dual_probe_mixed", LIB_M, 7)]


def random_libs():
    return [Lib(f"dual_probe_rand{s}", random_rows(s), 16, overlap=True) for s in RANDOM_SEEDS]


_LIBS = {}


def lib(name):
    if not _LIBS:
        for L in probe_libs() + random_libs():
            _LIBS[L.name] = L
    return _LIBS[name]


def all_libs():
    lib("dual_probe_a")
    return list(_LIBS.values())


# ------------------------------------------------------------------------------------------------ reference jets
_JET_CACHE = {}


def _jet_functions(expr):
    key = sp.srepr(expr)
    if key not in _JET_CACHE:
        v = (A_, B_, W_)
        g = [sp.diff(expr, s) for s in v]
        H = [sp.diff(gi, s) for gi in g for s in v]
        exprs = [expr] + g + H
        f_mp = sp.lambdify(v, exprs, modules=[{"Softplus": _mp_softplus, "Sigmoid": _mp_sigmoid}, "mpmath"])
        f_np = sp.lambdify(v, exprs, modules=[{"Softplus": _np_softplus, "Sigmoid": _np_sigmoid}, "numpy"])
        _JET_CACHE[key] = (f_mp, f_np)
    return _JET_CACHE[key]


@dataclass
class Jet:
    v: float
    g: np.ndarray            # (3,) over (a, b, w)
    H: np.ndarray            # (3, 3)

    @property
    def scale(self):
        return max(1.0, abs(self.v), float(np.max(np.abs(self.g))), float(np.max(np.abs(self.H))))

    def finite(self):
        return bool(np.isfinite(self.v) and np.all(np.isfinite(self.g)) and np.all(np.isfinite(self.H)))


def _expr(fn, at):
    return sp.sympify(fn(SymMath(at), A_, B_, W_))


def jet_ref(fn, at):
    """Exact jet of fn at the fp32 point at = (a, b, w): sympy derivatives of the branch taken there, evaluated in mpmath."""
    f_mp, _ = _jet_functions(_expr(fn, at))
    with mpmath.workdps(40):
        out = [float(t) for t in f_mp(*(mpmath.mpf(float(v)) for v in at))]
    return Jet(out[0], np.array(out[1:4]), np.array(out[4:]).reshape(3, 3))


def jet_f32(fn, at):
    """The same textbook formulas evaluated in numpy float32: independent of dual.h; its error sets the tolerance."""
    _, f_np = _jet_functions(_expr(fn, at))
    with np.errstate(all="ignore"):
        out = [float(np.asarray(t, dtype=np.float32).reshape(-1)[0]) for t in f_np(*(np.array([v], dtype=np.float32) for v in at))]
    return Jet(out[0], np.array(out[1:4]), np.array(out[4:]).reshape(3, 3))


def jet_errors(got, ref):
    """(value, first, second) errors of a jet against the reference, in units of the reference's scale."""
    S = ref.scale
    return np.array([abs(got.v - ref.v), np.max(np.abs(got.g - ref.g)), np.max(np.abs(got.H - ref.H))]) / S


def tolerances(fn, points):
    """FACTOR x max(E_row, 2^-23) per derivative order over `points`."""
    E = np.zeros(3)
    for at in points:
        E = np.maximum(E, jet_errors(jet_f32(fn, at), jet_ref(fn, at)))
    assert np.all(np.isfinite(E)), E
    return FACTOR * np.maximum(E, EPS32)


def h_jet(w):
    return jet_ref(lambda M, a, b, ww: H_FN(M, ww), (0.0, 0.0, w))


# ------------------------------------------------------------------------------------------------ edges (cost side only)
def _ulp(v, k):
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return float(v)


@dataclass
class Edge:
    lib: str
    row: str
    at: tuple                 # (a, b, w)
    kind: str = "jet"         # "jet": the reference jet at `at`; "angle0": the jet at a = 0 (sincos beyond 1e15: documented
    label: str = ""           # sin = 0, cos = 1); "nan": value and a-derivatives are NaN

    @property
    def id(self):
        return f"{self.row}-{self.label}"


def edges():
    E = []
    add = lambda *a, **k: E.append(Edge(*a, **k))
    add("dual_probe_b", "fabs_u", (0.0, 0.0, 1.5), label="fabs0")
    add("dual_probe_b", "fabs_u", (-0.0, 0.0, 1.5), label="fabs-0")
    add("dual_probe_a", "fmax2", (0.7, 0.7, 0.5), label="tie")
    add("dual_probe_a", "fmin2", (0.7, 0.7, 0.5), label="tie")
    add("dual_probe_mixed", "fmax_a0", (0.0, 0.0, 0.5), label="tie")
    add("dual_probe_mixed", "fmin_1a", (1.0, 0.0, 0.5), label="tie")
    add("dual_probe_mixed", "eq_branch", (0.7, 0.7, 0.5), label="equal")
    add("dual_probe_mixed", "ne_branch", (0.7, 0.7, 0.5), label="equal")
    for k in range(1, 9):
        for d in (-1, 0, 1):
            add("dual_probe_c", "sincos_mix", (_ulp(k * np.pi / 4, d), 1.0, 0.5), label=f"{k}pi/4{d:+d}ulp")
    for lab, a in (("2048-", _ulp(2048.0, -1)), ("2048", 2048.0), ("2048+", _ulp(2048.0, 1)), ("-2048-", -_ulp(2048.0, 1)),
                   ("1e6", 1.0e6), ("-1e6", -1.0e6 - 7.0), ("1e9", 1.0e9), ("1e15", 1.0e15)):
        add("dual_probe_c", "sincos_mix", (f32(a), 1.0, 0.5), label=lab)
    for lab, a in (("2e15", 2.0e15), ("-1e30", -1.0e30)):
        add("dual_probe_c", "sincos_mix", (f32(a), 1.0, 0.5), kind="angle0", label=lab)
    for lab, a in (("inf", np.inf), ("-inf", -np.inf)):
        add("dual_probe_c", "sincos_mix", (a, 1.0, 0.5), kind="nan", label=lab)
    for a in (50.0, -50.0, 5000.0, -5000.0):
        add("dual_probe_b", "softplus2", (a, 0.0, 0.5), label=f"bz{2 * a:g}")
    for d in (2.5, -2.5, 250.0, -250.0):
        add("dual_probe_b", "softplus40", (0.5 + d, 0.0, 0.5), label=f"bz{40 * d:g}")
    for a, w in ((20.0, 1.0e6), (-20.0, -1.0e6), (9.0, 3.0e4)):
        add("dual_probe_a", "tanh_atan", (a, 0.0, w), label=f"sat{a:g}")
    add("dual_probe_a", "sqrt1", (1.0e-6, 0.0, 0.5), label="1e-6")
    add("dual_probe_a", "log_u", (1.0e-6, 0.0, 0.5), label="1e-6")
    add("dual_probe_a", "pow3_u", (-1.5, 0.0, 0.5), label="negbase")
    add("dual_probe_a", "pow3_u", (0.0, 0.0, 0.5), label="x0e3")
    for e in (0, 1, 2):
        add("dual_probe_c", f"pow{e}", (0.0, 0.0, 0.5), label=f"x0e{e}")
    for ed in E:
        ed.at = tuple(float(np.float32(v)) for v in ed.at)
    return E


def edge_reference(ed):
    """-> (reference jet or None for "nan", tolerances)."""
    fn = lib(ed.lib).row(ed.row).fn
    if ed.kind == "nan":
        return None, None
    at = (0.0,) + ed.at[1:] if ed.kind == "angle0" else ed.at
    return jet_ref(fn, at), tolerances(fn, [at])


# ------------------------------------------------------------------------------------------------ host driver (CPU test)
def host_driver_source(libs):
    """A C++ program over csrc/dual.h built for the host: reads lines "<function index> <a> <b> <w>" (hex floats) and prints,
    per line, the float value, value + derivative along each of (a, b, w) from Dual<float>, and for each pair of directions
    (j, c) the four parts of Dual<Dual<float>>."""
    fns, cases = [], []
    idx = 0
    index = {}
    for L in libs:
        ns = f"lib_{L.name}"
        fns.append(f"namespace {ns} {{\n{L.helpers()}\n}}")
        for r in L.rows:
            index[(L.name, r.name)] = idx
            ib = r.ib if r.ib >= 0 else r.ia
            cases.append(f"    case {idx}: x[{r.ia}] = a; if ({ib} != {r.ia}) x[{ib}] = b; return {ns}::g{r.k}<T>(x, u);")
            idx += 1
    n_max = max(L.n for L in libs)
    src = f"""// generated by tests/dual_probe.py: csrc/dual.h on the host (qt_sincos / qt_softplus from tests/dual_host_shim.h)
#define QT_DUAL_HOST
#include <cstdio>
#include "dual_host_shim.h"
#include "dual.h"
namespace probe {{
using qtad::abs; using qtad::atan; using qtad::cos; using qtad::exp; using qtad::fabs; using qtad::fmax; using qtad::fmin;
using qtad::log; using qtad::pow; using qtad::primal; using qtad::sin; using qtad::sincos; using qtad::softplus;
using qtad::sqrt; using qtad::square; using qtad::tan; using qtad::tanh;
{chr(10).join(fns)}
template <class T>
static T eval(int k, const T& a, const T& b, const T& w) {{
  T x[{n_max}], u[1] = {{w}};
  for (int i = 0; i < {n_max}; ++i) x[i] = T(0.0f);
  switch (k) {{
{chr(10).join(cases)}
  }}
  return T(0.0f);
}}
}}  // namespace probe
int main() {{
  using probe::eval;
  using D = qtad::Dual<float>;
  using DD = qtad::Dual<D>;
  int k;
  float z[3];
  while (std::scanf("%d %a %a %a", &k, &z[0], &z[1], &z[2]) == 4) {{
    std::printf("%a", eval<float>(k, z[0], z[1], z[2]));
    for (int j = 0; j < 3; ++j) {{
      const D r = eval<D>(k, D(z[0], j == 0), D(z[1], j == 1), D(z[2], j == 2));
      std::printf(" %a %a", r.v, r.d);
    }}
    for (int j = 0; j < 3; ++j)
      for (int c = 0; c < 3; ++c) {{
        const DD r = eval<DD>(k, DD(D(z[0], j == 0), D(c == 0, 0.0f)), DD(D(z[1], j == 1), D(c == 1, 0.0f)),
                              DD(D(z[2], j == 2), D(c == 2, 0.0f)));
        std::printf(" %a %a %a %a", r.v.v, r.v.d, r.d.v, r.d.d);
      }}
    std::printf("\\n");
  }}
  return 0;
}}
"""
    return src, index
