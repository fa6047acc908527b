"""csrc/dual.h compiled for the host (QT_DUAL_HOST; qt_sincos / qt_softplus from tests/dual_host_shim.h) against exact fp64
derivatives: value, first and second derivative of every row of the probe table (tests/dual_probe.py) and of the seeded
random expressions, through Dual<float> and Dual<Dual<float>>, at the rows' main points and at the edges that do not depend
on the device's own sincos (ties, kinks, saturation, pow at a zero base).  The algebra is what is checked here: the device
math functions are measured by tests/test_dual_algebra_gpu.py.  Built with the host sanitizers where the toolchain has
their runtimes."""
import os
import subprocess

import numpy as np
import pytest

import dual_probe as dp
from conftest import ROOT

CSRC = os.path.join(ROOT, "quattro-transformer-ilqr_amd", "csrc")
CLANG = "/opt/rocm/llvm/bin/clang++"            # the host compiler that ships with the device toolchain


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = CLANG
    work = tmp_path_factory.mktemp("dual_host")
    src, index = dp.host_driver_source(dp.all_libs())
    (work / "driver.cpp").write_text(src)
    base = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-I", CSRC,
            "-I", os.path.join(ROOT, "tests"), str(work / "driver.cpp"), "-o", str(work / "driver")]
    # host sanitizers when their runtimes are installed next to the compiler; the plain build otherwise
    r = subprocess.run(base + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(work / "driver")], input="", capture_output=True, text=True).returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)      # (no runtimes, or a preloaded library in front of them)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(cases):
        """cases: [(library, row, (a, b, w))] -> per case (float value, Dual<float> jets, Dual<Dual<float>> jets)."""
        text = "".join(f"{index[(ln, rn)]} {float(a).hex()} {float(b).hex()} {float(w).hex()}\n" for ln, rn, (a, b, w) in cases)
        out = subprocess.run([str(work / "driver")], input=text, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-4000:]
        lines = out.stdout.strip().splitlines()
        assert len(lines) == len(cases)
        res = []
        for ln in lines:
            t = [float.fromhex(s) if s not in ("nan", "-nan", "inf", "-inf") else float(s) for s in ln.split()]
            assert len(t) == 1 + 6 + 36
            d1 = np.array(t[1:7]).reshape(3, 2)
            d2 = np.array(t[7:]).reshape(3, 3, 4)
            res.append((t[0], d1, d2))
        return res
    return run


def _check(what, res, ref, tol):
    """Every copy of the value, the gradient (from both levels and both seeds) and the Hessian against the reference jet."""
    v, d1, d2 = res
    S = ref.scale
    e0 = max(abs(v - ref.v), np.max(np.abs(d1[:, 0] - ref.v)), np.max(np.abs(d2[:, :, 0] - ref.v))) / S
    e1 = max(np.max(np.abs(d1[:, 1] - ref.g)), np.max(np.abs(d2[:, :, 1] - ref.g[:, None])),
             np.max(np.abs(d2[:, :, 2] - ref.g[None, :]))) / S
    e2 = np.max(np.abs(d2[:, :, 3] - ref.H)) / S
    assert np.max(np.abs(d2[:, :, 3] - d2[:, :, 3].T)) / S <= 2 * tol[2], what         # (computed independently: H[j, c], H[c, j])
    err = np.array([e0, e1, e2])
    assert np.all(err <= tol), (what, err, tol)         # (a NaN anywhere fails)
    return err


@pytest.mark.parametrize("libname", [L.name for L in dp.all_libs()])
def test_host_dual_jets_match_fp64_derivatives(driver, libname):
    L = dp.lib(libname)
    cases = [(L.name, r.name, r.point(p)) for r in L.rows for p in range(dp.NPTS)]
    res = driver(cases)
    i = 0
    for r in L.rows:
        pts = [r.point(p) for p in range(dp.NPTS)]
        tol = dp.tolerances(r.fn, pts)
        worst = np.zeros(3)
        for at in pts:
            ref = dp.jet_ref(r.fn, at)
            assert ref.finite()
            worst = np.maximum(worst, _check((r.name, at), res[i], ref, tol))
            i += 1
        print(f"{L.name}/{r.name}: host error / S  value {worst[0]:.1e}  first {worst[1]:.1e}  second {worst[2]:.1e}  (bounds {tol})")


HOST_EDGES = [e for e in dp.edges() if e.kind == "jet" and not (e.row == "sincos_mix" and abs(e.at[0]) > 100.0)]


@pytest.mark.parametrize("edge", HOST_EDGES, ids=[e.id for e in HOST_EDGES])
def test_host_dual_edges(driver, edge):
    """Ties and kinks (first argument's branch; fabs(0) = +x), sincos at multiples of pi / 4 +- 1 ulp, softplus / tanh / atan
    saturated, sqrt / log at 1e-6, pow with a negative base, and pow(x, e) at x = 0 for e = 0, 1, 2, 3 (finite, exact)."""
    ref, tol = dp.edge_reference(edge)
    res = driver([(edge.lib, edge.row, edge.at)])[0]
    _check(edge.id, res, ref, tol)


def test_random_expression_references_are_finite_and_bounded():
    """The seeds of the random libraries were chosen so that every reference jet is finite with scale < 1e4: checked here on
    the reference alone, at the stage points and with the final cost's control value."""
    for L in dp.random_libs():
        for r in L.rows:
            for p in range(dp.NPTS):
                for w in (dp.W_ITEM[p], dp.WF):
                    a, b, _ = r.point(p)
                    j = dp.jet_ref(r.fn, (a, b, dp.f32(w)))
                    assert j.finite() and j.scale < dp.RANDOM_SCALE_MAX, (r.name, p, j.scale)
