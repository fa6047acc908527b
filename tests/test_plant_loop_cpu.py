"""Host-side checks of the plant / gain-feedback closed loop (quattro_track_f32, quattro_mpc_run_plant_f32, BatchedMPC.run's
plant, plant_phys, replan_every and feedback): argument errors come back before any HIP call, so none of this needs a GPU."""
import ctypes
import os

import numpy as np
import pytest

import __graft_entry__ as entry


@pytest.fixture(scope="module")
def lib():
    from quattro_ilqr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    return _lib.load()


def _quad_params():
    from quattro_ilqr_amd import models
    md = models.quadrotor_model()
    p = md._build_c_params()           # (a private copy: the tests below change its fields)
    return md, p


def _copy(p):
    from quattro_ilqr_amd import _lib
    c = _lib.ModelParams()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(p), ctypes.sizeof(p))
    return c


def _bad_plants(p):
    out = []
    for field, value in (("model_id", 1 if p.model_id != 1 else 2), ("n", p.n + 1), ("m", p.m + 1), ("dt", 2.0 * p.dt)):
        c = _copy(p)
        setattr(c, field, value)
        out.append((field, c))
    return out


def _check_entries(lib, p):
    """Both entries of `lib` refuse each bad argument with QUATTRO_ERR_BAD_ARG; `one` is never dereferenced."""
    from quattro_ilqr_amd import _lib
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(1)
    arr6 = (ctypes.c_float * 6)(1.0, 0.5, 0.25, 0.1, 0.05, 0.01)
    B, N = 4, 10

    def run(n_steps=10, hold=5, feedback=0, max_iter=5, plant=None):
        return lib.quattro_mpc_run_plant_f32(ctypes.byref(p), one, one, one, B, N, 1e-6, arr6, 6, 1e-3, max_iter, n_steps, one, one,
                                             one, null, one, one, one, one, one, one, null, one, 1 << 30,
                                             None if plant is None else ctypes.byref(plant), null, hold, feedback, null)

    def track(n_steps=5, plant=None, x0=one):
        return lib.quattro_track_f32(ctypes.byref(p), None if plant is None else ctypes.byref(plant), null, x0, one, one, one, 1,
                                     B, N, n_steps, null, one, one, null)

    # (a call whose arguments are all good gets as far as the workspace check — `one` is not 256-byte aligned — and stops there:
    #  the refusals below are the entry's verdict on the argument named, not on something else)
    assert run() == _lib.ERR_WORKSPACE
    assert run(hold=0) == _lib.ERR_BAD_ARG
    assert run(hold=-1) == _lib.ERR_BAD_ARG
    assert run(n_steps=N + 1, hold=N + 1) == _lib.ERR_BAD_ARG           # hold outside 1..N
    assert run(n_steps=10, hold=3) == _lib.ERR_BAD_ARG                  # n_steps % hold != 0
    assert run(n_steps=0) == _lib.ERR_BAD_ARG
    assert run(feedback=1, max_iter=0) == _lib.ERR_BAD_ARG              # feedback needs gains
    assert run(feedback=0, max_iter=0) == _lib.ERR_WORKSPACE            # (without feedback max_iter = 0 is legal, as in quattro_mpc_run_f32)
    assert run(hold=N, n_steps=2 * N) == _lib.ERR_WORKSPACE             # hold = N is inside the range
    for field, plant in _bad_plants(p):
        assert run(plant=plant) == _lib.ERR_BAD_ARG, field
        assert track(plant=plant) == _lib.ERR_BAD_ARG, field
    other = _copy(p)                   # a plant may differ in integrator, phys and cost
    other.integrator = 1 - p.integrator
    other.phys[0] = 1.3 * p.phys[0]
    other.q[0] = 0.0
    assert run(plant=other) == _lib.ERR_WORKSPACE
    assert track(n_steps=N + 1) == _lib.ERR_BAD_ARG                     # tracks rows of ONE nominal: n_steps <= N
    assert track(n_steps=0) == _lib.ERR_BAD_ARG
    assert track(x0=null) == _lib.ERR_BAD_ARG
    other.integrator = 7
    assert track(plant=other) == _lib.ERR_UNSUPPORTED and run(plant=other) == _lib.ERR_UNSUPPORTED


def test_plant_entries_refuse_bad_arguments_before_any_launch(lib):
    _, p = _quad_params()
    _check_entries(lib, p)


def test_user_model_library_exports_and_checks_the_plant_entries(lib):
    """A user-model library exports both symbols and checks them alike (its phys are the model's free parameters)."""
    from quattro_ilqr_amd import _lib, user_model
    md = user_model.example_planar_model()
    raw = ctypes.CDLL(md.lib_path)
    assert hasattr(raw, "quattro_track_f32") and hasattr(raw, "quattro_mpc_run_plant_f32")
    _check_entries(_lib.load_for(md), md._build_c_params())


def test_batched_mpc_run_validates_the_plant_options_on_the_host():
    """The three ValueErrors of BatchedMPC.run come before any tensor is placed on the device: on a machine without a GPU
    anything later would fail in another way."""
    pytest.importorskip("torch")
    from quattro_ilqr_amd import BatchedMPC, models
    md = models.quadrotor_model()
    mpc = BatchedMPC(md, 10, max_iter=3, tf_window=0)
    x0 = np.tile(np.asarray(md.x_ref, dtype=np.float32), (3, 1))
    for bad in (models.cartpole_model(), models.quadrotor_model(dt=0.02), md.with_(name="quadrotor2")):
        with pytest.raises(ValueError, match="plant"):
            mpc.run(x0, 4, plant=bad)
    with pytest.raises(ValueError, match="plant_phys"):
        mpc.run(x0, 4, plant_phys=np.ones((3, 5), dtype=np.float32))
    with pytest.raises(ValueError, match="plant_phys"):
        mpc.run(x0, 4, plant_phys=np.ones((2, 7), dtype=np.float32))
    with pytest.raises(ValueError, match="replan_every"):
        mpc.run(x0, 4, replan_every=3)
    with pytest.raises(ValueError, match="replan_every"):
        mpc.run(x0, 22, replan_every=11)           # longer than the horizon
    # an admissible plant passes the host checks (and, here, reaches the device or fails to)
    from quattro_ilqr_amd import ops
    ops.check_plant(md, md.with_(integrator="rk4", phys=(1.2,) + md.phys[1:], q=(0.0,) * 12))
