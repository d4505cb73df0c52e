"""CPU: the MPC's model as csrc/mpc_model.h states it once (ODE, RK4 x 4, affine probe; generic in the scalar) through
amk__mpc_dynamics, the host-only entry the handle's A, B, c (refresh_dynamics) and amk_mpc_eval_gamma's d/d tau block both come from,
against the oracle's mpco_affine.  No device."""
import ctypes as C

import numpy as np
import pytest

from avoid_mpc_amd import capi, synth
from tests import _oracle

DT = 0.033
TAUS = [list(synth.DEFAULT_TAU),            # config/mpc_parameters.yaml
        [0.01, 0.01, 0.01, 0.0],            # the constructor's default (HighLvlMpc.cpp:13-16)
        [3.5, 11.25, 7.0, 2.0]]             # every axis its own, a tau_yaw that the model must ignore
DRAGS = [(0.0, 0.0, 0.0), (0.033, 0.05, 0.2)]
CASES = [(t, d) for t in TAUS for d in DRAGS]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def dynamics(tau, drag, with_dtau):
    lib = capi.load()
    tau, drag = np.array(tau, np.float64), np.array(drag, np.float64)
    A, B, c = np.zeros((10, 10)), np.zeros((10, 4)), np.zeros(10)
    dtau = np.zeros((3, 150)) if with_dtau else None
    assert lib.amk__mpc_dynamics(_vp(tau), _vp(drag), DT, _vp(A), _vp(B), _vp(c), _vp(dtau) if with_dtau else None) == 0
    return A, B, c, dtau


def oracle_affine(tau, drag):
    A, B, c = np.zeros((10, 10)), np.zeros((10, 4)), np.zeros(10)
    with _oracle.oracle_drag(drag):   # restores the default (off) on exit
        _oracle.load_oracle().mpco_affine(np.array(tau, np.float64), DT, A.reshape(-1), B.reshape(-1), c)
    return A, B, c


@pytest.mark.parametrize("tau,drag", CASES)
def test_probe_matches_oracle(tau, drag):
    """A, B, c against mpco_affine.  The bound is what the parent's refresh_dynamics (its ode_host / rk4_host, built stand-alone for the
    host with the library's compiler at -O3) differs from the oracle by at these six cases, times 4 for a compiler's reassociation
    freedom in the oracle's C: measured 0.0 in every entry of every case -- the two are the same operations in the same order -- so the
    bound is 4 x 0 = 0, bit equality."""
    measured = 0.0
    A, B, c, _ = dynamics(tau, drag, False)
    Ao, Bo, co = oracle_affine(tau, drag)
    for name, x, y in (("A", A, Ao), ("B", B, Bo), ("c", c, co)):
        d = np.abs(x - y).max()
        print(name, tau, drag, d)
        assert d <= 4 * measured, (name, d)


@pytest.mark.parametrize("tau,drag", CASES)
def test_value_part_of_the_dual_run_is_the_plain_run(tau, drag):
    plain = dynamics(tau, drag, False)
    dual = dynamics(tau, drag, True)
    for x, y in zip(plain[:3], dual[:3]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("tau,drag", CASES)
def test_dtau_matches_central_differences_of_the_oracle(tau, drag):
    """d(A, B, c)/d tau_a, a = 0..2 (tau_yaw has no block: the model does not read it), against central differences of mpco_affine with
    h = 1e-6 max(1, |tau_a|).  1e-6 relative to the largest entry of each block: truncation (h^2) and round-off (eps / h) of the
    quotient are near 1e-9, so the bound is loose by design."""
    *_, dtau = dynamics(tau, drag, True)
    assert dtau.shape == (3, 150)
    for a in range(3):
        h = 1e-6 * max(1.0, abs(tau[a]))
        tp, tm = list(tau), list(tau)
        tp[a] += h; tm[a] -= h
        hi, lo = oracle_affine(tp, drag), oracle_affine(tm, drag)
        fd = np.concatenate([((x - y) / (tp[a] - tm[a])).reshape(-1) for x, y in zip(hi, lo)])   # A 100 | B 40 | c 10
        err = np.abs(dtau[a] - fd).max()
        print(tau, drag, a, err, np.abs(fd).max())
        assert np.abs(fd).max() > 0
        assert err <= 1e-6 * np.abs(fd).max(), (a, err)


def _rows_of_A(j):   # the reference's chains p <- v <- a per axis, yaw on its own (mpc_obstacle_casadi.py:106-122)
    return {j} if j < 4 else ({j - 4, j} if j < 7 else {j - 7, j - 3, j})


def _rows_of_B(a):
    return {3} if a == 3 else {a, 4 + a, 7 + a}


@pytest.mark.parametrize("tau,drag", CASES)
def test_pattern_of_the_probed_A_and_B(tau, drag):
    """The non-zeros of the probed A and B are the rows rows_of_A / rows_of_B (mpc_model.h) declare, restated here: 19 and 10."""
    A, B, _, dtau = dynamics(tau, drag, True)
    assert [set(np.flatnonzero(A[:, j])) for j in range(10)] == [_rows_of_A(j) for j in range(10)]
    assert [set(np.flatnonzero(B[:, a])) for a in range(4)] == [_rows_of_B(a) for a in range(4)]
    assert np.count_nonzero(A) == 19 and np.count_nonzero(B) == 10
    for a in range(3):   # a derivative lives inside the pattern
        dA, dB = dtau[a, :100].reshape(10, 10), dtau[a, 100:140].reshape(10, 4)
        assert not np.any(dA[A == 0]) and not np.any(dB[B == 0])


def test_null_arguments_are_refused():
    lib = capi.load()
    x = np.zeros(100)
    assert lib.amk__mpc_dynamics(None, _vp(x), DT, _vp(x), _vp(x), _vp(x), None) == 1   # AMK_ERR_INVALID_ARG
