"""CPU: amk_sim_vehicle_step_body without a device -- the symbols and the struct are declared, listed, bound and exported and agree in
layout, every argument rule is refused before the device is asked for with the outputs unwritten, the header states the contract, the
kernel's resources.  And the numpy restatement (flight.body_step_ordered) is held to formulations written differently: hover as an
exact fixed point, the sign of the attitude loop against the bound of theta' = -k sin(theta), the steady state, the normalisation's
roundings in exact rational arithmetic, first-order convergence to an independent rotation-matrix integrator, the COG filter
against a deque, the split identity, and the body-frame drag an affine model cannot hold."""
import collections
import ctypes as C
import fractions
import json
import os
import re

import numpy as np
import pytest

from avoid_mpc_amd import build as amk_build
from avoid_mpc_amd import capi, flight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, NO_DEVICE = capi.AMK_ERR_INVALID_ARG, capi.AMK_ERR_NO_DEVICE
NAN, INF = float("nan"), float("inf")
U = 2.0 ** -53          # the unit roundoff of fp64; an ulp of 1 is 2 U
GZ = flight.GZ
CON_DT = 0.1
Q, RATE, F, HELD, HEAD, RING = flight.BODY_Q, flight.BODY_RATE, flight.BODY_F, flight.BODY_HELD, flight.BODY_HEAD, flight.BODY_RING


@pytest.fixture(scope="module")
def lib():
    amk_build.build()
    return capi.load()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _struct(p):
    return capi.SimBodyParams(float(p.h), int(p.n_sub), float(p.gz), float(p.k_att), float(p.rate_max), float(p.k_rate), float(p.k_thrust),
                              float(p.f_min), float(p.f_max), (C.c_double * 3)(*p.drag), float(p.yaw_cs), float(p.yaw_sn), int(p.cog_window),
                              (C.c_double * 16)(*p.cog_weight))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _state(S=1, p=(0.0, 0.0, 1.0), v=(0.0, 0.0, 0.0)):
    x = np.zeros((S, 10)); x[:, 0:3] = p; x[:, 4:7] = v
    return x, flight.body_state0(S, GZ)


def _quat(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def _rot(Twb):
    return np.asarray(Twb)[0, :3, :3]


def _angle(Ra, Rb):
    """The angle of Ra^T Rb, from the sine (accurate near 0) and the cosine"""
    M = Ra.T @ Rb
    e = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(np.arctan2(np.linalg.norm(e), 0.5 * (np.trace(M) - 1.0)))


def _acc2rotmat(T, cs=1.0, sn=0.0):
    z = np.asarray(T, float) / np.linalg.norm(T)
    y = np.cross(z, [cs, sn, 0.0]); y /= np.linalg.norm(y)
    return np.stack([np.cross(y, z), y, z], axis=1)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_and_the_struct_are_declared_listed_bound_and_agree(lib):
    hdr = open(os.path.join(ROOT, "include", "avoid_mpc_amd.h")).read()
    section = hdr[hdr.index("Sensor noise on the simulated depth frames"):]
    section = section[section.index("The rigid-body vehicle"):]               # declared, after the sensor noise's section
    for name, n_args in (("amk_sim_body_reset", 4), ("amk_sim_vehicle_step_body", 8), ("amk_sim_vehicle_step_body_host", 7)):
        assert re.search(r"^int " + name + r"\(", section, re.M), name
        assert name in capi.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args, name
    assert capi.missing_symbols() == []
    assert "#define AMK_SIM_BODY_DOUBLES 64" in section and re.search(r"#define AMK_SIM_COG_MAX\s+16", section)
    assert (capi.AMK_SIM_BODY_DOUBLES, capi.AMK_SIM_COG_MAX) == (flight.BODY_DOUBLES, flight.COG_MAX) == (64, 16)
    fields = re.search(r"typedef struct amk_sim_body_params \{(.*?)\} amk_sim_body_params;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    decls = [(d.split()[0], n.strip()) for d in fields.split(";") if d.strip() for n in d.split(None, 1)[1].split(",")]
    names = tuple(re.sub(r"\[.*\]", "", n) for _, n in decls)
    assert names == flight.BODY_FIELDS == tuple(n for n, _ in capi.SimBodyParams._fields_)
    # the layout a C compiler gives the header's struct (every member at the next multiple of its own alignment) is ctypes' own
    offset = 0
    for ctype, n in decls:
        size = {"double": 8, "int": 4}[ctype]
        count = {"drag[3]": 3, "cog_weight[AMK_SIM_COG_MAX]": 16}.get(n, 1)
        offset = (offset + size - 1) // size * size
        field = getattr(capi.SimBodyParams, re.sub(r"\[.*\]", "", n))
        assert (field.offset, field.size) == (offset, size * count), n
        offset += size * count
    assert C.sizeof(capi.SimBodyParams) == (offset + 7) // 8 * 8 == 248
    assert RING + 3 * flight.COG_MAX <= flight.BODY_DOUBLES and (Q, RATE, F, HELD, HEAD, RING) == (0, 4, 7, 8, 9, 10)


def test_bad_arguments_are_refused_before_the_device_is_asked(lib):
    S = 3
    cmd = np.full((S, 3), 7.0); x = np.full((S, 10), 7.0); body = np.full((S, 64), 7.0); Twb = np.full((S, 16), 7.0)
    for fn, tail in ((lib.amk_sim_vehicle_step_body, (None,)), (lib.amk_sim_vehicle_step_body_host, ())):
        def call(c=_vp(cmd), xs=_vp(x), b=_vp(body), T=_vp(Twb), n=S, q=0.0, null_prm=False, **kw):
            p = None if null_prm else C.byref(_struct(flight.body_params(CON_DT, **dict(dict(h=CON_DT / 33), **kw))))
            return fn(p, c, xs, b, T, n, q, *tail)
        assert call(null_prm=True) == BAD and call(c=None) == BAD and call(xs=None) == BAD and call(b=None) == BAD
        assert call(n=0) == BAD and call(n=-2) == BAD and call(q=-1e-9) == BAD and call(q=NAN) == BAD
        assert call(h=0.0) == BAD and call(h=-1e-3) == BAD and call(h=NAN) == BAD
        assert call(n_sub=0) == BAD and call(n_sub=-1) == BAD and call(n_sub=4097) == BAD
        for name in ("gz", "k_att"):
            assert call(**{name: -1e-300}) == BAD and call(**{name: NAN}) == BAD, name
        assert call(rate_max=0.0) == BAD and call(rate_max=-1.0) == BAD and call(rate_max=NAN) == BAD
        for name in ("k_rate", "k_thrust"):
            assert call(**{name: 0.0}) == BAD and call(**{name: -0.5}) == BAD and call(**{name: 1.0 + 1e-12}) == BAD and call(**{name: NAN}) == BAD
        assert call(f_min=1.0, f_max=0.5) == BAD and call(f_min=NAN) == BAD and call(f_max=NAN) == BAD
        for k in range(3):
            for bad in (-1e-9, NAN):
                drag = [0.1, 0.1, 0.1]; drag[k] = bad
                assert call(drag=drag) == BAD, (k, bad)
        assert call(yaw_cs=NAN) == BAD and call(yaw_sn=NAN) == BAD
        assert call(cog_window=-1) == BAD and call(cog_window=17) == BAD
        w = flight.cog_weights()
        for window, bad in ((2, [1.0, -1.0]), (3, [1.0, 1.0, -2.5]), (2, [1.0, NAN]), (16, np.zeros(16)), (4, [NAN, 1.0, 1.0, 1.0])):
            assert call(cog_window=window, cog_weight=bad) == BAD, (window, bad)
        if lib.amk_device_count() <= 0:                                         # good calls reach the device question and nothing else
            assert call() == NO_DEVICE and call(T=None) == NO_DEVICE and call(q=1e6) == NO_DEVICE
            assert call(rate_max=INF) == NO_DEVICE and call(k_rate=1.0, k_thrust=1.0) == NO_DEVICE and call(n_sub=4096) == NO_DEVICE
            assert call(f_min=2.0, f_max=2.0) == NO_DEVICE and call(gz=0.0, k_att=0.0) == NO_DEVICE
            assert call(cog_window=0, cog_weight=np.zeros(16)) == NO_DEVICE     # (no weight is read without a filter)
            assert call(cog_window=1, cog_weight=[-1.0]) == NO_DEVICE
            assert call(cog_window=2, cog_weight=np.concatenate([w[:2], [-50.0]])) == NO_DEVICE   # (a weight behind the window is not read)
            assert call(cog_window=16) == NO_DEVICE and call(yaw_cs=0.6, yaw_sn=-0.8) == NO_DEVICE
    assert lib.amk_sim_body_reset(None, 1, GZ, None) == BAD and lib.amk_sim_body_reset(_vp(body), 0, GZ, None) == BAD
    assert lib.amk_sim_body_reset(_vp(body), S, -1.0, None) == BAD and lib.amk_sim_body_reset(_vp(body), S, NAN, None) == BAD
    if lib.amk_device_count() <= 0:
        assert lib.amk_sim_body_reset(_vp(body), S, GZ, None) == NO_DEVICE
    for a in (cmd, x, body, Twb):
        assert (a == 7.0).all()


def test_the_header_states_the_body_contract():
    hdr = open(os.path.join(ROOT, "include", "avoid_mpc_amd.h")).read()
    section = re.sub(r"\s*\*?\s+", " ", hdr[hdr.index("The rigid-body vehicle: a body with an attitude loop"):])
    for sentence in ("clamp(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v), so a NaN passes through", "R00 = 1.0 - 2.0 ((y y) + (z z))",
                     "R21 = 2.0 ((y z) + (w x))", "NO gz is added here, unlike AMK_SIM_ATT_ACCEL", "valid = n > 0 && m > 0",
                     "which is 0.5 (M21 - M12, M02 - M20, M10 - M01)", "wc_i = valid ? clamp(-(k_att e_i), -rate_max, rate_max) : 0.0",
                     "fc = clamp((T_0 R02 + T_1 R12) + T_2 R22, f_min, f_max)", "w_i <- w_i + k_rate (wc_i - w_i); f <- f + k_thrust (fc - f)",
                     "sb = (-(drag_0 vb_0), -(drag_1 vb_1), f - drag_2 vb_2)", "v_i <- v_i + h aw_i, then p_i <- p_i + h v_i with the NEW v",
                     "dw = -(((x w_0) + (y w_1)) + (z w_2))", "nq = sqrt(((w w + x x) + y y) + z z); q_i <- q_i / nq",
                     "sbar = s_0, the newest sample itself, with no division", "sbar = acc / W", "x[3], the yaw, is NOT written",
                     "x[7..9] is an OUTPUT only and never read", "the step leaves these words untouched",
                     "THE SIGN in step 2 is deliberate", "has no minus in front of (2 / attctrl_tau_) error_att", "runs to pi",
                     "is read as 0, so that no state makes the call touch memory that is not the scene's",
                     "Not offered: motor and rotor dynamics, moments and inertia"):
        assert sentence in section, sentence


def test_the_kernels_use_no_scratch(lib):
    """The state, R, T and R_d are 70 VGPRs before a temporary, so eight waves (64 VGPRs) cannot hold the sub-step without scratch
    (csrc/sim_body.hip, REGISTERS): what is held is no scratch, and that the occupancy is the four waves DESIGN.md records."""
    table = json.load(open(amk_build.RES))
    mine = {n: r for n, r in table.items() if "sim_body" in n}
    assert len(mine) == 2 and sum("sim_body_kernel" in n for n in mine) == 1 and sum("sim_body_reset_kernel" in n for n in mine) == 1, sorted(mine)
    for n, r in mine.items():
        print(n, r)                                                             # (the register counts are recorded in DESIGN.md, not gated)
        assert r["scratch_bytes_per_lane"] == 0 and r["occupancy"] >= 4, (n, r)
        assert r["lds_bytes"] == (8 * flight.COG_MAX if "reset" not in n else 0), (n, r)   # the filter's weights and nothing else
    src = open(os.path.join(ROOT, "avoid_mpc_amd", "csrc", "sim_body.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src and "asm" not in src
    assert src.count("__syncthreads()") == 1 and src.index("__syncthreads()") < src.index("if (s >= g.n_scenes) return;")


# ---- defaults ------------------------------------------------------------------------------------------------------------------------
def test_the_defaults_and_the_reference_filters_weights():
    p = flight.body_params(CON_DT)
    assert (p.n_sub, p.gz, p.k_att, p.rate_max, p.f_min, p.f_max, p.drag, p.cog_window) == (33, 9.81, 20.0, 10.0, 0.0, 4 * 9.81, (0.0, 0.0, 0.0), 10)
    assert p.h == CON_DT / 33 and p.k_rate == p.h / 0.03 and p.k_thrust == p.h / 0.05 and (p.yaw_cs, p.yaw_sn) == (1.0, 0.0)
    assert flight.body_params(CON_DT, n_sub=2).k_rate == 1.0                    # min(1, h / tau)
    w = flight.cog_weights()
    assert w.shape == (16,) and w[0] == 1.0 and w[1] == float(np.float32(0.8)) and np.array_equal(w, w.astype(np.float32).astype(np.float64))
    assert np.abs(w - 0.8 ** np.arange(16)).max() < 2.0 ** -24                  # each within a float32 rounding of decay^idx
    assert np.array_equal(p.cog_weight, w)
    b = flight.body_state0(3, GZ)
    assert b.shape == (3, 64) and (b[:, 0] == 1).all() and (b[:, F] == GZ).all() and np.count_nonzero(b) == 6


# ---- the restatement against formulations written differently ------------------------------------------------------------------------
@pytest.mark.parametrize("cog_window", [0, 1, 10])
def test_hover_is_an_exact_fixed_point(cog_window):
    """Level, at rest, cmd = (0, 0, gz): R_d = I, e = 0 and aw = 0 without rounding, so p, v, q, w and f keep their bits through 1000
    sub-steps.  x[7..9] is the filtered IMU sample rotated and less gravity: without the filter it is the newest sample, (0, 0, gz) - gz
    = 0 exactly.  With the filter it is (sum_i w_i gz) / (sum_i w_i) - gz, whose numerator and denominator are rounded separately:
    up to 2 (window - 1) + 1 roundings of a number near gz, which is the bound held here (the value is printed)."""
    prm = flight.body_params(CON_DT, n_sub=100, cog_window=cog_window)
    x0, b0 = _state(2, p=(1.25, -3.5, 1.7))
    x0[:, 3] = 0.3                                                             # the yaw is carried, not used
    cmd = np.tile([0.0, 0.0, GZ], (2, 1))
    x, body = x0, b0
    for _ in range(10):
        x, body, Twb = flight.body_step_ordered(prm, x, body, cmd)
        assert np.array_equal(_bits(x[:, :7]), _bits(x0[:, :7])) and np.array_equal(_bits(body[:, :8]), _bits(b0[:, :8]))
        assert np.array_equal(_bits(Twb[:, :3, :3]), _bits(np.tile(np.eye(3), (2, 1, 1))))
        if cog_window <= 1:
            assert np.array_equal(_bits(x), _bits(x0))
        else:
            print("window", cog_window, "x[9] =", x[0, 9], "=", x[0, 9] / (GZ * 2 * U), "ulp of gz")
            assert (x[:, 7:9] == 0).all() and (np.abs(x[:, 9]) <= (2 * (cog_window - 1) + 1) * U * GZ * (1 + 1e-6)).all()
    assert (body[:, HELD] == 16).all() and (body[:, HEAD] == 1000 % 16).all()
    assert (body[:, RING:RING + 48].reshape(2, 16, 3) == [0.0, 0.0, GZ]).all() and (body[:, 58:] == 0).all()


def _reference_flight(prm, p, v, q, cmd, periods, n_sub, sign=-1.0, tau_rate=None, tau_thrust=None):
    """The independent integrator: rotation MATRICES with matrix products and the exact Rodrigues exponential per step, n_sub sub-steps
    of con_dt / n_sub per period.  sign = -1 is the contract's rate command, +1 the reference's as written.  The lags are
    min(1, h / tau) as the caller of the contract computes them (None: the rates and the thrust follow at once).
    -> (p, v, R, a_w) after every period"""
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    Rd = _acc2rotmat(cmd, prm.yaw_cs, prm.yaw_sn)
    T, g, D = np.asarray(cmd, float), np.array([0.0, 0.0, prm.gz]), np.diag(prm.drag)
    h = CON_DT / n_sub
    k_rate = 1.0 if tau_rate is None else min(1.0, h / tau_rate)
    k_thrust = 1.0 if tau_thrust is None else min(1.0, h / tau_thrust)
    p, v, om, f = np.array(p, float), np.array(v, float), np.zeros(3), float(prm.gz)
    out = []
    for _ in range(periods):
        for _ in range(n_sub):
            M = Rd.T @ R
            e = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
            om = om + k_rate * (np.clip(sign * prm.k_att * e, -prm.rate_max, prm.rate_max) - om)
            f = f + k_thrust * (min(max(T @ R[:, 2], prm.f_min), prm.f_max) - f)
            a = R @ (np.array([0.0, 0.0, f]) - D @ (R.T @ v)) - g
            v = v + h * a
            p = p + h * v
            th = np.linalg.norm(om) * h
            K = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]]) * h
            A, B = (np.sin(th) / th, (1 - np.cos(th)) / th ** 2) if th > 1e-6 else (1 - th * th / 6, 0.5 - th * th / 24)
            R = R @ (np.eye(3) + A * K + B * (K @ K))
        out.append((p.copy(), v.copy(), R.copy(), a.copy()))
    return out


def test_the_attitude_loop_has_the_stable_sign():
    """k_rate = k_thrust = 1, no drag, no rate clamp, a constant command tilted theta_0 = 0.3 rad from the level start.  Then w = -k e,
    e = sin(theta) times the error axis, the axis stays fixed, and the continuous loop is theta' = -k sin(theta) <= -k c theta with
    c = sin(theta_0) / theta_0 (sin(t) / t decreases and theta never exceeds theta_0), so theta(t) <= theta_0 exp(-k c t).
    The explicit step's allowance: normalising q + (h / 2) q (0, w) is EXACTLY the rotation by 2 atan(u / 2) about w, u = h k sin(theta),
    and 2 atan(u / 2) >= u (1 - u^2 / 12); with u <= u_0 = h k sin(theta_0) a step gives theta+ <= theta (1 - h k c (1 - u_0^2 / 12))
    <= theta exp(-h k c (1 - delta)), delta = u_0^2 / 12.  So theta(t) <= theta_0 exp(-k c t (1 - delta)) + FLOOR, where FLOOR stands for
    the roundings of the measurement: nine entries of each rotation of at most four roundings, two products of such matrices, under
    64 roundings of numbers below 1 -- 64 U -- and as much again for the step's own arithmetic near the fixed point."""
    k_att, theta0, periods = 4.0, 0.3, 23
    prm = flight.body_params(CON_DT, k_att=k_att, k_rate=1.0, k_thrust=1.0, rate_max=INF, cog_window=0)
    cmd = 11.0 * np.array([[np.sin(theta0), 0.0, np.cos(theta0)]])               # in the x-z plane: R_d is the pitch by theta_0 itself
    Rd = _acc2rotmat(cmd[0])
    assert abs(_angle(np.eye(3), Rd) - theta0) < 1e-15 * 8
    c, delta, floor = np.sin(theta0) / theta0, (prm.h * k_att * np.sin(theta0)) ** 2 / 12, 128 * U
    bound = lambda t, slack=1.0 - delta: theta0 * np.exp(-k_att * c * t * slack) + floor
    (x, body), theta = _state(), [theta0]
    for t in range(periods):
        x, body, Twb = flight.body_step_ordered(prm, x, body, cmd)
        theta.append(_angle(Rd, _rot(Twb)))
        assert theta[-1] < theta[-2] and theta[-1] <= bound((t + 1) * CON_DT), (t, theta[-1], bound((t + 1) * CON_DT))
    print("theta after %.1f s: %.3g rad (bound %.3g)" % (periods * CON_DT, theta[-1], bound(periods * CON_DT)))
    assert theta[-1] < 1e-4
    # the test's own copy of the loop: with the contract's sign it follows the restatement and keeps the bound (the exponential's step is
    # u itself: no allowance needed); with the reference's sign as written it leaves the bound in the first period and runs to pi
    good = _reference_flight(prm, x[0, :3], (0, 0, 0), (1, 0, 0, 0), cmd[0], periods, prm.n_sub, sign=-1.0)
    flipped = _reference_flight(prm, x[0, :3], (0, 0, 0), (1, 0, 0, 0), cmd[0], 40, prm.n_sub, sign=+1.0)
    for t in range(periods):
        assert _angle(Rd, good[t][2]) <= bound((t + 1) * CON_DT, 1.0)
        assert abs(_angle(Rd, good[t][2]) - theta[t + 1]) <= 1e-3 * theta[t + 1] + floor   # (the two steps differ by O(u^2) per step)
    assert _angle(Rd, flipped[0][2]) > theta0 > bound(CON_DT) and _angle(Rd, flipped[-1][2]) > np.pi - 1e-3
    assert all(_angle(Rd, flipped[t + 1][2]) > _angle(Rd, flipped[t][2]) for t in range(20))


def test_the_steady_state_is_the_commanded_acceleration():
    """The default lags, no drag, a constant command T: the attitude loop with its rate lag is theta'' tau + theta' + k theta = 0 near
    the fixed point, under-damped at 4 k tau = 2.4 > 1 with the envelope exp(-t / (2 tau)) = exp(-16.7 t); the thrust lag decays as
    exp(-t / tau_thrust) = exp(-20 t) (the explicit steps (1 - h / tau)^n decay faster than their exponentials).  With 10 % off the
    slower rate for the coupling and the nonlinearity, what remains after t seconds of an initial error E is below 4 E exp(-15 t):
    E = theta_0 |T| + |f_0 - |T|| in acceleration, theta_0 in angle.  At t = 3 s that is 1e-18 of E, so the tolerance is the rounding
    floor of the expressions compared: under 64 roundings of numbers of size |T|."""
    prm = flight.body_params(CON_DT, cog_window=10)
    T = np.array([[3.0, -2.0, GZ + 1.0]])
    Rd = _acc2rotmat(T[0])
    theta0, nT = _angle(np.eye(3), Rd), float(np.linalg.norm(T))
    x, body = _state()
    for _ in range(30):
        x, body, Twb = flight.body_step_ordered(prm, x, body, T)
    left = 4.0 * np.exp(-15.0 * 30 * CON_DT)
    tol_a, tol_R = left * (theta0 * nT + abs(GZ - nT)) + 64 * U * nT, left * theta0 + 64 * U
    assert tol_a < 1e-13 and tol_R < 1e-14
    a_w = _rot(Twb) @ body[0, RING + 3 * ((int(body[0, HEAD]) - 1) % 16):][:3] - [0, 0, GZ]     # R s_b - g of the last sub-step
    print("a_w - (T - g):", a_w - (T[0] - [0, 0, GZ]), "angle to R_d:", _angle(Rd, _rot(Twb)), "tolerances", tol_a, tol_R)
    assert np.abs(a_w - (T[0] - [0, 0, GZ])).max() <= tol_a and np.abs(x[0, 7:10] - (T[0] - [0, 0, GZ])).max() <= tol_a
    assert _angle(Rd, _rot(Twb)) <= tol_R and np.abs(_rot(Twb) - Rd).max() <= tol_R
    assert abs(body[0, F] - nT) <= tol_a and np.abs(body[0, RATE:RATE + 3]).max() <= 20.0 * tol_R


def test_the_quaternion_and_the_rotation_stay_normal_to_a_few_roundings():
    """10^4 sub-steps under a wandering command.  Every sub-step ends in q / sqrt(q.q), so nothing accumulates: the computed q.q carries
    at most 4 U relative (three additions and the products), its root 2 U + U, each quotient U, so the exact |q|^2 - 1 is within
    2 (3 U + U) = 8 U.  R(q) of a q with |q|^2 = 1 + eps is (1 + eps) Rot - eps I, so R^T R - I has entries within 4 |eps| + O(eps^2), and
    each entry of R carries at most four roundings of numbers below 1 (4 U), which R^T R sees twice through rows of 1-norm <= sqrt(3):
    14 U.  Both are measured in exact rational arithmetic on the doubles the restatement returns."""
    prm = flight.body_params(CON_DT, n_sub=100, drag=(0.1, 0.1, 0.05))
    rng = np.random.default_rng(5)
    x, body = _state(2)
    worst_q = worst_R = fractions.Fraction(0)
    for call in range(100):
        cmd = np.array([0.0, 0.0, GZ]) + rng.uniform(-6.0, 6.0, (2, 3))
        x, body, Twb = flight.body_step_ordered(prm, x, body, cmd)
        for s in range(2):
            q = [fractions.Fraction(float(v)) for v in body[s, Q:Q + 4]]
            worst_q = max(worst_q, abs(sum(v * v for v in q) - 1))
            R = [[fractions.Fraction(float(Twb[s, i, j])) for j in range(3)] for i in range(3)]
            for i in range(3):
                for j in range(3):
                    worst_R = max(worst_R, abs(sum(R[k][i] * R[k][j] for k in range(3)) - (i == j)))
    print("|q.q - 1| <= %.2f U, |R^T R - I| <= %.2f U" % (float(worst_q) / U, float(worst_R) / U))
    assert worst_q <= 8 * U * (1 + 1e-9) and worst_R <= (4 * 8 + 14) * U
    assert np.isfinite(x).all() and np.abs(body[:, RATE:RATE + 3]).max() > 0.1   # and the body did turn


def test_the_position_converges_at_first_order_to_an_independent_integrator():
    """cmd = (3, -2, gz + 1), drag (0.1, 0.1, 0.05), the default lags, 30 periods: the position error against the rotation-matrix
    integrator at 2048 sub-steps per period halves with each doubling of n_sub.  The scheme is first order and so is the yardstick, so
    the ratio is (1 / n - 1 / 2048) / (1 / 2n - 1 / 2048): 2.008, 2.016, 2.03."""
    cmd, drag, periods = np.array([[3.0, -2.0, GZ + 1.0]]), (0.1, 0.1, 0.05), 30
    fine = flight.body_params(CON_DT, drag=drag)
    p_ref = _reference_flight(fine, (0.0, 0.0, 1.0), (0, 0, 0), (1, 0, 0, 0), cmd[0], periods, 2048, tau_rate=0.03, tau_thrust=0.05)[-1][0]
    err = []
    for n_sub in (8, 16, 32, 64):
        prm = flight.body_params(CON_DT, n_sub=n_sub, drag=drag)
        assert prm.k_rate == min(1.0, prm.h / 0.03) and prm.k_thrust == prm.h / 0.05
        x, body = _state()
        for _ in range(periods):
            x, body, _ = flight.body_step_ordered(prm, x, body, cmd)
        err.append(float(np.linalg.norm(x[0, :3] - p_ref)))
    ratios = [err[i] / err[i + 1] for i in range(3)]
    print("position errors", err, "ratios", ratios)
    assert all(1.6 <= r <= 2.4 for r in ratios), ratios
    assert err[-1] < 0.05 * np.linalg.norm(x[0, :3] - [0.0, 0.0, 1.0])          # and the error is small beside the distance flown


@pytest.mark.parametrize("cog_window", [0, 1, 2, 10, 16])
def test_the_cog_filter_against_a_deque(cog_window):
    """A twin flight of one-sub-step calls without a filter collects the samples; a deque holds them as COGFilter.cpp does (push back,
    pop the front beyond the window, the weighted mean from the newest); the flight under test runs the same sub-steps in calls of 1,
    2, 3, 5, 7, 4, 9 and 20 sub-steps, so the window fills from empty, wraps the 16-slot ring and crosses call boundaries part-filled."""
    kw = dict(drag=(0.3, 0.1, 0.2), h=CON_DT / 33)
    cmd = np.array([[2.0, 1.0, GZ + 0.5], [-1.0, 2.5, GZ - 1.0]])
    one = flight.body_params(CON_DT, n_sub=1, cog_window=0, **kw)
    weights = flight.cog_weights()
    (xa, ba), (xb, bb) = _state(2, v=(1.0, -0.5, 0.2)), _state(2, v=(1.0, -0.5, 0.2))
    window = [collections.deque(), collections.deque()]
    for n_sub in (1, 2, 3, 5, 7, 4, 9, 20):
        for _ in range(n_sub):
            xa, ba, _ = flight.body_step_ordered(one, xa, ba, cmd)
            for s in range(2):
                head = int(ba[s, HEAD])
                window[s].append([float(v) for v in ba[s, RING + 3 * ((head - 1) % 16):][:3]])
                if len(window[s]) > max(cog_window, 1):
                    window[s].popleft()
        xb, bb, Twb = flight.body_step_ordered(flight.body_params(CON_DT, n_sub=n_sub, cog_window=cog_window, **kw), xb, bb, cmd)
        assert np.array_equal(_bits(xa[:, :7]), _bits(xb[:, :7])) and np.array_equal(_bits(ba), _bits(bb))
        for s in range(2):
            assert len(window[s]) == min(int(bb[s, HELD]), max(cog_window, 1)) or cog_window == 0
            if cog_window <= 1:
                mean = window[s][-1]
            else:
                total, acc = 0.0, None
                for idx, sample in enumerate(reversed(window[s])):
                    wt = float(weights[idx])
                    acc = [wt * v for v in sample] if acc is None else [a + wt * v for a, v in zip(acc, sample)]
                    total = wt if idx == 0 else total + wt
                mean = [a / total for a in acc]
            R = Twb[s, :3, :3]
            want = [(float(R[i, 0]) * mean[0] + float(R[i, 1]) * mean[1]) + float(R[i, 2]) * mean[2] for i in range(3)]
            want[2] = want[2] - GZ
            assert np.array_equal(_bits(xb[s, 7:10]), _bits(np.array(want))), (n_sub, s, xb[s, 7:10], want)


def test_one_call_equals_two_calls_of_its_parts():
    rng = np.random.default_rng(11)
    S = 5
    cmd = np.array([0.0, 0.0, GZ]) + rng.uniform(-4.0, 4.0, (S, 3))
    x0, b0 = _state(S, v=(0.5, 0.2, -0.1))
    b0[:, 58:] = rng.uniform(-1, 1, (S, 6))                                     # the unused tail is carried untouched
    kw = dict(drag=(0.2, 0.1, 0.05), h=CON_DT / 33, yaw_cs=0.8, yaw_sn=0.6)
    warm = flight.body_step_ordered(flight.body_params(CON_DT, n_sub=7, **kw), x0, b0, cmd[::-1], 1e6)   # off the reset state
    for a, b in ((1, 1), (3, 30), (20, 13), (16, 17)):
        whole = flight.body_step_ordered(flight.body_params(CON_DT, n_sub=a + b, **kw), warm[0], warm[1], cmd, 1e6)
        first = flight.body_step_ordered(flight.body_params(CON_DT, n_sub=a, **kw), warm[0], warm[1], cmd, 1e6)
        second = flight.body_step_ordered(flight.body_params(CON_DT, n_sub=b, **kw), first[0], first[1], cmd, 1e6)
        for name, u, v in zip(("x", "body", "Twb"), whole, second):
            assert np.array_equal(_bits(u), _bits(v)), (a, b, name)
        assert np.array_equal(_bits(whole[1][:, 58:]), _bits(b0[:, 58:])) and np.array_equal(_bits(whole[0][:, 3]), _bits(x0[:, 3]))
    assert np.array_equal(_bits(warm[2][:, :3, 3]), _bits(np.rint(warm[0][:, :3] * 1e6) / 1e6)) and (warm[2][:, 3] == [0, 0, 0, 1]).all()
    assert not np.array_equal(warm[0], x0) and not np.may_share_memory(warm[0], x0)


def test_body_frame_drag_is_what_an_affine_model_cannot_hold():
    """Pitched about y by the 3-4-5 angle (cos 0.8, sin 0.6), flying along world x at 1 m/s, drag 1 / s on the body's x axis only, no
    thrust, no gravity, no attitude gain: the body's x axis is (0.8, 0, -0.6), v_b0 = 0.8, and the drag is -0.8 (0.8, 0, -0.6) =
    (-0.64, 0, +0.48) in the world: a VERTICAL acceleration out of a purely horizontal velocity, which no per-axis k_i v_i gives."""
    prm = flight.body_params(CON_DT, n_sub=1, gz=0.0, k_att=0.0, f_min=0.0, f_max=0.0, drag=(1.0, 0.0, 0.0), cog_window=0)
    x, body = _state(1, v=(1.0, 0.0, 0.0))
    body[0, Q:Q + 4] = [np.sqrt(0.9), 0.0, np.sqrt(0.1), 0.0]
    body[0, F] = 0.0
    x1, b1, Twb = flight.body_step_ordered(prm, x, body, np.array([[0.6, 0.0, 0.8]]))
    assert np.abs(_rot(Twb) - [[0.8, 0, 0.6], [0, 1, 0], [-0.6, 0, 0.8]]).max() < 8 * U
    assert np.abs(x1[0, 7:10] - [-0.64, 0.0, 0.48]).max() < 8 * U
    assert np.abs(x1[0, 4:7] - (np.array([1.0, 0, 0]) + prm.h * np.array([-0.64, 0, 0.48]))).max() < 8 * U and x1[0, 6] > 0
