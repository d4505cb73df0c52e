"""GPU: amk_mpc_eval_gamma's grad_p over the WHOLE parameter vector against the forward-mode reference of tests/_gamma_ref.py, at every
row of its case table (tests/test_gamma_ref.py proves the reference and the table on the CPU), in the device form on torch tensors
and through amk_mpc_eval_gamma_host, which must agree bit for bit.

The rule is per natural row (a stage's ten reference entries, a term's three obstacle coordinates, the target, Q_goal, every other
tail entry alone): |gpu - ref| <= RTOL * (largest |ref| of the row), RTOL that of tests/test_mpc_eval_gpu.py (same arithmetic, other
summation order, ocml against libm); the tau entries, signed sums, against RTOL * the sum of their addends' absolute values.  Rows
whose reference is exactly zero (padded obstacles, the zero-velocity stage) and the structural zeros (reference and obstacle stage
N - 1, the gains, tau_yaw) must be exactly zero.  A block-wide maximum would hide a far obstacle's row behind a near one."""
import ctypes as C

import numpy as np
import pytest

from tests import _gamma_ref as G
from tests.test_mpc_eval_gpu import RTOL

pytestmark = pytest.mark.gpu
CASES = [c[:3] for c in G.CASES]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _gamma_device(m, W, R, lam_f, lam_g, want_gx=True, want_gp=True, fill=None):
    """amk_mpc_eval_gamma on torch tensors (None: the NULL pointer) -> (grad_x, grad_p) as numpy, None where not asked for.
    fill: the outputs start from this value, not from torch.empty's."""
    import torch
    from avoid_mpc_amd import capi
    S = m.S
    dev = lambda a: None if a is None else torch.from_numpy(np.array(a, np.float64)).cuda()
    mk = lambda n: torch.full((S, n), float(fill), dtype=torch.float64, device="cuda") if fill is not None else \
        torch.empty((S, n), dtype=torch.float64, device="cuda")
    gx = mk(m.nx) if want_gx else None
    gp = mk(m.lib.amk_mpc_np(m.h)) if want_gp else None
    ins = [dev(W), dev(R), dev(lam_f), dev(lam_g)]
    capi.check(m.lib.amk_mpc_eval_gamma(m.h, *[capi.dptr(t) for t in ins], capi.dptr(gx), capi.dptr(gp), capi.stream_ptr(None)),
               "amk_mpc_eval_gamma")
    torch.cuda.synchronize()
    return (None if gx is None else gx.cpu().numpy()), (None if gp is None else gp.cpu().numpy())


def _gamma_host(m, W, R, lam_f, lam_g):
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    W, R, lam_f, lam_g = (np.array(a, np.float64) for a in (W, R, lam_f, lam_g))
    gx = np.zeros((m.S, m.nx)); gp = np.zeros((m.S, m.lib.amk_mpc_np(m.h)))
    assert m.lib.amk_mpc_eval_gamma_host(m.h, vp(W), vp(R), vp(lam_f), vp(lam_g), vp(gx), vp(gp)) == 0
    return gx, gp


def _configured(prm, S):
    from avoid_mpc_amd.host import MpcBatch
    m = MpcBatch(prm.T, prm.dt, prm.K, S); m.configure(prm)
    return m


def _by_setters(prm, S, tau, drag):
    """A handle that gets the weights, gains, limits and radius of prm by separate setter calls (not by configure), then tau and, where
    drag is not None, the drag."""
    from avoid_mpc_amd.host import MpcBatch
    m = MpcBatch(prm.T, prm.dt, prm.K, S)
    m.SetupWeights(prm.weights); m.SetupGains(prm.gain)
    m.SetDroneAccelLimits(prm.a_min_z, prm.a_max_z, prm.a_max_xy, prm.a_max_yaw_dot); m.SetDroneRadius(prm.radius)
    m.SetupTau(tau)
    if drag is not None:
        m.SetDragCoefficient(*drag)
    return m


@pytest.mark.parametrize("N,K,pset", CASES, ids=G.CASE_IDS)
def test_grad_p_matches_the_reference_row_by_row(N, K, pset):
    import torch
    c = G.case_inputs(N, K, pset)
    _, ref, tau_abs = G.case_reference(N, K, pset)
    prm, W, R, lam_f, lam_g = c["prm"], c["W"], c["R"], c["lam_f"], c["lam_g"]
    S, nx, ng = G.S, 10 + 14 * N, 10 + 10 * N
    m = _configured(prm, S)
    assert m.lib.amk_mpc_np(m.h) == ref.shape[1]
    gx, gp = _gamma_device(m, W, R, lam_f, lam_g)
    worst = {b: 0.0 for b in G.BLOCKS}
    bad = []
    for s in range(S):
        w, b = G.compare_rows(gp[s], ref[s], tau_abs[s], N, K, RTOL)
        worst = {k: max(worst[k], w[k]) for k in worst}
        bad += [(s,) + r for r in b]
    print("gamma rows", N, K, pset, " ".join("%s %.1e" % (k, worst[k]) for k in G.BLOCKS))
    assert not bad, bad[:20]
    for s in range(S):
        assert np.array_equal(gp[s, :10], -lam_g[s, :10])                 # x_init: g[0:10] = X_0 - x_init, exactly
    gxh, gph = _gamma_host(m, W, R, lam_f, lam_g)
    assert _same_bits(gx, gxh) and _same_bits(gp, gph)                    # the two forms, bit for bit
    # grad_x of the same launches: lam_f grad f + J' lam_g from amk_mpc_eval's own outputs, the existing identity and its bound
    out = m.eval(torch.from_numpy(W.copy()).cuda(), torch.from_numpy(R.copy()).cuda(), None, want=("grad_f", "jac_g"))
    torch.cuda.synchronize()
    grad_f, jac = out["grad_f"].cpu().numpy(), out["jac_g"].cpu().numpy()
    jc, jr = m.sparsity("jac_g")
    for s in range(S):
        Jd = np.zeros((ng, nx))
        for col in range(nx):
            Jd[jr[jc[col]:jc[col + 1]], col] = jac[s][jc[col]:jc[col + 1]]
        want = lam_f[s] * grad_f[s] + Jd.T @ lam_g[s]
        assert np.abs(gx[s] - want).max() <= 1e-12 * np.abs(want).max()
    # the scene stride: scene 2 alone in a one-scene handle returns the same bits
    m1 = _configured(prm, 1)
    gx1, gp1 = _gamma_device(m1, W[2:3], R[2:3], lam_f[2:3], lam_g[2:3])
    assert _same_bits(gx1[0], gx[2]) and _same_bits(gp1[0], gp[2])


@pytest.mark.parametrize("N,K", [(7, 3), (20, 8)])
def test_null_conventions(N, K):
    c = G.case_inputs(N, K, "B")
    prm, W, R, lam_f, lam_g = c["prm"], c["W"], c["R"], c["lam_f"], c["lam_g"]
    S = G.S
    m = _configured(prm, S)
    tail = 20 + 10 * N + 3 * K * N
    gx, gp = _gamma_device(m, W, R, lam_f, lam_g)
    # d_lam_f == NULL is 1.0
    a = _gamma_device(m, W, R, None, lam_g)
    b = _gamma_device(m, W, R, np.ones(S), lam_g)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and not _same_bits(a[1], gp)
    # d_lam_g == NULL is zero multipliers
    a = _gamma_device(m, W, R, lam_f, None)
    b = _gamma_device(m, W, R, lam_f, np.zeros_like(lam_g))
    assert not a[1][:, :10].any() and not a[1][:, tail + 4:tail + 8].any()
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and not _same_bits(a[1], gp)
    # an output not asked for leaves the other one's bits unchanged (the outputs start from a fill the kernel must overwrite)
    only_x = _gamma_device(m, W, R, lam_f, lam_g, want_gp=False, fill=np.nan)
    only_p = _gamma_device(m, W, R, lam_f, lam_g, want_gx=False, fill=np.nan)
    assert only_x[1] is None and only_p[0] is None
    assert _same_bits(only_x[0], gx) and _same_bits(only_p[1], gp)


@pytest.mark.parametrize("N,K", [(7, 3), (20, 8)])
def test_live_handle_dtau_cache(N, K):
    """d(A, B, c)/d tau is cached on the handle (ev_dtau) and depends on tau AND on the drag: a handle whose tau or drag changed after a
    first call against a fresh handle, device against device, bit for bit."""
    from avoid_mpc_amd import synth
    c = G.case_inputs(N, K, "B")
    prm, W, R, lam_f, lam_g = c["prm"], c["W"], c["R"], c["lam_f"], c["lam_g"]
    S = G.S
    tail = 20 + 10 * N + 3 * K * N
    tau_b, drag_b, tau_d, drag_2 = list(prm.tau), tuple(prm.drag), list(synth.DEFAULT_TAU), (0.1, 0.05, 0.02)
    assert tau_b != tau_d and drag_b != drag_2 and all(drag_b)
    call = lambda h: _gamma_device(h, W, R, lam_f, lam_g)
    fresh_b = call(_by_setters(prm, S, tau_b, drag_b))
    fresh_d = call(_by_setters(prm, S, tau_d, None))
    fresh_2 = call(_by_setters(prm, S, tau_b, drag_2))
    assert not _same_bits(fresh_b[1][:, tail + 4:tail + 7], fresh_d[1][:, tail + 4:tail + 7])
    # 1. set B's tau and drag, then the default tau and no drag on the same handle
    m = _by_setters(prm, S, tau_b, drag_b)
    first = call(m)
    assert _same_bits(first[0], fresh_b[0]) and _same_bits(first[1], fresh_b[1])
    m.SetupTau(tau_d); m.SetDragCoefficient(0.0)
    again = call(m)
    assert _same_bits(again[0], fresh_d[0]) and _same_bits(again[1], fresh_d[1])
    # 2. the other way round
    m = _by_setters(prm, S, tau_d, None)
    first = call(m)
    assert _same_bits(first[0], fresh_d[0]) and _same_bits(first[1], fresh_d[1])
    m.SetupTau(tau_b); m.SetDragCoefficient(*drag_b)
    again = call(m)
    assert _same_bits(again[0], fresh_b[0]) and _same_bits(again[1], fresh_b[1])
    # 3. the drag alone, tau unchanged
    m = _by_setters(prm, S, tau_b, drag_b)
    first = call(m)
    m.SetDragCoefficient(*drag_2)
    again = call(m)
    assert _same_bits(again[0], fresh_2[0]) and _same_bits(again[1], fresh_2[1])
    assert np.all(again[1][:, tail + 4:tail + 7] != first[1][:, tail + 4:tail + 7])
