"""CPU: tests/_gamma_ref.py proven before the device is compared with it -- the jet restatement's value against the numpy twin, its
gradient against central differences of the twin (the differences' own error: this proves the reference; the device is compared with
the reference, not with differences), and the case table reaching what it names."""
import numpy as np
import pytest

from avoid_mpc_amd import synth
from tests import _gamma_ref as G
from tests import _oracle, _pose

M = G.M
CASES = [c[:3] for c in G.CASES]


def _twin_gamma(x, p, N, K, dt, lam_f, lam_g):
    return lam_f * M.nlp_f(x, p, N, K) + lam_g @ M.nlp_g(x, p, N, K, dt)


@pytest.mark.parametrize("N,K,pset", CASES, ids=G.CASE_IDS)
def test_value_matches_the_numpy_twin(N, K, pset):
    c = G.case_inputs(N, K, pset)
    val, _, _ = G.case_reference(N, K, pset)
    with _oracle.oracle_drag(c["prm"].drag):
        for s in range(G.S):
            tw = _twin_gamma(c["W"][s], c["P"][s], N, K, c["prm"].dt, c["lam_f"][s], c["lam_g"][s])
            print(N, K, pset, s, abs(val[s] - tw) / abs(tw))
            assert abs(val[s] - tw) <= 1e-13 * abs(tw)


@pytest.mark.parametrize("i", range(len(CASES)), ids=G.CASE_IDS)
def test_gradient_matches_central_differences_of_the_twin(i):
    """Step 1e-6 max(1, |p_i|); all entries where np < 800, else a fixed random 200 and the whole tail; bound 1e-9 max|grad|: the
    truncation and rounding error of the differences (measured 2.3e-6 on 9e4).  One scene per case, another one from case to case
    (scene 0 holds the exact yaws, scene 1 the zero-velocity stage)."""
    N, K, pset = CASES[i]
    s = i % G.S
    c = G.case_inputs(N, K, pset)
    grad = G.case_reference(N, K, pset)[1][s]
    npar = M.p_len(N, K)
    idx = np.arange(npar)
    if npar >= 800:
        idx = np.unique(np.concatenate([np.random.default_rng(7).choice(npar - 34, 200, replace=False), np.arange(npar - 34, npar)]))
    p = c["P"][s]
    worst = 0.0
    with _oracle.oracle_drag(c["prm"].drag):
        for j in idx:
            h = 1e-6 * max(1.0, abs(p[j])); e = np.zeros(npar); e[j] = h
            fd = (_twin_gamma(c["W"][s], p + e, N, K, c["prm"].dt, c["lam_f"][s], c["lam_g"][s])
                  - _twin_gamma(c["W"][s], p - e, N, K, c["prm"].dt, c["lam_f"][s], c["lam_g"][s])) / (2 * h)
            worst = max(worst, abs(grad[j] - fd))
    print(N, K, pset, "scene", s, "worst |ref - fd|", worst, "on", np.abs(grad).max())
    assert worst <= 1e-9 * np.abs(grad).max()


def test_set_b_has_no_zero_weight_and_no_equal_rotated_pair():
    w = _pose.B["weights"]
    assert all(v != 0.0 for v in w) and w[10] != w[11] and w[14] != w[15]
    assert all(v > 0.0 for v in _pose.B["drag"]) and len(set(_pose.B["drag"])) == 3 and len(set(_pose.B["tau"][:3])) == 3
    d = synth.DEFAULT_WEIGHTS
    assert [i for i in range(25) if d[i] == 0.0] == [7, 8, 9, 10, 14, 17]


def test_the_table_spans_the_lane_map():
    """(N K) mod 64 and the trips of `for (e = lane; e < N * K; e += 64)`."""
    got = {(N, K): ((N * K) % 64, -(-N * K // 64)) for N, K, _ in CASES}
    assert got == {(2, 1): (2, 1), (2, 64): (0, 2), (7, 0): (0, 0), (7, 3): (21, 1), (10, 3): (30, 1), (17, 64): (0, 17),
                   (20, 8): (32, 3), (30, 8): (48, 4), (32, 64): (0, 32)}
    assert {(N, K) for N, K, p in CASES if p == "default"} == {(2, 1), (7, 3), (10, 3), (20, 8), (32, 64)}
    assert sum(p == "B" for _, _, p in CASES) == 7


@pytest.mark.parametrize("N,K,pset", [c for c in CASES if c[1] > 0], ids=[i for i, c in zip(G.CASE_IDS, CASES) if c[1] > 0])
def test_every_case_has_live_padded_and_still_terms(N, K, pset):
    c = G.case_inputs(N, K, pset)
    _, grad, _ = G.case_reference(N, K, pset)
    o0 = 10 + 10 * N
    live = padded = 0
    signs = set()
    for s in range(G.S):
        rows = np.abs(grad[s, o0:o0 + 3 * N * K]).reshape(N, K, 3).max(-1)
        rho, sv, radius = G.term_geometry(c["W"][s], c["P"][s], N, K)
        pad = M.split_p(c["P"][s], N, K)["obs"][:, :, 0] == 1e4
        # no live term in the subnormal range: exp underflows to exactly 0 or stays a normal number, for every term
        ex = np.exp(-32.0 * (rho - radius))
        assert np.all((ex == 0.0) | (ex >= 1e-280))
        assert np.all(rows[pad] == 0.0) and np.all(rows[N - 1] == 0.0)
        live += int((rows[:N - 1] > 1e-6).sum()); padded += int(pad[:N - 1].sum())
        signs |= set(np.sign(sv[:N - 1][rows[:N - 1] > 1e-6]))
        if s == 1:
            kz = G.zero_velocity_stage(N)
            assert not sv[kz].any() and not grad[s, o0 + 3 * K * kz:o0 + 3 * K * (kz + 1)].any()
            assert not pad[kz].all()       # ... and not because the stage holds padding only
    print(N, K, pset, "live", live, "padded", padded)
    # both signs of sv among the live terms; (2, 1) has one term per scene, scene 1's still: one live term and one padded one is all it holds
    assert live > 0 and padded > 0 and (signs == {-1.0, 1.0} or (N, K) == (2, 1))


@pytest.mark.parametrize("N,K", [(N, K) for N, K, p in CASES if p == "default"])
def test_default_weights_leave_half_of_the_yaw_entry_unevaluated(N, K):
    """The path px and vx weights (indices 10 and 14) are 0 in the default set, so the parts of d gamma / d yaw_ref they multiply are
    identically 0 there: the yaw entries are linear in the two weights (the reference at the weights perturbed once and twice as far differs
    from the default by d and 2 d), and d is not zero on any path stage.  This is why set B is in the table."""
    c = G.case_inputs(N, K, "default")
    s = 0
    yaw = slice(13, 13 + 10 * (N - 1), 10)
    tail = M.p_len(N, K) - 34
    g0 = G.case_reference(N, K, "default")[1][s][yaw]
    out = []
    for t in (1.0, 2.0):
        p = c["P"][s].copy()
        assert p[tail + 18] == 0.0 and p[tail + 22] == 0.0
        p[tail + 18] = 7.0 * t; p[tail + 22] = 0.5 * t
        out.append(G.gamma_ref(c["W"][s], p, N, K, c["prm"].dt, c["lam_f"][s], c["lam_g"][s], c["prm"].drag)[1][yaw])
    d1, d2 = out[0] - g0, out[1] - g0
    assert np.all(d1 != 0.0) and np.abs(d1).max() > 0.1 and np.abs(d2 - 2 * d1).max() <= 1e-12 * np.abs(d1).max()


def test_scene_zero_holds_the_exact_yaws():
    for N, K, pset in CASES:
        R = G.case_inputs(N, K, pset)["R"]
        yaws = R[:, 13:10 + 10 * N:10]
        assert np.all((yaws > -np.pi) & (yaws <= np.pi)) and np.abs(yaws).max() > 0.6
        if N >= 7:
            assert tuple(yaws[0, :4]) == G.EXACT_YAWS
