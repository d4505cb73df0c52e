"""CPU: the table of tests/_mpc_kn_cases.py does what it says -- every seed passes the admission conditions, the arrangements
put live collision terms where the device's later rounds are, the lane-map shapes the table claims are all there, and the oracle
itself is sound at the ends of the range (all-padding == K = 0 bit for bit; C == numpy twin at K = 0 and at N = 32, K = 64).
No GPU: what tests/test_mpc_kn_gpu.py compares the device WITH is checked here."""
import os
import sys

import numpy as np
import pytest

from tests import _mpc_kn_cases as KN
from tests import _oracle

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import mpc_oracle_np as M  # noqa: E402

IDS = [f"N{r.N}K{r.K}" for r in KN.ROWS]


def test_the_table_covers_the_lane_map_shapes():
    """(per, idle, K % per) of every row; the file fails if the table loses its K = 0, per = 64, no-idle-lane or
    one-slot-last-round rows, a row's seed count leaves 4 .. 8, or a passed-over seed is also used."""
    got = {(r.N, r.K): (KN.geometry(r.N, r.K)[1], KN.geometry(r.N, r.K)[3], r.K % KN.geometry(r.N, r.K)[1]) for r in KN.ROWS}
    assert got == {(2, 0): (64, 0, 0), (10, 0): (7, 1, 0), (10, 1): (7, 1, 1), (10, 7): (7, 1, 0), (10, 8): (7, 1, 1),
                   (10, 9): (7, 1, 2), (2, 64): (64, 0, 0), (3, 33): (32, 0, 1), (17, 64): (4, 0, 0), (20, 10): (3, 7, 1),
                   (22, 64): (3, 1, 1), (30, 33): (2, 6, 1), (30, 64): (2, 6, 0), (32, 64): (2, 2, 0)}
    rows = {(r.N, r.K): KN.geometry(r.N, r.K) for r in KN.ROWS}
    assert sum(K == 0 for _, K in rows) >= 2                                                       # generic and baked
    assert any(g[1] == 64 and K == 64 for (_, K), g in rows.items())                               # per = 64, full
    assert any(g[3] == 0 and g[2] >= 16 for g in rows.values())                                    # no idle lane, many rounds
    assert sum(g[4] == 1 and g[2] >= 2 for g in rows.values()) >= 4                                # one slot in the last round
    assert {g[2] for (_, K), g in rows.items() if K} >= {1, 2, 4, 16, 17, 22, 32}                  # rounds
    for (N, K), (ns, per, rounds, idle, last) in rows.items():
        assert ns * per + idle == 64 and per * (rounds - 1) < max(K, 1) <= max(per * rounds, 1)
    for r in KN.ROWS:
        assert 4 <= len(r.seeds) <= 8 and len(set(r.seeds)) == len(r.seeds) and not set(r.seeds) & set(r.passed_over), r
        assert r.kernel == ("baked" if r.N in (10, 20, 30) else "generic")


def test_arrangements_move_the_obstacle_block_only():
    N, K = 20, 10
    rec = KN.records(N, K)
    o0, t0 = 10 + 10 * N, 10 + 10 * N + 3 * K * N
    p = KN.obstacle_block(rec["packed"], N, K)
    for a in KN.ARRANGEMENTS:
        assert np.array_equal(rec[a][:, :o0], rec["packed"][:, :o0]) and np.array_equal(rec[a][:, t0:], rec["packed"][:, t0:])
    d = np.linalg.norm(p - rec["packed"][:, 10:o0].reshape(-1, N, 10)[:, :, None, :3], axis=3)
    assert np.all(np.diff(d, axis=2) >= 0)                                         # packed: ascending distance
    assert np.array_equal(KN.obstacle_block(rec["reversed"], N, K), p[:, :, ::-1])
    lo = KN.obstacle_block(rec["last_only"], N, K)
    assert np.all(lo[:, :, :K - 1] == KN.PAD) and np.array_equal(lo[:, :, K - 1], p[:, :, 0])
    assert np.all(KN.obstacle_block(rec["all_pad"], N, K) == KN.PAD)
    names, ref = KN.batch(N, K)
    assert names == list(KN.ARRANGEMENTS) and ref.shape == (4 * len(KN.row(N, K).seeds), 20 + 10 * N + 3 * K * N)


@pytest.mark.parametrize("r", KN.ROWS, ids=IDS)
def test_every_seed_passes_admission(r):
    """Status 0 within half the iteration cap, unmoved by eight 1e-13 perturbations, and (reversed, last_only) a live term in the
    last round of every scene: for every arrangement of every scene of the row."""
    prm = KN.prm_of(r.N, r.K)
    sols = KN.oracle_solutions(r.N, r.K)
    for a, R in KN.records(r.N, r.K).items():
        for s, seed in enumerate(r.seeds):
            why = KN.admit(prm, R[s], a, sols[a][s])
            assert why is None, (r.N, r.K, seed, why)
    its = [int(sol["info"][1]) for a in sols for sol in sols[a]]
    reg = [int(sol["info"][2]) for a in sols for sol in sols[a]]
    print(f"N = {r.N}, K = {r.K}: iterations {min(its)} .. {max(its)}, regularisations <= {max(reg)}")


@pytest.mark.parametrize("N,K", sorted({(r.N, r.K) for r in KN.STEP_ROWS}))
def test_every_step_scene_passes_admission(N, K):
    """The control-step scenes: every step converges and re-plans or solves at least once, and flags, u, x0array and the refilled
    reference path of both steps are unmoved by eight 1e-13 perturbations of the state quads and the reference path."""
    prm, scenes = KN.step_scenes(N, K)
    rows = [r for r in KN.STEP_ROWS if (r.N, r.K) == (N, K)]
    assert all(len(r.seeds) == 6 and r.seeds == rows[0].seeds and not set(r.seeds) & set(r.passed_over) for r in rows)
    for seed, sc in zip(rows[0].seeds, scenes):
        assert len(sc["cloud"]) == 50000
        why = KN.admit_step_scene(prm, sc)
        assert why is None, (N, K, seed, why)


def test_the_step_rows_are_the_ones_asked_for():
    assert [(r.N, r.K, r.tie_order) for r in KN.STEP_ROWS] == [(20, 1, 0), (20, 10, 0), (20, 33, 0), (20, 64, 0), (32, 64, 0), (20, 10, 1),
                                                               (20, 63, 2)]


@pytest.mark.parametrize("r", [r for r in KN.ROWS if r.K >= 2], ids=[i for i, r in zip(IDS, KN.ROWS) if r.K >= 2])
def test_live_terms_sit_where_the_row_says(r):
    """At the oracle's solution of `packed`: one scene at least has live and dormant terms, half the scenes at least have a live term
    in slot K - 1; at the solutions of `reversed` and `last_only` every scene has a live term in the last round."""
    prm = KN.prm_of(r.N, r.K)
    rec, sols = KN.records(r.N, r.K), KN.oracle_solutions(r.N, r.K)
    live = {a: [KN.live_terms(prm, rec[a][s], sols[a][s]["w"]) for s in range(len(r.seeds))] for a in rec}
    assert any(m.any() and not m.all() for m in live["packed"])
    assert 2 * sum(bool(m[:, r.K - 1].any()) for m in live["packed"]) >= len(r.seeds)
    for a in ("reversed", "last_only"):
        assert all(m[:, KN.last_round(r.N, r.K)].any() for m in live[a]), a
    assert not any(m.any() for m in live["all_pad"])
    if (r.N, r.K) == (2, 64):
        assert sum(bool(m.any()) for m in live["packed"]) >= 2
    print(f"N = {r.N}, K = {r.K}: live terms per scene (packed) {[int(m.sum()) for m in live['packed']]} of {(r.N - 1) * r.K}")


@pytest.mark.parametrize("r", [r for r in KN.ROWS if r.K >= 2], ids=[i for i, r in zip(IDS, KN.ROWS) if r.K >= 2])
def test_oracle_all_padding_equals_no_neighbours(r):
    """The oracle's solve of `all_pad` and its solve of the same scene's K = 0 record: the same bits in info, u, x0array and warm
    start (a padded term is exactly 0.0 with all its derivatives)."""
    prm0 = KN.prm_of(r.N, 0)
    rec, sols = KN.records(r.N, r.K), KN.oracle_solutions(r.N, r.K)
    for s in range(len(r.seeds)):
        z = KN.oracle_solve(prm0, KN.without_obstacles(rec["all_pad"][s], r.N, r.K))
        for k in ("info", "u", "x0", "w"):
            a, b = sols["all_pad"][s][k], z[k]
            assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b), \
                (r.N, r.K, r.seeds[s], k)


def test_k0_records_are_the_scenes_of_the_other_rows():
    """K = 0: the record built at K = 3 with the obstacle block cut out -- which is the record of ANY K without its block (the
    reference path, target and initial state of the first solve do not depend on K)."""
    for N in (2, 10):
        seeds = KN.row(N, 0).seeds
        k0 = KN.records(N, 0)["k0"]
        assert k0.shape == (len(seeds), 20 + 10 * N)
        assert np.array_equal(k0, KN.without_obstacles(KN.records(N, 3, seeds)["packed"], N, 3))
    assert np.array_equal(KN.records(10, 0)["k0"][:5], KN.without_obstacles(KN.records(10, 9)["packed"][:5], 10, 9))


@pytest.mark.parametrize("N,K", [(2, 0), (10, 0), (32, 64)])
def test_c_oracle_equals_numpy_twin_at_the_ends_of_the_range(N, K):
    """mpco_nlp_f / mpco_nlp_grad_f against oracle/mpc_oracle_np.py, at the oracle's solution of the row's first scenes and at a point
    1 m / 1 m/s away from it; bounds of tests/test_mpc_oracle.py::test_c_equals_numpy_on_values_and_derivatives (1e-10)."""
    lib = _oracle.load_oracle()
    prm = KN.prm_of(N, K)
    rec, sols = KN.records(N, K), KN.oracle_solutions(N, K)
    a = "k0" if K == 0 else "packed"
    rng = np.random.default_rng(7)
    for s in range(2):
        P = np.ascontiguousarray(np.concatenate([rec[a][s], prm.gain, prm.tau, prm.weights, [prm.radius]]))
        assert len(P) == lib.mpco_p_len(N, K) == M.p_len(N, K)
        for w in (sols[a][s]["w"], sols[a][s]["w"] + rng.normal(size=10 + 14 * N)):
            w = np.ascontiguousarray(w)
            df = abs(lib.mpco_nlp_f(w, P, N, K) - M.nlp_f(w, P, N, K))
            g = np.zeros_like(w); lib.mpco_nlp_grad_f(w, P, N, K, g)
            dg = np.abs(g - M.nlp_grad_f(w, P, N, K)).max()
            print(f"N = {N}, K = {K}: |f_c - f_np| = {df:.2e}, |grad_c - grad_np| = {dg:.2e}")
            assert df < 1e-10 and dg < 1e-10
