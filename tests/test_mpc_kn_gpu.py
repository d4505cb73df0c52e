"""GPU: the interior-point solve, amk_mpc_eval's neighbours and the control step across the neighbour-count range amk_mpc_create
accepts (0 <= K <= 64) and the horizons at which the collision terms' lane map (csrc/mpc_device_impl.h: evaluate,
update_term_multipliers; per = 64 / (N - 1) slots of every stage per round) changes shape.  The cases, their seeds and what each
reaches are the table of tests/_mpc_kn_cases.py, checked on the CPU by tests/test_mpc_kn_cases.py; every scene with K >= 2 is solved
in four arrangements of its obstacle block -- the step packs neighbours in ascending distance, so in `packed` the live terms sit in
the first rounds; `reversed` and `last_only` put them in the LAST round, `all_pad` has none.

Rules, unchanged: amk_mpc_solve against the oracle as tests/test_mpc_gpu.py states it (same info: u, x0array and warm start to
1e-6; other counts: both converged, 1e-4, counted as flipped; flipped <= max(1, cases // 100) per test); the step with `compare` of
tests/test_step_gpu.py; the budgeted schedule with `_steps` of tests/test_mpc_resume_gpu.py (bits).

Device against device, no tolerance: a problem whose neighbours are all padding, or whose collision weight is 0, is the problem of
the K = 0 handle.  The basis is in the code: collide_term returns exactly 0.0 for a dormant term (the squared-distance pre-test, or
c = lam * g with `!(c > 0)`) BEFORE any LDS add, cmax and cdev stay 0.0, the value sum gains + 0.0 per lane, MODE 2 sees c_ir = 0 and
only resets the term's own multipliers; nothing else in the solve reads K.  So info, u, x0array and the warm start are equal bit for
bit, in fp64 and under set_precision(32)."""
import numpy as np
import pytest

from avoid_mpc_amd import synth
from tests import _mpc_kn_cases as KN
from tests import _oracle
from tests._mpc_solve_both import _assert_flipped, _solve_both

pytestmark = pytest.mark.gpu
IDS = [f"N{r.N}K{r.K}" for r in KN.ROWS]


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def _assert_same_bits(a, b, label):
    for k in ("info", "u", "x0", "w"):
        for t, (x, y) in enumerate(zip(a[k], b[k])):
            assert np.array_equal(_bits(x), _bits(y)), (label, k, f"solve {t}", np.argwhere(_bits(x) != _bits(y))[:4].tolist(),
                                                         float(np.nanmax(np.abs(x - y))))


def _solve_gpu(prm, ref, bits=64, n_solves=2, max_iter=None):
    """n_solves device solves in a row from the kept warm start (the first cold, faster=True) -> dict of per-solve lists."""
    import torch
    from avoid_mpc_amd.host import MpcBatch
    g = MpcBatch(prm.T, prm.dt, prm.K, len(ref)); g.configure(prm); g.set_precision(bits)
    if max_iter is not None:
        g.set_solver_options(1e-4, max_iter)
    ref_d = torch.from_numpy(np.ascontiguousarray(ref)).cuda()
    out = dict(info=[], u=[], x0=[], w=[])
    for it in range(n_solves):
        u, x0, info = g.Solve(ref_d, faster=(it == 0))
        torch.cuda.synchronize()
        for k, v in (("info", info), ("u", u), ("x0", x0), ("w", g.get_warm_start())):
            out[k].append(v.cpu().numpy().copy())
    g.close()
    return out


# ---- a. the solve, fp64, against the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("r", KN.ROWS, ids=IDS)
def test_solve_matches_the_oracle_in_every_arrangement(r):
    """Every scene of the row in all its arrangements in ONE launch; two solves in a row from the kept warm start."""
    prm = KN.prm_of(r.N, r.K)
    names, ref = KN.batch(r.N, r.K)
    res = _solve_both(prm, ref, n_solves=2)
    assert np.all(res["info"][:, 0] == 0)
    ns, per, rounds, idle, last = KN.geometry(r.N, r.K)
    _assert_flipped(res, f"N = {r.N}, K = {r.K} (per {per}, rounds {rounds}, idle lanes {idle}; {r.kernel}), "
                         f"{len(r.seeds)} scenes x {names}, two solves")


# ---- b. nothing means nothing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("N,K", [(10, 9), (2, 64), (17, 64), (32, 64)])
def test_all_padding_equals_the_handle_without_neighbours(N, K, bits):
    """`all_pad` on a K handle against the same scenes' K = 0 records on a K = 0 handle, two solves each: the same bits (module
    docstring for the reason), fp64 and fp32."""
    rec = KN.records(N, K)["all_pad"]
    a = _solve_gpu(KN.prm_of(N, K), rec, bits)
    b = _solve_gpu(KN.prm_of(N, 0), KN.without_obstacles(rec, N, K), bits)
    _assert_same_bits(a, b, f"N = {N}: all_pad on K = {K} vs K = 0, fp{bits}")
    if bits == 64:
        assert np.all(a["info"][0][:, 0] == 0)
    assert np.all(np.isfinite(a["w"][1]))


# ---- c. collision weight 0 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(30, 64), (17, 64)])
def test_collision_weight_zero_equals_the_handle_without_neighbours(N, K):
    """collide_lambda (weights[24]) = 0 on `packed` and `reversed`: c = lam * g is 0.0, every term dormant, so the solves equal those
    of the K = 0 handle bit for bit, in fp64 and in fp32; and the fp32 result stays within the bound of
    tests/test_mpc_fp32_gpu.py::test_fp32_matches_fp64_oracle_on_the_smooth_part (|du|, |dw| <= 1e-4 against the fp64 oracle, the
    device capped at 40 iterations as there).  No fp32 accuracy claim is made for the full problem at these K."""
    rec = KN.records(N, K)
    ref = np.concatenate([rec["packed"], rec["reversed"]])
    prmK, prm0 = KN.prm_of(N, K), KN.prm_of(N, 0)
    for prm in (prmK, prm0):
        w = np.array(prm.weights, float); w[24] = 0.0; prm.weights = list(w)
    ref0 = KN.without_obstacles(ref, N, K)
    for bits, cap in ((64, None), (32, 40)):
        a = _solve_gpu(prmK, ref, bits, max_iter=cap)
        b = _solve_gpu(prm0, ref0, bits, max_iter=cap)
        _assert_same_bits(a, b, f"N = {N}, K = {K}, lambda = 0 vs K = 0, fp{bits}")
        if bits == 64:
            assert np.all(a["info"][0][:, 0] == 0)
    du = dw = 0.0
    for s in range(len(ref)):
        m = _oracle.MpcOracle(prmK.T, prmK.dt, K); m.configure(prmK)
        uc, xc, ic = m.Solve(ref[s], True)
        du = max(du, np.abs(a["u"][0][s] - uc).max()); dw = max(dw, np.abs(a["w"][0][s] - m.warm_start).max())
    print(f"N = {N}, K = {K}, collision weight 0: fp32 vs fp64 oracle |du| {du:.2e} |dw| {dw:.2e}")
    assert du <= 1e-4 and dw <= 1e-4


def test_fp32_on_the_packed_rows_prints_its_distance_to_the_fp64_optimum():
    """set_precision(32) on the `packed` scenes of every row with K >= 1: finite, inside the box; the median over a row's scenes of
    |u32 - u*|_inf (u* = the oracle's fp64 solution with the shipped options) is PRINTED, not asserted -- nothing measured supports a
    number for the full problem at these K."""
    for r in KN.ROWS:
        if r.K == 0:
            continue
        prm = KN.prm_of(r.N, r.K)
        a = _solve_gpu(prm, KN.records(r.N, r.K)["packed"], 32, n_solves=1)
        u32, w32 = a["u"][0], a["w"][0]
        lo = np.array([-prm.a_max_xy, -prm.a_max_xy, prm.a_min_z, -prm.a_max_yaw_dot])
        hi = np.array([prm.a_max_xy, prm.a_max_xy, prm.a_max_z, prm.a_max_yaw_dot])
        assert np.all(np.isfinite(w32)) and np.all(u32 >= lo) and np.all(u32 <= hi), (r.N, r.K)
        du = [np.abs(u32[s] - sol["u"]).max() for s, sol in enumerate(KN.oracle_solutions(r.N, r.K)["packed"])]
        print(f"fp32, packed, N = {r.N}, K = {r.K}: median |u32 - u*| {np.median(du):.3e}, max {np.max(du):.3e}, "
              f"status {a['info'][0][:, 0].tolist()}")


# ---- d. amk_mpc_eval on the baked kernels (the generic ones: GENERIC of tests/test_mpc_eval_gpu.py) ---------------------------
@pytest.mark.parametrize("N,K", [(10, 0), (20, 10), (30, 64)])
def test_eval_matches_oracle_at_baked_horizons_and_new_k(N, K):
    from tests.test_mpc_eval_gpu import _points_at, compare_eval_with_oracle
    prm, W, R = _points_at(KN.prm_of(N, K), 3, 21)
    print(N, K, "eval: worst relative error f %.2e grad_f %.2e hess_l %.2e" % compare_eval_with_oracle(prm, W, R))


# ---- e. the whole control step to its solution -------------------------------------------------------------------------------
_step_scenes = KN.step_scenes


@pytest.mark.parametrize("N,K,tie_order", [(r.N, r.K, r.tie_order) for r in KN.STEP_ROWS])
def test_step_matches_oracle_across_k(N, K, tie_order):
    """amk_step_batch, 6 scenes of 50 000 points (KN.STEP_ROWS: seeds admitted on the CPU), two steps (warm start carried over),
    re-plan passes included; tie_order 1: AMK_TIES_NANOFLANN on both handles, 2: AMK_TIES_AUTO, which asks the index for K + 1 = 64
    neighbours at K = 63."""
    import torch
    from tests.test_step_gpu import compare, run_both
    prm, scenes = _step_scenes(N, K)
    gpu, cpu = run_both(torch, scenes, prm, n_steps=2, tie_order=tie_order)
    w = compare(gpu, cpu)
    assert all(r["flags"][1] >= 1 and r["flags"][2] == 0 for r in cpu[0])
    print(f"step, N = {N}, K = {K}, tie order {tie_order}: worst |gpu - oracle| = {w:.3e}; solves/step = "
          f"{[int(r['flags'][1]) for r in cpu[0]]}, iterations = {[int(r['flags'][3]) for r in cpu[0]]}")


def _step_raw(kd_o, kd_e, mpc, prm, scenes, N):
    """amk_step_batch through the C ABI with outputs pre-set to -7 -> (status, outputs, ref path before, ref path after)."""
    import ctypes as C
    import torch
    from avoid_mpc_amd import capi
    S = len(scenes)
    sq = torch.from_numpy(np.stack([_oracle.scene_state_quads(sc, prm) for sc in scenes])).cuda()
    pos_x = torch.from_numpy(np.array([sc["pos"][0] for sc in scenes])).cuda()
    ref0 = torch.from_numpy(np.stack([sc["ref_path"] for sc in scenes])).cuda()
    ref = ref0.clone()
    out = dict(u=torch.full((S, 4), -7.0, dtype=torch.float64, device="cuda"),
               x0array=torch.full((S, N, 14), -7.0, dtype=torch.float64, device="cuda"),
               flags=torch.full((S, 4), -7, dtype=torch.int32, device="cuda"))
    sp = capi.StepParams(float(prm.speed), float(prm.safety_distance), int(prm.max_iter), 0)
    rc = capi.load().amk_step_batch(kd_o.h, kd_e.h, mpc.h, C.byref(sp), capi.dptr(sq), capi.dptr(pos_x), capi.dptr(ref),
                                    capi.dptr(out["u"]), capi.dptr(out["x0array"]), capi.dptr(out["flags"]), None)
    torch.cuda.synchronize()
    return rc, out, ref0, ref


def _kd_pair(scenes, tie_order=0):
    import torch
    from avoid_mpc_amd.host import KdBatch
    S = len(scenes)
    kd_o, kd_e = KdBatch(S, len(scenes[0]["cloud"])), KdBatch(S, len(scenes[0]["edge"]))
    kd_o.set_tie_order(tie_order); kd_e.set_tie_order(tie_order)
    kd_o.build(torch.from_numpy(np.stack([sc["cloud"] for sc in scenes])).cuda())
    kd_e.build(torch.from_numpy(np.stack([sc["edge"] for sc in scenes])).cuda())
    return kd_o, kd_e


def test_auto_step_refuses_k64_and_a_k0_handle_is_refused_by_every_step():
    """AMK_TIES_AUTO needs K + 1 <= AMK_MAX_K: at K = 64 the step returns AMK_ERR_UNSUPPORTED.  A handle created with K = 0 (served by
    amk_mpc_solve) is refused by amk_step_batch with AMK_ERR_INVALID_ARG (step_params_ok), in every tie order.  Neither writes an
    output or the reference path."""
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import MpcBatch
    N = 20
    for K, tie_order, want in ((64, capi.AMK_TIES_AUTO, capi.AMK_ERR_UNSUPPORTED), (0, capi.AMK_TIES_LOWEST_INDEX, capi.AMK_ERR_INVALID_ARG),
                               (0, capi.AMK_TIES_AUTO, capi.AMK_ERR_INVALID_ARG)):
        prm = KN.prm_of(N, K)
        scenes = [synth.make_scene(3000, 1300 + i, prm) for i in range(2)]
        kd_o, kd_e = _kd_pair(scenes, tie_order)
        mpc = MpcBatch(prm.T, prm.dt, K, len(scenes)); mpc.configure(prm)
        rc, out, ref0, ref = _step_raw(kd_o, kd_e, mpc, prm, scenes, N)
        assert rc == want, (K, tie_order, rc)
        assert all(bool((v == -7).all()) for v in out.values()) and torch.equal(ref, ref0), (K, tie_order)
        for h in (kd_o, kd_e, mpc):
            h.close()


@pytest.mark.parametrize("N,K", [(20, 33), (32, 64)])
def test_budgeted_step_returns_the_bits_of_the_plain_schedule_at_large_k(N, K):
    """tests/test_mpc_resume_gpu.py's criterion where a paused solve's term multipliers wait in a ybuf of many rounds: budgets
    (2, 0) and (5, 6) return the bits of the plain schedule (outputs, refilled reference path, warm start), two steps; at least one
    solve pauses (asserted as that file does)."""
    import torch
    from tests.test_mpc_resume_gpu import _steps
    prm, scenes = _step_scenes(N, K)
    plain = _steps(torch, scenes, prm, 0, 0)
    it = plain[0]["flags"][:, 3]
    paused_somewhere = False
    for budget, rounds in ((2, 0), (5, 6)):
        got = _steps(torch, scenes, prm, budget, rounds)
        for t in range(len(plain)):
            for k in plain[t]:
                assert np.array_equal(_bits(got[t][k]), _bits(plain[t][k])), (N, K, budget, rounds, t, k)
        paused_somewhere = paused_somewhere or budget * 3 < it.max()
    assert paused_somewhere
    print(f"N = {N}, K = {K}: iterations per step min / mean / max {it.min()} / {it.mean():.1f} / {it.max()}, solves per step "
          f"{plain[0]['flags'][:, 1].mean():.2f}: budgets (2, 0) and (5, 6) bit-identical")
