"""GPU: the control step's re-plan loop (amk_step_batch, amk_step_batch_host, amk_step_batch_frames; csrc/step.hip,
csrc/step_frames.hip, pack_ref_states in csrc/step_common.h) at every pass limit 1 .. 8 and on every decision edge, on the inputs of
tests/_step_loop_cases.py.

A. The ladder: one batch whose scenes leave the loop after 1, 2, ... 8 solves, with clouds of 2, K, 1 and 0 points and a scene that
   ends unsafe.  tests/test_step_loop_cases.py proves that every decision of every pass lies >= 1e-3 m from safety_distance in the
   oracle -- 1000 x the GPU-to-oracle tolerance -- so flags[0] and flags[1] are asserted with no allowance.
B. Pass 0 (mpc_max_iter = 1: P is packed before any solve and read through amk__mpc_ref_states), bit for bit: an obstacle exactly
   safety_distance from reference point 0 and one ulp to either side, clouds at every count rule, and the snap's re-query in its
   four forms.  And needReplan's `<=` on equality, which shows one pass later: in the solve count at mpc_max_iter = 2.

The state quads are handed over between guard rows of other states: a pass that reads a row outside its batch's own shows in P.

Seen to bite on an MI355X (one-line changes in builds that were not kept): `>=` for `>` in plan_scene fails
test_snap_decision_on_the_threshold; `<` for `<=` in pack_ref_states fails test_need_replan_on_the_threshold; row `iter - 1` of
d_state_quad fails test_ladder_at_every_pass_limit (and 32 more); a solve that ignores done[s] fails test_ladder_at_every_pass_limit,
the host, one-frame, three-frame and budget tests.  Dropping the done[s] test of a SEARCH kernel (step_knn_grid_row) fails nothing, and
no test of results can make it: a finished or paused scene's reference path no longer changes, so the search repeats the answers of
the scene's last pass into buffers that plan / pack and the solve, which do test done[s], never read again -- that guard saves work."""
import ctypes as C

import numpy as np
import pytest

from tests import _frames_cases as fc
from tests import _step_loop_cases as lc
from tests.test_step_frames_edges_gpu import _bits, assert_P_exact, assert_flags01, assert_outputs, gpu_frames
from tests import _oracle

pytestmark = pytest.mark.gpu
KEYS = ("u", "x0array", "ref_path", "flags", "P")
FORMS = {"bucketed": dict(), "scan": dict(scan=True), "nanoflann": dict(tie=(1, 1)), "auto": dict(tie=(2, 0))}


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                                                                         b.view(np.int64) if b.dtype == np.float64 else b)


class Batch:
    """The two indices of a list of single-frame scenes, built once; step() runs one control step on a fresh MPC batch."""

    def __init__(self, scenes, tie=(0, 0), scan=False):
        import torch
        from avoid_mpc_amd import capi
        from avoid_mpc_amd.host import KdBatch
        self.scenes, self.S = scenes, len(scenes)
        self.kd = []
        for key, t in (("cloud", tie[0]), ("edge", tie[1])):
            nmax = max(max(len(sc[key]) for sc in scenes), 1)
            buf = np.zeros((self.S, nmax, 3), np.float32); cnt = np.zeros(self.S, np.int32)
            for s, sc in enumerate(scenes):
                buf[s, :len(sc[key])] = sc[key]; cnt[s] = len(sc[key])
            kd = KdBatch(self.S, nmax)
            if scan:
                capi.check(capi.load().amk__kd_set_mode(kd.h, 1), "scan mode")
            kd.set_tie_order(t)
            kd.build(torch.from_numpy(buf).cuda(), torch.from_numpy(cnt).cuda())
            self.kd.append(kd)

    def close(self):
        for kd in self.kd:
            kd.close()

    def inputs(self, prm):
        """(state quads [S, m, 10] between two guard blocks of the same size, pos_x [S], ref_path [S, N, 10]).  The guards hold
        states that are no scene's (the first and last scene's, half a metre and half a metre per second off): a pass that reads
        a row before or behind its batch's own stays inside the buffer and shows in P."""
        sq = np.zeros((self.S + 2, prm.max_iter, 10))
        sq[1:-1] = np.stack([_oracle.scene_state_quads(sc, prm) for sc in self.scenes])
        sq[0] = sq[1] + 0.5; sq[-1] = sq[-2] - 0.5
        return sq, np.array([sc["pos"][0] for sc in self.scenes]), np.stack([sc["ref_path"] for sc in self.scenes])

    def step(self, prm, entry="device", budget=None):
        """entry: device (amk_step_batch) | host (amk_step_batch_host) | frames1 (amk_step_batch_frames, one frame, no pose)
        -> dict(u, x0array, ref_path, flags, P, sq) as numpy arrays"""
        import torch
        from avoid_mpc_amd import capi
        from avoid_mpc_amd.host import MpcBatch, step_batch, step_batch_frames
        S = self.S
        mpc = MpcBatch(prm.T, prm.dt, prm.K, S); mpc.configure(prm)
        if budget:
            mpc.set_solve_budget(*budget)
        sq, pos_x, ref = self.inputs(prm)
        try:
            if entry == "host":
                u = np.zeros((S, 4)); x0 = np.zeros((S, mpc.N, 14)); flags = np.zeros((S, 4), np.int32)
                sqh = np.ascontiguousarray(sq[1:-1])
                sp = capi.StepParams(float(prm.speed), float(prm.safety_distance), int(prm.max_iter), 0)
                vp = lambda a: a.ctypes.data_as(C.c_void_p)
                capi.check(capi.load().amk_step_batch_host(self.kd[0].h, self.kd[1].h, mpc.h, C.byref(sp), vp(sqh), vp(pos_x), vp(ref),
                                                           vp(u), vp(x0), vp(flags)), "amk_step_batch_host")
                out = dict(u=u, x0array=x0, ref_path=ref, flags=flags)
            else:
                dsq = torch.from_numpy(sq).cuda()[1:-1]
                dref = torch.from_numpy(ref).cuda(); dpx = torch.from_numpy(pos_x).cuda()
                if entry == "device":
                    o = step_batch(self.kd[0], self.kd[1], mpc, prm, dsq, dpx, dref)
                else:
                    o = step_batch_frames([self.kd[0]], [self.kd[1]], mpc, prm, dsq, dpx, dref)
                torch.cuda.synchronize()
                out = dict(u=o["u"].cpu().numpy(), x0array=o["x0array"].cpu().numpy(), ref_path=dref.cpu().numpy(),
                           flags=o["flags"].cpu().numpy())
            out["P"] = mpc.ref_states()
            out["sq"] = sq[1:-1]
            return out
        finally:
            mpc.close()


def check_against_oracle(g, runs, N, K, what):
    """a. flags[0] and flags[1] the oracle's, no allowance.  b. the x_init block of P is bit for bit the row of d_state_quad of the
    scene's newest solve.  c. u, x0array, ref_path and P within 1e-6 of the oracle's by the flag rule of assert_outputs."""
    assert_flags01(g["flags"], runs)
    for s, r in enumerate(runs):
        p = int(g["flags"][s][1])
        assert p >= 1
        assert np.array_equal(_bits(fc.split_P(g["P"][s], N, K)[0]), _bits(g["sq"][s][p - 1])), (what, s, p)
        same = np.array_equal(g["flags"][s], r["flags"])
        d = np.abs(g["P"][s] - r["ref_log"][p - 1]).max()
        assert d <= (1e-6 if same else 1e-4), (what, s, "P", d)
    assert_outputs(g, runs, what)


def check_prefix(g, g8, m, what):
    """d. A scene that left the loop before pass m returns at the limit m, bit for bit, what it returns at the limit 8."""
    n = 0
    for s in range(len(g["flags"])):
        if g["flags"][s][1] < m:
            n += 1
            for k in KEYS:
                assert _same_bits(g[k][s], g8[k][s]), (what, m, s, k)
    return n


@pytest.fixture(scope="module", params=lc.SIZES, ids=lambda p: f"T{p[0]}-K{p[1]}")
def ladder(request):
    """The ladder's handles and its run through amk_step_batch at every limit m = 1 .. 8 (made once, shared, never modified)"""
    T, K = request.param
    b = Batch(lc.ladder(T, K)[0])
    runs = {m: b.step(lc.params(T, K, m)) for m in range(1, lc.MAX_PASSES + 1)}
    yield T, K, b, runs
    b.close()


def test_ladder_at_every_pass_limit(ladder):
    T, K, b, runs = ladder
    N = lc.params(T, K).N
    finished = 0
    for m in range(1, lc.MAX_PASSES + 1):
        oracle = lc.ladder_oracle(T, K, m)
        check_against_oracle(runs[m], oracle, N, K, f"amk_step_batch m = {m}")
        p8 = [int(r["flags"][1]) for r in lc.ladder_oracle(T, K, lc.MAX_PASSES)]
        assert [int(f[1]) for f in runs[m]["flags"]] == [min(p, m) for p in p8]
        finished += check_prefix(runs[m], runs[lc.MAX_PASSES], m, "amk_step_batch")
    assert finished >= 2 * sum(range(8))     # two scenes per solve count p, each finished at every limit above p
    assert runs[lc.MAX_PASSES]["flags"][-1][0] == 0 and (runs[lc.MAX_PASSES]["flags"][:-1, 0] == 1).all()


def test_ladder_scenes_alone(ladder):
    """e. Scenes with 1, 4 and 8 solves and the unsafe one, each in a batch of its own: the bits they return inside the ladder."""
    T, K, b, runs = ladder
    scenes, kinds = lc.ladder(T, K)
    for kind in (1, 4, 8, "unsafe"):
        s = kinds.index(kind)
        one = Batch([scenes[s]])
        try:
            g = one.step(lc.params(T, K))
        finally:
            one.close()
        for k in KEYS:
            assert _same_bits(g[k][0], runs[lc.MAX_PASSES][k][s]), (kind, s, k)


def test_ladder_through_the_host_entry(ladder):
    T, K, b, runs = ladder
    prm = lc.params(T, K)
    g = b.step(prm, entry="host")
    check_against_oracle(g, lc.ladder_oracle(T, K, lc.MAX_PASSES), prm.N, K, "amk_step_batch_host m = 8")
    for k in KEYS:
        assert _same_bits(g[k], runs[lc.MAX_PASSES][k]), k


def test_ladder_through_one_frame_of_the_frames_entry(ladder):
    """amk_step_batch_frames with one frame and no pose at every limit: a to d, and the bits of amk_step_batch."""
    T, K, b, runs = ladder
    N = lc.params(T, K).N
    got = {m: b.step(lc.params(T, K, m), entry="frames1") for m in range(1, lc.MAX_PASSES + 1)}
    for m, g in got.items():
        check_against_oracle(g, lc.ladder_oracle(T, K, m), N, K, f"amk_step_batch_frames, one frame, m = {m}")
        check_prefix(g, got[lc.MAX_PASSES], m, "amk_step_batch_frames")
        for k in KEYS:
            assert _same_bits(g[k], runs[m][k]), (m, k, np.argwhere(g[k] != runs[m][k])[:4].tolist())


@pytest.mark.parametrize("T,K", lc.SIZES)
def test_ladder_in_three_frames_under_a_camera(T, K):
    prm = lc.params(T, K)
    scenes = lc.ladder_frames(T, K)
    g = gpu_frames(scenes, prm, lc.LADDER_CAM)
    g["sq"] = np.stack([fc.state_quads(sc, prm) for sc in scenes])
    runs = lc.ladder_frames_oracle(T, K)
    check_against_oracle(g, runs, prm.N, K, "amk_step_batch_frames, three frames, m = 8")
    assert len({int(f[1]) for f in g["flags"]}) >= 5 and g["flags"][-1][0] == 0


@pytest.mark.parametrize("budget", [(3, 0), (3, 2)])
def test_ladder_under_a_solve_budget(ladder, budget):
    """amk_mpc_set_solve_budget: the scenes of a launch are in different passes (each reads ITS row of d_state_quad through its own
    pass counter) -- the plain schedule's bits."""
    T, K, b, runs = ladder
    g = b.step(lc.params(T, K), budget=budget)
    for k in KEYS:
        assert _same_bits(g[k], runs[lc.MAX_PASSES][k]), (budget, k, np.argwhere(g[k] != runs[lc.MAX_PASSES][k])[:4].tolist())


@pytest.mark.parametrize("bad", [0, -1, 9])
def test_pass_limits_outside_1_to_8_are_refused(bad):
    import torch
    from avoid_mpc_amd import capi
    from avoid_mpc_amd.host import MpcBatch
    T, K = lc.SIZES[1]
    scenes = lc.ladder(T, K)[0][:2]
    b = Batch(scenes)
    prm = lc.params(T, K)
    S, N = 2, prm.N
    mpc = MpcBatch(T, prm.dt, K, S); mpc.configure(prm)
    sq, pos_x, ref0 = b.inputs(prm)
    sp = capi.StepParams(float(prm.speed), float(prm.safety_distance), bad, 0)
    lib = capi.load()
    try:
        dsq = torch.from_numpy(sq).cuda()[1:-1]; dpx = torch.from_numpy(pos_x).cuda()
        for entry in ("device", "frames"):
            dref = torch.from_numpy(ref0).cuda()
            out = dict(u=torch.full((S, 4), -7.0, dtype=torch.float64, device="cuda"),
                       x0array=torch.full((S, N, 14), -7.0, dtype=torch.float64, device="cuda"),
                       flags=torch.full((S, 4), -7, dtype=torch.int32, device="cuda"))
            tail = (mpc.h, C.byref(sp), capi.dptr(dsq), capi.dptr(dpx), capi.dptr(dref), capi.dptr(out["u"]), capi.dptr(out["x0array"]),
                    capi.dptr(out["flags"]), None)
            if entry == "device":
                rc = lib.amk_step_batch(b.kd[0].h, b.kd[1].h, *tail)
            else:
                oa = (C.c_void_p * 1)(b.kd[0].h); ea = (C.c_void_p * 1)(b.kd[1].h)
                rc = lib.amk_step_batch_frames(oa, ea, 1, None, None, *tail)
            torch.cuda.synchronize()
            assert rc == capi.AMK_ERR_INVALID_ARG, (entry, bad, rc)
            assert all(bool((v == -7).all()) for v in out.values()) and np.array_equal(dref.cpu().numpy(), ref0), (entry, bad)
        u = np.full((S, 4), -7.0); x0 = np.full((S, N, 14), -7.0); flags = np.full((S, 4), -7, np.int32); ref = ref0.copy()
        sqh = np.ascontiguousarray(sq[1:-1])
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = lib.amk_step_batch_host(b.kd[0].h, b.kd[1].h, mpc.h, C.byref(sp), vp(sqh), vp(pos_x), vp(ref), vp(u), vp(x0), vp(flags))
        assert rc == capi.AMK_ERR_INVALID_ARG, ("host", bad, rc)
        assert (u == -7).all() and (x0 == -7).all() and (flags == -7).all() and np.array_equal(ref, ref0)
    finally:
        mpc.close(); b.close()


# ------------------------------------------------------------------------------------------------ B. decision edges at pass 0
def _pass0_both(scenes, K, sd, key, form, entry="device"):
    """The scenes at mpc_max_iter = 1 in one form of the search: flags[0], flags[1] and P bit-identical to the oracle's.
    -> (gpu result, oracle runs, exact status of the obstacle handle)"""
    prm = lc.params(lc.EDGE_T, K, 1, sd)
    b = Batch(scenes, **FORMS[form])
    try:
        g = b.step(prm, entry=entry)
        status = b.kd[0].exact_status().cpu().numpy()
    finally:
        b.close()
    runs = lc.pass0_oracle(scenes, K, prm.safety_distance, key)
    assert_flags01(g["flags"], runs)
    assert_P_exact(g["P"], runs, prm.N, K, f"{key} {form} {entry}")
    return g, runs, status


def _snapped(g, scenes, N, K):
    return [not np.array_equal(fc.split_P(g["P"][s], N, K)[1][0, :3], sc["ref_path"][0, :3]) for s, sc in enumerate(scenes)]


@pytest.mark.parametrize("form", ["bucketed", "scan"])
@pytest.mark.parametrize("pair", sorted(lc.PAIRS))
@pytest.mark.parametrize("K", [1, 3, 8])
def test_snap_decision_on_the_threshold(K, pair, form):
    """`!(nearest > safety_distance)`: an obstacle EXACTLY safety_distance from reference point 0 snaps it; one ulp less does not."""
    scenes = lc.threshold_scenes(K, pair)
    sd = lc.PAIRS[pair][1]
    N = lc.params(lc.EDGE_T, K, 1).N
    for side in lc.SIDES:
        for entry in ("device", "frames1") if form == "bucketed" else ("device",):
            g, _, _ = _pass0_both(scenes, K, lc.side_value(sd, side), ("threshold", pair), form, entry)
            assert _snapped(g, scenes, N, K) == [lc.SNAPS[side]] * len(scenes), (side, entry)
            assert (g["flags"][:, 0] == 1).all()


@pytest.mark.parametrize("form", ["bucketed", "scan"])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_count_rules_of_both_clouds(K, form):
    """Obstacle clouds of 0, 1, 2, K - 1, K, K + 1 points x edge clouds of 0, 1, 2 points: `size > 1` for the nearest distance and
    for the edge point, `size > K` for the neighbours -- unsafe, snapped with padded rows, snapped with a full row."""
    scenes, sizes = lc.size_scenes(K)
    prm = lc.params(lc.EDGE_T, K, 1)
    for entry in ("device", "frames1") if form == "bucketed" else ("device",):
        g, _, _ = _pass0_both(scenes, K, prm.safety_distance, "sizes", form, entry)
        snapped = _snapped(g, scenes, prm.N, K)
        for s, (no, ne) in enumerate(sizes):
            assert snapped[s] == (no > 1 and ne > 1) and g["flags"][s][0] == (0 if no > 1 and ne <= 1 else 1), (no, ne, entry)
            ob = fc.split_P(g["P"][s], prm.N, K)[2]
            assert ((ob != fc.PAD).all() if no > K else (ob == fc.PAD).all()), (no, ne, entry)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_requery_of_the_snapped_point_in_four_forms(K):
    """The single-frame snap and its re-query through the bucketed index, the streaming scan, AMK_TIES_NANOFLANN and AMK_TIES_AUTO
    (obstacle handle): the snapped point 0 and row 0 of the obstacle block are the oracle's bit for bit, rows 1 .. N - 1 are the
    caller's.  On the lattice scenes (six-way tied edge points, tied first neighbours of the re-query) the oracle's answer is
    nanoflann's order: AMK_TIES_NANOFLANN gives it and AMK_TIES_AUTO gives the same bits."""
    from avoid_mpc_amd import capi
    prm = lc.params(lc.EDGE_T, K, 1)
    N = prm.N
    plain = lc.requery_scenes(K, False)
    for form in FORMS:
        g, runs, status = _pass0_both(plain, K, prm.safety_distance, ("requery", False), form)
        assert _snapped(g, plain, N, K) == [True] * 6 + [False] * 2, form
        for s, sc in enumerate(plain):
            path = fc.split_P(g["P"][s], N, K)[1]
            assert np.array_equal(_bits(path[1:]), _bits(sc["ref_path"][1:])), (form, s)
        if form == "auto":     # nothing tied: no scene got a tree
            assert (status == capi.AMK_EXACT_NOT_NEEDED).all(), status
    tied = lc.requery_scenes(K, True)
    g1, _, _ = _pass0_both(tied, K, prm.safety_distance, ("requery", True), "nanoflann")
    assert _snapped(g1, tied, N, K) == [True] * 6 + [False] * 2
    b = Batch(tied, tie=(capi.AMK_TIES_AUTO, capi.AMK_TIES_NANOFLANN))
    try:
        g2 = b.step(prm)
        status = b.kd[0].exact_status().cpu().numpy()
    finally:
        b.close()
    for k in ("flags", "P", "ref_path"):
        assert _same_bits(g2[k], g1[k]), k
    assert (status[:6] == capi.AMK_EXACT_IN_USE).all(), status      # the re-query's tie was seen and answered by the tree


@pytest.mark.parametrize("entry", ["device", "frames1"])
@pytest.mark.parametrize("T,K", lc.SIZES)
def test_need_replan_on_the_threshold(T, K, entry):
    """`sqrt(d2) <= safety_distance` in pack_ref_states: pass 1 snaps point 0 to an edge point EXACTLY safety_distance from its first
    neighbour.  On equality the scene re-plans (two solves at mpc_max_iter = 2); one ulp below it leaves the loop after one."""
    scenes = [lc.exit_threshold_scene(T, K, ox) for ox in lc.EXIT_OX]
    b = Batch(scenes)
    try:
        for side, solves in zip(lc.SIDES, (2, 1, 2)):
            prm = lc.params(T, K, 2, lc.side_value(lc.EXIT_SD, side))
            g = b.step(prm, entry=entry)
            runs = [lc.exit_oracle(T, K, ox, side) for ox in lc.EXIT_OX]
            assert [int(f[1]) for f in g["flags"]] == [solves] * len(scenes), (side, g["flags"])
            check_against_oracle(g, runs, prm.N, K, f"exit threshold {side} {entry}")
    finally:
        b.close()
