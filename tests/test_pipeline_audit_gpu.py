"""GPU: the pipeline's trajectory audit (amk_pipeline_set_path_audit / amk_pipeline_audit_outputs, Launch::path_audit and
pipeline_audit_veto_kernel in csrc/pipeline.hip).

Small synthetic scenes (synth.make_scene): S = 8 scenes of 3000 points, N = 10, two slots, TASK-mode frames with a command.  Once
with gang 2 and a partly filled gang on the slots' own obstacle index, once with a keyframe map.  Every comparison is bit for bit.

The radii, found on these scenes (the 24 scenes of the gang run; the 16 scenes of the map run's second period):
    3.0 m   the gang run: all 24 audits stop (stop 1), all 24 scenes have flags[0] == 1, all 24 are vetoed; the map run: 16 of 16
    1e-3 m  no audit stops in either run, nothing is vetoed
    0.3 m over the first 4 legs (REPORT only): 3 of 24 audits stop
(the clouds are dense -- 3000 points in 30 x 16 x 4 m -- so a sphere of 3 m around X0 always holds a point at t = 0, and a 1 mm
sphere along the predicted trajectory meets none).  The tests print the counts and assert only "some" and "none"."""
import ctypes as C

import numpy as np
import pytest

from avoid_mpc_amd import capi, synth

pytestmark = pytest.mark.gpu

S, NPTS, NEDGE = 8, 3000, 300
TINY, WIDE = 1e-3, 3.0
STEP_KEYS = ("u", "flags", "x0array", "ref_path")
AUDIT_KEYS = ("stop", "leg", "t", "free", "pts")


def prm_of():
    return synth.MpcParams(T=0.33, K=3, max_iter=2)


def task_frames(torch, prm, n_frames, seed0=7000):
    """n_frames TASK-mode frames: clouds, odometry x [S, 10] = [p, yaw, v, a], the initial mRefPath"""
    out = []
    for f in range(n_frames):
        scenes = [synth.make_scene(NPTS, seed0 + 17 * f + s, prm) for s in range(S)]
        x = np.stack([np.concatenate([sc["pos"], [sc["yaw"]], sc["vel"], sc["acc"]]) for sc in scenes])
        out.append(dict(cl=torch.from_numpy(np.stack([sc["cloud"] for sc in scenes])).cuda(),
                        ed=torch.from_numpy(np.stack([sc["edge"] for sc in scenes])[:, :NEDGE].copy()).cuda(),
                        x=x, odom=torch.from_numpy(x).cuda(), ref=torch.from_numpy(np.stack([sc["ref_path"] for sc in scenes])).cuda()))
    return out


def run_gang(torch, frames, mode, radius, n_legs=0):
    """two slots, gang 2, three frames: slot 0 launches a full gang, slot 1 a partly filled one at drain.
    -> (pipeline, tickets, per frame dict(u, flags, x0array, ref_path, cmd[, audit]))"""
    from avoid_mpc_amd.host import Pipeline
    prm = prm_of()
    pl = Pipeline(2, S, NPTS, NEDGE, prm, gang=2)
    if mode is not None:
        pl.set_path_audit(mode, radius, n_legs)
    cmds, tickets = [], []
    for fr in frames:
        cmds.append(torch.full((S, 3), -7.0, dtype=torch.float64, device="cuda"))
        tickets.append(pl.submit(fr["cl"], fr["ed"], ref_path_init=fr["ref"], odom=fr["odom"], cmd_out=cmds[-1]))
    pl.drain()
    res = []
    for t, cmd in zip(tickets, cmds):
        o = pl.outputs(t)
        o["cmd"] = cmd.cpu().numpy()
        if mode not in (None, capi.AMK_AUDIT_OFF):
            o["audit"] = pl.audit_outputs(t)
        res.append(o)
    return pl, tickets, res


@pytest.fixture(scope="module")
def gang_off():
    import torch
    frames = task_frames(torch, prm_of(), 3)
    pl, tickets, res = run_gang(torch, frames, None, 0.0)
    pl.close()
    assert tickets == [0, 2, 1]            # slot 0 positions 0 and 1, slot 1 position 0
    return frames, res


def audit_by_hand(torch, pl, tickets, res, radius, n_legs):
    """KdBatch.path_cast by the test on the returned x0array and the slot's own obstacle index, per ticket"""
    N = pl.N
    npts = (n_legs or N - 1) + 1
    out = {}
    for slot in range(2):
        path = np.zeros((2 * S, npts, 14))
        for t, o in zip(tickets, res):
            if t % 2 == slot:
                path[(t // 2) * S:(t // 2 + 1) * S] = o["x0array"][:, :npts]
        got = pl.kd(slot, 0).path_cast(torch.from_numpy(path).cuda(), radius * radius)
        torch.cuda.synchronize()
        for t in tickets:
            if t % 2 == slot:
                sl = slice((t // 2) * S, (t // 2 + 1) * S)
                out[t] = {k: got[k][sl].cpu().numpy() for k in ("stop", "leg", "t", "free", "pts", "indices")}
    return out


@pytest.mark.parametrize("radius,n_legs", [(WIDE, 0), (TINY, 0), (0.3, 4)])
def test_report_mode_keeps_the_answers_and_changes_nothing(gang_off, radius, n_legs):
    import torch
    frames, off = gang_off
    pl, tickets, res = run_gang(torch, frames, capi.AMK_AUDIT_REPORT, radius, n_legs)
    try:
        hand = audit_by_hand(torch, pl, tickets, res, radius, n_legs)
        for t, o, ref in zip(tickets, res, off):
            for k in STEP_KEYS + ("cmd",):
                assert np.array_equal(o[k], ref[k]), (t, k)
            for k in AUDIT_KEYS:
                assert np.array_equal(o["audit"][k], hand[t][k]), (t, k)
            assert np.array_equal(o["audit"]["src"], hand[t]["indices"]), t
            assert np.isfinite(o["audit"]["free"]).all()
        stops = np.concatenate([o["audit"]["stop"] for o in res])
        print(f"REPORT radius {radius} n_legs {n_legs}: stops {np.bincount(stops, minlength=3).tolist()} of {len(stops)}")
        if n_legs:
            assert (np.concatenate([o["audit"]["leg"] for o in res]) < n_legs).all()
    finally:
        pl.close()


@pytest.mark.parametrize("radius", [WIDE, TINY])
def test_slow_down_mode_vetoes_the_command_and_nothing_else(gang_off, radius):
    import torch
    from avoid_mpc_amd import flight
    frames, off = gang_off
    prm = prm_of()
    pl, tickets, res = run_gang(torch, frames, capi.AMK_AUDIT_SLOW_DOWN, radius)
    try:
        hand = audit_by_hand(torch, pl, tickets, res, radius, 0)
        vetoed = 0
        for fr, t, o, ref in zip(frames, tickets, res, off):
            for k in STEP_KEYS:
                assert np.array_equal(o[k], ref[k]), (t, k)
            for k in AUDIT_KEYS:
                assert np.array_equal(o["audit"][k], hand[t][k]), (t, k)
            flags = o["flags"].copy()
            veto = (flags[:, 0] == 1) & (o["audit"]["stop"] != 0)
            flags[veto, 0] = 0
            assert np.array_equal(o["cmd"], flight.command(o["u"], flags, fr["x"], prm)), t
            keep = ~veto
            assert np.array_equal(o["cmd"][keep], ref["cmd"][keep]), t
            vetoed += int(veto.sum())
        safe = int(sum((o["flags"][:, 0] == 1).sum() for o in res))
        print(f"SLOW_DOWN radius {radius}: {vetoed} of {safe} safe scenes vetoed")
        assert safe > 0
        assert (vetoed > 0) if radius == WIDE else (vetoed == 0)
    finally:
        pl.close()


def run_map(torch, frames, mode, radius):
    """two slots with a keyframe map, gang 1, two periods per slot (frames 0, 1 then 2, 3): the second period's map holds the
    first period's frame as well.  -> (pipeline, tickets of the second period, their results)"""
    from avoid_mpc_amd.host import Pipeline
    prm = prm_of()
    pl = Pipeline(2, S, NPTS, NEDGE, prm, keyframes=dict(max_frame_count=3, th_dist=0.2, th_count=50, depth_min=0.1))
    if mode is not None:
        pl.set_path_audit(mode, radius)
    cam = capi.FrameCamera(32.0, 32.0, 32.0, 24.0, 6.0, 64, 48)
    Twc = np.array([[0, 0, 1, -2.0], [-1, 0, 0, 0.0], [0, -1, 0, 1.5], [0, 0, 0, 1.0]])
    Tw = torch.from_numpy(np.repeat(Twc[None], S, 0).copy()).cuda()
    res, tickets = [], []
    for period in range(2):
        cmds, tickets = [], []
        for fr in frames[2 * period:2 * period + 2]:
            cmds.append(torch.full((S, 3), -7.0, dtype=torch.float64, device="cuda"))
            tickets.append(pl.submit(fr["cl"], fr["ed"], ref_path_init=fr["ref"] if period == 0 else None, odom=fr["odom"], cmd_out=cmds[-1],
                                     Twc_cur=Tw, cam=cam))
        pl.drain()
        res = []
        for t, cmd in zip(tickets, cmds):
            o = pl.outputs(t)
            o["cmd"] = cmd.cpu().numpy()
            if mode is not None:
                o["audit"] = pl.audit_outputs(t)
            res.append(o)
    return pl, tickets, res


def test_a_slot_with_a_keyframe_map_audits_against_the_map():
    import torch
    from avoid_mpc_amd import flight
    prm = prm_of()
    frames = task_frames(torch, prm, 4, seed0=8000)
    pl, _, off = run_map(torch, frames, None, 0.0)
    pl.close()
    for mode, radius in ((capi.AMK_AUDIT_REPORT, WIDE), (capi.AMK_AUDIT_SLOW_DOWN, WIDE), (capi.AMK_AUDIT_SLOW_DOWN, TINY)):
        pl, tickets, res = run_map(torch, frames, mode, radius)
        try:
            vetoed = 0
            for fr, t, o, ref in zip(frames[2:], tickets, res, off):
                for k in STEP_KEYS:
                    assert np.array_equal(o[k], ref[k]), (mode, t, k)
                got = pl.kfmap(t).path_cast(torch.from_numpy(o["x0array"]).cuda(), radius * radius)
                torch.cuda.synchronize()
                for k in AUDIT_KEYS:
                    assert np.array_equal(o["audit"][k], got[k].cpu().numpy()), (mode, t, k)
                assert np.array_equal(o["audit"]["src"], got["frame"].cpu().numpy()), (mode, t)
                flags = o["flags"].copy()
                veto = (flags[:, 0] == 1) & (o["audit"]["stop"] != 0) & (mode == capi.AMK_AUDIT_SLOW_DOWN)
                flags[veto, 0] = 0
                assert np.array_equal(o["cmd"], flight.command(o["u"], flags, fr["x"], prm)), (mode, t)
                vetoed += int(veto.sum())
            frames_seen = np.concatenate([o["audit"]["src"] for o in res])
            print(f"map, mode {mode} radius {radius}: vetoed {vetoed}, frames touched {sorted(set(frames_seen.tolist()))}")
            if mode == capi.AMK_AUDIT_SLOW_DOWN:
                assert (vetoed > 0) if radius == WIDE else (vetoed == 0)
        finally:
            pl.close()


def test_argument_rules():
    import torch
    from avoid_mpc_amd.host import KdBatch, Pipeline
    prm = prm_of()
    lib = capi.load()
    fr = task_frames(torch, prm, 1)[0]
    pl = Pipeline(1, S, NPTS, NEDGE, prm)
    try:
        N = pl.N
        INV, UNS = capi.AMK_ERR_INVALID_ARG, capi.AMK_ERR_UNSUPPORTED
        ptr = [C.c_void_p() for _ in range(6)]
        assert lib.amk_pipeline_audit_outputs(pl.h, 0, *[C.byref(p) for p in ptr]) == UNS       # nothing set yet
        call = lambda mode, radius, legs: lib.amk_pipeline_set_path_audit(pl.h, mode, radius, legs)
        assert call(3, 1.0, 0) == INV and call(-1, 1.0, 0) == INV and call(1, -1.0, 0) == INV and call(1, float("nan"), 0) == INV
        assert call(1, 1.0, N) == INV and call(1, 1.0, -1) == INV and lib.amk_pipeline_set_path_audit(None, 1, 1.0, 0) == INV
        assert lib.amk_pipeline_audit_outputs(pl.h, 0, *[C.byref(p) for p in ptr]) == UNS       # ... and a refused call changed nothing
        assert call(capi.AMK_AUDIT_REPORT, 0.5, N - 1) == capi.AMK_OK and call(capi.AMK_AUDIT_OFF, 0.0, 0) == capi.AMK_OK
        assert lib.amk_pipeline_audit_outputs(pl.h, 0, *[C.byref(p) for p in ptr]) == capi.AMK_OK and all(p.value for p in ptr)
        assert call(capi.AMK_AUDIT_REPORT, 0.5, 0) == capi.AMK_OK
        # a frame in flight: the setter is refused unless the frame has already finished (the staged case, which cannot race, is
        # the next test)
        t = pl.submit(fr["cl"], fr["ed"], ref_path_init=fr["ref"], odom=fr["odom"])
        busy = call(capi.AMK_AUDIT_OFF, 0.0, 0)
        assert busy == UNS or (busy == capi.AMK_OK and lib.amk_pipeline_query(pl.h, t) == 1)
        pl.wait(t)
        pl.wait(pl.submit(fr["cl"], fr["ed"], odom=fr["odom"]))      # the refusal left nothing behind: the next launch goes through
        # keyframe handles under the audit: refused at submit, nothing staged
        kd_o, kd_e = KdBatch(S, NPTS), KdBatch(S, NEDGE)
        assert call(capi.AMK_AUDIT_REPORT, 0.5, 0) == capi.AMK_OK
        with pytest.raises(capi.AmkError, match="status 4"):
            pl.submit(fr["cl"], fr["ed"], ref_path_init=fr["ref"], odom=fr["odom"], keyframes=[(kd_o, kd_e)])
        assert lib.amk_pipeline_query(pl.h, 0) == 1
        assert call(capi.AMK_AUDIT_OFF, 0.0, 0) == capi.AMK_OK
        kd_o.close(); kd_e.close()
    finally:
        pl.close()


def test_the_setter_is_refused_while_a_frame_is_staged():
    """an open gang holds a staged frame until it is full: AMK_ERR_UNSUPPORTED, the mode unchanged, deterministically"""
    import torch
    from avoid_mpc_amd.host import Pipeline
    prm = prm_of()
    lib = capi.load()
    fr = task_frames(torch, prm, 1)[0]
    pl = Pipeline(1, S, NPTS, NEDGE, prm, gang=2)
    try:
        t = pl.submit(fr["cl"], fr["ed"], ref_path_init=fr["ref"], odom=fr["odom"])
        assert lib.amk_pipeline_set_path_audit(pl.h, capi.AMK_AUDIT_REPORT, 1.0, 0) == capi.AMK_ERR_UNSUPPORTED
        pl.drain()
        ptr = [C.c_void_p() for _ in range(6)]
        assert lib.amk_pipeline_audit_outputs(pl.h, t, *[C.byref(p) for p in ptr]) == capi.AMK_ERR_UNSUPPORTED    # it changed nothing
        assert lib.amk_pipeline_set_path_audit(pl.h, capi.AMK_AUDIT_REPORT, 1.0, 0) == capi.AMK_OK               # after drain
    finally:
        pl.close()
