"""The solve on the device against the oracle, row by row, under the comparison rule of tests/test_mpc_gpu.py (module docstring
there): shared by tests/test_mpc_pose_gpu.py and tests/test_mpc_kn_gpu.py.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from tests import _pose

TOL = 1e-6


def _solve_both(prm, ref, n_solves=1, faster_first=True):
    """Every row of ref on the device (ONE launch per solve) and on the oracle, n_solves times from the kept warm start; compares
    with the rule of the module docstring.  -> dict(worst, flipped, cases, u / info of the device's first solve, w_cpu: the
    oracle's first solution)"""
    import torch
    from avoid_mpc_amd.host import MpcBatch
    S = len(ref)
    gpu = MpcBatch(prm.T, prm.dt, prm.K, S); gpu.configure(prm)
    ref_d = torch.from_numpy(np.ascontiguousarray(ref)).cuda()
    worst, flipped, first = 0.0, 0, None
    with _pose.oracle_under(prm) as make:
        cpu = [make() for _ in range(S)]
        for it in range(n_solves):
            u, x0, info = gpu.Solve(ref_d, faster=(faster_first and it == 0))
            torch.cuda.synchronize()
            u, x0, info = u.cpu().numpy(), x0.cpu().numpy(), info.cpu().numpy()
            warm = gpu.get_warm_start().cpu().numpy()
            fix = False
            for s in range(S):
                uc, xc, ic = cpu[s].Solve(ref[s], faster_first and it == 0)
                du, dx = np.abs(u[s] - uc).max(), np.abs(x0[s] - xc).max()
                if np.array_equal(info[s], ic):
                    dw = np.abs(warm[s] - cpu[s].warm_start).max()
                    assert max(du, dx, dw) <= TOL, (it, s, info[s], du, dx, dw)
                    worst = max(worst, du, dx, dw)
                else:   # rounding-level branch flip: same optimum, other counts
                    flipped += 1
                    assert info[s][0] == 0 and ic[0] == 0 and du <= 1e-4 and dx <= 1e-4, (it, s, info[s], ic, du, dx)
                    warm[s] = cpu[s].warm_start; fix = True      # keep the two sides on the same warm start
            if fix and it + 1 < n_solves:
                gpu.set_warm_start(torch.from_numpy(warm).cuda())
            if first is None:
                first = dict(u=u, info=info, w_cpu=np.stack([m.warm_start.copy() for m in cpu]))
    gpu.close()
    return dict(worst=worst, flipped=flipped, cases=S * n_solves, **first)


def _assert_flipped(r, label):
    print(f"{label}: max |gpu - oracle| = {r['worst']:.3e}, scenes with flipped counts: {r['flipped']}/{r['cases']}")
    assert r["worst"] <= TOL and r["flipped"] <= max(1, r["cases"] // 100)
