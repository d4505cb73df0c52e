"""CPU: the MPC's host half states its model, layouts and horizon dispatch once (csrc/mpc_model.h, mpc_handle.h with_horizon); what the
compiler makes of the kernels stays what it made of the copies.  The eight solve instantiations and the pack kernels that write the
scene record (pack_ref_states) are the hot path: every figure equal.  The eight NLP evaluation kernels: no scratch, the same LDS, no
more VGPRs.  Exactly these sixteen mpc_* kernels exist, compiled by the mpc_solve and mpc_eval units.  No compute calls
(tests/test_mpc_gpu.py, test_mpc_eval_gpu.py, test_casadi_plugin_gpu.py and the step tests run them)."""
import glob
import json
import os
import re

import pytest

from avoid_mpc_amd import build as amk_build

# kernel_resources.json of the commit before (595e9bb, the build's flags for gfx950):
# (kernel, leading template arguments as mangled) -> (vgprs, sgprs, scratch_bytes_per_lane, lds_bytes, occupancy)
SOLVE = {
    ("mpc_solve_kernel", "Li0E"): (184, 106, 0, 0, 2),
    ("mpc_solve_kernel", "Li10E"): (180, 106, 0, 0, 2),
    ("mpc_solve_kernel", "Li20E"): (180, 106, 0, 0, 2),
    ("mpc_solve_kernel", "Li30E"): (180, 106, 0, 0, 2),
    ("mpc_solve_kernel_f32", "Li0E"): (126, 106, 0, 0, 4),
    ("mpc_solve_kernel_f32", "Li10E"): (125, 106, 0, 0, 4),
    ("mpc_solve_kernel_f32", "Li20E"): (126, 106, 0, 0, 4),
    ("mpc_solve_kernel_f32", "Li30E"): (126, 106, 0, 0, 4),
}
EVAL = {
    ("mpc_eval_kernel", "Li0E"): (164, 83, 0, 0, 3),
    ("mpc_eval_kernel", "Li10E"): (160, 70, 0, 0, 3),
    ("mpc_eval_kernel", "Li20E"): (162, 70, 0, 0, 3),
    ("mpc_eval_kernel", "Li30E"): (162, 70, 0, 0, 3),
    ("mpc_eval_gamma_kernel", "Li0E"): (166, 106, 0, 0, 3),
    ("mpc_eval_gamma_kernel", "Li10E"): (164, 106, 0, 0, 3),
    ("mpc_eval_gamma_kernel", "Li20E"): (166, 106, 0, 0, 3),
    ("mpc_eval_gamma_kernel", "Li30E"): (166, 106, 0, 0, 3),
}
PACK = {   # every kernel that calls pack_ref_states (step_common.h): step.hip's, and step_frames.hip's merge
    ("step_plan_pack_kernel", "Lb0ELb0E"): (92, 70, 0, 808, 5),
    ("step_plan_pack_kernel", "Lb0ELb1E"): (48, 106, 0, 1296, 7),
    ("step_plan_pack_kernel", "Lb1ELb1E"): (48, 106, 0, 3224, 7),
    ("step_requery_pack_auto_kernel", ""): (27, 86, 0, 1928, 8),
    ("step_merge_plan_pack_kernel", "Lb0ELi0E"): (63, 106, 0, 5344, 7),
    ("step_merge_plan_pack_kernel", "Lb0ELi1E"): (63, 106, 0, 5344, 7),
    ("step_merge_plan_pack_kernel", "Lb0ELi2E"): (63, 106, 0, 5344, 7),
    ("step_merge_plan_pack_kernel", "Lb0ELi4E"): (70, 106, 0, 5344, 7),
    ("step_merge_plan_pack_kernel", "Lb0ELi16E"): (202, 106, 0, 5344, 2),
    ("step_merge_plan_pack_kernel", "Lb1ELi0E"): (81, 106, 0, 9952, 5),
    ("step_merge_plan_pack_kernel", "Lb1ELi4E"): (81, 106, 0, 9952, 5),
    ("step_merge_plan_pack_kernel", "Lb1ELi16E"): (202, 106, 0, 7272, 2),
}
FIELDS = ("vgprs", "sgprs", "scratch_bytes_per_lane", "lds_bytes", "occupancy")


@pytest.fixture(scope="module")
def table():
    amk_build.build()
    return json.load(open(amk_build.RES))


def _find(table, name, targs):
    """the one kernel whose own identifier is `name` (Itanium mangling writes it behind its length) with these leading template arguments"""
    key = f"{len(name)}{name}" + (f"I{targs}" if targs else "E")
    found = [n for n in table if key in n]
    assert len(found) == 1, (name, targs, found)
    return found[0]


def _row(r):
    return tuple(r[f] for f in FIELDS)


@pytest.mark.parametrize("parent", [SOLVE, PACK], ids=["solve", "pack"])
def test_the_hot_kernels_keep_every_figure(table, parent):
    for (name, targs), want in parent.items():
        n = _find(table, name, targs)
        print(n, table[n])
        assert _row(table[n]) == want, (name, targs, table[n])


def test_the_evaluation_kernels_grow_nothing(table):
    for (name, targs), (vgprs, _, scratch, lds, _) in EVAL.items():
        r = table[_find(table, name, targs)]
        print(name, targs, r)
        assert r["scratch_bytes_per_lane"] == 0 == scratch, (name, targs, r)   # the Hessian pattern's table did not land in scratch
        assert r["lds_bytes"] == lds, (name, targs, r)
        assert r["vgprs"] <= vgprs, (name, targs, r)


def test_exactly_these_sixteen_mpc_kernels_from_their_two_units(table):
    mine = sorted(n for n in table if re.search(r"\d+mpc_[a-z0-9_]*kernel", n))   # every kernel whose own name starts with mpc_
    want = sorted(_find(table, name, targs) for name, targs in list(SOLVE) + list(EVAL))
    assert mine == want and len(mine) == 16, mine
    per_object = {os.path.basename(p)[:-len(".o.res.json")]: list(json.load(open(p)))
                  for p in glob.glob(os.path.join(amk_build.OBJ, "*.o.res.json"))}
    for unit, kernels in per_object.items():
        here = sorted(n for n in kernels if n in mine)
        expect = {"mpc_solve": [n for n in want if "mpc_solve_kernel" in n], "mpc_eval": [n for n in want if "mpc_eval" in n]}.get(unit, [])
        assert here == sorted(expect), (unit, here)
    assert {"mpc_solve", "mpc_eval"} <= set(per_object), sorted(per_object)
