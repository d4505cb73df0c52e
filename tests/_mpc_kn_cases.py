"""The (horizon N, neighbour count K) cases of the interior-point solve across the range amk_mpc_create accepts (2 <= N <= 32,
0 <= K <= 64), their inputs and the oracle's answers.  Plain numpy + the CPU oracle; TEST INFRASTRUCTURE ONLY
(tests/test_mpc_kn_cases.py checks on the CPU that the table reaches what it says, tests/test_mpc_kn_gpu.py runs it on the device).

The collision terms of the solve (csrc/mpc_device_impl.h: evaluate, update_term_multipliers) run on one wave with the lane map
    ns = N - 1 (path stages), per = 64 / ns (slots per round), jl = lane / ns, k = lane - jl * ns,
    rounds j0 = 0, per, 2 per, ... < K, lane live iff jl < per and j0 + jl < K,
so the shape of the map changes with N and K: `rounds = ceil(K / per)`, `idle = 64 - ns * per` lanes never work, and the last round
holds `K % per` slots (all `per` when that is 0).  Each row below names what it reaches.

Inputs, as the other solve tests make them: the first vecRefStates of the oracle's control step on synth.make_scene(n, seed, prm)
with T = N * 0.033 + 1e-4, n = 50 000 for K >= 33 and 20 000 otherwise.  K = 0: the same scenes' record built at K = 3 with the
obstacle block cut out.  Every scene with K >= 2 appears in four ARRANGEMENTS of its obstacle block (reference path, target and
initial state untouched):
    packed     ascending distance, as the step writes it;
    reversed   each stage's K slots in reverse order: the nearest neighbours sit in the LAST round;
    last_only  slots 0 .. K - 2 hold the 1e4 padding, slot K - 1 that stage's nearest neighbour;
    all_pad    every slot holds the padding: the problem of the K = 0 record.

Seed admission (CPU only; `admit` below, asserted by tests/test_mpc_kn_cases.py).  Seeds are tried upwards from 400; a seed
enters a row only if, for the oracle and every arrangement of that row,
    * the solve ends with status 0 in at most MPC_DEFAULT_MAX_ITER / 2 iterations;
    * under eight perturbations of the whole vecRefStates by relative 1e-13 (default_rng(PERTURB_SEED)) the info stays the same
      and u, x0array and the warm start move by at most 1e-8 -- scenes whose counts hang on a comparison that is a tie to the
      last digits are the ones the device may flip, and the table keeps away from them;
    * (K >= 2) at the oracle's solutions of `reversed` and `last_only` a term of the last round is live, i.e. its clearance
      |o - p| - radius is below LIVE_CLEARANCE at some stage -- the last round is what those arrangements are for.
Seeds that failed are listed per row in `passed_over` with the condition they failed."""
import functools
from collections import namedtuple

import numpy as np

from avoid_mpc_amd import synth
from tests import _oracle, _pose

PAD = 1e4                  # AvoidanceStateMachine.cpp:223-226: every coordinate of a missing neighbour
LIVE_CLEARANCE = 1.148     # collide_term's pre-test: log(1 + exp(-32 c)) == 0 in fp64 beyond this clearance
ARRANGEMENTS = ("packed", "reversed", "last_only", "all_pad")
PERTURB_SEED, PERTURB_COUNT, PERTURB_REL, PERTURB_TOL = 20261020, 8, 1e-13, 1e-8

Row = namedtuple("Row", "N K kernel reaches seeds passed_over")

_NO_LAST = "reversed / last_only: no live term in the last round"
_TIE = "info or solution changes under a 1e-13 perturbation"
# Seeds beyond 431: at 20 000 points and K <= 10 (and at N = 2, where one stage decides) no scene of 400 ... 438 ends with live AND
# dormant terms in `packed`, which every row with K >= 2 must show once; 439 (475 at N = 2) is the first admitted seed that does.
ROWS = (
    Row(2, 0, "generic", "no collision term at all at the smallest horizon; ybuf sized by K > 0 ? K : 1; loops that never run",
        (400, 401, 402, 403, 404, 405), {}),
    Row(10, 0, "baked", "no collision term at all on a baked kernel", (400, 401, 402, 403, 404, 405), {}),
    Row(10, 1, "baked", "one slot, per = 7, lane 63 idle", (400, 401, 402, 403, 404, 405), {}),
    Row(10, 7, "baked", "exactly one full round", (400, 401, 402, 403, 404, 439), {}),
    Row(10, 8, "baked", "one slot over a round", (400, 401, 402, 403, 404, 439), {}),
    Row(10, 9, "baked", "two slots over a round", (400, 401, 402, 403, 404, 439), {}),
    Row(2, 64, "generic", "ns = 1, per = 64: one round in which all 64 lanes add into one stage's cells",
        (401, 405, 406, 407, 475), {400: _NO_LAST, 402: _NO_LAST, 403: _NO_LAST, 404: _NO_LAST}),
    Row(3, 33, "generic", "per = 32; a second round of one slot per stage", (400, 401, 402, 403, 404, 405), {}),
    Row(17, 64, "generic", "ns = 16, per = 4: no idle lane, 16 full rounds", (400, 402, 403, 404, 405), {401: _TIE}),
    Row(20, 10, "baked", "per = 3, 4 rounds, the last with one slot", (400, 401, 402, 403, 404, 439), {}),
    Row(22, 64, "generic", "per = 3, lane 63 idle, 22 rounds, the last with one slot", (400, 401, 402, 403, 405), {404: _TIE}),
    Row(30, 33, "baked", "per = 2, lanes 58-63 idle, 17 rounds, the last with one slot", (400, 401, 403, 405, 406),
        {402: _TIE, 404: _TIE}),
    Row(30, 64, "baked", "per = 2, lanes 58-63 idle, 32 full rounds", (401, 403, 405, 406), {400: _TIE, 402: _TIE, 404: _TIE}),
    Row(32, 64, "generic", "both maxima: the largest ybuf and vecRefStates", (400, 401, 403, 405), {402: _TIE, 404: _TIE}),
)


# The whole control step (amk_step_batch: search, plan, pack, up to three solves, two steps with the warm start carried over) at the
# new K: synth.make_scene(50 000, seed, prm), seeds tried upwards from 1300.  Admission, CPU only (`admit_step_scene`): under eight
# perturbations of the state quads and the reference path by relative 1e-13 the oracle's step keeps its flags in both steps and moves
# u, x0array and the refilled reference path by at most 1e-8.  At N = 20 every scene passes; at N = 32, K = 64 five of the first six
# change their iteration count by one to thirteen under the FIRST perturbation -- re-plan passes of a 32-stage problem with 1984
# terms end on ties -- and those are the scenes the device flips as well (two of them, against an allowance of one).
StepRow = namedtuple("StepRow", "N K tie_order seeds passed_over")
_STEP_TIE = "flags change under a 1e-13 perturbation"
_S6 = (1300, 1301, 1302, 1303, 1304, 1305)
STEP_ROWS = (
    StepRow(20, 1, 0, _S6, {}), StepRow(20, 10, 0, _S6, {}), StepRow(20, 33, 0, _S6, {}), StepRow(20, 64, 0, _S6, {}),
    StepRow(32, 64, 0, (1305, 1306, 1307, 1309, 1310, 1311),
            {1300: _STEP_TIE, 1301: _STEP_TIE, 1302: _STEP_TIE, 1303: _STEP_TIE, 1304: _STEP_TIE, 1308: _STEP_TIE}),
    StepRow(20, 10, 1, _S6, {}),      # AMK_TIES_NANOFLANN on both handles
    StepRow(20, 63, 2, _S6, {}),      # AMK_TIES_AUTO: K + 1 = 64 neighbours asked of the index
)


def step_row(N, K, tie_order=0):
    return next(r for r in STEP_ROWS if (r.N, r.K, r.tie_order) == (N, K, tie_order))


@functools.lru_cache(maxsize=None)
def step_scenes(N, K):
    """-> (prm, [scene]) of the step rows at (N, K) (the tie order does not change the scenes)."""
    prm = prm_of(N, K)
    return prm, [synth.make_scene(50000, s, prm) for s in next(r for r in STEP_ROWS if (r.N, r.K) == (N, K)).seeds]


def _oracle_two_steps(prm, sc, ko, ke, sq, ref_path):
    m = _oracle.MpcOracle(prm.T, prm.dt, prm.K); m.configure(prm)
    rp, out = np.ascontiguousarray(ref_path).copy(), []
    for _ in range(2):
        r = _oracle.step_oracle(ko, ke, m, prm, sq, sc["pos"][0], rp)
        out.append(dict(flags=r["flags"].copy(), u=r["u"].copy(), x0=r["x0array"].copy(), ref_path=rp.copy()))
    m.close()
    return out


def admit_step_scene(prm, sc):
    """The admission condition of a step scene -> None, or what it fails (a string)."""
    ko, ke = _oracle.kd_oracle(sc["cloud"]), _oracle.kd_oracle(sc["edge"])
    sq = _oracle.scene_state_quads(sc, prm)
    base = _oracle_two_steps(prm, sc, ko, ke, sq, sc["ref_path"])
    if any(b["flags"][1] < 1 or b["flags"][2] != 0 for b in base):
        return f"flags {[b['flags'].tolist() for b in base]}"
    rng = np.random.default_rng(PERTURB_SEED)
    for i in range(PERTURB_COUNT):
        got = _oracle_two_steps(prm, sc, ko, ke, sq * (1.0 + PERTURB_REL * rng.uniform(-1.0, 1.0, sq.shape)),
                                sc["ref_path"] * (1.0 + PERTURB_REL * rng.uniform(-1.0, 1.0, sc["ref_path"].shape)))
        for t, (b, g) in enumerate(zip(base, got)):
            if not np.array_equal(b["flags"], g["flags"]):
                return f"step {t}: flags {b['flags'].tolist()} -> {g['flags'].tolist()} under perturbation {i}"
            d = max(np.abs(b[k] - g[k]).max() for k in ("u", "x0", "ref_path"))
            if d > PERTURB_TOL:
                return f"step {t}: moves by {d:.1e} under perturbation {i}"
    return None


def geometry(N, K):
    """-> (ns, per, rounds, idle, last): stages, slots per round, rounds, idle lanes, slots in the last round (0 when K = 0)."""
    ns = N - 1
    per = 64 // ns
    rounds = -(-K // per)
    return ns, per, rounds, 64 - ns * per, (K - per * (rounds - 1) if K else 0)


def row(N, K):
    return next(r for r in ROWS if (r.N, r.K) == (N, K))


def prm_of(N, K, **kw):
    prm = synth.MpcParams(T=N * 0.033 + 1e-4, K=K, **kw)
    assert prm.N == N
    return prm


def arrangements_of(K):
    return ("k0",) if K == 0 else (("packed",) if K == 1 else ARRANGEMENTS)


def obstacle_block(ref, N, K):
    """A view [..., N, K, 3] of the obstacle triples of vecRefStates = x_init[10] | N ref rows of 10 | N K triples | target[10]."""
    o0 = 10 + 10 * N
    return ref[..., o0:o0 + 3 * K * N].reshape(ref.shape[:-1] + (N, K, 3))


def without_obstacles(ref, N, K):
    o0 = 10 + 10 * N
    return np.ascontiguousarray(np.concatenate([ref[..., :o0], ref[..., o0 + 3 * K * N:]], axis=-1))


def arrange(ref, N, K, name):
    """ref: packed vecRefStates [..., ref_len] -> the named arrangement (a copy)."""
    out = np.array(ref, dtype=np.float64, copy=True)
    src, dst = obstacle_block(np.asarray(ref, np.float64), N, K), obstacle_block(out, N, K)
    if name == "reversed":
        dst[...] = src[..., ::-1, :]
    elif name == "last_only":
        dst[...] = PAD
        dst[..., K - 1, :] = src[..., 0, :]
    elif name == "all_pad":
        dst[...] = PAD
    else:
        assert name == "packed", name
    return out


@functools.lru_cache(maxsize=None)
def _packed(N, K, seeds):
    if K == 0:
        return without_obstacles(_packed(N, 3, seeds), N, 3)
    return _pose.first_ref_states(50000 if K >= 33 else 20000, seeds, prm_of(N, K))


def records(N, K, seeds=None):
    """-> {arrangement: vecRefStates [S, ref_len]} of a row's scenes (seeds: the row's own)."""
    seeds = tuple(row(N, K).seeds if seeds is None else seeds)
    base = _packed(N, K, seeds)
    return {a: (base if a in ("k0", "packed") else arrange(base, N, K, a)) for a in arrangements_of(K)}


def batch(N, K):
    """A row as one batch, arrangement-major -> (names, ref [A * S, ref_len])."""
    rec = records(N, K)
    return list(rec), np.ascontiguousarray(np.concatenate(list(rec.values())))


def oracle_solve(prm, ref):
    """One cold Solve(faster=True) of the oracle -> dict(info, u, x0, w)."""
    m = _oracle.MpcOracle(prm.T, prm.dt, prm.K); m.configure(prm)
    u, x0, info = m.Solve(ref, True)
    out = dict(info=info.copy(), u=u.copy(), x0=x0.copy(), w=m.warm_start.copy())
    m.close()
    return out


@functools.lru_cache(maxsize=None)
def oracle_solutions(N, K):
    """-> {arrangement: [dict(info, u, x0, w) per scene]}: the oracle's cold solve of every record of the row."""
    prm = prm_of(N, K)
    return {a: [oracle_solve(prm, r) for r in R] for a, R in records(N, K).items()}


def live_terms(prm, ref, w):
    """bool [N - 1, K]: the collision terms whose clearance at the iterate w is below LIVE_CLEARANCE.  Term (k, j) couples the state
    X_{k+1} with obstacle triple (k, j); the last stage's triples are not read (the goal stage has no collision term)."""
    N, K = prm.N, prm.K
    X = np.stack([w[14 * (k + 1):14 * (k + 1) + 3] for k in range(N - 1)])
    o = obstacle_block(np.asarray(ref, np.float64), N, K)[:N - 1]
    return np.linalg.norm(o - X[:, None, :], axis=2) - prm.radius < LIVE_CLEARANCE


def last_round(N, K):
    ns, per, rounds, idle, last = geometry(N, K)
    return slice(per * (rounds - 1), K)


def admit(prm, ref, arrangement="packed", sol=None):
    """The admission conditions for one record -> None, or the condition it fails (a string)."""
    s = oracle_solve(prm, ref) if sol is None else sol
    if s["info"][0] != 0:
        return f"{arrangement}: status {s['info'][0]}"
    if s["info"][1] > _oracle.MPC_DEFAULT_MAX_ITER // 2:
        return f"{arrangement}: {s['info'][1]} iterations"
    if arrangement in ("reversed", "last_only") and not live_terms(prm, ref, s["w"])[:, last_round(prm.N, prm.K)].any():
        return f"{arrangement}: no live term in the last round"
    rng = np.random.default_rng(PERTURB_SEED)
    for i in range(PERTURB_COUNT):
        t = oracle_solve(prm, ref * (1.0 + PERTURB_REL * rng.uniform(-1.0, 1.0, ref.shape)))
        if not np.array_equal(t["info"], s["info"]):
            return f"{arrangement}: info {s['info'].tolist()} -> {t['info'].tolist()} under perturbation {i}"
        d = max(np.abs(t[k] - s[k]).max() for k in ("u", "x0", "w"))
        if d > PERTURB_TOL:
            return f"{arrangement}: solution moves by {d:.1e} under perturbation {i}"
    return None


def admit_seed(N, K, seed):
    prm = prm_of(N, K)
    for a, R in records(N, K, (seed,)).items():
        why = admit(prm, R[0], a)
        if why:
            return why
    return None
