"""Generates tests/golden/kd_ref_golden.npz: the REFERENCE's own answers (its nanoflann header compiled in place,
oracle/_ref; see oracle/ref_nanoflann.cpp and oracle/Makefile) on the clouds and queries of tests/test_kd_oracle.py and of
test_nanoflann_tie_order_mode in tests/test_kd_gpu.py, read back by tests/_oracle.py RefAnswers.

Run where the reference is present, after build():   python tests/golden/make_kd_ref_golden.py
The answers to the hostile queries (test_kd_oracle._hostile_queries: NaN, +-inf, overflow) are recorded in a CHILD process, one
per cloud: a crash of the reference on such an input is then a finding (the child's exit status is reported), not the end of
this script.
Per cloud (prefix): queries [Q, 3], cloud_sum (nansum over the points), size; per result count n and kind (search: indices,
squared distances, points; raw: indices, squared distances) the answers padded to n columns with their counts.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _oracle  # noqa: E402
from tests import test_kd_gpu as tg  # noqa: E402
from tests import test_kd_oracle as to  # noqa: E402


def record(out, prefix, cloud, queries, ns, strict=True, raw=False, allow_nonfinite=False):
    t = _oracle.kd_ref(cloud, strict=strict, allow_nonfinite=allow_nonfinite)
    assert t is not None, "oracle/_ref missing: build() with the reference present"
    queries = np.asarray(queries, np.float64).reshape(-1, 3)
    out[prefix + ".queries"] = queries
    out[prefix + ".cloud_sum"] = np.nansum(np.asarray(cloud, np.float64), axis=0)
    out[prefix + ".size"] = np.int64(t.size())
    for n in ns:
        for kind in ("search", "raw") if raw else ("search",):
            m = max(n, 1)
            idx = np.full((len(queries), m), -1, np.int32)
            d2 = np.full((len(queries), m), np.finfo(np.float64).max)
            pts = np.zeros((len(queries), m, 3), np.float32)
            cnt = np.zeros(len(queries), np.int32)
            for i, q in enumerate(queries):
                r = t.search(q, n) if kind == "search" else t.search_raw(q, n)
                cnt[i] = len(r[0])
                idx[i, :cnt[i]], d2[i, :cnt[i]] = r[0], r[1]
                if kind == "search":
                    pts[i, :cnt[i]] = r[2]
            key = f"{prefix}.n{n}.{kind}"
            out[key + ".idx"], out[key + ".d2"], out[key + ".cnt"] = idx, d2, cnt
            if kind == "search":
                out[key + ".pts"] = pts
    t.close()


def record_hostile_in_child(out, name):
    """hostile.<name>: the reference's answers for the hostile queries on the finite cloud <name>, made by a child process."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "hostile.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--hostile-child", name, path])
        assert r.returncode == 0, f"the reference ended with status {r.returncode} on the hostile queries of {name}: a finding"
        with np.load(path) as G:
            out.update({k: G[k] for k in G.files})


def hostile_child(name, path):
    out = {}
    record(out, "hostile." + name, to._clouds()[name], to._hostile_queries()[1], (1, 3, 8), raw=True)
    np.savez(path, **out)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--hostile-child":
        return hostile_child(sys.argv[2], sys.argv[3])
    out = {}
    for name in to.HOSTILE_CLOUDS:
        record_hostile_in_child(out, name)
    for name, cloud in to._clouds().items():
        record(out, name, cloud, to._queries(name, cloud), (1, 3, 8), raw=True)
    record(out, "nan_x", to._nan_x_cloud(), [[0.1, 0.2, 0.3]], (1, 8, 46, 47, 48, 60))
    cloud, qs = to._nan_y_cloud_and_queries()
    record(out, "nan_y", cloud, qs, (8,), allow_nonfinite=True)   # one NaN y among 50 points: known to build
    record(out, "empty", np.zeros((0, 3), np.float32), [[0.0, 0.0, 0.0]], (3,))
    cloud, qs = to._fma_cloud_and_queries()
    record(out, "fma", cloud, qs, (8,), strict=False)
    for name, cloud, qs in tg._tie_order_cases():
        record(out, "tie." + name, cloud, qs, (1, 3, 8, 10))
    path = os.path.join(ROOT, "tests", "golden", "kd_ref_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
