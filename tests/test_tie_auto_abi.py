"""CPU: the constants of the AMK_TIES_AUTO mode are the same in the public header and in the Python binding, the header
documents them, and the C++ adapter offers the mode by name."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _defines(text):
    out = {}
    for name, val in re.findall(r"^#define\s+(AMK_[A-Z0-9_]+)\s+\(?(-?\d+)\)?\s*(?:/\*.*)?$", text, re.M):
        out[name] = int(val)
    return out


def test_header_and_binding_agree_on_the_tie_order_constants():
    from avoid_mpc_amd import capi
    hdr = open(os.path.join(ROOT, "include", "avoid_mpc_amd.h")).read()
    d = _defines(hdr)
    names = ["AMK_TIES_LOWEST_INDEX", "AMK_TIES_NANOFLANN", "AMK_TIES_AUTO", "AMK_EXACT_OFF", "AMK_EXACT_IN_USE",
             "AMK_EXACT_GAVE_UP", "AMK_EXACT_TOO_DEEP", "AMK_EXACT_NOT_NEEDED", "AMK_MAX_K", "AMK_ERR_UNSUPPORTED"]
    for n in names:
        if n == "AMK_ERR_UNSUPPORTED":   # an enumerator, not a macro
            m = re.search(r"AMK_ERR_UNSUPPORTED\s*=\s*(\d+)", hdr)
            assert m and int(m.group(1)) == capi.AMK_ERR_UNSUPPORTED
            continue
        assert n in d, n
        assert d[n] == getattr(capi, n), (n, d[n], getattr(capi, n))
    assert d["AMK_TIES_AUTO"] == 2 and d["AMK_EXACT_NOT_NEEDED"] == 3
    assert len({d["AMK_TIES_LOWEST_INDEX"], d["AMK_TIES_NANOFLANN"], d["AMK_TIES_AUTO"]}) == 3
    assert len({d[n] for n in names[3:8]}) == 5


def test_cpp_adapter_offers_the_mode():
    hpp = open(os.path.join(ROOT, "include", "avoid_mpc_amd", "kd_tree_two.hpp")).read()
    assert "void SetTieOrder(int mode)" in hpp and "void SetNanoflannTieOrder(bool on)" in hpp
    assert "AMK_EXACT_NOT_NEEDED" in hpp
