"""The two entry points of the point rollout's two-wavefront form (m3_set_point_rollout_form, m3_point_rollout_form_used):
declared in the public header and bound in _lib.SYMBOLS with the same signatures.  Needs the library only to load."""
import ctypes as C
import os
import re

from m3p2i_aip_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"int": C.c_int, "m3_handle*": L._H}


def _declared(hdr, name):
    """(result, [argument types]) of `name` as the header declares it"""
    m = re.search(r"^(\w+)\s+%s\(([^)]*)\);" % re.escape(name), hdr, re.M)
    assert m, f"{name} is not declared in include/m3p2i_hip.h"
    args = [re.sub(r"\s*\w+$", "", a.strip()).replace(" ", "") for a in m.group(2).split(",")]
    return CTYPES[m.group(1)], [CTYPES[a] for a in args]


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    bound = {s[0]: (s[1], list(s[2])) for s in L.SYMBOLS}
    for name, expect in (("m3_set_point_rollout_form", (C.c_int, [L._H, C.c_int])),
                         ("m3_point_rollout_form_used", (C.c_int, [L._H]))):
        assert _declared(hdr, name) == expect, name
        assert bound[name] == expect, name
    assert "#define M3_ABI_VERSION 4" in hdr          # (appended functions: no struct changes)
    lib = L.load()
    assert lib.m3_point_rollout_form_used(None) == -1  # (null handle: as before the first rollout)
    assert lib.m3_set_point_rollout_form(None, 1) == -1   # M3_ERR_BAD_ARG
