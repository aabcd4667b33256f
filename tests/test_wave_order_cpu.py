"""The float64 reference of the wavefront order (tests/wave_order_ref.py) checked on its own, without a GPU: its permutation
against a brute-force construction, its bound against a float32 twin of itself on every input the GPU tests use
(tests/wave_order_cases.py), and the comparison's teeth -- it refuses the orders a wrong key would give."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import wave_order_cases as W
from tests import wave_order_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (K_global, k_offset, K_local, multi_modal): unsharded, both kinds of whole-mode shards, a shard the mode boundary cuts,
# the last shard (holds K_global - 1), a middle shard without any special sample
LAYOUTS = [(128, 0, 128, False), (200, 0, 200, False), (256, 0, 256, True), (257, 0, 257, True),
           (512, 0, 256, True), (512, 256, 256, True), (512, 192, 128, True), (512, 384, 128, True),
           (1024, 256, 128, True), (512, 256, 256, False)]


def _brute_force(keys, Kg, k0, Kl, mm, relabel):
    h = min(max(Kg // 2 - k0, 0), Kl) if mm else Kl
    slots = sorted(range(Kl), key=lambda i: (i >= h, keys[i], i))      # mode, key, index: a stable sort per mode
    if relabel:
        for g in (0, Kg // 2, Kg - 1):
            s = g - k0
            if 0 <= s < Kl:
                j = slots.index(s)
                slots[j] = slots[s]
                slots[s] = s
    return np.array(slots)


@pytest.mark.parametrize("Kg,k0,Kl,mm", LAYOUTS)
@pytest.mark.parametrize("relabel", [False, True])
def test_expected_perm_equals_a_brute_force_construction(Kg, k0, Kl, mm, relabel):
    rng = np.random.default_rng(Kg + 7 * k0 + Kl + mm)
    for ties in (False, True):
        keys = rng.standard_normal(Kl) * 300.0
        if ties:
            keys = np.round(keys / 50.0) * 50.0        # many equal keys: stability decides
        p = R.expected_perm(keys, Kg, k0, Kl, mm, relabel)
        assert np.array_equal(p, _brute_force(keys, Kg, k0, Kl, mm, relabel))
        assert R.compare(p, keys, Kg, k0, Kl, mm, relabel, 0.0) == 0.0


def test_half_local_and_specials_follow_order_block():
    assert R.half_local(512, 0, 512, True) == 256 and R.half_local(512, 0, 512, False) == 512
    assert R.half_local(512, 256, 256, True) == 0 and R.half_local(512, 0, 256, True) == 256
    assert R.half_local(512, 192, 128, True) == 64 and R.half_local(1024, 0, 128, True) == 128
    assert R.specials(512, 0, 512) == [0, 256, 511] and R.specials(512, 256, 256) == [0, 255]
    assert R.specials(512, 0, 256) == [0] and R.specials(1024, 256, 128) == []


def test_principal_axis_of_the_scenes():
    """the values tests/wave_order_cases.py states"""
    th = {n: float(R.principal_axis(s["box"], s["dyn"], W.OBSTACLE)) for n, s in W.SCENES.items()}
    assert th["row"] == 0.0
    assert abs(th["oblique"] - 0.5 * np.arctan2(2 * 87 / 9, 78 / 9 - 114 / 9)) < 1e-12 and abs(th["oblique"] - 0.887) < 1e-3
    assert abs(th["bound"] - (-1.385)) < 1e-3
    for n in ("oblique", "bound"):      # neither x nor y, and float32 agrees on the branch
        assert min(abs(np.sin(th[n])), abs(np.cos(th[n]))) > 0.15
        s = W.SCENES[n]
        assert abs(float(R.principal_axis(s["box"], s["dyn"], W.OBSTACLE, np.float32)) - th[n]) < 1e-6


@pytest.mark.parametrize("name", list(W.CASES))
def test_the_float32_twin_of_the_reference_stays_within_the_bound(name):
    """On every input of the GPU tests: rows pairwise distinct (the GPU tests recover the order from row bytes), the keys
    formed in float32 within tol of the float64 ones, and the order they give passes the comparison."""
    c = W.case(name)
    rows = {r.tobytes() for r in c["delta"]}
    assert len(rows) == c["K"], "noise rows are not pairwise distinct"
    for k0, Kl in c["blocks"]:
        keys, bound = W.block_keys(c, k0, Kl)
        k32 = R.keys32(c["delta"][k0:k0 + Kl], W.SIGMA, c["box"], c["dyn"], c["obs"]).astype(np.float64)
        err = float(np.abs(k32 - keys).max())
        print(f"{name} block {k0}+{Kl}: float32 twin error {err:.3g}, bound {bound:.3g} ({bound / max(err, 1e-300):.0f}x)")
        assert err <= bound
        assert bound < 0.05, "the bound is far below the spacing of the keys at these sizes"
        for relabel in (False, True):
            p32 = R.expected_perm(k32, c["K"], k0, Kl, c["mm"], relabel)
            R.compare(p32, keys, c["K"], k0, Kl, c["mm"], relabel, bound)


@pytest.mark.parametrize("name", ["multi_K256", "multi_K512_T30", "shards_K512"])
def test_the_comparison_refuses_keys_that_lost_their_precision(name):
    """A key that carries the mode as an offset of 1e9 in float32 (one ulp there is 64) leaves index order inside buckets
    of 64 key units: the comparison must refuse that order, and the order of a constant key."""
    c = W.case(name)
    for k0, Kl in c["blocks"]:
        keys, bound = W.block_keys(c, k0, Kl)
        h = R.half_local(c["K"], k0, Kl, c["mm"])
        if h == Kl:
            continue
        coarse = keys.astype(np.float32)
        coarse[h:] = (coarse[h:] + np.float32(1e9)) - np.float32(1e9)
        p = R.expected_perm(coarse.astype(np.float64), c["K"], k0, Kl, c["mm"], False)
        with pytest.raises(AssertionError, match="differs from the reference"):
            R.compare(p, keys, c["K"], k0, Kl, c["mm"], False, bound)
        with pytest.raises(AssertionError, match="differs from the reference"):
            R.compare(np.arange(Kl), keys, c["K"], k0, Kl, c["mm"], False, bound)


def test_the_comparison_refuses_what_is_no_order_of_the_block():
    c = W.case("multi_K256")
    keys, bound = W.block_keys(c, 0, 256)
    good = R.expected_perm(keys, 256, 0, 256, True, True)
    R.compare(good, keys, 256, 0, 256, True, True, bound)
    twice = good.copy()
    twice[5] = twice[6]
    with pytest.raises(AssertionError, match="not a permutation"):
        R.compare(twice, keys, 256, 0, 256, True, True, bound)
    with pytest.raises(AssertionError, match="special sample"):
        R.compare(R.expected_perm(keys, 256, 0, 256, True, False), keys, 256, 0, 256, True, True, bound)
    one_mode = R.expected_perm(keys, 256, 0, 256, False, False)
    with pytest.raises(AssertionError, match="left its mode's half"):
        R.compare(one_mode, keys, 256, 0, 256, True, False, bound)


def test_wave_order_entry_point_is_declared_bound_and_exported():
    from m3p2i_aip_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    assert "int m3_wave_order(m3_handle* h, const int** order_dev, int* n);" in hdr
    assert "#define M3_ABI_VERSION 4" in hdr          # (an appended function: no struct field, no buffer id)
    bound = {s[0]: (s[1], list(s[2])) for s in L.SYMBOLS}
    assert bound["m3_wave_order"] == (C.c_int, [L._H, C.POINTER(C.c_void_p), C.POINTER(C.c_int)])
    lib = L.load()
    p, n = C.c_void_p(1), C.c_int(7)
    assert lib.m3_wave_order(None, C.byref(p), C.byref(n)) == -1   # M3_ERR_BAD_ARG
