"""The point_env view conversions (csrc/point_views.hpp: write_body13, yaw_from_quat) built for the host and held to the
float64 reference of tests/point_views_ref.py over the whole circle and at its edges -- yaw near 0, +-pi/2 and +-pi, the exact
pairs, and every input once more with the unit-norm error (1 +- 2.4e-7) that the dynamics' renormalisation leaves in (c, s),
which at c = -1 gives c < -1.

Tolerances (absolute, none taken from what the code gives):
  * a quaternion component against quat_of_yaw: 2^-21 = 4.8e-7.  The input's norm error (<= 2.4e-7 relative) moves a half-angle
    component by <= 1.2e-7; three binary32 roundings (sum, root, quotient) of values <= 1 add <= 1.8e-7; 2^-21 is 1.6 x the sum.
  * | qz^2 + qw^2 - 1 | <= 2^-20: twice the component bound.
  * round trip (c, s) -> quaternion -> (c, s) against the normalised input: 2^-19 -- the component bound times the factor 4 of
    2 qz qw and 2 qz^2.
  * yaw_from_quat of a binary32-rounded float64 quaternion against (cos, sin): 2^-21 (the well-conditioned direction).
The form write_body13 had before (qw = sqrt(0.5 (1 + c)), qz = s / (2 qw)) fails the first three at the near-pi sets: worst
component error 2.0, | |q|^2 - 1 | 4.5, round trip 8.9 (host build of that form, same inputs; the present form: 2.9e-7,
3.5e-7, 8.3e-7).  For c >= 0 the present form
returns that form's bits, which the last test holds it to."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import point_views_ref as R
from tests.native_flags import host_flags

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_FLAGS = ["-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]
F = np.float32
SENTINEL = F(7.25)


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("point_views") / "libpoint_views_host.so")
    subprocess.check_call(["g++"] + host_flags(HOST_FLAGS) + ["-I" + os.path.join(HERE, "native", "shim"),
                           os.path.join(HERE, "native", "point_views_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.pv_write_body13.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.pv_yaw_from_quat.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def sets():
    return R.input_sets()


def write_rows(lib, cs, seed=1):
    """write_body13 on rows full of sentinels -> (inputs [n][7], rows [n][13])"""
    n = len(cs)
    rng = np.random.default_rng(seed)
    a = rng.uniform(-3, 3, (n, 7)).astype(F)
    a[:, 2:4] = cs
    a = np.ascontiguousarray(a)
    rows = np.full((n, 13), SENTINEL, F)
    lib.pv_write_body13(n, a.ctypes.data, rows.ctypes.data)
    return a, rows


def quats(lib, cs):
    return write_rows(lib, cs)[1][:, 5:7].copy()


def yaw_from_quat(lib, q):
    q = np.ascontiguousarray(q, F)
    cs = np.empty_like(q)
    lib.pv_yaw_from_quat(len(q), q.ctypes.data, cs.ctypes.data)
    return cs


def worst(err, cs):
    i = int(np.argmax(err))
    return f"worst {err[i]:.3e} at (c, s) = ({cs[i, 0]!r}, {cs[i, 1]!r}), {int((err > 0).sum())} of {len(err)} cases off"


def test_the_input_sets_are_the_ones_the_tolerances_were_derived_for(sets):
    assert len(sets) == 18 and sum(len(v) for v in sets.values()) == 3 * (20000 + 20000 + 3 * 2000 + 7)
    n = np.hypot(*sets["near_pi*(1-e)"].astype(np.float64).T)
    assert abs(np.abs(n - 1).max() - R.NORM_ERR) < 1e-7
    assert (np.abs(np.arctan2(*sets["near_pi"].astype(np.float64).T[::-1])) > np.pi - 0.0501).all()
    assert (sets["near_pi"][:, 1] > 0).any() and (sets["near_pi"][:, 1] < 0).any()           # both sides of +-pi
    assert sets["exact*(1+e)"][3, 0] < -1 and sets["exact*(1+e)"][4, 0] < -1                # 0.5 (1 + c) < 0
    assert np.signbit(sets["exact"][4, 1]) and not np.signbit(sets["exact"][3, 1])
    assert sets["exact"][5, 0] == np.nextafter(F(-1), F(0)) and sets["exact"][5, 1] == F(4.9e-4)


def test_write_body13_writes_the_row_and_leaves_z(host_lib, sets):
    a, rows = write_rows(host_lib, sets["circle"][:500])
    assert (rows[:, 2] == SENTINEL).all()
    for col, src in ((0, 0), (1, 1), (7, 4), (8, 5), (12, 6)):
        assert np.array_equal(rows[:, col].view(np.uint32), a[:, src].view(np.uint32)), col
    assert not rows[:, [3, 4, 9, 10, 11]].any()


def test_quaternion_against_the_float64_reference(host_lib, sets):
    bad = []
    for name, cs in sets.items():
        q = quats(host_lib, cs)
        err = R.quat_error(q[:, 0], q[:, 1], cs[:, 0], cs[:, 1])
        print(f"{name}: max |q - q64| = {err.max():.3e}")
        if not (err <= R.TOL_Q).all():          # (a NaN fails too)
            bad.append(f"{name}: {worst(np.where(err <= R.TOL_Q, 0.0, err), cs)}")
    assert not bad, f"tolerance {R.TOL_Q:.3e}: " + "; ".join(bad)


def test_quaternion_is_unit_with_qw_not_negative(host_lib, sets):
    bad = []
    for name, cs in sets.items():
        q = quats(host_lib, cs).astype(np.float64)
        err = np.abs(q[:, 0] ** 2 + q[:, 1] ** 2 - 1.0)
        print(f"{name}: max | |q|^2 - 1 | = {err.max():.3e}, min qw = {q[:, 1].min():.3e}")
        if not (err <= R.TOL_NORM).all() or not (q[:, 1] >= 0).all() or np.signbit(q[:, 1]).any():
            bad.append(f"{name}: {worst(np.where(err <= R.TOL_NORM, 0.0, err), cs)}, min qw {q[:, 1].min()!r}")
    assert not bad, f"tolerance {R.TOL_NORM:.3e}: " + "; ".join(bad)


def test_round_trip_returns_the_normalised_yaw(host_lib, sets):
    bad = []
    for name, cs in sets.items():
        back = yaw_from_quat(host_lib, quats(host_lib, cs)).astype(np.float64)
        c, s = R.unit(cs[:, 0], cs[:, 1])
        err = np.maximum(np.abs(back[:, 0] - c), np.abs(back[:, 1] - s))
        print(f"{name}: max round-trip error = {err.max():.3e}")
        if not (err <= R.TOL_TRIP).all():
            bad.append(f"{name}: {worst(np.where(err <= R.TOL_TRIP, 0.0, err), cs)}")
    assert not bad, f"tolerance {R.TOL_TRIP:.3e}: " + "; ".join(bad)


def old_quaternion(cs):
    """the form write_body13 had before, restated in binary32 numpy: qw = sqrt(max(0.5 (1 + c), 0)); qz = s / (2 qw), or
    (1, 0) where qw <= 1e-4"""
    c, s = cs[:, 0].astype(F), cs[:, 1].astype(F)
    qw = np.sqrt(np.maximum(F(0.5) * (F(1.0) + c), F(0.0)), dtype=F)
    ok = qw > F(1e-4)
    with np.errstate(divide="ignore", invalid="ignore"):
        qz = np.where(ok, s / (F(2.0) * qw), F(1.0)).astype(F)
    return np.stack([qz, np.where(ok, qw, F(0.0)).astype(F)], 1)


def test_front_half_circle_keeps_the_bits_of_the_form_it_replaces(host_lib, sets):
    """every recorded trace with |yaw| <= pi/2 stays valid"""
    seen = 0
    for name, cs in sets.items():
        front = cs[cs[:, 0] >= 0]
        seen += len(front)
        got, want = quats(host_lib, front), old_quaternion(front)
        neq = (got.view(np.uint32) != want.view(np.uint32)).any(1)
        assert not neq.any(), f"{name}: {int(neq.sum())} differ, first (c, s) = {front[neq][0]!r}: {got[neq][0]!r} != {want[neq][0]!r}"
    assert seen > 3 * (10000 + 2000 + 1000)      # half the circle, all of near_0, about half of each near-+-pi/2 set
    assert (old_quaternion(np.array([[1, 0], [0, 1], [-0.0, -1]], F)) ==
            np.array([[0, 1], [np.sqrt(F(0.5)), np.sqrt(F(0.5))], [-np.sqrt(F(0.5)), np.sqrt(F(0.5))]], F)).all()


def test_yaw_from_quat_against_the_float64_reference(host_lib):
    worst_all = 0.0
    yaws = dict(R.yaw_sets())
    ex = R.exact_cs().astype(np.float64)
    yaws["exact"] = np.arctan2(ex[:, 1], ex[:, 0])
    for name, yaw in yaws.items():
        q = np.stack([np.sin(0.5 * yaw), np.cos(0.5 * yaw)], 1).astype(F)
        assert (q[:, 1] >= 0).all()
        cs = yaw_from_quat(host_lib, q).astype(np.float64)
        err = np.maximum(np.abs(cs[:, 0] - np.cos(yaw)), np.abs(cs[:, 1] - np.sin(yaw)))
        print(f"{name}: max |(c, s) - (cos, sin)| = {err.max():.3e}")
        worst_all = max(worst_all, err.max())
        assert (err <= R.TOL_Q).all(), f"{name}: worst {err.max():.3e} at yaw {yaw[int(np.argmax(err))]!r}, tolerance {R.TOL_Q:.3e}"
        # and the reference's own inverse agrees with itself far inside the tolerance
        c64, s64 = R.yaw_of_quat(*R.quat_of_yaw(np.cos(yaw), np.sin(yaw)))
        assert max(np.abs(c64 - np.cos(yaw)).max(), np.abs(s64 - np.sin(yaw)).max()) < 1e-14
    assert worst_all > 0.0
