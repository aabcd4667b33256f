"""spline_fit.hpp (what k_spline_noise runs per thread) at the declared bounds of its fixed arrays, without a GPU and outside
python: tests/native/spline_fit_check.cpp -- its own main -- runs every degree with m = degree + 1, 63 and 64 points and
s = 0, 0.5 and 1e6, and the arguments the routine must refuse.  Built plain and with AddressSanitizer +
UndefinedBehaviorSanitizer (-fno-sanitize-recover=all: the first finding aborts), run directly: both builds must end with
status 0 and print the same checksums.  On the device the same arrays live in per-thread scratch, where an index past the
end corrupts a neighbour silently; here it is a report."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "m3p2i_aip_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"] + extra +
                          ["-I" + CSRC, os.path.join(HERE, "native", "spline_fit_check.cpp"), "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True)     # (run directly: nothing sanitized is loaded into python)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("splinefit_check")
    return build_and_run(d, "spline_fit_check", []), build_and_run(d, "spline_fit_check_san", SAN)


def test_the_fixed_arrays_hold_at_their_bounds_under_asan_and_ubsan(runs):
    plain, san = runs
    for r in (plain, san):
        assert r.returncode == 0 and r.stdout.endswith("spline_fit_check: ok\n") and "FAIL" not in r.stdout, r.stdout + r.stderr
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    assert san.stdout == plain.stdout


def test_every_combination_ran(runs):
    lines = [ln for ln in runs[0].stdout.splitlines() if ln.startswith("k=")]
    assert len(lines) == 27 and len({ln.split("checksum")[0] for ln in lines}) == 27
    # m = k + 1 has no interior knot to place (2k + 2 knots); m = 64 with s = 0 interpolates (m + k + 1 knots)
    for k in (1, 2, 3):
        assert any(ln.startswith(f"k={k} m={k + 1:2d} ") and f"knots {2 * k + 2:2d}..{2 * k + 2:2d}" in ln for ln in lines)
        assert any(ln.startswith(f"k={k} m=64 s=0 ") and f"..{64 + k + 1:2d} " in ln for ln in lines)
