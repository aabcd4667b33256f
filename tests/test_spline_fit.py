"""The product's smoothing-spline routine (m3p2i_aip_amd/csrc/spline_fit.hpp -- what the device
sampler runs per series) compiled for the host and compared with scipy's FITPACK
(splrep + splev, the calls the reference's sampler makes, mppi_utils.py bspline): the port follows
FITPACK's operation order, so the results are expected to be IDENTICAL, not merely close."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.native_flags import host_flags
from tests.spline_edge_series import EDGE_CASES, edge_series, rows_for, scipy_rows, set_fixed_series

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("splinefit") / "libsplinefit_host.so")
    subprocess.check_call(["g++"] + host_flags(["-O2", "-shared", "-fPIC", "-ffp-contract=off"]) +
                          [os.path.join(HERE, "native", "spline_fit_host.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.sf_fit_eval_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def fit(lib, Y, k, s, T):
    Y = np.ascontiguousarray(Y, np.float64)
    out = np.zeros((Y.shape[0], T))
    kn = np.zeros(Y.shape[0], np.int32)
    lib.sf_fit_eval_batch(Y.ctypes.data, Y.shape[0], Y.shape[1], k, s, T, out.ctypes.data, kn.ctypes.data)
    return out, kn


scipy_fit = scipy_rows


PLANNER_CASES = [(7, 30, 2, 0.5), (5, 20, 2, 0.5), (3, 12, 2, 0.5), (16, 64, 2, 0.5), (7, 30, 3, 0.5), (7, 30, 1, 0.5),
                 (7, 30, 2, 0.05), (7, 30, 2, 5.0), (12, 50, 2, 0.0), (32, 128, 2, 0.5)]


@pytest.mark.parametrize("m,T,k,s", PLANNER_CASES + EDGE_CASES)
def test_identical_to_scipy_fitpack(host_lib, m, T, k, s):
    """The first eleven series of every case are the fixed ones of tests/spline_edge_series.py (the first four as before).
    EDGE_CASES: the table k_spline_noise runs on the device (tests/test_device_sampler_edges_gpu.py), on the float32 series
    the device gets; the other cases keep their binary64 series."""
    seed = m * 1000 + T + k
    if (m, T, k, s) in EDGE_CASES:
        Y = edge_series(m, rows_for(m), seed).astype(np.float64)
    else:
        Y = set_fixed_series(np.random.default_rng(seed).standard_normal((rows_for(m), m)))
    out, kn = fit(host_lib, Y, k, s, T)
    ref, nref = scipy_fit(Y, k, s, T)
    np.testing.assert_array_equal(kn, nref)
    np.testing.assert_array_equal(out, ref)


@pytest.mark.parametrize("scramble", ["none", "faure"])
@pytest.mark.parametrize("K,nu,m", [(3000, 2, 16), (3000, 9, 11), (3000, 2, 64), (3000, 2, 2)])
def test_degree_one_without_smoothing_returns_its_input(host_lib, K, nu, m, scramble):
    """k = 1, s = 0, T = m: the evaluation abscissae are the data abscissae and the spline interpolates, so the fit -- rounded to
    float32 like the noise buffer -- IS its float32 input, bit for bit.  This is how tests/test_device_sampler_edges_gpu.py
    reads the device's Gaussian Halton knots out of the noise buffer.  (k = 2, 3 interpolate to ~1e-11 relative only: an exact 0.0
    among the knots comes back as 2.6e-18.)"""
    from m3p2i_aip_amd import sampling
    g = sampling.halton_gaussian(K, nu * m, scramble).numpy().reshape(K * nu, m)
    assert g.dtype == np.float32 and np.isfinite(g).all()
    out, kn = fit(host_lib, g, 1, 0.0, m)
    np.testing.assert_array_equal(kn, m + 2)                        # the interpolating spline: every interior point a knot
    np.testing.assert_array_equal(out.astype(np.float32), g)


def test_sampler_knots_reproduce_the_host_sampler(host_lib):
    """halton_knots -> spline_fit == halton_spline_delta (the scipy path pinned by golden G8)."""
    from m3p2i_aip_amd import sampling
    K, T, nu = 300, 30, 2
    knots = sampling.halton_knots(K, T, nu).numpy().astype(np.float64)          # [K, nu, n_knots]
    out, _ = fit(host_lib, knots.reshape(K * nu, -1), 2, 0.5, T)
    mine = out.reshape(K, nu, T).transpose(0, 2, 1).astype(np.float32)
    ref = sampling.halton_spline_delta(K, T, nu, workers=1).numpy()
    np.testing.assert_array_equal(mine, ref)
