"""The series and the case table that tests/test_spline_fit.py (host build of spline_fit.hpp, g++) and
tests/test_device_sampler_edges_gpu.py (k_spline_noise, hipcc for gfx950) both run against SciPy's FITPACK: the two
compilers see the same inputs.

A case is (n_knots, T, degree, s): m = n_knots data points on linspace(0, m, m), evaluated at linspace(0, m, T).  The table
holds what m3_set_noise_knots admits and the planner's own shapes never reach: degree 1 and 3, s = 0, m = degree + 1 (the
interpolating polynomial without an interior knot), m = 63 / 64 (every fixed array of spline_fit.hpp at its declared bound),
more knots than outputs, and an s far above every residual."""
import numpy as np

F32_005 = float(np.float32(0.05))       # the C API takes `smoothing` as a float: SciPy gets the rounded value

EDGE_CASES = [(2, 9, 1, 0.5), (4, 16, 3, 0.5), (64, 256, 2, 0.5), (64, 256, 3, 0.5), (64, 64, 1, 0.5), (63, 250, 2, 0.5),
              (7, 30, 2, F32_005), (16, 64, 2, 0.0), (64, 256, 2, 0.0), (33, 9, 2, 0.5), (7, 30, 2, 1e6)]
N_FIXED = 11


def rows_for(m):
    """1500 series for the small m, 300 where one SciPy fit takes a millisecond"""
    return 300 if m >= 63 else 1500


def set_fixed_series(Y):
    """Rows 0..10 of Y [rows, m] (standard-normal on entry, any float dtype) become the eleven fixed series, in Y's dtype."""
    rows, m = Y.shape
    assert rows >= N_FIXED
    i = np.arange(m)
    alt = np.where(i % 2 == 0, 1.0, -1.0)
    Y[0] = 0.0                          # degenerate: every residual is zero
    Y[1] = i                            # exactly polynomial
    Y[2] *= 1e-3                        # residual far below s = 0.5: the polynomial is accepted
    Y[3] *= 30.0                        # residual far above s: many knots, many p iterations
    Y[4] = 7.5                          # constant
    Y[5] = 3.0 * alt                    # the highest frequency m points can carry
    Y[6] = 0.0
    Y[6, m // 2] = 50.0                 # one spike: fpknot keeps splitting the same interval
    Y[7] = np.where(i < m // 2, -4.0, 4.0)   # a step
    Y[8] *= 1e4                         # stiff: the rational iteration on p starts far from its root
    Y[9] *= 1e-20                       # residuals near the bottom of the binary64 range once squared
    Y[10] = np.sqrt(0.5 / m) * alt      # the constant fit's residual is ~ s = 0.5: |fp - s| < acc on its boundary
    return Y


def edge_series(m, rows, seed):
    """float32 [rows, m]: what the device gets (k_spline_noise widens its float knots to binary64)."""
    Y = np.random.default_rng(seed).standard_normal((rows, m)).astype(np.float32)
    return set_fixed_series(Y)


def scipy_rows(Y, k, s, T):
    """splrep + splev(ext=3) per row of Y [rows, m] -- the reference sampler's calls (bspline()) -- as binary64 [rows, T], and the
    knot count of every fit"""
    import scipy.interpolate as si
    Y = np.asarray(Y, np.float64)
    m = Y.shape[1]
    x, xe = np.linspace(0, m, m), np.linspace(0, m, T)
    ref, n = np.zeros((Y.shape[0], T)), np.zeros(Y.shape[0], np.int32)
    for r in range(Y.shape[0]):
        tck = si.splrep(x, Y[r], k=k, s=s)
        ref[r], n[r] = si.splev(xe, tck, ext=3), len(tck[0])
    return ref, n
