"""tests/update_ref.py (the float64 restatement of the reference's update) against the reference's own recorded
outputs: the shifted trajectory costs of three consecutive commands of C2 (point_env push, K = 2000) and C4 (panda_env
reach, K = 4000, beta adapted after every call) from tests/golden/ref_golden_full.npz, fed through the restatement.
The weights, the adapted beta and the top-20 indices must be the reference's to float32 level, so the model the GPU
tests measure the kernels against is the reference and not only our reading of it."""
import os

import numpy as np
import pytest

from tests import update_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_golden_full.npz")


@pytest.mark.parametrize("tag,panda", [("c2", False), ("c4", True)])
def test_update_ref_reproduces_the_recorded_reference(tag, panda):
    g = np.load(GOLDEN)
    J, W, B, TI = g[f"full_{tag}_J"], g[f"full_{tag}_weights"], g[f"full_{tag}_beta"], g[f"full_{tag}_top_idx"]
    beta = 1.0                                            # mppi.py:184-187
    for call in range(J.shape[0]):
        b_used = beta
        w, eta, beta = R.exp_util(J[call], b_used, panda)
        # the reference computed in float32: ~1e-6 relative on the weights that carry the mean (|x| small), growing
        # with |x| = J / beta through the rounding of the exponent's argument; below 1e-30 its exp flushed
        big = w >= 1e-30
        x = J[call].astype(np.float64) / b_used
        np.testing.assert_allclose(W[call][big], w[big], rtol=2e-6 + 2.4e-7 * x[big].max(), err_msg=f"{tag} call {call}")
        assert np.all(np.abs(W[call][~big] - w[~big]) <= 1e-30)
        assert abs(float(B[call]) - beta) <= 1e-6 * beta, (call, B[call], beta)
        idx, vals = R.topk(w)
        assert np.array_equal(idx, TI[call]), (call, idx, TI[call])


def test_update_ref_search_and_filter_rules():
    """The search rule on a hand-made case (m3p2i.py:35-44), the flip of a grazing pass, the shift, the top-k and argmax
    tie rules and the filter (scipy's own) -- the pieces the golden pin above does not reach."""
    J = np.array([0.0, 0.3, 0.6, 0.9, 2.0], np.float32)
    r = R.update_infinite_beta(J, 1.0, 10, 3)
    # eta(beta = 1) = 2.83 < 3: one x1.2 step, then eta(1.2) = 3.05 in [3, 10]
    assert r["iters"] == 2 and r["steps"] == [1.2] and abs(r["beta"] - 1.2) < 1e-15
    assert r["beta32"] == float(np.float32(1.0) * np.float32(1.2))
    assert 3 <= r["eta"] <= 10
    f = R.update_infinite_beta(J, 1.0, 10, 3, flip_at=2)     # accepted pass 2 taken as outside: a step towards 3
    assert f["steps"] == [1.2, 1.2] and f["iters"] == 3
    a = np.arange(12, dtype=np.float32).reshape(6, 2)
    np.testing.assert_array_equal(R.shift_action(a), np.concatenate([a[1:], a[-1:]]))
    w = np.array([0.1, 0.3, 0.3, 0.2, 0.3])
    assert R.argmax_first(w) == 1
    idx, _ = R.topk(w, 4)
    assert list(idx) == [1, 2, 4, 3]
    import scipy.signal
    u = np.random.default_rng(0).standard_normal((30, 2))
    np.testing.assert_allclose(R.savgol(u), scipy.signal.savgol_filter(u, 9, 2, axis=0), rtol=0, atol=1e-15)
