"""float64 reference of the wavefront order of the point_env samples (numpy only).

Written from the definition in the comment of sampler.hip ("wavefront order of the samples") and from order_block
(m3_api.hip), not from the kernels:

  key(sample) = sum_t cumsum_t(s * delta) projected on (cos th, sin th)
  th          = 0.5 atan2(2 cxy, cxx - cyy): the principal axis of the positions of box, dyn-obs and obstacle
  s_j         = float32(sqrt(sigma_j)), the scale the host passes
  order       = stable sort by key inside each mode's part of the block; relabelling swaps the samples with a role of
                their own (0, K_global / 2, K_global - 1) back to their own slots

The device forms the key in float32, so two samples whose keys are closer than its rounding may trade places -- nothing
else may move.  `tol` bounds that rounding from the operation count and the magnitudes; it is derived, not tuned.
"""
import numpy as np


def principal_axis(box_xy, dyn_xy, obs_xy, dtype=np.float64):
    """th of the principal axis of the three positions, in `dtype` arithmetic"""
    f = dtype
    x = np.array([box_xy[0], dyn_xy[0], obs_xy[0]], f)
    y = np.array([box_xy[1], dyn_xy[1], obs_xy[1]], f)
    third = f(1.0) / f(3.0)
    mx, my = f(x.sum(dtype=f) * third), f(y.sum(dtype=f) * third)
    cxx = ((x - mx) * (x - mx)).sum(dtype=f)
    cyy = ((y - my) * (y - my)).sum(dtype=f)
    cxy = ((x - mx) * (y - my)).sum(dtype=f)
    return f(0.5) * np.arctan2(f(2.0) * cxy, cxx - cyy, dtype=f)


def _keys(delta, sigma_diag, box_xy, dyn_xy, obs_xy, f):
    d = np.asarray(delta, np.float32).astype(f)                                # [K, T, 2]
    assert d.ndim == 3 and d.shape[2] == 2, d.shape
    s = np.sqrt(np.asarray(sigma_diag, np.float32)[:2]).astype(np.float32).astype(f)   # sqrtf, as the host passes it
    th = principal_axis(box_xy, dyn_xy, obs_xy, f)
    ex, ey = np.cos(th, dtype=f), np.sin(th, dtype=f)
    scaled = (d * s).astype(f)
    c = np.zeros(d.shape[::2], f)                                              # [K, 2]: cumsum_t(s * delta)
    S = np.zeros(d.shape[::2], f)                                              # [K, 2]: its running sum over t
    M = 0.0
    for t in range(d.shape[1]):                                                # (in the order of the definition, so that
        c = (c + scaled[:, t]).astype(f)                                       # the float32 twin rounds where float32 does)
        S = (S + c).astype(f)
        M = max(M, float(np.abs(scaled[:, t]).max()), float(np.abs(c).max()), float(np.abs(S).max()))
    px, py = (S[:, 0] * ex).astype(f), (S[:, 1] * ey).astype(f)
    key = (px + py).astype(f)
    M = max(M, float(np.abs(px).max()), float(np.abs(py).max()), float(np.abs(key).max()))
    return key, M


def keys64(delta, sigma_diag, box_xy, dyn_xy, obs_xy):
    """(key[K] in float64, M = the largest magnitude any partial sum reaches)"""
    return _keys(delta, sigma_diag, box_xy, dyn_xy, obs_xy, np.float64)


def keys32(delta, sigma_diag, box_xy, dyn_xy, obs_xy):
    """The float32 twin of keys64: the same definition with every operation rounded to float32."""
    return _keys(delta, sigma_diag, box_xy, dyn_xy, obs_xy, np.float32)[0]


def tol(T, M):
    """Each of about 3T + 8 float32 operations (T scalings, 2T additions, the axis and the projection) rounds by at most
    2^-24 relative to a magnitude of at most 2M."""
    return 2.0 * (3 * T + 8) * 2.0 ** -24 * M


def half_local(K_global, k_offset, K_local, multi_modal):
    """first local index of the second mode inside the block, as order_block forms it"""
    h = K_global // 2 - k_offset
    if not multi_modal or h > K_local:
        h = K_local
    return max(h, 0)


def specials(K_global, k_offset, K_local):
    """local indices of the samples with a role of their own that fall inside the block, in the order they are fixed"""
    return [s - k_offset for s in (0, K_global // 2, K_global - 1) if 0 <= s - k_offset < K_local]


def expected_perm(keys, K_global, k_offset, K_local, multi_modal, relabel):
    """p[slot] = local index of the sample placed there"""
    keys = np.asarray(keys)
    assert keys.shape == (K_local,)
    h = half_local(K_global, k_offset, K_local, multi_modal)
    p = np.concatenate([np.argsort(keys[:h], kind="stable"), h + np.argsort(keys[h:], kind="stable")]).astype(np.int64)
    if relabel:
        for s in specials(K_global, k_offset, K_local):
            pos = int(np.nonzero(p == s)[0][0])     # the special's sorted position takes the displaced element
            p[pos], p[s] = p[s], s
    return p


def compare(p, keys, K_global, k_offset, K_local, multi_modal, relabel, bound):
    """The comparison of a device permutation with the reference.  Returns the largest position-wise key difference
    (for the record); raises AssertionError with the figures when a property does not hold."""
    p = np.asarray(p).astype(np.int64)
    keys = np.asarray(keys, np.float64)
    assert p.shape == (K_local,), p.shape
    assert np.array_equal(np.sort(p), np.arange(K_local)), "not a permutation of the block's samples"
    if relabel:
        for s in specials(K_global, k_offset, K_local):
            assert p[s] == s, f"special sample {s + k_offset} (local {s}) sits at slot {int(np.nonzero(p == s)[0][0])}"
    h = half_local(K_global, k_offset, K_local, multi_modal)
    assert (p[:h] < h).all() and (p[h:] >= h).all(), "a sample left its mode's half"
    ref = expected_perm(keys, K_global, k_offset, K_local, multi_modal, relabel)
    diff = np.abs(keys[p] - keys[ref])
    worst = float(diff.max())
    bad = int((diff > bound).sum())
    assert bad == 0, (f"{bad} of {K_local} slots hold a sample whose key differs from the reference's by more than {bound:.3g} "
                      f"(largest difference {worst:.6g} at slot {int(diff.argmax())})")
    return worst
