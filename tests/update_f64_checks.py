"""What tests/test_update_forms_f64_gpu.py and tests/test_sharded_update_f64_gpu.py share: the synthetic cost
distributions, the float32 error bound on the weights, the beta search with its grazing rule, and the comparison of
one update call's outputs with the float64 restatement of the reference (tests/update_ref.py).  The bounds are derived
in the docstring of tests/test_update_forms_f64_gpu.py; `extra` is what a sharded protocol's mixture adds to them
(derived in tests/test_sharded_update_f64_gpu.py).  No test lives here."""
import numpy as np

from tests import update_ref as R

U32 = 2.0 ** -24

_SG_GAIN = []


def sg_gain():
    if not _SG_GAIN:
        import scipy.signal
        _SG_GAIN.append(max(np.abs(np.array([scipy.signal.savgol_coeffs(9, 2, pos=p, use="dot") for p in range(9)])).sum(1)))
    return _SG_GAIN[0]


def stage_a_layout(K):
    """Costs that overflow top-k stage A's candidate list (TK_CAP = 1024) in every 4096-cost workgroup, all distinct:
    local index i = e * 256 + tid (tid = 64 * wave + lane, e < 16 register rows) holds lane * 1e-3 + e * 1e-5 +
    wave * 1e-6 (+ 0.1 per workgroup).  Each wave's threshold is its lanes' 20th smallest minimum, lane 19's
    row 0; every cost of lanes 0..18 lies below it: 19 * 16 * 4 > 1024 survivors."""
    i = np.arange(K)
    blk, loc = i // 4096, i % 4096
    e, tid = loc // 256, loc % 256
    return (0.1 * blk + (tid % 64) * 1e-3 + e * 1e-5 + (tid // 64) * 1e-6).astype(np.float32)


def stage_a_survivors(J):
    """What the kernel's stage A keeps of the first workgroup (update_common.hpp: topk_stage_a), counted on the host."""
    blk = np.full(4096, np.inf, np.float32)
    blk[:min(4096, len(J))] = J[:4096]
    rv = blk.reshape(16, 4, 64)                  # [row e][wave][lane]
    lane_min = rv.min(axis=0)                    # [wave][lane]
    tau = np.sort(lane_min, axis=1)[:, 19].min()
    return int((blk <= tau).sum())


def make_costs(dist, K, rng, call=0):
    a = np.abs(rng.standard_normal(K))
    if dist == "s1":
        return a.astype(np.float32)
    if dist in ("s1e-5", "s1e8"):
        return (float("1" + dist[2:]) * a).astype(np.float32)
    if dist == "cycle":   # Panda: eta > 20 and < 10 in turn, so the beta step goes both ways
        return ((1.0, 1e3, 0.03)[call % 3] * a).astype(np.float32)
    if dist == "offset":
        return (1e6 + rng.uniform(0, 1, K)).astype(np.float32)
    if dist == "neg":
        return (-50.0 - 3.0 * rng.standard_normal(K)).astype(np.float32)
    J = a.astype(np.float32) + np.float32(0.5)
    if dist == "dupmin":   # the minimum twice, on both sides of a 4096-sample workgroup boundary (of each half)
        for p in ((4095, 4096) if K > 4096 else (K // 3, K - 2)):
            J[p] = -1.0
        if K // 2 + 4097 < K:
            J[K // 2 + 4095] = J[K // 2 + 4096] = -1.0
        return J
    if dist == "tie":      # distinct costs whose float32 weights are equal: the first index of the max wins (3 and
        h = K // 2         # 3 + 256 share a thread in every form, 9 is another thread's)
        for base in (0, h):
            J[base + 3], J[base + (259 if h > 300 else 5)], J[base + 9] = 3e-9, 1e-9, 0.0
        return J
    if dist == "zeros":    # -0.0 and +0.0 (equal costs, ordered by index), three per half
        h = K // 2
        for base in (0, h):
            J[base + 2], J[base + 7], J[base + min(h - 1, 20)] = 0.0, -0.0, 0.0
        J[1] = -0.0
        return J
    if dist == "inf":
        J[rng.choice(K, 5, replace=False)] = np.inf
        return J
    if dist == "inf24":    # more than 4 of 24 at +inf: the top-20 holds +inf rows
        J[[1, 4, 9, 13, 17, 22]] = np.inf
        return J
    if dist == "stageA":
        J = stage_a_layout(K)
        assert stage_a_survivors(J) > 1024
        return J
    if dist == "stageB":   # every workgroup: 19 copies of F and 40 of C > F at its 20th place; the lists' first elements
        # are all F, so > 1024 of the 64 x 20 candidates pass stage B's bounds
        J = (10.0 + a).astype(np.float32)
        for b in range(K // 4096):
            pos = b * 4096 + rng.choice(4096, 59, replace=False)
            J[pos[:19]] = 1.0
            J[pos[19:]] = 2.0
        return J
    raise ValueError(dist)


def check_weights(w, J, beta, what, extra=0.0, only=None):
    """w (kernel, float32) against the float64 weights at `beta` with the bound of the module docstring
    (+ `extra`, relative: a sharded protocol's mixture).  only: w holds the weights of these indices of J."""
    w_ref, eta_ref = R.weights_at(J, beta)
    J64 = J.astype(np.float64)
    with np.errstate(invalid="ignore"):
        x = np.abs(J64 - J64.min()) / beta
    if only is not None:
        w_ref, x = w_ref[only], x[only]
    big = w_ref >= 1e-30
    err = np.abs(w.astype(np.float64) - w_ref)
    with np.errstate(invalid="ignore"):
        bad = big & ~(err <= (2e-5 + extra + 4 * U32 * np.where(big, x, 0.0)) * w_ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} weights off, first at {np.flatnonzero(bad)[:5]}: " \
                          f"{w[bad][:3]} vs {w_ref[bad][:3]}"
    assert np.all(err[~big] <= 1e-30), f"{what}: tiny weights off by {err[~big].max()}"
    return w_ref, eta_ref


def search_like_kernel(JJ, iters, what):
    """The float64 search of m3p2i.py:24-44; if the kernel made a different number of passes, the deciding pass must
    graze 3 or 10 and the reference is re-run with that decision reversed."""
    r = R.update_infinite_beta(JJ - JJ.astype(np.float64).min(), 1.0, 10, 3)
    if r["iters"] != iters:
        p = min(r["iters"], iters)
        eta_p = r["etas"][p - 1]
        assert min(abs(eta_p - 3.0) / 3.0, abs(eta_p - 10.0) / 10.0) <= 1e-5, \
            f"{what}: {iters} passes, reference {r['iters']}, eta at pass {p} = {eta_p!r}"
        r = R.update_infinite_beta(JJ - JJ.astype(np.float64).min(), 1.0, 10, 3, flip_at=p)
        assert r["iters"] == iters, (what, iters, r["iters"])
    assert abs(r["beta32"] - r["beta"]) <= r["iters"] * U32 * r["beta"] * 1.01
    return r


def new_state(mean, cov_diag):
    """What carries over from call to call on the reference's side."""
    return dict(mean_ref=np.asarray(mean, np.float64), beta64=1.0, beta32=np.float32(1.0), cov_ref=np.asarray(cov_diag, np.float64))


def check_call(L, get, info, J, A, S, st, *, K, nu, mode, cov, lambda_, ss, call, weights=None, extra=0.0, best_of=None):
    """One update call's outputs against the float64 reference on the whole J [K], A [T, K, nu], S [T, K, 4].
    get(buf) -> numpy array of a buffer; `weights`: (w, w1, w2) where they do not come from get() as they are (a
    sharded rank that materialises a slice: assembled by the caller).  st: new_state(), advanced here.
    best_of(w) -> index: the argmax rule where it is not "first index of the maximum of the returned weights" (the
    mixture of local softmins, whose returned weights are products rounded per rank)."""
    panda = nu == 9
    half = K // 2
    Akt = A.transpose(1, 0, 2)                         # [K, T, nu] (reference layout)
    tag = f"call {call}"
    w = get(L.BUF_WEIGHTS) if weights is None else weights[0]
    out = {b: get(b) for b in (L.BUF_MEAN, L.BUF_ACTION_OUT, L.BUF_TOP_IDX, L.BUF_TOP_TRAJS, L.BUF_BEST, L.BUF_COV)}
    # ---- weights, eta, beta, iters ----
    if mode == "multi":
        r = [search_like_kernel(J, info.iters, tag + " all"),
             search_like_kernel(J[:half], info.iters_1, tag + " mode 1"),
             search_like_kernel(J[half:], info.iters_2, tag + " mode 2")]
        assert np.float32(info.beta_1) == np.float32(r[1]["beta32"]) and \
            np.float32(info.beta_2) == np.float32(r[2]["beta32"]), (info.beta_1, info.beta_2, r[1]["beta32"], r[2]["beta32"])
        w1, w2 = (get(L.BUF_WEIGHTS_1), get(L.BUF_WEIGHTS_2)) if weights is None else weights[1:]
        wr, er = check_weights(w, J, r[0]["beta32"], tag + " weights", extra)
        w1r, e1r = check_weights(w1, J[:half], r[1]["beta32"], tag + " weights_1", extra)
        w2r, e2r = check_weights(w2, J[half:], r[2]["beta32"], tag + " weights_2", extra)
        for got, want in ((info.eta, er), (info.eta_1, e1r), (info.eta_2, e2r)):
            assert abs(got - want) <= (2e-5 + extra) * want, (tag, got, want)
        assert np.float32(info.beta) == np.float32(1.0)          # the persistent beta is never written
    else:
        b_used = (float(lambda_) if mode == "simple" else float(st["beta32"]))
        st["beta_used"] = b_used
        wr, er = check_weights(w, J, b_used, tag + " weights", extra)
        assert abs(info.eta - er) <= (2e-5 + extra) * er, (tag, info.eta, er)
        if mode == "single":
            # mppi.py:446-454: panda_env adapts beta after use; point_env keeps it
            _, eta64, nb64 = R.exp_util(J, st["beta64"], panda)
            step = nb64 / st["beta64"]
            if panda and (abs(eta64 - 20) <= 2e-5 * 20 or abs(eta64 - 10) <= 2e-5 * 10):
                step = info.beta / float(st["beta32"])               # a grazing eta: either side is right
            st["beta64"] *= step
            st["beta32"] = np.float32(st["beta32"] * np.float32(step)) if step != 1.0 else st["beta32"]
            assert np.float32(info.beta) == st["beta32"], (tag, info.beta, st["beta32"])
            assert abs(st["beta64"] - float(st["beta32"])) <= (call + 1) * 2 * U32 * st["beta64"]
    # ---- argmax (first index of the max of the returned weights), best rows ----
    bi = R.argmax_first(w) if best_of is None else best_of(wr)
    assert info.best_idx == bi, (tag, info.best_idx, bi)
    assert wr[bi] >= wr.max() * (1 - 1e-6)
    if mode == "multi":
        b1, b2 = R.argmax_first(w1), half + R.argmax_first(w2)
        assert (info.best_idx_1, info.best_idx_2) == (b1, b2), (tag, info.best_idx_1, info.best_idx_2, b1, b2)
        assert w1r[b1] >= w1r.max() * (1 - 1e-6) and w2r[b2 - half] >= w2r.max() * (1 - 1e-6)
        assert np.array_equal(get(L.BUF_BEST_1), A[:, b1])
        assert np.array_equal(get(L.BUF_BEST_2), A[:, b2])
    elif mode == "single":
        assert np.array_equal(out[L.BUF_BEST], A[:, bi])
    # ---- sums of the halves, pull preference (m3p2i.py:16-21) ----
    hp, hq = wr[:half].sum(), wr[half:].sum()
    assert abs(info.wsum_push - hp) <= 2e-5 + extra and abs(info.wsum_pull - hq) <= 2e-5 + extra, \
        (tag, info.wsum_push, hp, info.wsum_pull, hq)
    assert info.pull_preference == int(info.wsum_pull > info.wsum_push)
    if abs(hq - hp) > 1e-4:
        assert info.pull_preference == R.pull_preference(wr, half)
    # ---- top-k: the 20 largest reference weights, and the project's rule (ascending J, ties by index,
    # -0.0 == +0.0, as torch.argsort(J, stable=True)) ----
    ti = out[L.BUF_TOP_IDX].astype(np.int64)
    assert np.all((ti >= 0) & (ti < K)), ti
    _, vals = R.topk(wr)
    np.testing.assert_allclose(wr[ti], vals, rtol=1e-12, atol=0, err_msg=tag + " top-k weights")
    assert np.all(np.diff(wr[ti]) <= 0)
    want_ti = np.argsort(J, kind="stable")[:R.TOPK]
    assert np.array_equal(ti, want_ti), (tag, ti, want_ti)
    np.testing.assert_array_equal(out[L.BUF_TOP_TRAJS], S[:, ti][:, :, [0, 2]].transpose(1, 0, 2))
    # ---- means, filtered plan, covariance ----
    scale = float(np.abs(A).max())
    mtol = (1e-5 + extra) * scale
    mean_ref = st["mean_ref"]
    if mode == "simple":
        noise = Akt.astype(np.float64) - np.roll(mean_ref, -1, axis=0)[None]
        s = R.simple_update(J, noise, mean_ref, float(lambda_))
        mean_ref = s["U"]
    elif mode == "multi":
        m = R.update_multi_modal_distribution([dict(w=wr), dict(w=w1r), dict(w=w2r)], Akt, R.shift_action(mean_ref), ss, half)
        np.testing.assert_allclose(get(L.BUF_MEAN_1), m["mean_1"], rtol=0, atol=mtol, err_msg=tag)
        np.testing.assert_allclose(get(L.BUF_MEAN_2), m["mean_2"], rtol=0, atol=mtol, err_msg=tag)
        mean_ref = m["mean"]
    else:
        m = R.update_distribution(wr, Akt, R.shift_action(mean_ref), ss, st["cov_ref"] if cov else None)
        mean_ref = m["mean"]
        if cov:
            st["cov_ref"] = m["cov"]
            c = out[L.BUF_COV]
            np.testing.assert_allclose(c[0], m["cov"], rtol=0, atol=1e-5 * m["cov"].max(), err_msg=tag + " cov")
            np.testing.assert_allclose(c[1], m["scale_tril"], rtol=0, atol=1e-5 * m["scale_tril"].max(), err_msg=tag + " scale_tril")
    st["mean_ref"] = mean_ref
    np.testing.assert_allclose(out[L.BUF_MEAN], mean_ref, rtol=0, atol=mtol, err_msg=tag + " mean")
    np.testing.assert_allclose(out[L.BUF_ACTION_OUT], R.savgol(mean_ref), rtol=0, atol=sg_gain() * mtol,
                               err_msg=tag + " action_out")
    return wr
