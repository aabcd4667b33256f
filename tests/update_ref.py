"""The reference's update step restated in float64 (numpy, CPU only), from its formulas -- the yardstick of
tests/test_update_forms_f64_gpu.py and pinned to the reference's recorded outputs by tests/test_update_ref_golden.py.

Every function takes the float32 costs / actions as given and computes in float64.  File:line references are to the
reference package (planners/motion_planner/mppi.py, planners/motion_planner/m3p2i.py, utils/skill_utils.py).

One deliberate extra: the beta searches also return `beta32`, the same chain of x0.9 / x1.2 steps carried out as
binary32 products.  The reference multiplies a Python float; the HIP kernels carry beta in binary32.  After n steps the
two differ by at most n * 2^-24 relatively, and a weight exp(-x) moves by |x| times that, which at |x| ~ 70 and n ~ 200
is far above a float32-level bar on the weights.  So the tests evaluate the float64 formulas at `beta32` and check the
two chains against each other separately.
"""
import numpy as np

TOPK = 20                 # mppi.py:248
STEP_SIZE_COV = 0.7       # mppi.py:202
KAPPA = 0.005             # mppi.py:203
SGF_WINDOW, SGF_ORDER = 9, 2   # mppi.py:190-191


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def exp_util(J, beta, panda):
    """mppi.py:430-456 (_exp_util): weights = exp(-(J - min J) / beta) / eta; panda_env then adapts beta for the NEXT
    call (eta > 20: x0.9, eta < 10: x1.2).  Returns (weights, eta, beta_next)."""
    J = _f64(J)
    x = -(J - J.min()) / float(beta)
    e = np.exp(x)
    eta = e.sum()
    nb = float(beta)
    if panda:
        if eta > 20:
            nb = nb * 0.9
        elif eta < 10:
            nb = nb * 1.2
    return e / eta, eta, nb


def update_infinite_beta(costs, beta=1.0, eta_u_bound=10.0, eta_l_bound=3.0, flip_at=None, max_passes=5000):
    """m3p2i.py:24-44: exp(-costs / beta) until eta lies in [eta_l_bound, eta_u_bound]; beta x0.9 above, x1.2 below.
    `costs` are already shifted by their minimum (m3p2i.py:53-55).  Returns a dict: exp_, eta, beta (the beta of the
    accepted pass), beta32 (the same chain in binary32 products), iters (passes), etas (eta of every pass), steps.

    flip_at (1-based pass): reverse the decision of that one pass -- an accepted eta that grazes a bound is taken as
    outside it (step towards the nearer bound), a grazing rejected one as inside.  What a float32 search does when its
    eta lands on the other side of a bound than the float64 one; the caller checks that the graze is real."""
    c = _f64(costs)
    b, b32 = float(beta), np.float32(beta)
    etas, steps = [], []
    for it in range(1, max_passes + 1):
        e = np.exp(-c / b)
        eta = e.sum()
        etas.append(eta)
        if eta > eta_u_bound:
            step = 0.9
        elif eta < eta_l_bound:
            step = 1.2
        else:
            step = None
        if flip_at == it:
            if step is None:
                step = 0.9 if abs(eta - eta_u_bound) < abs(eta - eta_l_bound) else 1.2
            else:
                step = None
        if step is None:
            return dict(exp_=e, eta=eta, beta=b, beta32=float(b32), iters=it, etas=etas, steps=steps)
        b = b * step
        b32 = np.float32(b32 * np.float32(step))
        steps.append(step)
    raise AssertionError("beta search did not converge")


def multi_modal_exp_util(J, half, flips=(None, None, None)):
    """m3p2i.py:46-64 (_multi_modal_exp_util): three independent searches, each from beta = 1 (self.beta, beta_1 and
    beta_2 are never written back), over all costs, the first half_K and the rest.  Returns [all, mode 1, mode 2] as
    the dicts of update_infinite_beta, each with its normalised weights under "w"."""
    J = _f64(J)
    out = []
    for JJ, fl in ((J, flips[0]), (J[:half], flips[1]), (J[half:], flips[2])):
        r = update_infinite_beta(JJ - JJ.min(), 1.0, 10, 3, flip_at=fl)
        r["w"] = r["exp_"] / r["eta"]
        out.append(r)
    return out


def weights_at(J, beta):
    """exp(-(J - min J) / beta) / eta at a given beta, and eta (mppi.py:437-443, m3p2i.py:32-33 + 62-64)."""
    J = _f64(J)
    e = np.exp(-(J - J.min()) / float(beta))
    return e / e.sum(), e.sum()


def shift_action(a):
    """mppi.py:266-273 (_shift_action): roll one step towards the front, the last row kept."""
    a = _f64(a)
    return np.concatenate([a[1:], a[-1:]], axis=0)


def argmax_first(w):
    """torch.argmax (mppi.py:494, m3p2i.py:73-74): the first index of the maximum."""
    return int(np.argmax(np.asarray(w)))


def topk(w, k=TOPK):
    """torch.topk(weights, 20) (mppi.py:248): the k largest weights in descending order, ties by ascending index."""
    w = np.asarray(w)
    idx = np.argsort(-w, kind="stable")[:k]
    return idx, w[idx]


def savgol(u):
    """mppi.py:257-263: scipy.signal.savgol_filter(u, 9, 2, deriv=0, delta=1.0, axis=0, mode='interp', cval=0.0)."""
    import scipy.signal
    return scipy.signal.savgol_filter(_f64(u), SGF_WINDOW, SGF_ORDER, deriv=0, delta=1.0, axis=0, mode="interp", cval=0.0)


def update_distribution(w, actions, mean_shifted, step_size_mean, cov=None):
    """mppi.py:485-516 (_update_distribution) after _exp_util: best row, new mean and (update_cov) the diagonal
    covariance step.  actions: [K, T, nu]; mean_shifted: the mean after _shift_action (mppi.py:236).
    Returns dict(best_idx, best, mean, cov, scale_tril)."""
    A = _f64(actions)
    w = _f64(w)
    bi = argmax_first(w)
    new_mean = np.einsum("k,ktj->tj", w, A)
    mean = (1.0 - step_size_mean) * _f64(mean_shifted) + step_size_mean * new_mean
    out = dict(best_idx=bi, best=A[bi], mean=mean)
    if cov is not None:
        delta = A - mean[None]
        cov_update = np.einsum("k,ktj->tj", w, delta ** 2).mean(axis=0)
        c = (1.0 - STEP_SIZE_COV) * _f64(cov) + STEP_SIZE_COV * cov_update + KAPPA
        out["cov"], out["scale_tril"] = c, np.sqrt(c)
    return out


def update_multi_modal_distribution(r, actions, mean_shifted, step_size_mean, half):
    """m3p2i.py:66-87 (_update_multi_modal_distribution), r = multi_modal_exp_util(...): per-mode best rows (argmax of
    each mode's weights), per-mode means (plain weighted sums), the blended mean of all samples."""
    A = _f64(actions)
    w, w1, w2 = r[0]["w"], r[1]["w"], r[2]["w"]
    b1, b2 = argmax_first(w1), argmax_first(w2)
    return dict(best_idx_1=b1, best_idx_2=half + b2, best_1=A[b1], best_2=A[half + b2],
                mean_1=np.einsum("k,ktj->tj", w1, A[:half]), mean_2=np.einsum("k,ktj->tj", w2, A[half:]),
                mean=(1.0 - step_size_mean) * _f64(mean_shifted) + step_size_mean * np.einsum("k,ktj->tj", w, A))


def simple_update(J, noise, U, lambda_):
    """mppi.py:220-233 (mppi_mode 'simple'): U rolled (torch.roll, wrapping), weights
    exp(-(J - min J) / lambda_) / eta (skill_utils.py:3-4 with beta = min J, factor = 1 / lambda_),
    U += sum_k w_k noise_k.  noise: [K, T, nu]; U: [T, nu] before the roll.  Returns dict(w, eta, U)."""
    Ur = np.roll(_f64(U), -1, axis=0)
    w, eta = weights_at(J, lambda_)
    return dict(w=w, eta=eta, U=Ur + np.einsum("k,ktj->tj", w, _f64(noise)))


def pull_preference(w, half):
    """m3p2i.py:16-21: int(sum of the second half's weights > sum of the first half's)."""
    w = _f64(w)
    return int(w[half:].sum() > w[:half].sum())
