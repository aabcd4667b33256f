"""Reference of the in-kernel noise stream (m3p2i_aip_amd/csrc/noise_stream.hpp), written from the spec
in plain numpy and independent of oracle/ (a helper of tests/test_noise_stream_{cpu,gpu}.py, not a test).

The stream, per (seed, call, k, t, pair):

    x   = seed ^ (0xD1B54A32D192ED03 * (call + 1 mod 2^32))  ^  (k << 32 | t << 8 | pair)        (uint64)
    a, b = splitmix64(x), splitmix64(x)                         s = (lo a, hi a, lo b, hi b)      (uint32 x 4)
    r0, r1 = xoshiro128++(s), xoshiro128++(s)
    u0  = ((r0 >> 8) + 1) / 2^24  in (0, 1],     u1 = (r1 >> 8) / 2^24  in [0, 1)                 (exact in f32 and f64)
    z0, z1 = sqrt(-2 ln u0) * (cos, sin)(2 pi u1)              component j of a sample uses pair j // 2, member j % 2
    d_j = mu_j + sum_{q <= j} L[j][q] z_q

The integer part is exact uint64 / uint32 arithmetic; everything after the uniforms is binary64 here.

L as the library stores it (m3_create, m3_api.hip): the configuration holds noise_sigma as binary32.  With off-diagonal
entries (`full_sigma`) the Cholesky factor is formed in binary64 FROM THOSE binary32 entries and each entry of L is rounded
to binary32 once, when it is copied into the device matrix (`mats[i] = (float)chol[i]`).  For a diagonal sigma L is the
diagonal `scale_tril` = sqrtf(noise_sigma_diag[j]): a binary32 square root of the binary32 variance (m3_sample_noise and
the rollouts form it the same way), which is also what rounding the binary64 root once gives (sqrt is correctly rounded and
binary64 carries more than 2 * 24 + 2 bits).  mu is binary32.

Error bound (ISSUE / DESIGN section 5, derived, not tuned).  eps = 2^-24 is binary32's unit roundoff; logf within p ulp,
cosf / sinf within q ulp (1 ulp <= 2 eps relative):
    rad = sqrtf(-2 logf(u0))      relative error <= (p + 1) eps          (the root halves logf's 2 p eps and rounds once)
    ang = fl(2pi_f32 * u1)        absolute error <= 2 pi * 1.5 eps       (2pi_f32 is 0.47 eps off, the product rounds once)
                                  which moves cos / sin by at most 9.42 eps ABSOLUTE
    cosf / sinf                   2 q eps absolute (|cos| <= 1)
    rad * cosf(ang)               one more rounding, eps
    => |z - z_ref| <= rad_ref * eps * (p + 2 q + 11.4)  +  one binary32 ulp of z_ref
The first two sources scale rad by |cos| resp. |sin| -- different factors -- so the bound is in units of rad, not of z: a
`k * ulp(z)` bound is wrong next to a zero crossing of cos or sin.
    d_j: with e_q the bound of z_q and A_j = |mu_j| + sum_q |L_jq| (|z_q| + e_q): the roundings of all products together are
    <= eps * A_j, each of the j additions and the addition of mu is <= eps * A_j:
    |d_j - d_ref_j| <= sum_q |L_jq| e_q + (j + 2) * eps * A_j        (diagonal sigma: one product, one addition: 2 eps A_j)
"""
import numpy as np

EPS = 2.0 ** -24
CALL_MULT = np.uint64(0xD1B54A32D192ED03)
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
Z_MAX = float(np.sqrt(2.0 * 24.0 * np.log(2.0)))    # u0 >= 2^-24: |z| <= sqrt(-2 ln 2^-24) = 5.768...

# the distributions of the reference traces opt_navr and panda_opt_rand (tests/golden/make_golden.py), one definition for the
# CPU test, the GPU test and tests/noise_stream_runs.py
NAVR_MU, NAVR_SIG = [0.3, -0.2], [[3.0, 1.0], [1.0, 2.0]]
PANDA_SIG = [[0.0] * 9 for _ in range(9)]
for _i in range(7):
    PANDA_SIG[_i][_i] = 10.0
PANDA_SIG[7][7] = PANDA_SIG[8][8] = 0.8
PANDA_SIG[0][1] = PANDA_SIG[1][0] = 4.0
PANDA_SIG[2][5] = PANDA_SIG[5][2] = -3.0
PANDA_MU = [0.2, -0.1, 0.0, 0.1, 0.0, 0.0, -0.2, 0.0, 0.0]
PANDA_DIAG = [10.0] * 7 + [0.8] * 2


def _u64(a):
    return np.asarray(a, dtype=np.uint64)


def call_constant(call):
    """0xD1B54A32D192ED03 * (call + 1), the call + 1 formed in 32 bits (call = 2^32 - 1 wraps to 0), the product in 64."""
    c1 = (_u64(call) + np.uint64(1)) & np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        return CALL_MULT * c1


def key(seed, call, k, t, pair):
    """The 64-bit key of (seed, call, k, t, pair); arguments broadcast.  k, t, pair are the kernel's 32-bit unsigned values:
    t and pair are OR-ed in unmasked (t << 8 reaches bit 39 only for t >= 2^24, which no handle has)."""
    ctr = (_u64(k) << np.uint64(32)) | (_u64(t) << np.uint64(8)) | _u64(pair)
    return (_u64(seed) ^ call_constant(call)) ^ ctr


def _splitmix64(x):
    """One splitmix64 step on the state array x (in place); returns the output."""
    with np.errstate(over="ignore"):
        x += _GOLDEN
        z = x.copy()
        z ^= z >> np.uint64(30)
        z *= _M1
        z ^= z >> np.uint64(27)
        z *= _M2
        z ^= z >> np.uint64(31)
    return z


def _rotl32(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def _xoshiro128pp(s):
    """One xoshiro128++ step on the list s of four uint32 arrays (updated in place); returns the output."""
    with np.errstate(over="ignore"):
        result = _rotl32(s[0] + s[3], 7) + s[0]
    t = s[1] << np.uint32(9)
    s[2] ^= s[0]
    s[3] ^= s[1]
    s[1] ^= s[2]
    s[0] ^= s[3]
    s[2] ^= t
    s[3] = _rotl32(s[3], 11)
    return result


def raw_from_key(x):
    """(r0, r1), uint32, of the keys x (uint64; not modified)."""
    x = np.array(x, dtype=np.uint64, copy=True, ndmin=1)
    a = _splitmix64(x)
    b = _splitmix64(x)
    lo = np.uint64(0xFFFFFFFF)
    s = [(a & lo).astype(np.uint32), (a >> np.uint64(32)).astype(np.uint32),
         (b & lo).astype(np.uint32), (b >> np.uint64(32)).astype(np.uint32)]
    r0 = _xoshiro128pp(s)
    r1 = _xoshiro128pp(s)
    return r0, r1


def raw(seed, call, k, t, pair):
    x = key(seed, call, k, t, pair)
    r0, r1 = raw_from_key(x)
    return r0.reshape(np.shape(x)), r1.reshape(np.shape(x))


def uniform_ints(r0, r1):
    """(n0, n1) with u0 = n0 / 2^24 in (0, 1], u1 = n1 / 2^24 in [0, 1): int64."""
    return (r0 >> np.uint32(8)).astype(np.int64) + 1, (r1 >> np.uint32(8)).astype(np.int64)


def uniforms(r0, r1):
    n0, n1 = uniform_ints(r0, r1)
    return n0 * EPS, n1 * EPS            # exact: 24-bit integers times a power of two


def gauss_from_raw(r0, r1):
    """binary64 Box-Muller: (z0, z1, rad)."""
    u0, u1 = uniforms(r0, r1)
    rad = np.sqrt(-2.0 * np.log(u0))
    ang = (2.0 * np.pi) * u1
    return rad * np.cos(ang), rad * np.sin(ang), rad


def gauss(seed, call, k, t, pair):
    r0, r1 = raw(seed, call, k, t, pair)
    return gauss_from_raw(r0, r1)


def z_bound(z_ref, rad_ref, p, q):
    """|z - z_ref| for a binary32 evaluation with logf within p ulp, cosf / sinf within q ulp (module docstring)."""
    ulp = np.spacing(np.abs(z_ref).astype(np.float32)).astype(np.float64)
    return rad_ref * EPS * (p + 2.0 * q + 11.4) + ulp


def factor(nu, sigma=None, sigma_diag=None):
    """L [nu][nu] as m3_create stores it (module docstring), returned as binary64 values of binary32 numbers, and whether
    it is the full (off-diagonal) form."""
    if sigma is not None:
        s32 = np.asarray(sigma, dtype=np.float32).reshape(nu, nu)
        full = bool(np.any(s32[~np.eye(nu, dtype=bool)] != 0.0))
        if full:
            L = np.linalg.cholesky(s32.astype(np.float64))
            return L.astype(np.float32).astype(np.float64), True
        sigma_diag = np.diag(s32)
    d32 = np.asarray(sigma_diag, dtype=np.float32)
    return np.diag(np.sqrt(d32).astype(np.float32).astype(np.float64)), False


def standard_normals(seed, call, K, T, nu, k0=0):
    """z [T][K][nu'] with nu' = 2 * ceil(nu / 2) (the unused member of an odd nu's last pair included) and rad of the same
    shape: binary64."""
    npair = (nu + 1) // 2
    k = (k0 + np.arange(K, dtype=np.uint64))[None, :, None]
    t = np.arange(T, dtype=np.uint64)[:, None, None]
    p = np.arange(npair, dtype=np.uint64)[None, None, :]
    z0, z1, rad = gauss(seed, call, k, t, p)
    z = np.stack([z0, z1], axis=-1).reshape(T, K, 2 * npair)
    r = np.stack([rad, rad], axis=-1).reshape(T, K, 2 * npair)
    return z, r


def table(seed, call, K, T, nu, mu=None, sigma=None, sigma_diag=None, k0=0, p=2, q=2):
    """The table m3_sample_noise writes, [T][K][nu] for global samples k0 .. k0 + K - 1: (d_ref, bound, rad_ref), binary64.
    `bound` is the per-element error bound of the module docstring for a binary32 evaluation with p, q ulp functions;
    rad_ref [T][K][nu] is the Box-Muller radius of the pair each component's own z comes from."""
    L, full = factor(nu, sigma, sigma_diag)
    mu = np.zeros(nu) if mu is None else np.asarray(mu, dtype=np.float32).astype(np.float64)
    z, rad = standard_normals(seed, call, K, T, nu, k0)
    z, rad = z[..., :nu], rad[..., :nu]
    e = z_bound(z, rad, p, q)
    d = mu + z @ L.T
    aL = np.abs(L)
    A = np.abs(mu) + (np.abs(z) + e) @ aL.T
    rnd = (np.arange(nu) + 2.0) if full else np.full(nu, 2.0)
    bound = e @ aL.T + rnd * EPS * A
    return d, bound, rad


class Extremes:
    """The named edge cases of a nu = 2 table (pair 0), from the integer reference alone, fed block by block: the n
    smallest u0, every u0 = 1, the n largest u1, and the u1 nearest 1/4, 1/2 and 3/4 -- each a list of (call, k, t), ordered
    by value, ties by (call, k, t)."""
    TARGETS = (("u1_quarter", 1 << 22), ("u1_half", 1 << 23), ("u1_three_quarters", 3 << 22))

    def __init__(self, n=64):
        self.n = n
        self.cand = {"u0_small": [], "u0_one": [], "u1_large": [], **{tag: [] for tag, _ in self.TARGETS}}
        self.min_n0 = 1 << 24

    def _keep(self, tag, score, n, call, k0, T):
        """score [T][K'] (smaller = more extreme): the n smallest of this block join the candidates."""
        flat = score.reshape(-1)
        idx = np.argpartition(flat, n)[:n] if n < flat.size else np.arange(flat.size)
        idx = np.flatnonzero(flat <= flat[idx].max())
        t, i = np.unravel_index(idx, score.shape)
        self.cand[tag] += [(int(s), call, k0 + int(ii), int(tt)) for s, ii, tt in zip(flat[idx], i, t)]
        self.cand[tag] = sorted(self.cand[tag])[:n]

    def add(self, call, k0, n0, n1):
        """n0, n1 [T][K'] (uniform_ints) of samples k0 .. k0 + K' - 1 of one call."""
        T = n0.shape[0]
        self.min_n0 = min(self.min_n0, int(n0.min()))
        self._keep("u0_small", n0, self.n, call, k0, T)
        self._keep("u1_large", -n1, self.n, call, k0, T)
        for tag, target in self.TARGETS:
            self._keep(tag, np.abs(n1 - target), 1, call, k0, T)
        t, i = np.nonzero(n0 == 1 << 24)
        self.cand["u0_one"] += [(0, call, k0 + int(ii), int(tt)) for ii, tt in zip(i, t)]

    def result(self):
        out = {}
        for tag, c in self.cand.items():
            c = sorted(c)
            if tag in ("u0_small", "u1_large"):
                c = c[:self.n]
            elif tag != "u0_one":
                c = c[:1]
            out[tag] = [x[1:] for x in c]
        return out


def extremes(seed, calls, K, T, n=64, block=32768):
    ex = Extremes(n)
    t = np.arange(T, dtype=np.uint64)[:, None]
    for c in calls:
        for k0 in range(0, K, block):
            k = np.arange(k0, min(K, k0 + block), dtype=np.uint64)[None, :]
            ex.add(c, k0, *uniform_ints(*raw(seed, c, k, t, 0)))
    return ex


def compare_table(got, seed, call, T, nu, mu=None, sigma=None, sigma_diag=None, k0=0, p=2, q=2, block=16384):
    """got: a binary32 table [T][K][nu] of samples k0 .. k0 + K - 1 against `table`, block by block over k.  Returns
    (n_bad, worst_ratio, message): the number of elements beyond their bound, the largest |got - ref| / bound, and a
    description of the worst element (its (k, t, j), values, radius and the error in units of rad_ref * eps)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.ndim == 3 and got.shape[0] == T and got.shape[2] == nu, (got.dtype, got.shape)
    K = got.shape[1]
    n_bad, worst, msg = 0, -1.0, ""
    for b0 in range(0, K, block):
        n = min(block, K - b0)
        d, bound, rad = table(seed, call, n, T, nu, mu, sigma, sigma_diag, k0 + b0, p, q)
        g = got[:, b0:b0 + n].astype(np.float64)
        err = np.abs(g - d)
        err[~np.isfinite(g)] = np.inf
        ratio = err / bound
        n_bad += int((ratio > 1.0).sum())
        m = float(ratio.max())
        if m > worst:
            t, i, j = np.unravel_index(int(ratio.argmax()), ratio.shape)
            worst = m
            msg = ("call %d k %d t %d j %d: got %.9g, reference %.17g, |diff| %.3g = %.2f rad*eps (rad %.6g), bound %.3g"
                   % (call, k0 + b0 + i, t, j, g[t, i, j], d[t, i, j], err[t, i, j],
                      err[t, i, j] / (rad[t, i, j] * EPS) if rad[t, i, j] > 0 else float("inf") if err[t, i, j] > 0 else 0.0,
                      rad[t, i, j], bound[t, i, j]))
    return n_bad, worst, msg


# The table the value tests run on, and its edge cases by name (call, k, t), found by `extremes` (the integer reference alone)
# and re-derived by tests/test_noise_stream_cpu.py in every run.
BIG_TABLE = dict(seed=0, K=524288, T=30, calls=(0, 1, 2, 3))
BIG_TABLE_EXTREMES = {'u0_one': [(0, 436826, 27), (1, 332294, 28), (1, 338530, 17), (2, 34374, 4), (3, 298436, 7)],
 'u0_small': [(0, 452764, 26), (1, 247100, 2), (3, 399683, 5), (2, 521154, 9), (3, 476293, 5), (0, 370694, 18),
              (1, 415553, 26), (1, 446553, 25), (2, 171825, 11), (3, 410430, 7), (0, 71066, 5), (0, 281563, 13),
              (2, 98161, 27), (1, 94167, 19), (1, 112387, 14), (2, 125417, 5), (2, 503500, 1), (3, 201951, 7),
              (3, 293465, 22), (0, 149919, 29), (0, 281886, 4), (1, 389298, 0), (1, 485562, 7), (2, 70985, 7),
              (3, 250802, 6), (0, 101019, 0), (2, 254057, 6), (2, 302269, 1), (2, 452236, 20), (1, 17259, 12),
              (2, 325209, 29), (3, 52429, 19), (0, 88140, 3), (0, 262317, 21), (0, 362101, 6), (1, 500982, 12),
              (2, 244653, 6), (2, 473250, 1), (3, 386773, 11), (3, 423946, 21), (0, 143186, 3), (0, 403634, 24),
              (0, 428748, 2), (1, 27985, 19), (1, 167910, 12), (1, 253368, 17), (3, 451410, 6), (0, 14931, 22),
              (1, 147835, 8), (3, 176729, 13), (3, 402050, 2), (0, 296238, 1), (0, 486160, 6), (1, 135054, 18),
              (2, 255177, 11), (2, 256687, 3), (2, 295149, 25), (2, 329818, 11), (3, 388666, 8), (2, 449147, 5),
              (3, 254490, 8), (3, 403384, 14), (0, 188094, 14), (1, 199867, 27)],
 'u1_half': [(0, 438872, 23)],
 'u1_large': [(0, 31657, 5), (1, 218228, 15), (1, 458010, 20), (1, 468916, 3), (1, 497165, 23), (1, 499669, 21),
              (3, 34762, 29), (3, 253143, 22), (0, 157190, 2), (0, 103140, 14), (0, 120298, 17), (0, 344141, 3),
              (1, 323202, 10), (2, 304092, 23), (3, 126668, 12), (3, 140340, 14), (3, 229089, 28), (0, 438872, 4),
              (3, 98379, 14), (3, 235329, 22), (3, 520502, 16), (2, 100866, 15), (2, 277905, 3), (3, 472739, 26),
              (0, 88603, 12), (0, 456748, 29), (1, 374236, 16), (1, 482986, 21), (2, 249292, 23), (3, 407727, 4),
              (0, 442955, 23), (1, 68272, 14), (1, 381896, 26), (1, 426537, 6), (1, 480711, 16), (3, 173504, 24),
              (0, 238116, 14), (1, 413741, 29), (3, 509553, 27), (0, 50581, 0), (0, 85977, 21), (0, 399824, 19),
              (1, 322232, 1), (3, 16005, 11), (0, 5430, 10), (1, 418183, 24), (2, 95105, 12), (2, 480568, 1),
              (3, 180526, 19), (0, 287800, 2), (1, 431566, 5), (3, 272171, 19), (1, 200211, 1), (2, 95192, 14),
              (3, 55265, 29), (3, 474800, 25), (0, 235067, 10), (1, 15594, 7), (1, 295020, 10), (2, 158006, 14),
              (3, 193301, 17), (1, 318665, 27), (1, 481424, 27), (1, 517557, 22)],
 'u1_quarter': [(0, 263764, 8)],
 'u1_three_quarters': [(0, 408633, 27)]}
