"""The in-kernel noise stream on the device against the float64 reference of tests/noise_stream_ref.py:

  * `m3_sample_noise` (k_sample_noise) element by element within the derived bound, p = q = 2 (device logf / cosf / sinf),
    point_env and panda_env, diagonal and full sigma, K ragged against every block size, k beyond 2^16, calls 0 .. 3, and the
    named extremes of the K = 524 288 table one by one;
  * shards: a shard handle's table is rows [k_offset, k_offset + K_local) of the unsharded table, as bytes;
  * the three generation sites (point rollout, Panda rollout, k_sample_noise) agree as values: with the action assembly
    configured to the identity, BUF_ACTIONS of command c is the table m3_sample_noise returned just before command c;
  * determinism: two handles in one process and one in a fresh child process leave byte-identical buffers over six commands.

Device maxima: every case prints `worst |got - ref| / bound` and the worst element in rad eps per call; no device figure
is recorded in this file or in DESIGN.md section 5 yet (the host build's is: 7.21 rad eps).
At K = 524 288 x T = 30 two point shapes run (unit diagonal sigma: the table is z itself and carries the named extremes;
the opt_navr mu + full sigma: the shaping and its bound at k > 2^16).  Dropped at that size, on the cost of the float64
reference alone (3 s per call per pair on one core: 4 calls x 5 pairs = 60 s per nu = 9 shape, against a GPU suite of 98 s):
panda_diag, panda_full and point_diag (sigma 3.0), which run at K <= 4001; the Panda sites run at K <= 4001."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import noise_stream_ref as R
from tests import noise_stream_runs as RUNS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1e30
NAVR_MU, NAVR_SIG = R.NAVR_MU, R.NAVR_SIG                  # opt_navr (tests/golden/make_golden.py)
PANDA_MU, PANDA_SIG, PANDA_DIAG = R.PANDA_MU, R.PANDA_SIG, R.PANDA_DIAG   # panda_opt_rand
GOAL7 = [0.2, 0.2, 1.115, 0.0, 0.0, 0.0, 1.0]

SHAPES = {
    "point_diag": dict(env="point_env", nu=2, sigma_diag=[3.0, 3.0]),
    "point_unit": dict(env="point_env", nu=2, sigma_diag=[1.0, 1.0]),     # (the table IS z: the error in units of rad eps)
    "point_full": dict(env="point_env", nu=2, mu=NAVR_MU, sigma=NAVR_SIG),
    "panda_diag": dict(env="panda_env", nu=9, sigma_diag=PANDA_DIAG),
    "panda_full": dict(env="panda_env", nu=9, mu=PANDA_MU, sigma=PANDA_SIG),
}


def make_engine(shape, K, T, seed=0, simple=True, identity=False, **kw):
    """A sampling_random handle of SHAPES[shape].  identity: the assembly leaves the noise as it is (limits at +-1e30, u_scale 1,
    no null action, zero plan -- set_plan before each command)."""
    from m3p2i_aip_amd.engine import HipEngine, make_config
    s = SHAPES[shape]
    nu = s["nu"]
    lim = [BIG] * nu if identity else ([3.0] * 2 if nu == 2 else [2.0] * 7 + [1.5] * 2)
    extra = dict(lambda_=0.05, pre_height_diff=0.05, dt=0.01) if s["env"] == "panda_env" else dict(lambda_=0.5)
    eng = HipEngine(make_config(K=K, T=T, nu=nu, env_type=s["env"], mode_simple=simple, sampling_random=True,
                                sample_null_action=not identity, u_per_command=T, u_min=[-x for x in lim], u_max=lim,
                                noise_sigma_diag=s.get("sigma_diag"), noise_sigma=s.get("sigma"), noise_mu=s.get("mu"),
                                seed=seed, **extra, **kw))
    if s["env"] == "panda_env":
        eng.set_objective("reach", GOAL7, gripper_cmd=0)
    else:
        eng.set_objective("navigation", (-3.0, 3.0))
    return eng


def ref_kw(shape):
    s = SHAPES[shape]
    return dict(mu=s.get("mu"), sigma=s.get("sigma"), sigma_diag=s.get("sigma_diag"))


# ------------------------------------------------------------------------------------ m3_sample_noise vs the reference
SIZES = [(100, 10), (1000, 20), (4001, 20)]      # C1; ragged against 64, 256 and the T * Kl blocks of 256
CASES = [(sh, K, T) for sh in ("point_diag", "point_full", "panda_diag", "panda_full") for K, T in SIZES]
CASES.append(("point_unit", R.BIG_TABLE["K"], R.BIG_TABLE["T"]))      # the table is z itself: the named extremes, rad eps units
CASES.append(("point_full", R.BIG_TABLE["K"], R.BIG_TABLE["T"]))      # mu, the full 2 x 2 factor and its roundings at k > 2^16


@pytest.mark.parametrize("shape,K,T", CASES, ids=["%s-K%d-T%d" % c for c in CASES])
def test_sample_noise_matches_the_reference_within_the_derived_bound(shape, K, T):
    seed = R.BIG_TABLE["seed"] if K == R.BIG_TABLE["K"] else 7
    nu = SHAPES[shape]["nu"]
    eng = make_engine(shape, K, T, seed=seed)
    t0 = time.time()
    worst_all = 0.0
    for call in range(4):                        # the call count advances by commands
        assert eng.info().calls == call
        got = eng.sample_noise().cpu().numpy().copy()
        assert got.shape == (T, K, nu)
        n_bad, worst, msg = R.compare_table(got, seed, call, T, nu, p=2, q=2, **ref_kw(shape))
        print("\n%s K %d T %d call %d: worst |got - ref| / bound = %.3f -- %s" % (shape, K, T, call, worst, msg))
        assert n_bad == 0, "%d elements beyond the bound (p = q = 2); worst: %s" % (n_bad, msg)
        worst_all = max(worst_all, worst)
        if shape == "point_unit":
            _assert_named_extremes(got, seed, call)
        eng.command(sync_host=True)
    print("%s K %d T %d: %.1f s" % (shape, K, T, time.time() - t0))
    eng.close()


def _assert_named_extremes(got, seed, call):
    """The edge cases of the table by name (found by the integer reference; tests/test_noise_stream_cpu.py re-derives them)."""
    for tag, named in R.BIG_TABLE_EXTREMES.items():
        for (c, k, t) in named:
            if c != call:
                continue
            r0, r1 = R.raw(seed, [c], [k], [t], 0)
            n0, n1 = R.uniform_ints(r0, r1)
            z0, z1, rad = R.gauss_from_raw(r0, r1)
            for m, z in enumerate((z0, z1)):
                g = float(got[t, k, m])
                b = float(R.z_bound(z, rad, 2, 2)[0])
                assert np.isfinite(g) and abs(g - float(z[0])) <= b, (
                    "%s (call %d, k %d, t %d) u0 = %d/2^24 u1 = %d/2^24 member %d: device %.9g, reference %.17g, "
                    "|diff| %.3g > bound %.3g (rad %.6g)" % (tag, c, k, t, n0[0], n1[0], m, g, z[0], abs(g - z[0]), b, rad[0]))
            if tag == "u0_one":
                assert got[t, k, 0] == 0.0 and got[t, k, 1] == 0.0, (tag, c, k, t, got[t, k])
    assert np.abs(got).max() <= np.float32(R.Z_MAX) * (1 + 4 * R.EPS)


# ------------------------------------------------------------------------------------ shards see the global k
def _shard_splits():
    return {"2": [500, 500], "3": [300, 251, 450], "8": [125] * 8}


@pytest.mark.parametrize("n", ["2", "3", "8"])
@pytest.mark.parametrize("shape", ["point_full", "panda_full"])
def test_a_shard_table_is_its_rows_of_the_unsharded_table(shape, n):
    sizes = _shard_splits()[n]
    K, T, seed = sum(sizes), 20, 11
    for call in (0, 3):
        whole = make_engine(shape, K, T, seed=seed)
        whole.set_call_count(call)
        full = whole.sample_noise().cpu().numpy().copy()
        whole.close()
        off = 0
        for Kl in sizes:
            sh = make_engine(shape, K, T, seed=seed, K_local=Kl, k_offset=off)
            sh.set_call_count(call)
            part = sh.sample_noise().cpu().numpy().copy()
            sh.close()
            assert part.shape == (T, Kl, SHAPES[shape]["nu"])
            assert part.tobytes() == np.ascontiguousarray(full[:, off:off + Kl]).tobytes(), (
                "shard [%d, %d) of %d, call %d: not the unsharded table's rows" % (off, off + Kl, K, call))
            off += Kl


# ------------------------------------------------------------------------------------ the three sites agree
UNIT_CORR2 = [[1.0, 0.6], [0.6, 1.0]]                       # unit diagonal: quirk Q4's second scaling is by 1
UNIT_CORR9 = [[1.0 if i == j else 0.0 for j in range(9)] for i in range(9)]
UNIT_CORR9[0][1] = UNIT_CORR9[1][0] = 0.4
UNIT_CORR9[2][5] = UNIT_CORR9[5][2] = -0.3
UNIT_CORR9[7][8] = UNIT_CORR9[8][7] = 0.999
SHAPES["point_unit_corr"] = dict(env="point_env", nu=2, mu=NAVR_MU, sigma=UNIT_CORR2)
SHAPES["panda_unit_corr"] = dict(env="panda_env", nu=9, mu=PANDA_MU, sigma=UNIT_CORR9)

# (shape, simple, K, T, panda lanes per sample); point K selects the plain, _occ2 and _occ3 builds: one wavefront per 64
# samples, _occ2 above M3_SIMDS = 1024 wavefronts and _occ3 above 4 * M3_SIMDS (m3_internal.hpp: rollout_two_waves /
# rollout_three_waves) -- 70 016 samples are 1094 wavefronts, 524 288 are 8192.  The library does not report the build it
# launched: if those thresholds move, these K values have to move with them.
SITES = [("point_full", True, 4001, 20, 0), ("point_unit_corr", False, 4001, 20, 0), ("point_diag", True, 100, 10, 0),
         ("point_full", True, 70016, 12, 0), ("point_unit_corr", False, 524288, 12, 0)]
SITES += [(sh, simple, 1000, 12, lps) for lps in (1, 8, 16) for sh, simple in (("panda_full", True), ("panda_unit_corr", False))]
SITES.append(("panda_diag", True, 4001, 12, 0))


@pytest.mark.parametrize("shape,simple,K,T,lps", SITES,
                         ids=["%s-%s-K%d-T%d-lps%d" % (s, "simple" if m else "halton_random", K, T, l) for s, m, K, T, l in SITES])
def test_rollout_and_sample_noise_generate_the_same_values(shape, simple, K, T, lps):
    """With the assembly at the identity, BUF_ACTIONS of command c == the table m3_sample_noise wrote before command c.
    Rows excluded, exactly: halton-spline mode zeroes the noise of sample K - 1 (mppi.py:392, quirk Q6's row); simple mode
    excludes none; no handle here is multi-modal (whose specials would be samples 0 and K / 2)."""
    from m3p2i_aip_amd import _lib as L
    nu = SHAPES[shape]["nu"]
    eng = make_engine(shape, K, T, seed=5, simple=simple, identity=True)
    if lps:
        eng.set_panda_lanes_per_sample(lps)
    excluded = [] if simple else [K - 1]
    assert len(excluded) <= 3
    keep = np.ones(K, bool)
    keep[excluded] = False
    for call in range(4 if K <= 70016 else 2):
        eng.set_plan(L.BUF_MEAN, np.zeros((T, nu), np.float32))
        noise = eng.sample_noise().cpu().numpy().copy()
        eng.command(sync_host=True)
        act = eng.buffer(L.BUF_ACTIONS).cpu().numpy()
        if lps:
            assert eng.panda_lanes_per_sample_used() == lps
        assert np.isfinite(noise).all() and np.abs(noise).max() > 1.0
        same = (act == noise)                    # as values: 0 + (-0) is +0
        bad = np.argwhere(~same[:, keep])
        assert bad.size == 0, "call %d: %d elements differ; first (t, kept row, j) = %s: rollout %r, m3_sample_noise %r" % (
            call, len(bad), bad[0], act[:, keep][tuple(bad[0])], noise[:, keep][tuple(bad[0])])
        for k in excluded:
            assert np.all(act[:, k] == 0.0)      # (the excluded row is the zero-noise sample on a zero plan)
    eng.close()


# ------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("name", RUNS.CONFIGS)
def test_two_handles_and_a_fresh_process_leave_identical_bytes(name, tmp_path):
    plan_a, a = RUNS.run(name)
    plan_b, b = RUNS.run(name)
    out = str(tmp_path / "child.npz")
    r = subprocess.run([sys.executable, "-m", "tests.noise_stream_runs", name, out], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    plan_c, c = RUNS.load(out)
    assert plan_a.tobytes() == plan_b.tobytes() == plan_c.tobytes(), "the plan before the first command differs"
    for other, who in ((b, "a second handle in this process"), (c, "a handle in a fresh process")):
        d = RUNS.first_difference(a, other)
        assert d is None, "%s: %s differs first, at command %d, from %s" % (name, d[1], d[0], who)
    # the stream is what the reference says it is, in every one of the six calls (C1: seed 0)
    if name == "c1":
        for call in range(RUNS.N_COMMANDS):
            n_bad, worst, msg = R.compare_table(a[call]["NOISE"], 0, call, 10, 2, sigma_diag=[3.0, 3.0], p=2, q=2)
            assert n_bad == 0, msg


def test_c1_initial_plan_is_torchs_global_generator_and_nothing_else_differs():
    """What docs/NOTEBOOK.md once recorded as "C1's dump is not reproducible": simple mode draws its initial plan U from torch's
    GLOBAL generator (mppi.py:129-134), which a process that does not call torch.manual_seed seeds from the clock.  Under two
    different torch seeds the plan before the first command differs, and with it everything the rollout and the update
    write; the noise tables -- a function of cfg.seed and the call count -- are the same bytes."""
    plan_a, a = RUNS.run("c1", torch_seed=1)
    plan_b, b = RUNS.run("c1", torch_seed=2)
    assert plan_a.tobytes() != plan_b.tobytes()
    for call in range(RUNS.N_COMMANDS):
        assert a[call]["NOISE"].tobytes() == b[call]["NOISE"].tobytes(), call
    assert RUNS.first_difference(a, b) == (0, "ACTIONS")
