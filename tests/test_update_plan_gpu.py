"""The update plan (csrc/update_plan.hpp) on the device: same bits as the library had before one executor walked a plan.

tests/golden/update_plan_parent.npz was recorded from the library of the commit before the plan existed (bcfdbc8), by this
file's record mode:

    python -m tests.test_update_plan_gpu --record --lib <path of that commit's libm3p2i_hip.so>

It holds raw arrays and error texts only.  One case per form and protocol, each at the smallest shape that reaches it, the
cost vectors from update_f64_checks.make_costs:

    k_update_small, single                     K = 20
    k_update_small, multi, 512-thread instance K = 2049
    Panda small                                nu = 9, K = 20
    phases path (m3_update, m3_finalize)       K = 21
    three-launch form, multi fused             K = 8193 (costs written by the caller: k_mins' minima)
    ... inside m3_command                      K = 8193 (the rollout's minima)
    five-launch path                           K = 8193 after set_update_launches(5)
    unfused finalize                           T * nu = 2050 (nu = 2 has no product 2049: the first beyond 2048)
    protocols 0 / 1-single / 1-multi / 2 / 3   4 shards of 20 samples, T = 12, sharded_update_driver's engines and exchange

Every buffer that is compared is written before the call, so that what a form leaves alone is defined too.  Compared bit for
bit: plan, means, best rows, weights, top_idx, top trajectories, m3_info; and every refusal's code and text.  Kernels and
arguments are unchanged, so no tolerance applies.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "update_plan_parent.npz")
OUT_BUFS = ("BUF_ACTION_OUT", "BUF_MEAN", "BUF_MEAN_1", "BUF_MEAN_2", "BUF_BEST", "BUF_BEST_1", "BUF_BEST_2", "BUF_WEIGHTS",
            "BUF_WEIGHTS_1", "BUF_WEIGHTS_2", "BUF_TOP_IDX", "BUF_TOP_TRAJS")

# (id, K, T, nu, mode, dist, entry)
UNSHARDED = [
    ("small_single_K20", 20, 12, 2, "single", "s1", "fused"),
    ("small_multi512_K2049", 2049, 12, 2, "multi", "s1", "fused"),
    ("small_panda_K20", 20, 12, 9, "single", "cycle", "fused"),
    ("phases_K21", 21, 12, 2, "single", "s1", "phases"),
    ("phases_multi_K21", 21, 12, 2, "multi", "s1", "phases"),
    ("three_launch_K8193", 8193, 12, 2, "multi", "s1", "fused"),
    ("three_launch_command_K8193", 8193, 12, 2, "multi", "s1", "command"),
    ("five_launch_K8193", 8193, 12, 2, "multi", "s1", "five"),
    ("unfused_finalize_T1025", 20, 1025, 2, "single", "s1", "fused"),
]
# (id, proto, mode)
SHARDED = [("proto0_single", 0, "single"), ("proto0_multi", 0, "multi"), ("proto1_single", 1, "single"), ("proto1_multi", 1, "multi"),
           ("proto2", 2, "multi"), ("proto3", 3, "multi")]


def _seed(name):
    return sum(map(ord, name))


def _init_outputs(L, eng, rng):
    """every compared buffer gets defined content: what a form does not write stays as written here"""
    for name in OUT_BUFS:
        t = eng.buffer(getattr(L, name))
        if name.startswith("BUF_WEIGHTS") or name in ("BUF_ACTION_OUT", "BUF_TOP_TRAJS", "BUF_TOP_IDX"):
            t.zero_()
        else:
            t.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(t.shape)).astype(np.float32)))


def _outputs(L, eng, prefix, out):
    from tests.sharded_update_driver import INFO_FIELDS
    for name in OUT_BUFS:
        out[f"{prefix}/{name}"] = eng.buffer(getattr(L, name)).cpu().numpy().copy()
    i = eng.info()
    out[f"{prefix}/info"] = np.array([float(getattr(i, f)) for f in INFO_FIELDS], np.float64)


def run_unsharded(name, K, T, nu, mode, dist, entry, out):
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipEngine, make_config
    from tests.sharded_update_driver import smooth_noise
    from tests.update_f64_checks import make_costs
    kw = dict(u_min=[-2.0] * 7 + [-1.5] * 2, u_max=[2.0] * 7 + [1.5] * 2, noise_sigma_diag=[10.0] * 7 + [0.8] * 2,
              lambda_=0.05, dt=0.01, env_type="panda_env") if nu == 9 else \
        dict(u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3], lambda_=1.0)
    eng = HipEngine(make_config(K=K, T=T, nu=nu, multi_modal=mode == "multi", **kw))
    try:
        if entry == "five":
            eng.set_update_launches(5)
        rng = np.random.default_rng(_seed(name))
        _init_outputs(L, eng, rng)
        if entry == "command":   # the costs are the rollout's own
            eng.set_noise(smooth_noise(K, T, nu, _seed(name)))
            eng.set_objective("push_pull", (-3.75, -3.75))
            eng.set_world_point_raw(np.array([0.0, 1.5, 0, 0, 0, 2, 1, 0, 0, 0, 0, -2, 2, 1, 0, 0, 0, 0], np.float32))
            eng.command()
        else:
            eng.buffer(L.BUF_TRAJ_COST).copy_(torch.from_numpy(make_costs(dist, K, rng)))
            eng.buffer(L.BUF_ACTIONS).copy_(torch.from_numpy(rng.uniform(-3, 3, (T, K, nu)).astype(np.float32)))
            eng.buffer(L.BUF_STATES).copy_(torch.from_numpy(rng.uniform(-5, 5, (T, K, 4)).astype(np.float32)))
            if entry == "phases":
                eng.update()
                eng.finalize()
            else:
                eng.update_finalize()
        torch.cuda.synchronize()
        _outputs(L, eng, name, out)
    finally:
        eng.close()


def run_sharded(name, proto, mode, out):
    from m3p2i_aip_amd import _lib as L
    from tests.sharded_update_driver import Case, HipBackend, exchange, smooth_noise
    from tests.update_f64_checks import make_costs
    case = Case(name, proto, mode, [20, 20, 20, 20], "s1")
    backend = HipBackend()
    engines = [backend.engine(case, r) for r in range(4)]
    try:
        rng = np.random.default_rng(_seed(name))
        K, T, nu, off = case.K, case.T, case.nu, case.offsets
        for e in engines:
            _init_outputs(L, e, np.random.default_rng(_seed(name) + 1))   # (the replicated state: the same on every rank)
        if case.regen:
            delta = smooth_noise(K, T, nu, _seed(name))
            for e in engines:
                e.set_noise(delta)
                backend.prepare_rollout(e, case)
                e.rollout()
            backend.sync()
        J = make_costs("s1", K, rng)
        A = rng.uniform(-3, 3, (T, K, nu)).astype(np.float32)
        S = rng.uniform(-5, 5, (T, K, 4)).astype(np.float32)
        for r, e in enumerate(engines):
            lo, hi = off[r], off[r + 1]
            e.buffer(L.BUF_TRAJ_COST).copy_(torch.from_numpy(J[lo:hi]))
            if not case.regen:
                e.buffer(L.BUF_ACTIONS).copy_(torch.from_numpy(np.ascontiguousarray(A[:, lo:hi])))
                e.buffer(L.BUF_STATES).copy_(torch.from_numpy(np.ascontiguousarray(S[:, lo:hi])))
        exchange(L, case, engines)
        backend.sync()
        for r, e in enumerate(engines):
            _outputs(L, e, f"{name}/rank{r}", out)
    finally:
        for e in engines:
            e.close()


def _refusal(call):
    from m3p2i_aip_amd import _lib as L
    with pytest.raises(L.M3Error) as ei:
        call()
    return str(ei.value)


def run_refusals(out):
    """code and text of every refusal that the update plan or a protocol predicate decides"""
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipEngine, make_config
    from tests.sharded_update_driver import Case, HipBackend
    texts = {}
    eng = HipEngine(make_config(K=20, T=12, nu=2, u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3]))
    try:
        texts["update_b_unsharded"] = _refusal(eng.update_b)
        texts["p2p_export_unsharded"] = _refusal(eng.p2p_export)
        texts["set_noise_global_unsharded"] = _refusal(
            lambda: eng._ck(eng.lib.m3_set_noise_global(eng._h, np.zeros((20, 12, 2), np.float32).ctypes.data, 0)))
    finally:
        eng.close()
    backend = HipBackend()
    for proto, mode in ((0, "multi"), (1, "single"), (1, "multi"), (2, "multi"), (3, "multi")):
        e = backend.engine(Case("r", proto, mode, [20, 20, 20, 20], "s1"), 1)
        try:
            tag = f"proto{proto}_{mode}"
            texts[f"command_{tag}"] = _refusal(e.command)
            texts[f"update_finalize_{tag}"] = _refusal(e.update_finalize)
            if proto != 3:
                texts[f"update_b_{tag}"] = _refusal(e.update_b)
                if proto:
                    texts[f"p2p_channel1_{tag}"] = _refusal(lambda: e.p2p_put(1))
            if mode == "multi" and proto:
                texts[f"set_noise_{tag}"] = _refusal(
                    lambda: e._ck(e.lib.m3_set_noise(e._h, np.zeros((20, 12, 2), np.float32).ctypes.data, 0)))
                texts[f"sample_noise_{tag}"] = _refusal(lambda: e._ck(e.lib.m3_sample_noise(e._h)))
        finally:
            e.close()
    e = backend.engine(Case("long", 2, "multi", [20, 20], "s1", T=1025), 1)   # T * nu = 2050
    try:
        texts["finalize_proto2_long_plan"] = _refusal(e.finalize)
    finally:
        e.close()
    for k, v in texts.items():
        out[f"refusal/{k}"] = np.array(v)


def _case_ids():
    return [c[0] for c in UNSHARDED] + [c[0] for c in SHARDED] + ["refusals"]


def _run(case_id, out):
    for c in UNSHARDED:
        if c[0] == case_id:
            return run_unsharded(*c, out)
    for c in SHARDED:
        if c[0] == case_id:
            return run_sharded(*c, out)
    return run_refusals(out)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case_id", _case_ids())
def test_same_bits_as_before_the_plan(case_id, golden):
    got = {}
    _run(case_id, got)
    want = {k: v for k, v in golden.items() if k == case_id or k.startswith(("refusal/" if case_id == "refusals" else case_id + "/"))}
    assert sorted(got) == sorted(want) and got, (sorted(got), sorted(want))
    for k, v in got.items():
        w = want[k]
        if k.startswith("refusal/"):
            assert str(v) == str(w), (k, str(v), str(w))
        else:
            assert v.dtype == w.dtype and v.shape == w.shape and v.tobytes() == w.tobytes(), \
                (k, int((v.view(np.uint8) != w.view(np.uint8)).sum()) if v.shape == w.shape else (v.shape, w.shape))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--lib", required=True, help="the libm3p2i_hip.so to record from")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    assert a.record
    os.environ["M3P2I_HIP_LIB"] = os.path.abspath(a.lib)   # (before m3p2i_aip_amd._lib is imported)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    rec = {}
    for cid in _case_ids():
        _run(cid, rec)
        print("recorded", cid, flush=True)
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
