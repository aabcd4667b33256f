"""What m3_batch_command, the two episode-set creates and m3_episodes_tick answer for every combination of the sections a batch or
a set was created with and the kind of handle it is handed: the return code, the error text and, for an
accepted call, the launch counts, against tests/golden/batch_refusals.json.

The fixture was recorded by THIS file from the library as it stood before the sections were described once (commit deafd63):
M3_BATCH_REFUSALS_RECORD=<path> writes what the calls answer to <path> instead of comparing, with M3P2I_HIP_LIB naming that
library.  It is never recorded from the code under test.  K = 64, T = 4, one handle per kind; every call is a one-handle call but
the pairs (two environments in one call, a handle listed twice).  The accepted calls' results are pinned byte for byte against
m3_command by the batch and episode tests of each section; here only that they are accepted, and in how many launches."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipEngine, make_config  # noqa: E402
from tests import panda_scene_fixture as PX  # noqa: E402
from tests import point_scene_fixture as X  # noqa: E402
from tests import rollout_scenes_fixture as R  # noqa: E402
from tests.test_batch_command_gpu import PK, _noise  # noqa: E402
from tests.test_point_scene_gpu import W_TUNED  # noqa: E402

F = np.float32
K, T = 64, 4
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_refusals.json")
RECORD = os.environ.get("M3_BATCH_REFUSALS_RECORD")
BITS = (L.BATCH_SECTION_PANDA_RUNTIME, L.BATCH_SECTION_POINT_ROLLOUT_SCENES, L.BATCH_SECTION_POINT_PRIORS)
MASKS = [sum(c) for r in range(4) for c in itertools.combinations(BITS, r)]      # all 8
PANDA_PK = dict(u_min=PX.UMIN, u_max=PX.UMAX, noise_sigma_diag=PX.SIG, lambda_=0.05, pre_height_diff=0.05, dt=0.01)
IDX = [1, 7, 20, 40]


def _seqs(nu):
    return np.random.default_rng(3).standard_normal((len(IDX), T, nu)).astype(F)


def _point(kind, **cfg):
    e = HipEngine(make_config(T=T, nu=2, filter_u=False, **{**PK, "K": K, **cfg}))
    if not e.cfg.sim_only:
        e.set_noise(_noise(e.cfg.K_local, T, 7))
        e.set_objective("push", [-1.0, -1.0])
    if "weights" in kind:
        e.set_point_cost_weights(W_TUNED)
    if "scene" in kind:
        e.set_point_scene(X.CUSTOM)
    if "rows" in kind or "priors" in kind:
        _point_state(e, kind)
    return e


def _point_state(e, kind):
    """the arena per sample and the prior samples of the kind, set or cleared"""
    e.set_point_rollout_scenes(R.cycle_rows(K) if "rows" in kind else None)
    e.set_prior_samples(_seqs(2) if "priors" in kind else None, IDX)


def _panda(kind):
    e = HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", filter_u=False, **PANDA_PK))
    e.set_objective("reach", np.array(PX.GOAL, F), gripper_cmd=1)
    e.set_noise(np.random.default_rng(5).standard_normal((K, T, 9)).astype(F))
    if kind == "weights":
        e.set_panda_cost_weights(dict(pick_ori=25.0))
    if kind == "rows":
        e.set_panda_rollout_scenes([PX.SCENES["mu"]] + [None] * (K - 1))
    if kind == "priors":
        e.set_panda_prior_samples(_seqs(9), IDX)
    return e


POINT_KINDS = ("plain", "weights", "scene", "rows", "priors", "priors_rows")
PANDA_KINDS = ("literal", "weights", "rows", "priors")


@pytest.fixture(scope="module")
def handles():
    h = {"point_" + k: _point(k) for k in POINT_KINDS}
    h.update({"panda_" + k: _panda(k) for k in PANDA_KINDS})
    h["sharded"] = _point("plain", K=2 * K, K_local=K)
    h["sim_only"] = _point("plain", sim_only=True)
    yield h
    for e in h.values():
        e.close()


@pytest.fixture(scope="module")
def golden():
    """the recorded answers; in record mode an empty dict that the tests fill and the module writes out at its end"""
    if not RECORD:
        with open(GOLDEN) as f:
            yield json.load(f)
        return
    got = {}
    yield got
    with open(RECORD, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")


def _settle(golden, part, got):
    if RECORD:
        golden[part] = got
        return
    want = golden[part]
    assert sorted(got) == sorted(want), part
    different = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not different, (part, different)


def _batches(lib):
    """every way to create a batch: (name, handle)"""
    torch.zeros(1, device=DEV)
    made = []
    for name, create in ([("create", lambda out: lib.m3_batch_create(0, 2, out)),
                          ("create_ex_runtime", lambda out: lib.m3_batch_create_ex(0, 2, L.BATCH_PANDA_RUNTIME, out))] +
                         [("sections_%d" % m, lambda out, m=m: lib.m3_batch_create_sections(0, 2, m, out)) for m in MASKS]):
        b = C.c_void_p()
        assert create(C.byref(b)) == 0, name
        made.append((name, b))
    return made


def _command(lib, b, engines):
    arr = (C.c_void_p * len(engines))(*[e._h.value for e in engines])
    rc = lib.m3_batch_command(b, arr, len(engines), None)
    torch.cuda.synchronize()
    if rc != 0:
        return [rc, lib.m3_batch_last_error(b).decode(), None]
    roll, upd = C.c_int(), C.c_int()
    assert lib.m3_batch_launches(b, C.byref(roll), C.byref(upd)) == 0
    return [0, "", [roll.value, upd.value]]


def test_batch_command_for_every_creation_and_every_kind_of_handle(handles, golden):
    lib = L.load()
    cases = {name: [e] for name, e in handles.items()}
    cases["pair_point_then_panda"] = [handles["point_plain"], handles["panda_literal"]]
    cases["pair_panda_then_point"] = [handles["panda_literal"], handles["point_plain"]]
    cases["pair_listed_twice"] = [handles["point_plain"], handles["point_plain"]]
    got, batches = {}, _batches(lib)
    try:
        for name, b in batches:
            for case, engines in cases.items():
                got[f"{name}/{case}"] = _command(lib, b, engines)
    finally:
        for _, b in batches:
            lib.m3_batch_destroy(b)
    assert len(got) == 10 * (len(POINT_KINDS) + len(PANDA_KINDS) + 2 + 3)
    _settle(golden, "batch_command", got)


@pytest.fixture(scope="module")
def point_world():
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    w = IsaacGymWrapper(IsaacGymConfig(), "point_env", num_envs=1, device=DEV)
    yield w._engine
    w.stop_sim()


EPS_FLAGS = (0, L.EPISODES_ROLLOUT_SCENES, L.EPISODES_PRIORS, L.EPISODES_ROLLOUT_SCENES | L.EPISODES_PRIORS)
SPEC = (L.EpisodeSpec * 1)()
SPEC[0].task, SPEC[0].dyn_phase, SPEC[0].suction, SPEC[0].kp_suction = L.TASKS["push"], 0, L.SUCTION_OFF, 400.0
SPEC[0].goal[0], SPEC[0].goal[1] = -3.0, 3.0


def _episodes_create(lib, world, e, flags):
    """(answer, the set or None) of m3_episodes_create_ex for the one planner e"""
    if e._action_out is None and not e.cfg.sim_only:
        e.set_action_out(torch.zeros(T, e.cfg.nu, device=DEV))
    arr, eps = (C.c_void_p * 1)(e._h.value), C.c_void_p()
    rc = lib.m3_episodes_create_ex(world._h, arr, SPEC, 1, 64, 0, flags, C.byref(eps))
    return [rc, "" if rc == 0 else lib.m3_episodes_last_error(None).decode()], (eps if rc == 0 else None)


def test_episodes_create_for_every_flag_and_every_kind_of_planner(handles, point_world, golden):
    lib = L.load()
    got = {}
    for flags in EPS_FLAGS:
        for name, e in handles.items():
            got[f"flags_{flags}/{name}"], eps = _episodes_create(lib, point_world, e, flags)
            if eps:
                lib.m3_episodes_destroy(eps)
    _settle(golden, "episodes_create", got)


def test_episodes_tick_for_every_set_batch_and_planner_state(handles, point_world, golden):
    """the planner is plain when the set is created and gets its arena per sample or its priors afterwards, so that every set takes
    it: the early refusals of m3_episodes_tick (one in the set's name, two in m3_batch_command's), m3_episodes_tick's refusal of
    priors in a set without the flag, and the accepted ticks"""
    lib = L.load()
    e = handles["point_plain"]
    got, batches = {}, _batches(lib)[2:]      # (the 8 masks: m3_batch_create and _create_ex make masks 0 and 1)
    try:
        for flags in EPS_FLAGS:
            for state in ("rows", "priors", "priors_rows"):
                answer, eps = _episodes_create(lib, point_world, e, flags)
                assert answer[0] == 0, answer
                try:
                    _point_state(e, state)
                    for name, b in batches:
                        rc = lib.m3_episodes_tick(eps, b)
                        torch.cuda.synchronize()
                        roll, upd = C.c_int(), C.c_int()
                        assert lib.m3_batch_launches(b, C.byref(roll), C.byref(upd)) == 0
                        assert lib.m3_episodes_running(eps) == 1          # (an ended episode would command nothing)
                        got[f"flags_{flags}/{state}/{name}"] = ([0, "", [roll.value, upd.value]] if rc == 0 else
                                                                 [rc, lib.m3_episodes_last_error(eps).decode(), None])
                finally:
                    _point_state(e, "plain")
                    lib.m3_episodes_destroy(eps)
    finally:
        for _, b in batches:
            lib.m3_batch_destroy(b)
    assert len(got) == 4 * 3 * 8
    _settle(golden, "episodes_tick", got)


def test_panda_episodes_create_for_both_modes_and_every_kind_of_planner(handles, golden):
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    lib = L.load()
    w = IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=1, device=DEV)
    got = {}
    try:
        for flags in (0, L.PANDA_EPISODES_RUNTIME):
            for name, e in handles.items():
                if e._action_out is None and not e.cfg.sim_only:
                    e.set_action_out(torch.zeros(T, e.cfg.nu, device=DEV))
                arr, eps = (C.c_void_p * 1)(e._h.value), C.c_void_p()
                rc = lib.m3_panda_episodes_create_ex(w._engine._h, arr, 1, 8, 0, 0, flags, C.byref(eps))
                got[f"flags_{flags}/{name}"] = [rc, "" if rc == 0 else lib.m3_panda_episodes_last_error(None).decode()]
                if rc == 0:
                    lib.m3_panda_episodes_destroy(eps)
    finally:
        w.stop_sim()
    _settle(golden, "panda_episodes_create", got)
