"""The return code and the complete m3_last_error text of every refusal of the per-handle scene and cost-weight entry points of
both environments -- the rows per environment / per sample, the single scene, the instance switches, the cost weights -- as
literals, plus what the getters answer and what a refused call leaves behind.  Raw ctypes through _lib only, so the file says
the same about any build of the library; handles with K_local = 8, T = 2, one planner and one sim_only handle per environment.
No kernel is launched."""
import ctypes as C

import pytest

from m3p2i_aip_amd import _lib as L

pytestmark = pytest.mark.gpu

OK, BAD_ARG, SHAPE, STATE, UNSUPPORTED = 0, -1, -3, -4, -5
KL = 8
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(scope="module")
def handles(lib):
    """{(env, sim_only): handle}"""
    out = {}
    for env, name in ((L.ENV_POINT, "point"), (L.ENV_PANDA, "panda")):
        for sim_only in (0, 1):
            c = L.Config()
            lib.m3_default_config(C.byref(c), env)
            c.K_global, c.K_local, c.k_offset, c.T, c.u_per_command = 24, KL, 8, 2, 2     # (a planner needs K >= 20)
            c.filter_u, c.sim_only = 0, sim_only
            if sim_only:
                c.K_global, c.k_offset = KL, 0
            h = C.c_void_p()
            rc = lib.m3_create(C.byref(c), C.byref(h))
            assert rc == OK, lib.m3_last_error(None)
            out[name, "sim" if sim_only else "planner"] = h
    yield out
    for h in out.values():
        lib.m3_destroy(h)


def err(lib, h):
    return lib.m3_last_error(h).decode()


def point(**kw):
    return L.PointSceneFields(**{**L.POINT_SCENE_DEFAULTS, **kw})


def panda(**kw):
    return L.panda_scene_fields(kw)


def array(struct, rows):
    arr = (struct * len(rows))()
    for i, r in enumerate(rows):
        arr[i] = r
    return arr


# kind -> (struct, a scene from overrides, the other environment's name, a field to tell rows apart)
KIND = {"point": (L.PointSceneFields, point, "panda"), "panda": (L.PandaSceneFields, panda, "point")}
# (kind, per sample) -> setter, getter, flag query, the handle kind that takes it
ROWS = {
    ("point", False): ("m3_set_point_scene_rows", "m3_get_point_scene_row", "m3_point_scene_rows_set", "sim"),
    ("point", True): ("m3_set_point_rollout_scenes", "m3_get_point_rollout_scene", "m3_point_rollout_scenes_set", "planner"),
    ("panda", False): ("m3_set_panda_scene_rows", "m3_get_panda_scene_row", "m3_panda_scene_rows_set", "sim"),
    ("panda", True): ("m3_set_panda_rollout_scenes", "m3_get_panda_rollout_scene", "m3_panda_rollout_scenes_set", "planner"),
}
WRONG_ENV = {
    "m3_set_point_scene_rows": "m3_set_point_scene_rows: point_env only",
    "m3_set_point_rollout_scenes": "m3_set_point_rollout_scenes: point_env only",
    "m3_set_panda_scene_rows": "m3_set_panda_scene_rows: panda_env only",
    "m3_set_panda_rollout_scenes": "m3_set_panda_rollout_scenes: panda_env only",
}
WRONG_HANDLE = {
    "m3_set_point_scene_rows": "m3_set_point_scene_rows: sim_only handles only (a planner's rollouts share one model: m3_set_point_scene)",
    "m3_set_point_rollout_scenes": "m3_set_point_rollout_scenes: planner handles only (the environments of a sim_only handle: m3_set_point_scene_rows)",
    "m3_set_panda_scene_rows": "m3_set_panda_scene_rows: sim_only handles only (the samples of a planner's rollout: m3_set_panda_rollout_scenes)",
    "m3_set_panda_rollout_scenes": "m3_set_panda_rollout_scenes: planner handles only (the environments of a sim_only handle: m3_set_panda_scene_rows)",
}
# one bad row in the middle: (overrides of row 3, what the message says after "row 3: ")
BAD_ROWS = {
    "point": [(dict(box_m=NAN), "box_m is not finite"), (dict(obs_y=INF), "obs_y is not finite"),
              (dict(box_hx=0.0), "box_hx must be > 0"), (dict(mu_rb=-0.5), "mu_rb must be >= 0"),
              (dict(wall=0.2), "wall must be > robot_r"), (dict(robot_r=4.0), "wall must be > robot_r")],
    "panda": [(dict(table=(0, 0, 1, 0.6, NAN, 0.025)), "table[4] is not finite"), (dict(base=(-0.45, -INF, 1.125)), "base[1] is not finite"),
              (dict(shelf=(0.5, 0, 1.175, 0.1, 0.1, 0.0)), "shelf[5] must be > 0"), (dict(cube_m=-1.0), "cube_m must be > 0"),
              (dict(mu=-0.25), "mu must be >= 0")],
}
GOOD = {"point": [dict(mu_rb=0.1 + 0.05 * i) for i in range(KL)], "panda": [dict(mu=0.5 + 0.05 * i) for i in range(KL)]}
OTHER = {"point": [dict(box_m=10.0 + i) for i in range(KL)], "panda": [dict(obs_m=1.0 + i) for i in range(KL)]}


@pytest.mark.parametrize("kind,per_sample", sorted(ROWS))
def test_rows_setter_refusals_and_what_they_leave(lib, handles, kind, per_sample):
    setter, getter, flag, takes = ROWS[kind, per_sample]
    struct, make, other_env = KIND[kind]
    setter, getter, flag = getattr(lib, setter), getattr(lib, getter), getattr(lib, flag)
    who = ROWS[kind, per_sample][0]
    h = handles[kind, takes]
    good = array(struct, [make(**r) for r in GOOD[kind]])
    nine = array(struct, [make()] * (KL + 1))
    out = struct()
    # null handle: no message anywhere
    before = err(lib, None)
    assert setter(None, good, KL) == BAD_ARG and getter(None, 0, C.byref(out)) == BAD_ARG and flag(None) == BAD_ARG
    assert err(lib, None) == before
    # wrong environment, wrong handle kind: before the arguments are looked at
    for wrong in ("planner", "sim"):
        assert setter(handles[other_env, wrong], None, 0) == UNSUPPORTED and err(lib, handles[other_env, wrong]) == WRONG_ENV[who]
        assert getter(handles[other_env, wrong], 0, C.byref(out)) == UNSUPPORTED and err(lib, handles[other_env, wrong]) == WRONG_ENV[who]
    wrong = handles[kind, "planner" if takes == "sim" else "sim"]
    for args in ((good, KL), (None, 0)):
        assert setter(wrong, *args) == STATE and err(lib, wrong) == WRONG_HANDLE[who]
    assert flag(wrong) == 0 and getter(wrong, 0, C.byref(out)) == STATE and err(lib, wrong) == WRONG_HANDLE[who]
    # the feature off: the getter's code, whatever the row
    assert setter(h, None, 0) == OK and flag(h) == 0
    for row in (0, -1, KL):
        assert getter(h, row, C.byref(out)) == STATE
    assert getter(h, 0, None) == BAD_ARG
    # n = K_local -+ 1
    assert setter(h, good, KL - 1) == SHAPE and err(lib, h) == who + ": n is 7, the handle's K_local 8"
    assert setter(h, nine, KL + 1) == SHAPE and err(lib, h) == who + ": n is 9, the handle's K_local 8"
    assert flag(h) == 0
    # set; the getter's codes with the feature on (and no word in the handle's error text from it)
    assert setter(h, good, KL) == OK and flag(h) == 1
    text = err(lib, h)
    for row in range(KL):
        assert getter(h, row, C.byref(out)) == OK and bytes(out) == bytes(good[row]), row
    assert getter(h, -1, C.byref(out)) == BAD_ARG and getter(h, KL, C.byref(out)) == BAD_ARG and getter(h, 0, None) == BAD_ARG
    assert err(lib, h) == text
    # one bad row in the middle of other rows: refused with the row and the field, and nothing changed
    for overrides, what in BAD_ROWS[kind]:
        rows = [make(**r) for r in OTHER[kind]]
        rows[3] = make(**{**OTHER[kind][3], **overrides})
        assert setter(h, array(struct, rows), KL) == BAD_ARG and err(lib, h) == f"{who}: row 3: {what}", what
        assert flag(h) == 1
        for row in range(KL):
            assert getter(h, row, C.byref(out)) == OK and bytes(out) == bytes(good[row]), (what, row)
    assert setter(h, good, KL + 1) == SHAPE and flag(h) == 1
    assert getter(h, 5, C.byref(out)) == OK and bytes(out) == bytes(good[5])
    # a second set reuses the blocks; null clears and does not read n
    other = array(struct, [make(**r) for r in OTHER[kind]])
    assert setter(h, other, KL) == OK and getter(h, 7, C.byref(out)) == OK and bytes(out) == bytes(other[7])
    assert setter(h, None, KL + 5) == OK and flag(h) == 0 and getter(h, 0, C.byref(out)) == STATE
    assert setter(h, None, -3) == OK and flag(h) == 0


SINGLE = {"point": ("m3_set_point_scene", "m3_get_point_scene"), "panda": ("m3_set_panda_scene", "m3_get_panda_scene")}


@pytest.mark.parametrize("kind", sorted(SINGLE))
def test_single_scene_setter_refusals_and_the_two_flags(lib, handles, kind):
    who = SINGLE[kind][0]
    setter, getter = getattr(lib, SINGLE[kind][0]), getattr(lib, SINGLE[kind][1])
    struct, make, other_env = KIND[kind]
    out = struct()
    before = err(lib, None)
    assert setter(None, None) == BAD_ARG and getter(None, C.byref(out)) == BAD_ARG and err(lib, None) == before
    for wrong in ("planner", "sim"):
        hw = handles[other_env, wrong]
        assert setter(hw, None) == UNSUPPORTED and err(lib, hw) == f"{who}: {kind}_env only"
        assert getter(hw, C.byref(out)) == UNSUPPORTED and err(lib, hw) == f"{who}: {kind}_env only"
    for takes, per_sample in (("sim", False), ("planner", True)):
        h = handles[kind, takes]
        set_rows, flag = getattr(lib, ROWS[kind, per_sample][0]), getattr(lib, ROWS[kind, per_sample][2])
        other_flag = getattr(lib, ROWS[kind, not per_sample][2])
        kept = make(**OTHER[kind][2])
        assert setter(h, C.byref(kept)) == OK
        assert set_rows(h, array(struct, [make(**r) for r in GOOD[kind]]), KL) == OK and flag(h) == 1 and other_flag(h) == 0
        # a refused set: the message names the field, the scene and the rows stand
        for overrides, what in BAD_ROWS[kind]:
            bad = make(**overrides)
            assert setter(h, C.byref(bad)) == BAD_ARG and err(lib, h) == f"{who}: {what}", what
            assert getter(h, C.byref(out)) == OK and bytes(out) == bytes(kept) and flag(h) == 1
        assert getter(h, None) == BAD_ARG
        # an accepted one switches both flags off (null: the defaults)
        assert setter(h, None) == OK and flag(h) == 0 and other_flag(h) == 0
        assert getter(h, C.byref(out)) == OK and bytes(out) == bytes(make())
        assert getattr(lib, ROWS[kind, per_sample][1])(h, 0, C.byref(struct())) == STATE


INSTANCE = {
    "m3_set_point_scene_instance": ("point", "m3_set_point_scene_instance: point_env only", "m3_set_point_scene_instance: -1 (by the values), 0 or 1"),
    "m3_set_weighted_cost_instance": ("point", "m3_set_weighted_cost_instance: point_env only", "m3_set_weighted_cost_instance: -1 (by the weights), 0 or 1"),
    "m3_set_panda_scene_instance": ("panda", "m3_set_panda_scene_instance: panda_env only", "m3_set_panda_scene_instance: -1 (by the values), 0 or 1"),
    "m3_set_panda_weighted_cost_instance": ("panda", "m3_set_panda_weighted_cost_instance: panda_env only",
                                            "m3_set_panda_weighted_cost_instance: -1 (by the weights), 0 or 1"),
}


@pytest.mark.parametrize("name", sorted(INSTANCE))
def test_instance_setter_refusals(lib, handles, name):
    kind, wrong_env, out_of_range = INSTANCE[name]
    fn = getattr(lib, name)
    before = err(lib, None)
    assert fn(None, 0) == BAD_ARG and err(lib, None) == before
    for takes in ("planner", "sim"):
        hw = handles[KIND[kind][2], takes]
        assert fn(hw, 2) == UNSUPPORTED and err(lib, hw) == wrong_env          # (the environment before the value)
        h = handles[kind, takes]
        for on in (-2, 2, 7):
            assert fn(h, on) == BAD_ARG and err(lib, h) == out_of_range, on
        for on in (1, 0, -1):
            assert fn(h, on) == OK


WEIGHTS = {
    "point": ("m3_set_point_cost_weights", "m3_get_point_cost_weights", L.PointCostWeights, L.COST_WEIGHT_DEFAULTS,
              [("nav_dist", NAN, "m3_set_point_cost_weights: nav_dist is not finite"),
               ("push_align", INF, "m3_set_point_cost_weights: push_align is not finite"),
               ("pull_align", -INF, "m3_set_point_cost_weights: pull_align is not finite")],
              "m3_set_point_cost_weights: point_env only"),
    "panda": ("m3_set_panda_cost_weights", "m3_get_panda_cost_weights", L.PandaCostWeights, L.PANDA_COST_WEIGHT_DEFAULTS,
              [("reach_dist", NAN, "m3_set_panda_cost_weights: reach_dist is not finite"),
               ("pick_ori", INF, "m3_set_panda_cost_weights: pick_ori is not finite"),
               ("place_grip", -INF, "m3_set_panda_cost_weights: place_grip is not finite")],
              "m3_set_panda_cost_weights: panda_env only"),
}


@pytest.mark.parametrize("kind", sorted(WEIGHTS))
def test_cost_weight_setter_refusals(lib, handles, kind):
    set_name, get_name, struct, defaults, bad, wrong_env = WEIGHTS[kind]
    setter, getter = getattr(lib, set_name), getattr(lib, get_name)
    out = struct()
    before = err(lib, None)
    assert setter(None, None) == BAD_ARG and getter(None, C.byref(out)) == BAD_ARG and err(lib, None) == before
    for takes in ("planner", "sim"):
        hw = handles[KIND[kind][2], takes]
        assert setter(hw, None) == UNSUPPORTED and err(lib, hw) == wrong_env
        assert getter(hw, C.byref(out)) == UNSUPPORTED and err(lib, hw) == wrong_env
        h = handles[kind, takes]
        first = next(iter(defaults))
        kept = struct(**{**defaults, first: -2.5})              # (any finite value, a negative one too)
        assert setter(h, C.byref(kept)) == OK
        for field, value, text in bad:
            w = struct(**{**defaults, field: value})
            assert setter(h, C.byref(w)) == BAD_ARG and err(lib, h) == text
            assert getter(h, C.byref(out)) == OK and bytes(out) == bytes(kept)
        assert getter(h, None) == BAD_ARG
        assert setter(h, None) == OK and getter(h, C.byref(out)) == OK and bytes(out) == bytes(struct(**defaults))
