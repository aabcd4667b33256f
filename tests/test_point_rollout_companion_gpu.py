"""The two-wavefront form of the point_env rollout (dynamics wavefront + companion wavefront; rollout_point_kernel.hpp:
rollout_point_body2, DESIGN.md section 6 "Companion wavefront").  Every case makes two handles that differ only in
m3_set_point_rollout_form (0 and 1), runs the same commands on both and compares the BITS of everything a command leaves.

Shapes: T = 12 (the shortest horizon the Halton spline accepts) and K in {64, 65, 100}: one exact wavefront, one lane in a
second workgroup, a partial wavefront -- whose last lane is the `is_last` / null-action sample.  K = 1 (a lone lane) is below
what a planner handle accepts (K >= 20: the top-k), so that case is a shard of one sample -- the LAST one, again the
null-action sample -- and compares what m3_rollout leaves.
Scenes: the handles' initial scene, and the corner scene of bench.py's corner_scene (box in the wall corner, dyn-obs beside
it, the robot on top: every pair inside its broad-phase range, so the rare substep instances run under the form).
World source: world0 (m3_set_world_point_raw) and the bound simulator tensors (sim_dof)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipEngine, make_config  # noqa: E402

PK = dict(u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3])
T = 12
BOX_ACTOR, DYN_ACTOR, N_ACTORS = 6, 5, 11
COMMAND_BUFS = dict(states=L.BUF_STATES, actions=L.BUF_ACTIONS, cost_horizon=L.BUF_COST_HORIZON, cost_total=L.BUF_TRAJ_COST,
                    weights=L.BUF_WEIGHTS, plan=L.BUF_ACTION_OUT, mean=L.BUF_MEAN, pending=L.BUF_PENDING_FORCE)
ROLLOUT_BUFS = {k: COMMAND_BUFS[k] for k in ("states", "actions", "cost_horizon", "cost_total", "pending")}
GOALS = dict(navigation=(2.0, -2.0), push=(-1.0, -1.0), pull=(0.0, 0.0))


def _scene(name, call):
    """raw world: robot x y vx vy | box x y c s vx vy w | dyn-obs x y c s vx vy w; moved a little every call"""
    w = np.zeros(18, np.float32)
    if name == "corner":       # bench.py corner_scene: walls' inner faces at +-3.95, boxes 0.4 x 0.4, robot radius 0.2, 5 mm gaps
        w[0:2] = (-3.745, -3.34)
        w[4:7] = (-3.745, -3.745, 1.0)
        w[11:14] = (-3.34, -3.745, 1.0)
    else:                      # the initial scene of a fresh handle's neighbourhood: robot above the box, dyn-obs away
        w[0:2] = (0.1 + 0.05 * call, 0.5 - 0.04 * call)
        w[2:4] = (0.2, -0.1)
        w[4:7] = (0.1, 0.0 - 0.03 * call, 1.0)
        w[11:14] = (-2.0 + 0.1 * call, 2.0, 1.0)
        w[15] = -0.2
    return w


class Pair:
    """Two handles made the same way but for the rollout form: engs[0] form 0, engs[1] form `form`."""

    def __init__(self, K, task, scene="initial", bind=False, form=1, T=T, lanes=None, weights=None, K_global=None, k_offset=0,
                 **cfg_kw):
        self.scene, self.bind, self.engs = scene, bind, []
        if bind:
            self.dof = torch.zeros(1, 4, device="cuda:0")
            self.root = torch.zeros(1, N_ACTORS, 13, device="cuda:0")
            self.root[..., 6] = 1.0
        for f in (0, form):
            shard = dict(K_local=K, k_offset=k_offset) if K_global else {}
            e = HipEngine(make_config(K=K_global or K, T=T, nu=2, **shard, **PK, **cfg_kw))
            if not (e.cfg.sampling_random or e.cfg.mode_simple):
                e.set_noise_halton(T // 4, 2, 0.5, "none")
            e.set_objective(task, GOALS[task])
            e.set_point_rollout_form(f)
            if lanes:
                e.set_rollout_lanes(lanes)
            if weights:
                e.set_point_cost_weights(weights)
            if bind:
                e.bind_sim_point(self.dof, self.root, BOX_ACTOR, DYN_ACTOR)
            assert e.point_rollout_form_used() == -1
            self.engs.append(e)

    def set_world(self, call):
        w = _scene(self.scene, call)
        if not self.bind:
            for e in self.engs:
                e.set_world_point_raw(w)
            return
        self.dof[0] = torch.tensor([w[0], w[2], w[1], w[3]])
        for actor, o in ((BOX_ACTOR, 4), (DYN_ACTOR, 11)):
            half = math.atan2(float(w[o + 3]), float(w[o + 2])) / 2
            self.root[0, actor, 0:2] = torch.tensor(w[o:o + 2])
            self.root[0, actor, 3:7] = torch.tensor([0.0, 0.0, math.sin(half), math.cos(half)])
            self.root[0, actor, 7:9] = torch.tensor(w[o + 4:o + 6])
            self.root[0, actor, 12] = float(w[o + 6])

    def run(self, calls=3, rollout_only=False):
        bufs = ROLLOUT_BUFS if rollout_only else COMMAND_BUFS
        for c in range(calls):
            self.set_world(c)
            for e in self.engs:
                e.rollout() if rollout_only else e.command()
            torch.cuda.synchronize()
            a, b = self.engs
            for name, which in bufs.items():
                x, y = a.buffer(which), b.buffer(which)
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"call {c}: {name} differs between the forms"
            assert torch.isfinite(a.buffer(L.BUF_TRAJ_COST)).all()
            if not rollout_only:
                assert bytes(a.info()) == bytes(b.info()), f"call {c}: m3_info differs"
        return [e.point_rollout_form_used() for e in self.engs]

    def close(self):
        for e in self.engs:
            e.close()


@pytest.fixture
def pair():
    made = []

    def make(*a, **kw):
        made.append(Pair(*a, **kw))
        return made[-1]
    yield make
    for p in made:
        p.close()


@pytest.mark.parametrize("bind", [False, True], ids=["world0", "sim_dof"])
@pytest.mark.parametrize("scene", ["initial", "corner"])
@pytest.mark.parametrize("task", ["navigation", "push"])
def test_three_commands_leave_the_same_bits_in_both_forms(pair, task, scene, bind):
    for K in (64, 65, 100):
        assert pair(K, task, scene, bind).run() == [0, 1], K


@pytest.mark.parametrize("scene", ["initial", "corner"])
@pytest.mark.parametrize("task", ["navigation", "push"])
def test_a_lone_lane(pair, task, scene):
    """K_local = 1: the last sample of K_global = 64 (the null-action sample), rollouts only (a shard has no m3_command)"""
    assert pair(1, task, scene, K_global=64, k_offset=63).run(rollout_only=True) == [0, 1]


@pytest.mark.parametrize("task", ["navigation", "push"])
def test_other_solver_settings_run_the_build_with_the_scene_as_an_argument(pair, task):
    """not the reference's substeps / solver passes: k_rollout_point2 instead of k_rollout_point2_ref"""
    assert pair(100, task, "corner", substeps=3, solver_iters=4).run() == [0, 1]


def test_thirty_two_lanes_per_wavefront(pair):
    """K = 100 over four half-filled workgroups; the form is whatever the rule gives for a forced 1: the form exists"""
    assert pair(100, "push", lanes=32).run() == [0, 1]


def test_automatic_rule_takes_the_form_where_it_was_measured_to_pay(pair):
    """form -1 (the default) against form 0: same bits whichever it picks; the pick is a form the library knows"""
    used = pair(100, "push", form=-1).run()
    assert used[0] == 0 and used[1] in (0, 1)


@pytest.mark.parametrize("case", ["pull", "general_instance", "weights", "tables_do_not_fit"])
def test_fall_backs_keep_the_one_wavefront_kernel(pair, case):
    kw = dict(pull=dict(K=64, task="pull"),
              general_instance=dict(K=64, task="push", mode_simple=True, sampling_random=True, u_per_command=10),
              weights=dict(K=64, task="push", weights=dict(push_align=2.5)),
              tables_do_not_fit=dict(K=64, task="push", T=40))[case]    # 16 + 40 * 2048 bytes > 64 KB of LDS
    assert pair(**kw).run() == [0, 0]


def test_knob_refuses_other_values():
    e = HipEngine(make_config(K=64, T=T, nu=2, **PK))
    try:
        for bad in (2, -2):
            with pytest.raises(L.M3Error):
                e.set_point_rollout_form(bad)
    finally:
        e.close()
