"""What a planner's _bind_world tells its engine about the scene rows of the wrapper it follows, for both kinds of scene (the
point_env arena, the panda_env workspace), on a recording stand-in engine and wrapper: the engine calls of every step of one
sequence, as literals.  No GPU, no library."""
import pytest


class _Engine:
    """records (method, argument) of the four calls a planner makes about scenes"""

    def __init__(self):
        self.calls = []

    def _record(self, name, arg):
        self.calls.append((name, list(arg) if isinstance(arg, list) else arg))

    def set_point_scene(self, scene=None, **kw):
        self._record("set_point_scene", scene)

    def set_panda_scene(self, scene=None, **kw):
        self._record("set_panda_scene", scene)

    def set_point_rollout_scenes(self, rows=None):
        self._record("set_point_rollout_scenes", rows)

    def set_panda_rollout_scenes(self, rows=None):
        self._record("set_panda_rollout_scenes", rows)


class _Sim:
    num_envs = 4


# env_type, the wrapper's single scene and rows, the planner's own rows, the engine's two setters, a field of the kind
KINDS = {
    "point": ("point_env", "point_scene", "point_scenes", "_rollout_scenes", "set_point_scene", "set_point_rollout_scenes", "mu_rb"),
    "panda": ("panda_env", "panda_scene", "panda_scenes", "_panda_rollout_scenes", "set_panda_scene", "set_panda_rollout_scenes", "mu"),
}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_bind_world_pushes_the_followed_rows_once_and_again_only_for_a_reason(kind):
    from m3p2i_aip_amd import planner
    env_type, sim_scene, sim_rows, own_rows, set_scene, set_rows, f = KINDS[kind]
    sim = _Sim()
    p = object.__new__(planner.MPPI)
    p.env_type, p.K, p.K_local, p.k_offset = env_type, 8, 4, 4       # the second shard of two
    p._engine, p._sim, p._bound_sim = _Engine(), sim, sim             # (the binding of the views is not what this is about)
    calls = p._engine.calls

    def bind():
        del calls[:]
        p._bind_world()
        return list(calls)

    # the wrapper has one environment per local sample and rows: they are followed, pushed once
    setattr(sim, sim_rows, [{f: 0.1}, {f: 0.2}, None, {f: 0.4}])
    assert bind() == [(set_rows, [{f: 0.1}, {f: 0.2}, None, {f: 0.4}])]
    # the same list again: nothing
    assert bind() == []
    # an equal but distinct list: nothing
    setattr(sim, sim_rows, [{f: 0.1}, {f: 0.2}, None, {f: 0.4}])
    assert bind() == []
    # the single scene changes: the scene, then the rows again (the single scene cleared the library's)
    setattr(sim, sim_scene, {f: 0.5})
    assert bind() == [(set_scene, {f: 0.5}), (set_rows, [{f: 0.1}, {f: 0.2}, None, {f: 0.4}])]
    assert bind() == []
    # the wrapper loses its rows while the planner has rows of its own (the global list): its shard's slice
    setattr(p, own_rows, [{f: 1.0}, {f: 1.1}, {f: 1.2}, {f: 1.3}, {f: 1.4}, {f: 1.5}, {f: 1.6}, {f: 1.7}])
    setattr(sim, sim_rows, None)
    assert bind() == [(set_rows, [{f: 1.4}, {f: 1.5}, {f: 1.6}, {f: 1.7}])]
    assert bind() == []
    # ... and the same without rows of its own: the rows are cleared
    setattr(sim, sim_rows, [{f: 0.7}, None, None, None])
    assert bind() == [(set_rows, [{f: 0.7}, None, None, None])]
    setattr(p, own_rows, None)
    setattr(sim, sim_rows, None)
    assert bind() == [(set_rows, None)]
    assert bind() == []
    # follow_sim_scene = False: nothing, whatever the wrapper holds
    p.follow_sim_scene = False
    setattr(sim, sim_rows, [{f: 0.9}, {f: 0.9}, {f: 0.9}, {f: 0.9}])
    setattr(sim, sim_scene, {f: 0.6})
    assert bind() == []
