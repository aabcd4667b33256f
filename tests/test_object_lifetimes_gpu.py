"""Every C object gives back what it took: m3_owned_blocks_live() -- the entries of all ledgers of the process
(m3p2i_aip_amd/csrc/owned_blocks.hpp) -- rises when an object is created, does not move across the second call of an entry
point that allocates lazily, and is exactly back at its start once the objects are closed in the order a user closes them;
three cycles end where they began.  (Device-wide free memory is not used: other tenants of the card move it.)  The counts are
asserted as "rises" and "returns" only: exact counts would pin the allocation layout."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from m3p2i_aip_amd import _lib as L  # noqa: E402
from m3p2i_aip_amd.engine import HipBatch, HipEngine, HipEpisodes, HipPandaEpisodes, make_config  # noqa: E402
from tests.test_batch_command_gpu import PK  # noqa: E402
from tests.test_batch_panda_gpu import GOALS, PK as PANDA_PK  # noqa: E402

K, T = 64, 12


def live():
    return int(L.load().m3_owned_blocks_live())


def created(make):
    """make() with the count risen by at least 1"""
    n = live()
    obj = make()
    assert live() >= n + 1, (n, live())
    return obj


def twice(call):
    """a lazily allocating entry point: whatever the first call took, the second identical call takes nothing"""
    call()
    n = live()
    call()
    assert live() == n, (n, live())


def noise(k, nu, seed):
    return np.random.default_rng(seed).standard_normal((k, T, nu)).astype(np.float32)


def point_planner(k=K, seed=1):
    e = created(lambda: HipEngine(make_config(K=k, T=T, nu=2, **PK)))
    e.set_objective("push", (-3.0, 3.0))
    twice(lambda: e.set_noise(noise(k, 2, seed)))            # from the host: the staging block
    e.set_action_out(torch.zeros(T, 2, device="cuda:0"))
    return e


def panda_planner(seed=1):
    e = created(lambda: HipEngine(make_config(K=K, T=T, nu=9, env_type="panda_env", **PANDA_PK)))
    e.set_objective("reach", GOALS["reach"], gripper_cmd=1)
    twice(lambda: e.set_noise(noise(K, 9, seed)))
    e.set_action_out(torch.zeros(T, 9, device="cuda:0"))
    return e


def cycle_point_planner():
    e = point_planner()
    twice(lambda: e.set_point_rollout_scenes([dict(obs_x=-1.0 + 0.01 * i) for i in range(K)]))
    assert e.point_rollout_scenes_set()
    twice(lambda: e.enable_timing(True))
    twice(e.rollout)
    twice(e.command)
    assert e.timing().total_ms > 0.0
    e.close()
    # the wavefront order exists from K_local = 128: its three blocks come with the first rollout
    e = point_planner(k=128, seed=2)
    n = live()
    e.rollout()
    assert live() > n
    twice(e.rollout)
    torch.cuda.synchronize()
    e.close()


def cycle_panda_planner():
    e = panda_planner()
    twice(e.command)
    torch.cuda.synchronize()
    e.close()


def cycle_regen_shards():
    kw = dict(K=2 * K, K_local=K, T=T, nu=2, multi_modal=True, shard_mix=2, **PK)
    shards = [created(lambda r=r: HipEngine(make_config(k_offset=r * K, **kw))) for r in range(2)]
    delta = noise(2 * K, 2, 3)
    for e in shards:
        assert e.needs_global_noise
        twice(lambda: e.set_noise(delta))                    # a global upload: a temporary, gone when the call returns
    n = live()
    shards[0].p2p_connect_local(shards)                      # every peer's exchange block comes to life here
    assert live() >= n + 2
    for e in shards:
        twice(lambda: e.p2p_connect_local(shards))
        assert e.p2p_status()[0] == -1
    for e in shards:
        e.close()


def cycle_point_world():
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    n_rows = 4
    sim = created(lambda: IsaacGymWrapper(IsaacGymConfig(dt=0.05), "point_env", num_envs=n_rows))
    world = sim._engine
    twice(lambda: world.set_point_scene_rows([dict(obs_x=-1.0 + 0.1 * i) for i in range(n_rows)]))
    batch = created(lambda: HipBatch(n_rows))
    planners = [point_planner(seed=10 + i) for i in range(n_rows)]
    spec = [("push", (-3.0, 3.0), 0, L.SUCTION_OFF, 400.0)] * n_rows
    eps = created(lambda: HipEpisodes(world, planners, spec, max_ticks=10))
    twice(lambda: eps.tick(batch))
    assert eps.ticks_done == 2
    eps.close()
    batch.close()
    for e in planners:
        e.close()
    world.close()


def cycle_panda_world():
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    n_rows = 2
    sim = created(lambda: IsaacGymWrapper(IsaacGymConfig(dt=0.01), "panda_env", num_envs=n_rows))
    world = sim._engine
    batch = created(lambda: HipBatch(n_rows))
    planners = [panda_planner(seed=20 + i) for i in range(n_rows)]
    eps = created(lambda: HipPandaEpisodes(world, planners, max_ticks=10, settle_ticks=0))
    eps.observe()
    eps.act_first([world] * n_rows, [0] * n_rows)            # tick 0 commands nothing (the world's kept targets stand in)

    def tick():
        eps.observe()
        eps.act(batch, [0] * n_rows)

    twice(tick)
    assert eps.ticks_done == 3
    torch.cuda.synchronize()
    eps.close()
    batch.close()
    for e in planners:
        e.close()
    world.close()


@pytest.mark.parametrize("cycle", [cycle_point_planner, cycle_panda_planner, cycle_regen_shards, cycle_point_world, cycle_panda_world],
                         ids=lambda f: f.__name__[6:])
def test_the_live_count_rises_with_an_object_and_returns_when_it_is_closed(cycle):
    gc.collect()     # (engines that earlier tests left unreferenced give their blocks back now, not in the middle of a cycle)
    start = live()
    for _ in range(3):
        cycle()
        assert live() == start, (start, live())
