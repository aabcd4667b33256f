"""The point_env step mode's view conversions on the device, held to the float64 reference of tests/point_views_ref.py:
SoA world -> views (k_sim_push, k_sim_step, k_episodes_post: write_body13) and views -> SoA world (k_sim_pull,
k_sim_shift_pull, the bound rollout: yaw_from_quat), at yaws near +-pi and +-pi/2 and at the exact pairs, with and without
the unit-norm error of the dynamics' renormalisation.  n in {1, 63, 65, 257}: a ragged tail on the 64-wide step kernels and
on the 256-wide pull / push / shift kernels.  Tolerances: tests/test_point_views_cpu.py derives them; positions, velocities
and every element that must not be written are compared bit for bit."""
import numpy as np
import pytest

from tests import point_views_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = np.float32
U = np.uint32
SIZES = [1, 63, 65, 257]
VIEWS = ("dof_state", "root_state", "rigid_body_state", "net_contact_force")
YAWS = (np.pi - 1e-3, -np.pi + 3e-4, 0.5 * np.pi)       # the hand-off's and the episodes' box yaws


def make_sim(n):
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    sim = IsaacGymWrapper(IsaacGymConfig(dt=0.05), "point_env", num_envs=n)
    sim._engine.use_torch_stream()
    return sim, sim._engine.buffer(L.BUF_SIM_WORLD)


def world_rows(n, moving, seed=5):
    """f32 [28][n]: one edge yaw per environment for the box, another for the dyn-obs; distinct positions, apart from each
    other, the obstacle and the walls; moving: distinct velocities, pending and contact forces (else zero: a world at rest)"""
    rng = np.random.default_rng(seed)
    w = np.zeros((R.ROWS_WORLD, n), F)
    w[0:2] = rng.uniform(-3.2, -1.2, (2, n))                        # robot
    w[4], w[5] = rng.uniform(0.5, 3.0, n), rng.uniform(-3.2, -1.0, n)   # box
    w[11], w[12] = rng.uniform(-3.2, -1.0, n), rng.uniform(0.8, 3.2, n)  # dyn-obs
    cs = R.edge_cs(n + 11)
    w[6:8], w[13:15] = cs[:n].T, cs[11:].T
    if moving:
        for rows in ((2, 3), (8, 9, 10), (15, 16, 17), range(18, 28)):
            for r in rows:
                w[r] = rng.uniform(0.1, 2.0, n) * rng.choice([-1.0, 1.0], n)
    return w


def put_sentinels(sim):
    sent = {}
    for name in VIEWS:
        t = getattr(sim, "_" + name)
        t.copy_((7.25 + torch.arange(t.numel(), dtype=torch.float64)).to(torch.float32).reshape(t.shape))
        sent[name] = t.cpu().numpy().copy()
    return sent


def read_views(sim):
    torch.cuda.synchronize()
    return {name: getattr(sim, "_" + name).cpu().numpy() for name in VIEWS}


def check_quat(q, c, s, what):
    """the three assertions of the CPU test on quaternions [..., 2] = (qz, qw) of the yaws (c, s)"""
    q = q.astype(np.float64)
    err = R.quat_error(q[..., 0], q[..., 1], c, s)
    print(f"{what}: max |q - q64| = {err.max():.3e}")
    i = np.unravel_index(int(np.argmax(np.where(np.isnan(err), np.inf, err))), err.shape)
    assert (err <= R.TOL_Q).all(), f"{what}: |q - q64| = {err[i]:.3e} > {R.TOL_Q:.3e} at (c, s) = ({c[i]!r}, {s[i]!r}): q = {q[i]}"
    nrm = np.abs(q[..., 0] ** 2 + q[..., 1] ** 2 - 1.0)
    assert (nrm <= R.TOL_NORM).all(), f"{what}: | |q|^2 - 1 | = {nrm.max():.3e} > {R.TOL_NORM:.3e}"
    assert (q[..., 1] >= 0).all() and not np.signbit(q[..., 1]).any(), f"{what}: qw < 0"
    back = R.yaw_of_quat(q[..., 0], q[..., 1])
    cu, su = R.unit(c, s)
    trip = np.maximum(np.abs(back[0] - cu), np.abs(back[1] - su))
    assert (trip <= R.TOL_TRIP).all(), f"{what}: the yaw of q is {trip.max():.3e} > {R.TOL_TRIP:.3e} from the world's"


def check_views(got, world, sent, what):
    """every element the reference lists as written equals it (quaternions of the turning bodies: check_quat); every other
    element still holds its sentinel"""
    want = R.views_of_world(world)
    actor, body = R._names()[:2]
    for name in VIEWS:
        g, w = got[name], want[name]
        assert g.shape == w.shape, (name, g.shape, w.shape)
        keep = np.isnan(w)
        turning = np.zeros(w.shape, bool)
        if name in ("root_state", "rigid_body_state"):
            for b in ("box", "dyn-obs"):
                turning[:, (actor if name == "root_state" else body)[b], 5:7] = True
        assert (~keep).any() and (keep.any() or name == "dof_state"), name      # (dof_state is written whole)
        assert np.array_equal(g[keep].view(U), sent[name][keep].view(U)), \
            f"{what}: {name}: {int((g[keep].view(U) != sent[name][keep].view(U)).sum())} elements that must not be written changed"
        exact = ~keep & ~turning
        neq = g[exact].view(U) != w[exact].astype(F).view(U)
        assert not neq.any(), f"{what}: {name}: {int(neq.sum())} written elements differ, first {g[exact][neq][0]!r} != {w[exact][neq][0]!r}"
    for name, index in (("root_state", actor), ("rigid_body_state", body)):
        for b, r0 in (("box", R.BOX), ("dyn-obs", R.DYN)):
            check_quat(got[name][:, index[b], 5:7], world[r0 + 2].astype(np.float64), world[r0 + 3].astype(np.float64),
                       f"{what}: {name}[{b}]")


@pytest.mark.parametrize("n", SIZES)
def test_push_writes_the_reference_views_and_nothing_else(n):
    sim, soa = make_sim(n)
    try:
        w = world_rows(n, moving=True)
        soa.copy_(torch.from_numpy(w))
        sent = put_sentinels(sim)
        sim._engine.sim_push_state()
        check_views(read_views(sim), w, sent, f"push n={n}")
    finally:
        sim.stop_sim()


@pytest.mark.parametrize("n", SIZES)
def test_step_of_a_world_at_rest_writes_the_reference_views(n):
    sim, soa = make_sim(n)
    try:
        w = world_rows(n, moving=False)
        soa.copy_(torch.from_numpy(w))
        sent = put_sentinels(sim)
        sim.set_dof_velocity_target_tensor(torch.zeros(n, 2, device="cuda:0"))
        sim.step()
        got = read_views(sim)
        after = soa.cpu().numpy()
        # nothing moves, so the dynamics leaves the orientations alone: the edge yaws are what the step's view writer gets
        for r in (6, 7, 13, 14):
            assert np.array_equal(after[r].view(U), w[r].view(U)), r
        assert np.array_equal(after[[0, 1, 4, 5, 11, 12]], w[[0, 1, 4, 5, 11, 12]])
        check_views(got, after, sent, f"step n={n}")
    finally:
        sim.stop_sim()


def fresh_views(sim, n, seed=9):
    """float32-rounded float64 quaternions of the edge yaws and fresh positions, velocities in dof_state and root_state"""
    rng = np.random.default_rng(seed)
    actor = R._names()[0]
    dof = rng.uniform(-3, 3, (n, 4)).astype(F)
    root = sim._root_state.cpu().numpy().copy()
    cs = R.edge_cs(n + 5).astype(np.float64)
    for b, off in (("box", 0), ("dyn-obs", 5)):
        yaw = np.arctan2(cs[off:off + n, 1], cs[off:off + n, 0])
        row = root[:, actor[b]]
        row[:, 0:2] = rng.uniform(-3, 3, (n, 2))
        row[:, 5], row[:, 6] = np.sin(0.5 * yaw), np.cos(0.5 * yaw)
        row[:, 7:9] = rng.uniform(-1, 1, (n, 2))
        row[:, 12] = rng.uniform(-2, 2, n)
    return dof, root


def check_world(after, before, dof, root, what):
    want = R.world_of_views(dof, root)
    for r in range(18):
        if r in (6, 7, 13, 14):
            err = np.abs(after[r].astype(np.float64) - want[r])
            assert (err <= R.TOL_Q).all(), f"{what}: SoA row {r}: {err.max():.3e} > {R.TOL_Q:.3e}"
        else:
            assert np.array_equal(after[r].view(U), want[r].astype(F).view(U)), f"{what}: SoA row {r}"
    assert np.array_equal(after[18:].view(U), before[18:].view(U)), f"{what}: a pull touched the pending or contact forces"


@pytest.mark.parametrize("n", SIZES)
def test_pull_and_shift_give_the_reference_world(n):
    sim, soa = make_sim(n)
    try:
        before = np.ascontiguousarray(7.25 + np.arange(R.ROWS_WORLD * n, dtype=np.float64).reshape(R.ROWS_WORLD, n), F)
        soa.copy_(torch.from_numpy(before))
        dof, root = fresh_views(sim, n)
        sim._dof_state.copy_(torch.from_numpy(dof))
        sim.set_actor_root_state_tensor(torch.from_numpy(root).to("cuda:0"))
        torch.cuda.synchronize()
        assert np.array_equal(sim._root_state.cpu().numpy().view(U), root.view(U))       # (a pull leaves the views alone)
        check_world(soa.cpu().numpy(), before, dof, root, f"pull n={n}")
        # the shift: present in the view and in the SoA world
        row = R._names()[0]["dyn-obs"]
        d = (F(0.01), F(-0.37), F(0.125))
        sim._engine.sim_shift_actor(row, *map(float, d))
        torch.cuda.synchronize()
        shifted = root.copy()
        for k in range(3):
            shifted[:, row, k] = root[:, row, k] + d[k]
        assert np.array_equal(sim._root_state.cpu().numpy().view(U), shifted.view(U))
        check_world(soa.cpu().numpy(), before, dof, shifted, f"shift n={n}")
        assert not np.array_equal(shifted[:, row, 0], root[:, row, 0])
    finally:
        sim.stop_sim()


def handoff_world(oracle, yaw):
    """oracle world: the robot against the box's lower face and moving into it, so that the box's yaw enters the contact"""
    w = oracle.init_world(1)[0]
    w[0:2], w[4:6] = (0.05, 1.62), (0.3, 1.5)
    w[oracle.W_B + 2], w[oracle.W_B + 3] = np.cos(yaw), np.sin(yaw)
    return w


def raw18(w31):
    w = np.asarray(w31, F)
    return np.concatenate([w[[0, 1, 4, 5]], w[7:14], w[14:21]])


def test_hand_off_of_the_world_to_a_planner(oracle):
    """The closed loop's path: world A's views -> a planner wrapper's SoA world (pull) and -> a bound rollout."""
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.engine import HipEngine, make_config
    K, T = 64, 3
    A, soa_a = make_sim(1)
    B, soa_b = make_sim(65)
    actor = R._names()[0]
    # (T = 3 is below the filter's window)
    engs = [HipEngine(make_config(K=K, T=T, nu=2, filter_u=False, u_min=[-3, -3], u_max=[3, 3], noise_sigma_diag=[3, 3]))
            for _ in range(2)]
    try:
        for e in engs:
            e.use_torch_stream()
            e.set_objective("push", (-1.0, -1.0))
            e.set_noise(np.zeros((K, T, 2), F))
        bound, raw = engs
        bound.bind_sim_point(A._dof_state, A._root_state, actor["box"], actor["dyn-obs"])
        ocfg = oracle.make_cfg(K, T, 2, task="push", goal=(-1.0, -1.0), filter_u=False)
        for yaw in YAWS:
            w31 = handoff_world(oracle, yaw)
            a18 = raw18(w31)
            soa_a[:18, 0].copy_(torch.from_numpy(a18))
            A._engine.sim_push_state()
            cu, su = R.unit(w31[oracle.W_B + 2], w31[oracle.W_B + 3])
            # planner wrapper B adopts A's row, broadcast (what the planner side of a closed loop does every tick)
            B._root_state[:] = A._root_state
            B._dof_state[:] = A._dof_state
            B.set_dof_state_tensor(B._dof_state)
            B.set_actor_root_state_tensor(B._root_state)
            torch.cuda.synchronize()
            b = soa_b.cpu().numpy()
            err = max(np.abs(b[6] - cu).max(), np.abs(b[7] - su).max())
            print(f"yaw {yaw!r}: planner (c, s) off by {err:.3e}")
            assert err <= R.TOL_TRIP, f"yaw {yaw!r}: the planner's (c, s) is {err:.3e} > {R.TOL_TRIP:.3e} from the world's"
            rest = [r for r in range(18) if r not in (6, 7)]
            assert np.array_equal(b[rest].view(U), np.repeat(a18[rest, None], 65, 1).view(U))
            # the bound rollout against the oracle run from the float64-normalised (c, s); the states record the robot only, so
            # the trajectory cost is compared as well.  Tolerance: twice the oracle's own spread over (c, s) moved by up to 2^-19.
            runs = []
            for dc in (-1.0, -0.5, 0.0, 0.5, 1.0):
                for ds in (-1.0, -0.5, 0.0, 0.5, 1.0):
                    wp = w31.copy()
                    wp[oracle.W_B + 2], wp[oracle.W_B + 3] = cu + dc * R.TOL_TRIP, su + ds * R.TOL_TRIP
                    opl = oracle.OraclePointPlanner(ocfg, np.zeros((K, T, 2), F))
                    opl.command(wp)
                    runs.append((opl.last["J"].astype(np.float64), opl.last["states"][:, 0].astype(np.float64)))
            J0, S0 = runs[12]
            tol_J = 2.0 * max(np.abs(J - J0).max() for J, _ in runs)
            tol_S = 2.0 * max(np.abs(S - S0).max() for _, S in runs)
            w0 = w31.copy()
            w0[oracle.W_B + 2], w0[oracle.W_B + 3] = cu, su
            for e, name in ((raw, "raw"), (bound, "bound")):
                e.reset()
                if e is raw:
                    e.set_world_point_raw(raw18(w0))
                e.command(sync_host=True)
                J = e.buffer(L.BUF_TRAJ_COST).cpu().numpy().astype(np.float64)
                S = e.states.cpu().numpy()[:, 0].astype(np.float64)
                dJ, dS = np.abs(J - J0).max(), np.abs(S - S0).max()
                print(f"yaw {yaw!r} {name}: |J - oracle| = {dJ:.3e} (oracle spread x 2 = {tol_J:.3e}), first state {dS:.3e} ({tol_S:.3e})")
                if e is raw:        # the same binary32 world: the oracle's bits
                    assert dJ == 0.0 and dS == 0.0, (yaw, dJ, dS)
                else:
                    assert dJ <= tol_J, f"yaw {yaw!r}: trajectory cost {dJ:.3e} from the oracle's, twice its spread is {tol_J:.3e}"
                    assert dS <= tol_S, f"yaw {yaw!r}: first state {dS:.3e} from the oracle's, twice its spread is {tol_S:.3e}"
    finally:
        for e in engs:
            e.close()
        A.stop_sim()
        B.stop_sim()


def test_lockstep_episode_traces_carry_the_reference_quaternion():
    """k_episodes_post: the trace row of a tick holds the box quaternion of the views, written by the push before tick 0 and by
    the post kernel's step after it; both against the SoA world they were written from, and against the yaw that was set --
    there with the round trip of the pre kernel's pull on top (2^-19 in (c, s), so 2^-20 in a half-angle component)."""
    from m3p2i_aip_amd import _lib as L
    from m3p2i_aip_amd.episodes import build_set
    es = build_set([("config_point", ["task=push", "goal=[-3,3]"], None)] * 3, max_ticks=2, trace=True)
    try:
        real = es.real
        ib = int(real._get_actor_index_by_name("box"))
        yaw = np.array(YAWS)
        real._root_state[:, ib, 5] = torch.from_numpy(np.sin(0.5 * yaw).astype(F)).to("cuda:0")
        real._root_state[:, ib, 6] = torch.from_numpy(np.cos(0.5 * yaw).astype(F)).to("cuda:0")
        real.set_actor_root_state_tensor(real._root_state)
        real._engine.sim_push_state()
        soa = real._engine.buffer(L.BUF_SIM_WORLD)
        torch.cuda.synchronize()
        held = [soa.cpu().numpy()[6:8].astype(np.float64)]
        es.start()                                       # tick 0
        torch.cuda.synchronize()
        held.append(soa.cpu().numpy()[6:8].astype(np.float64))
        while es.running:
            es.tick()
        st, tr = es.eps.status(with_trace=True)
        assert es.eps.ticks_done == 2 and all(s["done_tick"] == 1 and not s["success"] for s in st), st
        for t in range(2):
            check_quat(tr[t, :, 4:6], held[t][0], held[t][1], f"trace tick {t}")
            err = R.quat_error(tr[t, :, 4], tr[t, :, 5], np.cos(yaw), np.sin(yaw))
            assert (err <= R.TOL_Q + 0.5 * t * R.TOL_TRIP).all(), (t, err)
    finally:
        es.close()
