"""The planar contact dynamics spec against MECHANICS, not against its own twin.

PhysX cannot be pinned; HIP == oracle bit for bit only says that two implementations of one written
spec agree.  These tests anchor the spec itself to closed-form answers a rigid-body simulator with the reference's
parameters (isaacgym_wrapper.py:10-31, :341-344, pointRobot.urdf, config/point_env/*.yaml) has to give:
implicit velocity drive, Coulomb ground friction, inelastic impacts that conserve linear and angular momentum and never
create energy, the drive / friction force balance of a steady push, bounded penetration under the drive's full effort,
mirror symmetry.  The CPU tests run the oracle; the `gpu` tests run the same scenes through the product
(`IsaacGymWrapper.step()` -> `m3_sim_step`, the kernel the rollouts share their substep with)."""
import numpy as np
import pytest

H, MU_B, G, M_BOX, M_ROBOT, D_DRIVE = 0.025, 0.75, 9.8, 16.0, 10.0, 600.0


def lonely_box(O, box, robot=(3.0, -3.0), dyn=(-3.0, -3.0)):
    w = O.init_world(1)
    w[0, 0:2] = robot
    w[0, O.W_B:O.W_B + 7] = box
    w[0, O.W_D:O.W_D + 7] = [dyn[0], dyn[1], 1, 0, 0, 0, 0]
    return w


# ---------------------------------------------------------------- closed forms (shared by the CPU and the GPU tests)
def drive_response(n_steps, u):
    """m dv/dt = D (u - v), implicit Euler per substep: v' = (v + a u) / (1 + a), a = h D / m = 1.5."""
    a = H * D_DRIVE / M_ROBOT
    return np.asarray(u, np.float64) * (1.0 - (1.0 / (1.0 + a)) ** (2 * n_steps))


def slide(v0, n_steps):
    """Coulomb friction on a sliding box: v -= mu g h per substep, clamped at rest; x += h v."""
    v, x, out = float(v0), 0.0, []
    for _ in range(n_steps):
        for _ in range(2):
            v = max(0.0, v - MU_B * G * H)
            x += H * v
        out.append((x, v))
    return np.asarray(out)


# ---------------------------------------------------------------- CPU: the oracle
def test_velocity_drive_is_the_implicit_damper(oracle):
    O = oracle
    sc = O.default_scene()
    w = lonely_box(O, [3.0, 3.0, 1, 0, 0, 0, 0], robot=(0.0, 0.0))
    u = np.array([[3.0, -1.5]], np.float32)
    for n in range(1, 7):
        O.step_batch(sc, w, u)
        np.testing.assert_allclose(w[0, 4:6], drive_response(n, u[0]), rtol=2e-6)
    # effort limit (pointRobot.urdf:35,43: 1000 N): a 10 m/s request from rest is clamped to F_max h / m per substep
    w = lonely_box(O, [3.0, 3.0, 1, 0, 0, 0, 0], robot=(0.0, 0.0))
    sc2 = O.default_scene()
    sc2.drive_fmax = 100.0
    O.step_batch(sc2, w, np.array([[3.0, 0.0]], np.float32))
    np.testing.assert_allclose(w[0, 4], 2 * 100.0 * H / M_ROBOT, rtol=1e-6)


def test_ground_friction_is_coulomb(oracle):
    O = oracle
    sc = O.default_scene()
    w = lonely_box(O, [0, 0, 1, 0, 2.0, 0, 0])
    z = np.zeros((1, 2), np.float32)
    want = slide(2.0, 8)
    for n in range(8):
        O.step_batch(sc, w, z)
        np.testing.assert_allclose(w[0, O.W_B + 4], want[n, 1], atol=2e-6)
        np.testing.assert_allclose(w[0, O.W_B + 0], want[n, 0], atol=2e-6)
    assert w[0, O.W_B + 4] == 0.0                       # comes to rest exactly (no creep, no sign flip)
    assert abs(w[0, O.W_B + 0] - 2.0 ** 2 / (2 * MU_B * G)) < 0.03     # ~ v0^2 / (2 mu g), up to the discretisation
    # spinning in place: the friction torque mu m g r_eq decelerates at a constant rate and stops the box
    w = lonely_box(O, [0, 0, 1, 0, 0, 0, 3.0])
    alpha_h = MU_B * M_BOX * G * sc.box_req / sc.box_I * H
    O.step_batch(sc, w, z)
    np.testing.assert_allclose(w[0, O.W_B + 6], 3.0 - 2 * alpha_h, rtol=1e-5)
    np.testing.assert_allclose(w[0, O.W_B + 2] ** 2 + w[0, O.W_B + 3] ** 2, 1.0, atol=2e-7)   # (cos, sin) stays a unit vector
    O.step_batch(sc, w, z)
    assert abs(w[0, O.W_B + 6]) < 1e-12      # stopped: 1 / I is a rounded reciprocal, a fused row leaves ~1e-8 of the spin ...
    for _ in range(3):
        O.step_batch(sc, w, z)
    assert abs(w[0, O.W_B + 6]) < 1.2e-38    #  ... every substep again, down to a subnormal, which the spec counts as rest:
    th = w[0, O.W_B + 2:O.W_B + 4].copy()
    O.step_batch(sc, w, z)
    np.testing.assert_array_equal(w[0, O.W_B + 2:O.W_B + 4], th)      # the orientation is not touched any more
    # a body at rest stays at rest, bit for bit
    w = lonely_box(O, [0.3, -0.4, np.cos(0.3), np.sin(0.3), 0, 0, 0])
    w0 = w.copy()
    for _ in range(5):
        O.step_batch(sc, w, z)
    np.testing.assert_array_equal(w[0, O.W_B:O.W_B + 7], w0[0, O.W_B:O.W_B + 7])


def momenta(O, sc, w):
    p, L, E = np.zeros(2), 0.0, 0.0
    for b, m, inertia in ((O.W_B, sc.box_m, sc.box_I), (O.W_D, sc.dyn_m, sc.dyn_I)):
        x, y, _, _, vx, vy, om = w[0, b:b + 7].astype(np.float64)
        p += m * np.array([vx, vy])
        L += m * (x * vy - y * vx) + inertia * om
        E += 0.5 * m * (vx * vx + vy * vy) + 0.5 * inertia * om * om
    return p, L, E


def test_impacts_conserve_momentum_and_never_create_energy(oracle):
    """No ground friction (scene parameter), so the box / dyn-obs pair is an isolated system: contact impulses are
    internal -- equal, opposite, applied at one point -- and restitution is 0 (PhysX default material)."""
    O = oracle
    sc = O.default_scene()
    sc.box_mu_g = 0.0
    sc.dyn_mu_g = 0.0
    z = np.zeros((1, 2), np.float32)
    # head-on, equal masses: perfectly inelastic -> both leave at v0 / 2
    w = lonely_box(O, [0, 0, 1, 0, 2.0, 0, 0])
    w[0, O.W_D:O.W_D + 7] = [0.8, 0, 1, 0, 0, 0, 0]
    for _ in range(8):
        O.step_batch(sc, w, z)
    np.testing.assert_allclose(w[0, [O.W_B + 4, O.W_D + 4]], [1.0, 1.0], atol=1e-6)
    assert abs((w[0, O.W_D] - w[0, O.W_B]) - 0.4) < 1e-4          # touching, neither apart nor interpenetrating
    # oblique, off-centre, spinning, with friction between the two bodies
    rng = np.random.default_rng(5)
    hits = 0
    for case in range(12):
        th = rng.uniform(-0.7, 0.7)
        w = lonely_box(O, [0, rng.uniform(-0.25, 0.25), np.cos(th), np.sin(th), rng.uniform(1.0, 2.5), rng.uniform(-0.4, 0.4),
                           rng.uniform(-2, 2)])
        w[0, O.W_D:O.W_D + 7] = [0.9, 0, 1, 0, rng.uniform(-1.0, 0.0), 0, 0]
        p0, L0, E0 = momenta(O, sc, w)
        E_prev = E0
        for _ in range(16):
            O.step_batch(sc, w, z)
            p, L, E = momenta(O, sc, w)
            np.testing.assert_allclose(p, p0, atol=2e-4)
            assert abs(L - L0) < 2e-4
            assert E <= E_prev * (1 + 1e-6)
            E_prev = E
        hits += E_prev < 0.98 * E0
    assert hits >= 10          # (the cases really collide)


def test_steady_push_balances_drive_and_friction(oracle):
    """Robot behind the box, target 3 m/s: the pair settles where the damper's force equals the box's ground friction,
    v = u - mu m g / D, and the contact force the robot feels (`net_contact_force`, what get_motion_cost reads) is
    that friction force."""
    O = oracle
    sc = O.default_scene()
    w = lonely_box(O, [-0.55, 0, 1, 0, 0, 0, 0], robot=(-1.0, 0.0))
    u = np.array([[3.0, 0.0]], np.float32)
    for _ in range(20):
        O.step_batch(sc, w, u)
    v = 3.0 - MU_B * M_BOX * G / D_DRIVE
    np.testing.assert_allclose(w[0, 4], v, rtol=1e-3)
    np.testing.assert_allclose(w[0, O.W_B + 4], w[0, 4], rtol=1e-6)           # moving together
    np.testing.assert_allclose(w[0, O.W_FC_R], -MU_B * M_BOX * G, rtol=2e-3)
    assert abs(w[0, O.W_B + 1]) < 1e-6 and abs(w[0, O.W_B + 6]) < 1e-6         # a centred push does not turn the box


def rb_separation(w, O):
    x, y, c, s = w[0, O.W_B:O.W_B + 4]
    dx, dy = w[0, 0] - x, w[0, 1] - y
    lx, ly = c * dx + s * dy, -s * dx + c * dy
    return float(np.hypot(lx - np.clip(lx, -0.2, 0.2), ly - np.clip(ly, -0.2, 0.2)) - 0.2)


def box_wall_penetration(w, O, wall):
    x, y, c, s = w[0, O.W_B:O.W_B + 4]
    xs = [x + c * sx * 0.2 - s * sy * 0.2 for sx in (-1, 1) for sy in (-1, 1)]
    ys = [y + s * sx * 0.2 + c * sy * 0.2 for sx in (-1, 1) for sy in (-1, 1)]
    return float(max(max(np.abs(xs)), max(np.abs(ys))) - wall)


def test_penetration_stays_bounded_under_full_effort(oracle):
    """The drive at its effort limit (1000 N) squeezing the box against a wall: contacts are soft (Baumgarte 0.2, six
    passes) but bounded -- a few centimetres, not growing -- and everything comes to rest."""
    O = oracle
    sc = O.default_scene()
    w = lonely_box(O, [3.05, 0.05, np.cos(0.1), np.sin(0.1), 0, 0, 0], robot=(2.6, 0.0))
    u = np.array([[3.0, 0.0]], np.float32)
    worst_rb, worst_bw = 0.0, 0.0
    for _ in range(300):
        O.step_batch(sc, w, u)
        worst_rb = max(worst_rb, -rb_separation(w, O))
        worst_bw = max(worst_bw, box_wall_penetration(w, O, sc.wall))
    assert worst_rb < 0.03 and worst_bw < 0.03      # (spec v1.5: 2.6 cm against the wall, the squeezed box turns more freely while it slides)
    assert abs(w[0, 4]) < 1e-3 and abs(w[0, O.W_B + 4]) < 1e-3
    assert abs(w[0, 0]) <= sc.wall - sc.robot_r + 0.01           # the robot stays inside the walls too


def mirror_y(w, O):
    m = w.copy()
    m[0, 1], m[0, 5] = -w[0, 1], -w[0, 5]
    for b in (O.W_B, O.W_D):
        for j in (1, 3, 5, 6):          # y, sin, vy, omega
            m[0, b + j] = -w[0, b + j]
    return m


def mirror_x(w, O):
    m = w.copy()
    m[0, 0], m[0, 4] = -w[0, 0], -w[0, 4]
    for b in (O.W_B, O.W_D):
        for j in (0, 3, 4, 6):          # x, sin, vx, omega
            m[0, b + j] = -w[0, b + j]
    return m


@pytest.mark.parametrize("axis", ["x", "y"])
def test_the_spec_has_no_handedness(oracle, axis):
    """A mirrored world under mirrored controls gives the mirrored trajectory -- EXACTLY (every operation of the
    robot-box contact rows, the friction cone and the yaw update is sign-symmetric in binary32), through 24 steps of pushing
    and turning the box.  (Box against WALL contacts process their two corners in a fixed order, as every
    sequential-impulse solver does; there the mirror image differs by that order and the test stops before them.)"""
    O = oracle
    sc = O.default_scene()
    rng = np.random.default_rng(1)
    if axis == "y":
        w1 = lonely_box(O, [0.0, 2.0, 1, 0, 0, 0, 0], robot=(-0.3, 1.2), dyn=(-0.6, 2.3))
        mirror, flip = mirror_y, 1
    else:
        w1 = lonely_box(O, [0.0, -2.0, 1, 0, 0, 0, 0], robot=(-0.3, -1.2), dyn=(-0.6, -2.3))
        mirror, flip = mirror_x, 0
    w2 = mirror(w1, O)
    pushed = 0
    for n in range(24):
        u = (np.array([[0.3, 0.8 if axis == "y" else -0.8]]) * 3 * rng.uniform(0.5, 1) + rng.uniform(-1, 1, (1, 2))).astype(np.float32)
        um = u.copy()
        um[0, flip] = -u[0, flip]
        O.step_batch(sc, w1, u)
        O.step_batch(sc, w2, um)
        np.testing.assert_array_equal(mirror(w1, O)[0, :21], w2[0, :21])
        pushed += abs(w1[0, O.W_FC_B]) + abs(w1[0, O.W_FC_B + 1]) > 0
    assert pushed >= 10 and abs(w1[0, O.W_B + 6]) + abs(w1[0, O.W_B + 3]) > 1e-3    # contact, and the box turned


def test_external_force_acts_during_the_next_step_only(oracle):
    """apply_rigid_body_force_tensors (cost_functions.py:76, quirk Q5): the suction force set now pushes the box during
    the next step and is cleared by it.  Spec v1.7: it is consumed by that step's FIRST substep -- dv = F (dt / substeps) / m
    (minus what ground friction takes); with the scene field of the fit tool at 0 (spec v1.6's reading) it acts in every
    substep, dv = F dt / m."""
    O = oracle
    sc = O.default_scene()
    sc.box_mu_g = 0.0
    z = np.zeros((1, 2), np.float32)
    assert sc.fext_substeps == 1 and sc.substeps == 2
    sc.fext_substeps = 0
    w = lonely_box(O, [0, 0, 1, 0, 0, 0, 0])
    w[0, O.W_FEXT_B:O.W_FEXT_B + 2] = [80.0, -40.0]
    O.step_batch(sc, w, z)
    np.testing.assert_allclose(w[0, O.W_B + 4:O.W_B + 6], np.array([80.0, -40.0]) * 0.05 / M_BOX, rtol=1e-6)
    sc.fext_substeps = 1
    w = lonely_box(O, [0, 0, 1, 0, 0, 0, 0])
    w[0, O.W_FEXT_B:O.W_FEXT_B + 2] = [80.0, -40.0]
    O.step_batch(sc, w, z)
    np.testing.assert_allclose(w[0, O.W_B + 4:O.W_B + 6], np.array([80.0, -40.0]) * (0.05 / sc.substeps) / M_BOX, rtol=1e-6)
    assert w[0, O.W_FEXT_B] == 0.0 and w[0, O.W_FEXT_B + 1] == 0.0
    v = w[0, O.W_B + 4:O.W_B + 6].copy()
    O.step_batch(sc, w, z)
    np.testing.assert_array_equal(w[0, O.W_B + 4:O.W_B + 6], v)      # no force, no friction: it coasts


def test_discretisation_is_close_to_its_refinement(oracle):
    """The reference's PhysX settings (2 substeps, 6 passes: isaacgym_wrapper.py:10,28) against a 16-substep, 60-pass
    solve of the same spec: after 1.5 s of noisy pushing the box's end position differs by a few per cent of the
    distance it travelled (contact pushing amplifies differences; the median over 20 pushes is the statement)."""
    O = oracle
    rng = np.random.default_rng(0)

    def run(substeps, iters, U, w0):
        sc = O.default_scene()
        sc.substeps, sc.iters = substeps, iters
        w = w0.copy()
        for u in U:
            O.step_batch(sc, w, u[None])
        return w

    rel = []
    for _ in range(20):
        w0 = O.init_world(1)
        w0[0, 0:2] = [rng.uniform(-0.5, 0.5), rng.uniform(0.8, 1.4)]
        toward = np.array([0 - w0[0, 0], 2 - w0[0, 1]])
        U = (3 * toward / np.linalg.norm(toward) + rng.normal(0, 1.0, (30, 2))).clip(-3, 3).astype(np.float32)
        a, b = run(2, 6, U, w0), run(16, 60, U, w0)
        travelled = np.hypot(*(b[0, 7:9] - w0[0, 7:9]))
        assert travelled > 0.3
        rel.append(np.hypot(*(a[0, 7:9] - b[0, 7:9])) / travelled)
    assert np.median(rel) < 0.10


# ---------------------------------------------------------------- GPU: the product's own step (shipped scene constants)
def _sim(world_row):
    torch = pytest.importorskip("torch")
    from m3p2i_aip_amd.isaacgym_wrapper import IsaacGymConfig, IsaacGymWrapper
    from tests.test_planner_api_gpu import world_to_tensors
    sim = IsaacGymWrapper(IsaacGymConfig(dt=0.05), "point_env", num_envs=1, device="cuda:0")
    dof, root = world_to_tensors(sim, world_row)
    sim.set_dof_state_tensor(dof)
    sim.set_actor_root_state_tensor(root)
    return sim, torch


def test_spec_reciprocal_is_a_division_to_the_last_place(oracle):
    """Planar spec v1.6 replaces the substep's IEEE divisions (a contact's effective masses, the friction coupling's factors, the
    orientation update's 1 / (1 + a^2)) by a fixed sequence: bit-trick seed + three Newton steps in residual form.  Mechanics does
    not notice: over the range those sites see (1e-6 .. 1e6 and the neighbourhoods of powers of two) the result is the correctly
    rounded quotient for more than 99.9 % of inputs and within one unit in the last place for every one of them."""
    import ctypes as C
    lib = oracle.load()
    lib.m3o_spec_rcp.restype = C.c_float
    lib.m3o_spec_rcp.argtypes = [C.c_float]
    rng = np.random.default_rng(5)
    xs = np.concatenate([np.exp(rng.uniform(np.log(1e-6), np.log(1e6), 20000)), 1.0 + rng.uniform(0.0, 1e-3, 2000),
                         2.0 ** rng.integers(-20, 20, 200) * (1.0 + rng.choice([-1, 0, 1], 200) * 2.0 ** -23),
                         [1.0, 2.0, 0.5, 3.0, 1.0 / 16.0, 1.0 / 10.0, 0.1625]]).astype(np.float32)
    got = np.array([lib.m3o_spec_rcp(float(x)) for x in xs], np.float32)
    exact = np.float32(1.0) / xs
    ulps = np.abs(got.view(np.int32).astype(np.int64) - exact.view(np.int32).astype(np.int64))
    assert ulps.max() <= 1 and (ulps == 0).mean() > 0.999, (ulps.max(), (ulps == 0).mean())
    assert lib.m3o_spec_rcp(1.0) == 1.0 and lib.m3o_spec_rcp(2.0) == 0.5 and lib.m3o_spec_rcp(0.0625) == 16.0


@pytest.mark.gpu
def test_product_step_obeys_the_same_closed_forms(oracle):
    O = oracle
    # velocity drive
    sim, torch = _sim(lonely_box(O, [3.0, 3.0, 1, 0, 0, 0, 0], robot=(0.0, 0.0))[0])
    u = torch.tensor([[3.0, -1.5]], device="cuda:0")
    for n in range(1, 5):
        sim.set_dof_velocity_target_tensor(u)
        sim.step()
        np.testing.assert_allclose(sim.robot_vel[0].cpu().numpy(), drive_response(n, [3.0, -1.5]), rtol=2e-6)
    # Coulomb slide
    sim, torch = _sim(lonely_box(O, [0, 0, 1, 0, 2.0, 0, 0])[0])
    want = slide(2.0, 8)
    zero = torch.zeros(1, 2, device="cuda:0")
    for n in range(8):
        sim.set_dof_velocity_target_tensor(zero)
        sim.step()
        np.testing.assert_allclose(sim.get_actor_position_by_name("box")[0, 0].item(), want[n, 0], atol=2e-6)
        np.testing.assert_allclose(sim.get_actor_velocity_by_name("box")[0, 0].item(), want[n, 1], atol=2e-6)
    # steady push: drive force == ground friction
    sim, torch = _sim(lonely_box(O, [-0.55, 0, 1, 0, 0, 0, 0], robot=(-1.0, 0.0))[0])
    u = torch.tensor([[3.0, 0.0]], device="cuda:0")
    for _ in range(20):
        sim.set_dof_velocity_target_tensor(u)
        sim.step()
    v = 3.0 - MU_B * M_BOX * G / D_DRIVE
    np.testing.assert_allclose(sim.robot_vel[0, 0].item(), v, rtol=1e-3)
    np.testing.assert_allclose(sim.get_actor_velocity_by_name("box")[0, 0].item(), sim.robot_vel[0, 0].item(), rtol=1e-6)


# ================================================================ panda_env: chain spec
@pytest.fixture(scope="module")
def P():
    import oracle.panda as P
    P.lib()
    return P


# joint origins of franka_panda.urdf:27-242 (xyz, roll; every revolute axis is z, the fingers slide along +y / -y)
PANDA_URDF = [((0, 0, 0.333), 0.0), ((0, 0, 0), -np.pi / 2), ((0, -0.316, 0), np.pi / 2), ((0.0825, 0, 0), np.pi / 2),
              ((-0.0825, 0.384, 0), -np.pi / 2), ((0, 0, 0), np.pi / 2), ((0.088, 0, 0), np.pi / 2)]
PANDA_HAND = ((0, 0, 0.107), -np.pi / 4)      # panda_hand_joint: fixed on link7, yaw -45 deg
PANDA_FINGER_Z = 0.0584
PANDA_BASE = (-0.45, 0.0, 1.125)              # panda.yaml:8


def generic_chain(q, base=PANDA_BASE):
    """Textbook forward kinematics in binary64 from the URDF numbers: T = T * Trans(xyz) * Rx(roll) * Rz(q); `base`: where the
    arm stands (the default room's, or a workspace's of m3_set_panda_scene)."""
    def rx(a):
        c, s = np.cos(a), np.sin(a)
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])

    def rz(a):
        c, s = np.cos(a), np.sin(a)
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])

    R, p = np.eye(3), np.array(base, np.float64)
    for (xyz, roll), qj in zip(PANDA_URDF, q[:7]):
        p = p + R @ np.array(xyz)
        R = R @ rx(roll) @ rz(qj)
    link7 = p.copy()
    p = p + R @ np.array(PANDA_HAND[0])
    R = R @ rz(PANDA_HAND[1])
    left = p + R @ np.array([0, q[7], PANDA_FINGER_Z])
    right = p + R @ np.array([0, -q[8], PANDA_FINGER_Z])
    return dict(link7=link7, hand=p, R=R, left=left, right=right)


def test_panda_fk_is_the_urdf_chain(P):
    sc = P.default_scene()
    rng = np.random.default_rng(11)
    lo, hi = np.array(sc.qlo), np.array(sc.qhi)
    for _ in range(200):
        q = rng.uniform(lo, hi)
        L = P.fk(sc, q.astype(np.float32))
        want = generic_chain(q.astype(np.float32).astype(np.float64))
        np.testing.assert_allclose(L["pos"][7], want["link7"], atol=3e-6)
        np.testing.assert_allclose(L["pos"][8], want["hand"], atol=3e-6)
        np.testing.assert_allclose(L["pos"][9], want["left"], atol=3e-6)
        np.testing.assert_allclose(L["pos"][10], want["right"], atol=3e-6)
        np.testing.assert_allclose(L["ay"][8], want["R"][:, 1], atol=3e-6)
        np.testing.assert_allclose(L["az"][8], want["R"][:, 2], atol=3e-6)


def test_panda_servo_is_the_implicit_damper_with_the_urdf_effort_limits(P):
    """q' = (q' + a u) / (1 + a), a = h D / I, the change per substep limited to effort h / I (franka_panda.urdf: 87 / 12 /
    20), velocities to the URDF's limits -- every dof, random targets, from rest."""
    sc = P.default_scene()
    h = sc.dt / sc.substeps
    inertia, effort, vlim = np.array(sc.inertia, np.float64), np.array(sc.effort, np.float64), np.array(sc.vlim, np.float64)
    rng = np.random.default_rng(2)
    for case in range(20):
        w = P.init_world(1)
        u = rng.uniform(-2.0, 2.0, (1, 9)).astype(np.float32)
        u[0, 7:] = rng.uniform(-0.15, 0.15, 2)
        v = np.zeros(9)
        a = h * sc.drive_damping / inertia
        for n in range(6):
            P.step_batch(sc, w, u)
            for _ in range(sc.substeps):
                dv = (v + a * u[0]) / (1 + a) - v
                v = np.clip(v + np.clip(dv, -effort * h / inertia, effort * h / inertia), -vlim, vlim)
            free = np.ones(9, bool)
            free[7:] = (w[0, P.W_Q + 7:P.W_Q + 9] > 1e-6) & (w[0, P.W_Q + 7:P.W_Q + 9] < 0.04 - 1e-6)   # (fingers off their stops)
            np.testing.assert_allclose(w[0, P.W_QD:P.W_QD + 9][free], v[free], rtol=3e-6, atol=1e-7)
            v[~free] = w[0, P.W_QD:P.W_QD + 9][~free]


def test_panda_cube_free_fall_landing_and_coulomb_slide(P):
    """A free cube: exact free fall (g h^2 sums); it lands on the table top through its four corner contacts, comes to
    rest within 0.2 mm of it and goes to sleep; pushed sideways it decelerates with mu g (the four friction rows
    together), the table reporting the reaction mu m g (what get_motion_cost reads), and stops dead."""
    sc = P.default_scene()
    h, z = sc.dt / sc.substeps, np.zeros((1, 9), np.float32)
    w = P.init_world(1)
    w[0, P.W_CUBEA + 2] = 1.5
    v, zz = 0.0, 1.5
    for n in range(20):
        P.step_batch(sc, w, z)
        for _ in range(sc.substeps):
            v -= sc.g * h
            zz += h * v
        np.testing.assert_allclose(w[0, P.W_CUBEA + 2], zz, atol=5e-6)
        np.testing.assert_allclose(w[0, P.W_CUBEA + 9], v, rtol=1e-5)
    for _ in range(100):
        P.step_batch(sc, w, z)
    assert w[0, P.W_CUBEA + 2] == pytest.approx(1.025 + sc.cube_half, abs=2e-4)      # landed on the table top, at rest
    assert np.all(w[0, P.W_CUBEA + 7:P.W_CUBEA + 13] == 0) and w[0, P.W_AWAKE] == 0.0   # ... asleep
    assert abs(w[0, P.W_CUBEA + 6]) > 0.9999                                          # ... and flat
    # sliding on the table: mu g per unit mass, reaction mu m g on the table, rest
    w[0, P.W_CUBEA + 7] = 0.5
    row = np.ascontiguousarray(w[0]); P.infer_state(sc, row); w[0] = row      # (a moving cube is loaded awake)
    assert w[0, P.W_AWAKE] == 1.0
    x0 = w[0, P.W_CUBEA]
    vx = 0.5
    for n in range(8):
        P.step_batch(sc, w, z)
        moving = vx > 0
        vx = max(0.0, vx - 2 * sc.mu * sc.g * h)
        np.testing.assert_allclose(w[0, P.W_CUBEA + 7], vx, atol=0.02)
        if moving and vx > 0.05:
            np.testing.assert_allclose(w[0, P.W_FT], sc.mu * sc.cube_m * sc.g, rtol=0.05)
            np.testing.assert_allclose(w[0, P.W_FT + 2], -sc.cube_m * sc.g, rtol=0.02)     # and its weight
    assert np.all(w[0, P.W_CUBEA + 7:P.W_CUBEA + 13] == 0) and w[0, P.W_AWAKE] == 0.0
    assert w[0, P.W_CUBEA] - x0 == pytest.approx(0.5 ** 2 / (2 * sc.mu * sc.g), rel=0.25)   # stopping distance v0^2 / 2 mu g
    assert abs(w[0, P.W_CUBEA + 6]) > 0.999                                            # it slid, it did not tumble


def _down_pose(P, sc, x, y, clearance):
    """gripper pointing straight down, finger tips `clearance` above the table top at (x, y)"""
    from tests.test_device_dynamics_on_host import _ik_down
    return _ik_down(P, sc, np.array([x, y, 1.025 + (0.0584 + sc.tip_z + sc.tip_r) + clearance]))


def _point_jacobian(P, sc, q, x):
    L = P.fk(sc, q)
    J = np.zeros((3, 9))
    for j in range(7):
        J[:, j] = np.cross(L["az"][j + 1], x - L["pos"][j + 1])
    return J, L


def test_panda_descent_into_the_table_stops_and_reports_the_effort_limited_force(P):
    """Spec v2, contact response.  The gripper is driven straight down onto the table at 0.2 m/s: the finger tip
    stops AT the table top (never deeper than 2 mm while the drives keep pushing), the joints stall, and the table
    reports the force the saturated drives can exert -- checked as Newton's law per joint with a bounded drive torque:
    I_i dq'_i / h - (J^T f)_i = tau_i with |tau_i| <= effort_i (franka_panda.urdf: 87 / 12 N m) for every joint that is
    not on a joint stop, and |tau_i| = effort_i for at least one of them once the descent has stalled."""
    sc = P.default_scene()
    sc.substeps, sc.dt = 1, 0.005          # one substep per step: the reported force is the step's
    h = 0.005
    w = P.init_world(1)
    z = np.zeros((1, 9), np.float32)
    for _ in range(20):
        P.step_batch(sc, w, z)
    w[0, :9] = _down_pose(P, sc, 0.35, 0.0, 0.02)
    w[0, 7], w[0, 8] = 0.04, 0.0
    I, eff = np.array(sc.inertia), np.array(sc.effort)
    gaps, ratios, speeds, forces = [], [], [], []
    for t in range(70):                     # 0.1 s of approach, 0.25 s of pushing
        q0, qd0 = w[0, :9].copy(), w[0, 9:18].copy()
        Jh, L = _point_jacobian(P, sc, q0, P.fk(sc, q0)["pos"][8])
        u = np.zeros((1, 9), np.float32)
        u[0, :7] = np.clip(np.linalg.pinv(Jh[:, :7]) @ np.array([0, 0, -0.2]), -2.0, 2.0)   # (the planner's bounds, mppi/panda.yaml)
        tl, tr = L["pos"][9] + sc.tip_z * L["az"][8], L["pos"][10] + sc.tip_z * L["az"][8]
        P.step_batch(sc, w, u)
        n_grip = P.last_rows()[0]
        f = -w[0, P.W_FT:P.W_FT + 3].astype(np.float64)          # on the gripper
        L1 = P.fk(sc, w[0, :9])
        gaps.append(min(L1["pos"][9][2], L1["pos"][10][2]) + sc.tip_z * L1["az"][8][2] - sc.tip_r - 1.025)
        speeds.append(abs((Jh[:, :7] @ w[0, 9:16])[2]))
        if n_grip == 1 and np.linalg.norm(f) > 0:
            s = 0 if tl[2] < tr[2] else 1
            J, _ = _point_jacobian(P, sc, q0, (tl if s == 0 else tr) - np.array([0, 0, sc.tip_r]))
            J[:, 7 + s] = (1 - 2 * s) * L["ay"][8]
            tau = I * (w[0, 9:18] - qd0) / h - J.T @ f
            free = w[0, 9:16] != 0.0                               # (a joint on a stop is held by the stop)
            ratios.append(np.abs(tau[:7][free] / eff[:7][free]).max())
            forces.append(f[2])
    first = next(i for i, g in enumerate(gaps) if g < 1e-3)
    assert 15 < first < 40 and speeds[first - 5] == pytest.approx(0.2, rel=0.1)   # it arrived at the commanded speed
    assert min(gaps) > -2e-3 and max(gaps[first:]) < 1e-3             # ... and stays at the surface, within 2 mm
    assert max(speeds[first + 5:]) < 0.05                              # stalled (the hand only pivots about the tip)
    assert len(ratios) > 15 and max(ratios) < 1.02                     # bounded drive torques explain every force
    assert max(ratios[5:]) > 0.98                                      # ... and a drive is at its limit
    assert 100 < max(forces) < 400                                     # (N: 87 N m over a ~0.4 m lever)


def _descend_over_cubeA(P, sc, dy, steps=60):
    """open gripper, pointing straight down, hand `dy` off cubeA's centre along the pads' closing direction, lowered at 0.1 m/s
    from 4 cm above the grasp height to the grasp height; returns the world, cubeA's start, the rows seen, the hand's heights and
    the heights of the -y finger tip's lowest point, both above the cube's centre"""
    from tests.test_device_dynamics_on_host import _ik_down
    w = P.init_world(1)
    z = np.zeros((1, 9), np.float32)
    for _ in range(30):
        P.step_batch(sc, w, z)
    c0 = w[0, P.W_CUBEA:P.W_CUBEA + 3].copy()
    w[0, :9] = _ik_down(P, sc, np.array([c0[0], c0[1] + dy, c0[2] + sc.grasp_z + 0.04]))
    w[0, 7], w[0, 8] = 0.04, 0.04
    w[0, 9:18] = 0.0
    rows, heights, tips = [], [], []
    for t in range(steps):
        q0 = w[0, :9].copy()
        L = P.fk(sc, q0)
        Jh, _ = _point_jacobian(P, sc, q0, L["pos"][8])
        u = np.zeros((1, 9), np.float32)
        vz = -0.1 if L["pos"][8][2] > c0[2] + sc.grasp_z else 0.0
        u[0, :7] = np.clip(np.linalg.pinv(Jh[:, :7]) @ np.array([0, 0, vz]), -2.0, 2.0)
        u[0, 7:] = 1.5                                           # fingers commanded open (the reach phase's override)
        P.step_batch(sc, w, u)
        rows.append(P.last_rows()[0])
        L1 = P.fk(sc, w[0, :9])
        heights.append(L1["pos"][8][2] - c0[2])
        tips.append(L1["pos"][10][2] + sc.tip_z * L1["az"][8][2] - sc.tip_r - c0[2])     # bottom of the -y finger's tip sphere
    return w[0], c0, rows, heights, np.array(tips)


def test_panda_open_gripper_comes_down_over_an_off_centre_cube(P):
    """Spec v2.1, the capture volume.  The reference's shipped planner size brings the open gripper down 2-3 cm off the cube's
    centre line.  With the cube's centre BETWEEN the pads (2.5 cm off: a finger's pad overlaps the cube by a centimetre) the
    finger tips' spheres do not act on cubeA -- the pads will, position level, once they close -- and the cube is not touched:
    under v2.0 a tip landed on its edge and knocked it (39 of 60 picks at that size; now 60).  With the cube's centre BEYOND a
    pad's face (5 cm off) the gripper is not over the cube but on it: the tip lands on the cube's top and stops there."""
    sc = P.default_scene()
    w, c0, rows, heights, _ = _descend_over_cubeA(P, sc, 0.025)
    assert np.array_equal(w[P.W_CUBEA:P.W_CUBEA + 3], c0) and w[P.W_AWAKE] == 0.0 and w[P.W_HELD] == 0.0
    assert max(rows) == 0 and heights[-1] == pytest.approx(sc.grasp_z, abs=3e-3)          # down at the grasp height, nothing touched
    w, c0, rows, heights, tip_bottom = _descend_over_cubeA(P, sc, 0.05)
    on = [i for i, r in enumerate(rows) if r >= 1]                                         # the tip's contact row against cubeA
    # it stands ON the cube and stalls there for a quarter of a second -- SUNK up to a centimetre into it: a stated limit of
    # the spec: arm (kilograms, drives of 87 N m) on cube (125 g) on table is a chain of mass ratio 1000 : 1
    # that seven Gauss-Seidel sweeps do not converge on; the velocity it leaves lets the tip in until Baumgarte balances it
    assert len(on) >= 15 and tip_bottom[on].min() > sc.cube_half - 0.012
    assert abs(tip_bottom[on[-1]] - tip_bottom[on[-10]]) < 1e-3
    # (then the cube, pressed at 1.5 cm from its edge by a hand that drifts sideways, slides out from under the tip)
    assert w[P.W_HELD] == 0.0 and np.linalg.norm(w[P.W_CUBEA:P.W_CUBEA + 2] - c0[:2]) > 5e-3


def test_panda_finger_sweep_moves_cubeB(P):
    """A closed gripper swept sideways at cube height pushes the sleeping cubeB away: the cube wakes, moves with the
    finger, the finger's force on it is reported (get_motion_cost reads cubeB's net contact force), and once the finger
    has passed it comes to rest on the table and goes back to sleep."""
    sc = P.default_scene()
    w = P.init_world(1)
    z = np.zeros((1, 9), np.float32)
    for _ in range(10):
        P.step_batch(sc, w, z)
    B0 = w[0, P.W_CUBEB:P.W_CUBEB + 3].copy()
    assert w[0, P.W_AWAKE + 1] == 0.0
    from tests.test_device_dynamics_on_host import _ik_down
    w[0, :9] = _ik_down(P, sc, np.array([B0[0] - 0.08, B0[1], 1.05 + 0.0584 + sc.tip_z]))
    w[0, 7:9] = 0.0
    woke, fmax = False, 0.0
    for t in range(60):
        Jh, _ = _point_jacobian(P, sc, w[0, :9].copy(), P.fk(sc, w[0, :9])["pos"][8])
        u = np.zeros((1, 9), np.float32)
        u[0, :7] = np.linalg.pinv(Jh[:, :7]) @ np.array([0.25, 0, 0])
        u[0, 7:] = -1.5
        P.step_batch(sc, w, u)
        woke = woke or w[0, P.W_AWAKE + 1] == 1.0
        fmax = max(fmax, np.abs(w[0, P.W_FB:P.W_FB + 2]).sum())
    for t in range(60):                     # the gripper withdraws, the cube stays behind and settles
        Jh, _ = _point_jacobian(P, sc, w[0, :9].copy(), P.fk(sc, w[0, :9])["pos"][8])
        u = np.zeros((1, 9), np.float32)
        if t < 20:
            u[0, :7] = np.linalg.pinv(Jh[:, :7]) @ np.array([-0.25, 0, 0.1])
        u[0, 7:] = -1.5
        P.step_batch(sc, w, u)
    B1 = w[0, P.W_CUBEB:P.W_CUBEB + 3]
    assert woke and fmax > 0.5                                   # N, well above get_motion_cost's 0.1 threshold
    assert np.linalg.norm(B1[:2] - B0[:2]) > 0.03                # pushed away ...
    assert B1[2] == pytest.approx(1.05, abs=1e-3) and w[0, P.W_AWAKE + 1] == 0.0 and np.all(w[0, P.W_CUBEB + 7:P.W_CUBEB + 13] == 0)
    assert np.array_equal(w[0, P.W_CUBEA:P.W_CUBEA + 3], P.init_world(1)[0, P.W_CUBEA:P.W_CUBEA + 3]) is False   # (cubeA settled too)


@pytest.mark.parametrize("offset,stays", [(0.0, True), (0.011, True), (0.02, True), (0.03, False), (0.04, False)])
def test_panda_cube_released_on_cubeB_rests_or_tips_over_the_edge(P, offset, stays):
    """cubeA released 4 mm above cubeB, displaced by `offset` along x (and 4 mm along y, yawed by 2 degrees): with its
    centre of mass over cubeB's top face (offset < 2.5 cm) it lands, stays and the stack goes to sleep; beyond the
    edge it tips over it and ends on the table next to cubeB -- angular dynamics of a free cube on its face-to-face
    contact points."""
    sc = P.default_scene()
    w = P.init_world(1)
    z = np.zeros((1, 9), np.float32)
    for _ in range(10):
        P.step_batch(sc, w, z)
    B = w[0, P.W_CUBEB:P.W_CUBEB + 3].copy()
    w[0, P.W_CUBEA:P.W_CUBEA + 3] = B + np.array([offset, 0.004, 0.054], np.float32)
    w[0, P.W_CUBEA + 3:P.W_CUBEA + 7] = (0, 0, np.sin(np.radians(1.0)), np.cos(np.radians(1.0)))
    w[0, P.W_CUBEA + 7:P.W_CUBEA + 13] = 0
    row = np.ascontiguousarray(w[0]); P.infer_state(sc, row); w[0] = row
    assert w[0, P.W_AWAKE] == 1.0                        # in the air: awake
    for _ in range(150):
        P.step_batch(sc, w, z)
    A = w[0, P.W_CUBEA:P.W_CUBEA + 3]
    assert np.all(w[0, P.W_AWAKE:P.W_AWAKE + 2] == 0.0)   # everything has come to rest
    if stays:
        assert A[2] == pytest.approx(1.10, abs=1.5e-3) and abs(A[0] - B[0] - offset) < 5e-3
        assert abs(w[0, P.W_CUBEA + 6]) > 0.999           # flat (rotated about z only)
    else:
        assert A[2] == pytest.approx(1.05, abs=1.5e-3) and A[0] - B[0] > 0.045      # on the table, beyond cubeB
    assert np.linalg.norm(w[0, P.W_CUBEB:P.W_CUBEB + 2] - B[:2]) < 0.01


def test_panda_resting_stack_is_loaded_asleep_and_a_hovering_cube_is_not(P):
    """The wrapper's tensors carry no sleep bit: a loaded world's cube is asleep iff it is at rest ON something -- the
    table, the shelf_stand, or the other cube with its centre over it."""
    sc = P.default_scene()
    w = P.init_world(1)[0]
    w[P.W_CUBEA + 2] = w[P.W_CUBEB + 2] = 1.05
    for dz, dx, want in ((0.05, 0.0, 0.0), (0.0505, 0.011, 0.0), (0.0505, 0.03, 1.0), (0.056, 0.0, 1.0)):
        v = w.copy()
        v[P.W_CUBEA:P.W_CUBEA + 3] = v[P.W_CUBEB:P.W_CUBEB + 3] + np.array([dx, 0, dz], np.float32)
        P.infer_state(sc, v)
        assert v[P.W_AWAKE] == want and v[P.W_AWAKE + 1] == 0.0, (dz, dx)
    v = w.copy(); v[P.W_CUBEA + 7] = 1e-3                  # moving: awake
    P.infer_state(sc, v)
    assert v[P.W_AWAKE] == 1.0
    v = P.init_world(1, cube_on_shelf=True)[0]; v[P.W_CUBEA + 2] = 1.325 + 0.025
    P.infer_state(sc, v)
    assert v[P.W_AWAKE] == 0.0                             # on the shelf_stand


def test_panda_inertias_are_the_mesh_derived_diagonal(P):
    """The joint inertias of the spec are the diagonal of the joint-space mass matrix at the initial pose, computed from
    the reference's collision meshes at the default density (tools/panda_inertia.py, run in the build container; the
    numbers are committed constants) -- here: the constants of the oracle's scene are those, and the servo's time constant
    I / D stays far below the substep for every joint (the drive dominates: a = h D / I between 1.4 and 1000)."""
    sc = P.default_scene()
    want = [1.32, 2.12, 1.30, 0.918, 0.0271, 0.0366, 0.0030, 0.022, 0.022]
    np.testing.assert_allclose(np.array(sc.inertia), want, rtol=1e-6)
    a = (sc.dt / sc.substeps) * sc.drive_damping / np.array(sc.inertia)
    assert a.min() > 1.4 and a.max() < 1001


def test_panda_held_cube_is_rigid_with_the_hand(P):
    from tests.panda_worlds import grasp_world
    sc = P.default_scene()
    w = grasp_world(P, sc)[None].copy()

    def rel(w):
        L = P.fk(sc, w[0, P.W_Q:P.W_Q + 9])
        ax = np.cross(L["ay"][8], L["az"][8])
        d = w[0, P.W_CUBEA:P.W_CUBEA + 3].astype(np.float64) - L["pos"][8]
        return np.array([d @ ax, d @ L["ay"][8], d @ L["az"][8]])

    r0 = rel(w)
    rng = np.random.default_rng(4)
    for n in range(60):
        u = rng.uniform(-1.0, 1.0, (1, 9)).astype(np.float32)
        u[0, 7:] = -1.5
        P.step_batch(sc, w, u)
        assert w[0, P.W_HELD] == 1.0
        np.testing.assert_allclose(rel(w), r0, atol=5e-6)
    assert np.linalg.norm(w[0, P.W_CUBEA:P.W_CUBEA + 3] - grasp_world(P, sc)[P.W_CUBEA:P.W_CUBEA + 3]) > 0.01   # it really moved
