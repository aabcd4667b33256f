"""Host-side ancillary controllers for PRIOR SAMPLES (MPPI.set_prior_samples / m3_set_prior_samples): small, cheap
proposals of whole control sequences that a few of the K rollouts take verbatim, as in Biased-MPPI.  point_env: the control is
the robot's velocity command (vx, vy), tracked by the velocity servo; the controllers below roll the robot forward
KINEMATICALLY (x += u * dt) -- they know nothing of contacts, which is what the rollout is for.

Both return float32 arrays [n, T, 2]: the controls of steps 0 .. T-1 of the NEXT command's horizon.
"""
from __future__ import annotations

import numpy as np

F = np.float32


def _drive(pos, target, T, dt, speed):
    """T steps of a saturated proportional drive from pos to target: each step covers what is left of the way, at most speed *
    dt of it.  Returns (controls [T, 2], end point)."""
    pos = np.asarray(pos, np.float64).copy()
    target = np.asarray(target, np.float64)
    u = np.zeros((T, 2), np.float64)
    for t in range(T):
        d = target - pos
        dist = float(np.hypot(d[0], d[1]))
        if dist > 0.0:
            v = min(dist / dt, speed)
            u[t] = d / dist * v
        pos = pos + u[t] * dt
    return u, pos


def go_to(robot_xy, target_xy, T, dt, u_max, speeds=(1.0, 0.75, 0.5, 0.25)):
    """A straight line to a point: one sequence per speed factor, the speed limit `factor * min(u_max)` (so that the velocity
    vector stays inside the box of control limits in every direction).  Once the point is reached the controls are zero."""
    lim = float(np.min(np.abs(np.asarray(u_max, np.float64))))
    out = np.zeros((len(speeds), int(T), 2), F)
    for j, f in enumerate(speeds):
        out[j] = _drive(robot_xy, target_xy, int(T), float(dt), float(f) * lim)[0]
    return out


def push_behind(robot_xy, box_xy, goal_xy, T, dt, u_max, speeds=(1.0, 0.75, 0.5, 0.25), standoff=0.45, reach=0.05):
    """Go behind the box and push: drive to the point `standoff` behind the box on the goal-box line, then toward the goal.
    One sequence per speed factor.  `reach`: how close to the stand-off point counts as there."""
    box, goal = np.asarray(box_xy, np.float64), np.asarray(goal_xy, np.float64)
    away = box - goal
    n = float(np.hypot(away[0], away[1]))
    away = away / n if n > 0.0 else np.array([1.0, 0.0])
    behind = box + standoff * away
    lim = float(np.min(np.abs(np.asarray(u_max, np.float64))))
    out = np.zeros((len(speeds), int(T), 2), F)
    for j, f in enumerate(speeds):
        pos = np.asarray(robot_xy, np.float64).copy()
        target = behind
        for t in range(int(T)):
            if target is behind and float(np.hypot(*(behind - pos))) <= reach:
                target = goal
            u, pos = _drive(pos, target, 1, float(dt), float(f) * lim)
            out[j, t] = u[0]
    return out


CONTROLLERS = {"go_to": go_to, "push_behind": push_behind}


# ---- panda_env (MPPI.set_panda_prior_samples / m3_set_panda_prior_samples): the control is the joint velocity command of the
# seven arm joints and the two fingers, tracked by the velocity servo.  Float32 arrays [n, T, 9] ----
def hold(T, n=1):
    """Stay where you are: zero velocity commands."""
    return np.zeros((int(n), int(T), 9), F)


def _drive_joint(q, target, T, dt, speed):
    """_drive for one joint: each step covers what is left of the way, at most speed * dt of it; zero once there."""
    q, target = float(q), float(target)
    u = np.zeros(T, np.float64)
    for t in range(T):
        d = target - q
        if d != 0.0:
            u[t] = np.sign(d) * min(abs(d) / dt, speed)
        q = q + u[t] * dt
    return u


def joint_go_to(q, q_target, T, dt, u_max, speeds=(1.0, 0.75, 0.5, 0.25)):
    """Keep going to a joint configuration, KINEMATICALLY (q += u * dt): per joint the saturated proportional drive of _drive,
    at `factor * |u_max[j]|`, and zero once the joint is there; one sequence per speed factor.  q: the arm's (and, if given,
    the fingers') positions now; q_target: seven targets (the columns 7 and 8 of the fingers stay zero) or nine (they follow
    q_target[7:])."""
    q = np.asarray(q, np.float64).reshape(-1)
    q_target = np.asarray(q_target, np.float64).reshape(-1)
    if q_target.shape[0] not in (7, 9) or q.shape[0] < q_target.shape[0]:
        raise ValueError(f"joint_go_to: q_target has {q_target.shape[0]} entries (7 or 9) and q {q.shape[0]} (at least as many)")
    lim = np.abs(np.asarray(u_max, np.float64)).reshape(-1)
    out = np.zeros((len(speeds), int(T), 9), F)
    for s, f in enumerate(speeds):
        for j in range(q_target.shape[0]):
            out[s, :, j] = _drive_joint(q[j], q_target[j], int(T), float(dt), float(f) * float(lim[j]))
    return out


PANDA_CONTROLLERS = {"hold": hold, "joint_go_to": joint_go_to}
