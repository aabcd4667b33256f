"""Shared pieces of the prior-controller tests (tests/test_prior_controllers_cpu.py, tests/test_prior_controllers_gpu.py): the
host build of csrc/prior_controllers.hpp as a program (tests/native/prior_controllers_host.cpp), the inputs, the float64
reference with the positions it passes through, and the bound on |binary32 - float64| -- derived here, not fitted.

THE BOUND.  eps = 2^-24 (unit roundoff of binary32), T steps of dt, X = the largest |coordinate| among robot, box, goal and the
stand-off point, speed = the sequence's speed limit.  Every operation of the header is one correctly rounded binary32 operation
(relative error <= eps); constants below are rounded up to cover the second-order terms.
  One drive step with exact inputs: d_c = t_c - p_c (1 eps); dist = sqrt(dx dx + dy dy): the radicand 2 eps, the root halves
  it and adds 1, d's own error adds 1: 3 eps; v = min(dist / dt, speed): 4 eps (speed = factor * lim: 1 eps); u_c = (d_c / dist)
  * v: 1 + 3 + 1 + 4 + 1 = 10 eps of |u_c| <= speed; the reference's own rounding to float32 adds 1.  Over both components:
      du  = 16 eps speed                                   (sqrt(2) * 11 = 15.6)
  p_c' = p_c + u_c dt: the product 1 eps, the sum eps |p_c'|:
      dp  = 16 eps speed dt + 1.5 eps X                    (sqrt(2) * (11 eps speed dt + eps X))
  The stand-off point: away_c = b_c - g_c (1 eps), its length 3 eps, the quotient 5 eps of a number <= 1, times standoff 6 eps,
  plus b_c: eps X:
      dh  = 9 eps standoff + 1.5 eps X                     (sqrt(2) * (6 eps standoff + eps X));  0 for go_to
  How errors travel.  The exact step is p' = p + clip(t - p) with clip the projection on the ball of radius speed * dt: it is
  1-Lipschitz in p and in t.  So the position error obeys e(0) = 0, e(k + 1) <= e(k) + dh + dp, that is e(k) <= k (dh + dp);
  and u = clip'((t - p) / dt) with clip' the projection on the ball of radius speed: its error at step k is at most
  (e(k) + dh) / dt + du.  Near the target u = d / dt: the position error enters divided by dt.  The bound on every control:
      bound = ((T - 1) (dh + dp) + dh) / dt + du
  The switch of push_behind is a discontinuity: the above holds while both sides take the same decision at every test, which
  they do when the float64 reference keeps | |behind - pos| - reach | above e(T) + dh + 3 eps * (2 sqrt(2) X) (position and
  stand-off errors, and the 3 eps of the norm itself) -- the tests assert the guard 1e-3 on the reference and that this sum is
  below it.
"""
import os
import subprocess

import numpy as np

from m3p2i_aip_amd import priors as A

F = np.float32
EPS = 2.0 ** -24
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "prior_controllers_host.cpp")
GO_TO, PUSH_BEHIND = 1, 2
DT, STANDOFF, REACH = F(0.05), F(0.45), F(0.05)
FACTORS = (1.0, 0.75, 0.5, 0.25)           # of min|u_max| = 2.0
U_MAX = ((2.0, 2.0), (3.0, -2.0))          # the second asymmetric, its smaller limit negative: |.| is exercised
HORIZONS = (12, 30)
GUARD = 1e-3
# (robot, box, goal)
INPUTS = [
    ((0.0, 0.0), (1.0, 1.0), (-3.0, 3.0)),
    ((-1.5, 0.5), (0.2, -0.3), (3.0, 3.0)),
    ((2.0, -2.0), (1.0, 1.0), (1.0, 1.0)),         # the box at the goal
    ((0.3, 0.1), (0.0, 0.0), (-3.0, -3.0)),        # the switch happens mid-horizon
    ((1.318, 1.318), (1.0, 1.0), (-3.0, -3.0)),    # the switch happens at step 0
    ((1.0, 1.0), (0.0, 0.0), (1.0, 1.0)),          # go_to: the robot exactly at its target
    ((0.45, -2.0), (0.0, -2.0), (-3.0, -2.0)),     # push_behind: the robot exactly at the stand-off point (0.45 = fl32(0.45) + 0)
]


def f32(v):
    return np.asarray(v, F)


def build(tmp, extra=("-O2",)):
    """the host program; -ffp-contract=off as for the library"""
    out = os.path.join(str(tmp), "prior_controllers_host" + ("_san" if any("sanitize" in f for f in extra) else ""))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fno-fast-math"] + list(extra) +
                          [SRC, "-o", out])
    return out


def _hex(v):
    return "%08x" % int(np.asarray(v, F).view(np.uint32))


def run(prog, cases, env=None):
    """cases: dicts (kind, T, dt, u_max, standoff, reach, robot, box, goal, factors) -> list of float32 arrays [n, T, 2]"""
    lines = []
    for c in cases:
        fl = [c["dt"], c["u_max"][0], c["u_max"][1], c["standoff"], c["reach"], *c["robot"], *c["box"], *c["goal"], *c["factors"]]
        lines.append(" ".join([str(c["kind"]), str(len(c["factors"])), str(c["T"])] + [_hex(v) for v in fl]))
    r = subprocess.run([prog], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-2000:])
    rows = r.stdout.strip().split("\n")
    assert len(rows) == len(cases), (len(rows), len(cases))
    out = []
    for c, row in zip(cases, rows):
        w = np.array([int(x, 16) for x in row.split()], np.uint32)
        out.append(w.view(F).reshape(len(c["factors"]), c["T"], 2))
    return out


def case(kind, T, u_max, robot, box, goal, factors=FACTORS, dt=DT, standoff=STANDOFF, reach=REACH):
    """every float rounded to binary32 once: both sides start from the same numbers"""
    return dict(kind=kind, T=int(T), dt=F(dt), u_max=f32(u_max), standoff=F(standoff), reach=F(reach), robot=f32(robot),
                box=f32(box), goal=f32(goal), factors=f32(factors))


def all_cases():
    return [case(kind, T, um, *inp) for kind in (GO_TO, PUSH_BEHIND) for T in HORIZONS for um in U_MAX for inp in INPUTS]


def reference(c):
    """priors.go_to / priors.push_behind on the case's numbers (float64 inside, float32 out): [n, T, 2]"""
    args = (c["T"], float(c["dt"]), c["u_max"].astype(np.float64), [float(f) for f in c["factors"]])
    if c["kind"] == GO_TO:
        return A.go_to(c["robot"].astype(np.float64), c["goal"].astype(np.float64), *args)
    return A.push_behind(c["robot"].astype(np.float64), c["box"].astype(np.float64), c["goal"].astype(np.float64), *args,
                         standoff=float(c["standoff"]), reach=float(c["reach"]))


def replay(c):
    """the float64 controller written out once more, keeping what priors.py does not return: (controls [n, T, 2] float64,
    margins: | |behind - pos| - reach | at every test the unswitched push_behind makes, switched flags [n, T])"""
    T, dt = c["T"], float(c["dt"])
    lim = float(np.min(np.abs(c["u_max"].astype(np.float64))))
    robot, box, goal = (c[k].astype(np.float64) for k in ("robot", "box", "goal"))
    away = box - goal
    n = float(np.hypot(*away))
    away = away / n if n > 0.0 else np.array([1.0, 0.0])
    behind = box + float(c["standoff"]) * away
    out, margins = np.zeros((len(c["factors"]), T, 2)), []
    switched = np.zeros((len(c["factors"]), T), bool)
    for j, f in enumerate(c["factors"]):
        pos, sw = robot.copy(), c["kind"] == GO_TO
        for t in range(T):
            if not sw:
                gap = float(np.hypot(*(behind - pos)))
                margins.append(abs(gap - float(c["reach"])))
                sw = gap <= float(c["reach"])
            switched[j, t] = sw
            d = (goal if sw else behind) - pos
            dist = float(np.hypot(*d))
            if dist > 0.0:
                out[j, t] = d / dist * min(dist / dt, float(f) * lim)
            pos = pos + out[j, t] * dt
    return out, margins, switched


def extent(c):
    return float(max(np.abs(c["robot"]).max(), np.abs(c["box"]).max(), np.abs(c["goal"]).max())) + float(c["standoff"])


def bounds(c):
    """(bound on every control of the case, what the switch guard must exceed) -- the module docstring"""
    T, dt, X = c["T"], float(c["dt"]), extent(c)
    speed = float(np.max(c["factors"])) * float(np.min(np.abs(c["u_max"])))
    du = 16 * EPS * speed
    dp = 16 * EPS * speed * dt + 1.5 * EPS * X
    dh = 9 * EPS * float(c["standoff"]) + 1.5 * EPS * X if c["kind"] == PUSH_BEHIND else 0.0
    control = ((T - 1) * (dh + dp) + dh) / dt + du
    decision = T * (dh + dp) + dh + 3 * EPS * 2 * np.sqrt(2.0) * X
    return control, decision
