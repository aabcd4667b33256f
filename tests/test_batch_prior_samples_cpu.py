"""Batched command and lockstep episodes of point_env planners with prior samples (M3_BATCH_SECTION_POINT_PRIORS,
M3_EPISODES_PRIORS), the parts that need no GPU: the defines and what the library says to them without a
device, the five-section layout of the argument table as a host program (tests/native/batch_table_layout_host.cpp in its mode `pr`, once plain
and once under -fsanitize=address,undefined), and the Python layer's rules."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from m3p2i_aip_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


# ------------------------------------------------------------------ 1. defines and bits
def test_the_defines_and_the_bits_without_a_device():
    main = open(os.path.join(ROOT, "include", "m3p2i_hip.h")).read()
    ext = open(os.path.join(ROOT, "include", "m3p2i_hip_ext.h")).read()
    assert "#define M3_ABI_VERSION 4" in main
    for define, value in (("M3_BATCH_SECTION_POINT_PRIORS", 32), ("M3_EPISODES_PRIORS", 8)):
        assert re.search(rf"^#define {define} {value}$", ext, re.M), define
        assert define not in main.replace("M3_BATCH_SECTION_POINT_PRIORS, M3_EPISODES_PRIORS", "")   # (one pointer in a comment)
    assert (L.BATCH_SECTION_POINT_PRIORS, L.EPISODES_PRIORS) == (32, 8)
    # the older bits keep their values
    assert (L.BATCH_SECTION_PANDA_RUNTIME, L.BATCH_SECTION_POINT_ROLLOUT_SCENES, L.EPISODES_ROLLOUT_SCENES) == (1, 2, 1)
    lib = L.load()
    # (no batch can be created without a device: an accepted bit gets as far as the next check, an unknown one does not)
    for bits in (32, 32 | 2, 32 | 1):
        out = C.c_void_p(1)
        assert lib.m3_batch_create_sections(0, 0, bits, C.byref(out)) == -1 and out.value is None
        assert b"max_handles must be in 1 .. 65535" in lib.m3_batch_last_error(None)
    for bits in (64, 16, 8, 4, 32 | 64, 32 | 16):
        out = C.c_void_p(1)
        assert lib.m3_batch_create_sections(0, 0, bits, C.byref(out)) == -1 and out.value is None
        assert b"m3_batch_create_sections: unknown section bits" in lib.m3_batch_last_error(None)
    out = C.c_void_p(1)
    assert lib.m3_batch_create_ex(0, 4, 32, C.byref(out)) == -1 and b"unknown flag bits" in lib.m3_batch_last_error(None)
    for flags in (8, 8 | 1):
        eps = C.c_void_p(1)
        assert lib.m3_episodes_create_ex(None, None, None, 1, 1, 0, flags, C.byref(eps)) == -1 and eps.value is None
        assert lib.m3_episodes_last_error(None) == b"m3_episodes_create: null argument"
    for flags in (16, 2, 4, 8 | 16, 8 | 2):
        eps = C.c_void_p(1)
        assert lib.m3_episodes_create_ex(None, None, None, 1, 1, 0, flags, C.byref(eps)) == -1 and eps.value is None
        assert lib.m3_episodes_last_error(None) == b"m3_episodes_create_ex: unknown flag bits"


# ------------------------------------------------------------------ 2. the five-section layout, as a host program
def _build(tmp, extra=("-O2",)):
    out = str(tmp / "batch_table_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + list(extra) +
                          [os.path.join(HERE, "native", "batch_table_layout_host.cpp"), "-o", out])
    return out


def _run(prog):
    r = subprocess.run([prog, "pr"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    m = re.fullmatch(r"(\d+) checks, 0 failures\n", r.stdout)
    assert m and int(m.group(1)) > 10000, r.stdout


def test_every_five_section_split_is_aligned_ordered_disjoint_and_fits_the_slot(tmp_path):
    _run(_build(tmp_path))


def test_the_layout_program_under_the_sanitizers(tmp_path):
    _run(_build(tmp_path, extra=("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")))


# ------------------------------------------------------------------ 3. the Python layer
def test_command_batch_keeps_its_value_error_without_the_switch():
    from m3p2i_aip_amd import planner
    from tests.test_prior_controllers_cpu import _planner
    p = _planner()
    p.set_prior_controller("go_to", 2)
    with pytest.raises(ValueError, match=r"planner 0 has prior samples \(set_prior_samples\), which only its own command\(\)"):
        planner.command_batch([p], [np.zeros(4, np.float32)])
    # with the switch that check passes: the next one speaks (the stand-in engine is no HipEngine)
    with pytest.raises(ValueError, match="planner 0 does not run on the HIP library"):
        planner.command_batch([p], [np.zeros(4, np.float32)], point_priors=True)
    import inspect
    from m3p2i_aip_amd import engine, episodes
    for fn in (engine.HipBatch.__init__, engine.HipEpisodes.__init__, planner.command_batch, episodes.PointEpisodeSet.__init__,
               episodes.build_set, episodes.run_point_episodes):
        assert inspect.signature(fn).parameters["point_priors"].default is False, fn


def test_a_lockstep_set_takes_device_controllers_only():
    from m3p2i_aip_amd import compat
    from m3p2i_aip_amd.episodes import _check_episode_priors
    compat.install(force_standins=True)
    size = ["mppi.num_samples=64", "mppi.horizon=12"]
    host = compat.make_config("config_point", size + ["prior_samples={controller: go_to, n: 4}"])
    dev = compat.make_config("config_point", size + ["prior_samples={controller: go_to, n: 4, device: true}"])
    _check_episode_priors(compat.make_config("config_point", size), 0, False)
    _check_episode_priors(dev, 0, True)
    for flag in (False, True):
        with pytest.raises(ValueError, match="episode 3 asks for prior samples from a host controller"):
            _check_episode_priors(host, 3, flag)
    with pytest.raises(ValueError, match="episode 2 asks for prior samples .*only on request"):
        _check_episode_priors(dev, 2, False)

    class _P:
        def set_prior_controller(self, *a):
            self.got = a

    p = _P()
    compat.set_device_prior_controller(compat.make_config("config_point", ["task=push"] + size + ["prior_samples={controller: push_behind, n: 4, device: true}"]), p)
    assert p.got == ("push_behind", 4, [0, 1, 2, 3])
    compat.set_device_prior_controller(compat.make_config("config_point", ["task=navigation"] + size + ["prior_samples={controller: push_behind, n: 3, device: true}"]), p)
    assert p.got == ("go_to", 3, [0, 1, 2])          # (as the host path: no box to go behind)
    compat.set_device_prior_controller(compat.make_config("config_point", ["task=push_pull", "multi_modal=True"] + size + ["prior_samples={controller: push_behind, n: 4, device: true}"]), p)
    assert p.got == ("push_behind", 4, [1, 2, 33, 34])
