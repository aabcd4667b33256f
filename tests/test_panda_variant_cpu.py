"""Which panda_env kernels a handle runs (csrc/panda_variant.hpp) without a GPU.

A host program (tests/native/panda_variant_host.cpp, its own main) walks every input of the decision -- the 3 x 3 settings of
m3_set_panda_scene_instance / m3_set_panda_weighted_cost_instance x the 2^5 flags (workspace default, weights default, workspace
per sample, workspace per environment, sim_only): 288 inputs -- and compares, for the rollout, the step, the views, the cost and
the batch, the header's variant, both "used" records and the refusal that wins with the if-chains m3_api.hip had before the
header existed, transcribed into the program.  It also checks directly: all defaults give the literal kernels and both records 0;
rows on a side give the rows kernels and panda_scene_used = 1; the batch variant is 2 exactly with a workspace per sample; the
cost side never depends on geometry alone.  The same program is built and run once under -fsanitize=address,undefined.
"""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp, extra=("-O2",)):
    out = str(tmp / "panda_variant_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + list(extra) +
                          [os.path.join(HERE, "native", "panda_variant_host.cpp"), "-o", out])
    return out


def _run(prog, env=None):
    r = subprocess.run([prog], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    m = re.fullmatch(r"(\d+) checks, 0 failures\n", r.stdout)
    # 288 inputs; per input 2 predicates, 5 sides x 4 compared fields, 5 batch facts, 2 orders of the refusals: at least 29
    assert m and int(m.group(1)) >= 288 * 29, r.stdout
    return r.stderr


def test_every_input_decides_as_the_if_chains_did(tmp_path):
    _run(_build(tmp_path))


def test_the_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    prog = _build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    err = _run(prog, env=env)
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-2000:]
