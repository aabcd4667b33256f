"""Which kernels an importance-weight update runs, on which view, under which protocol (csrc/update_plan.hpp) without a GPU.

A host program (tests/native/update_plan_host.cpp, its own main) walks the full product of the decision's inputs -- shard_mix
0..3 x unsharded / 2 / 4 / 32 ranks x single / simple / simple with cfg.multi_modal / multi x nu 2 / 9 (and 1, for T * nu = 2048 |
2049 exactly) x three horizons per nu (short, the last product <= 2048, the first beyond) x K at 20, 2048, 4096, 8192, 16384,
131072 each with -1 / 0 / +1, as K_global and (sharded) as K_local: 18144 handles; per handle five launches on / off x rollout
minima on / off x the entry points m3_update (phases and fused), m3_update_finalize / m3_command, m3_update_b, m3_finalize --
and compares the header's protocol predicates, allocation answers, refusals (code and text) and ordered launch steps with their
views, destinations, flags and tails with the code of m3_api.hip / update_small.hip as it stood before the header existed,
transcribed into the program.  Zero differences; nothing sampled.  The same program is built and run once under
-fsanitize=address,undefined.
"""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp, extra=("-O2",)):
    out = str(tmp / "update_plan_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + list(extra) +
                          [os.path.join(HERE, "native", "update_plan_host.cpp"), "-o", out])
    return out


def _run(prog, env=None):
    r = subprocess.run([prog], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    m = re.fullmatch(r"(\d+) handles, (\d+) checks, 0 failures\n", r.stdout)
    # 4 shard_mix x (1 + 3 * 2) rank layouts x 4 modes x 3 nu x 3 T x 18 K; per handle 12 facts + 2 x 2 x 5 entries with at least
    # 4 comparisons each (refused or not, count, tail)
    assert m and int(m.group(1)) == 4 * 7 * 4 * 3 * 3 * 18 and int(m.group(2)) >= int(m.group(1)) * (12 + 20 * 4), r.stdout
    return r.stderr


def test_every_input_plans_as_the_if_chains_did(tmp_path):
    _run(_build(tmp_path))


def test_the_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    prog = _build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    err = _run(prog, env=env)
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-2000:]
