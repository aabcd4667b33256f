"""The layout of m3_batch_command's argument table (csrc/batch_table_layout.hpp) without a GPU.

A host program (tests/native/batch_table_layout_host.cpp, its own main) runs the product's layout function over every split
(n_plain, n_weighted, n_scene) with a sum of at most 12 and max_handles in {1, 2, 3, 7, 12}: every section starts on a multiple of
16, sections do not overlap, the order is plain / weighted / scene / update, and the total never exceeds what m3_batch_create
sizes a slot with for that max_handles.  The same program is built and run once under -fsanitize=address,undefined.
"""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp, extra=("-O2",)):
    out = str(tmp / "batch_table_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + list(extra) +
                          [os.path.join(HERE, "native", "batch_table_layout_host.cpp"), "-o", out])
    return out


def _run(prog, env=None):
    r = subprocess.run([prog], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    m = re.fullmatch(r"(\d+) checks, 0 failures\n", r.stdout)
    assert m and int(m.group(1)) > 10000, r.stdout
    return r.stderr


def test_every_split_is_aligned_ordered_disjoint_and_fits_the_slot(tmp_path):
    _run(_build(tmp_path))


def test_the_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    prog = _build(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    err = _run(prog, env=env)
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-2000:]
