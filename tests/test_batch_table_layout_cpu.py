"""The layout of m3_batch_command's argument table (csrc/batch_table_layout.hpp) without a GPU.

A host program (tests/native/batch_table_layout_host.cpp, its own main; mode `sections`) runs the product's one layout function
over every split (n_plain, n_weighted, n_scene) with a sum of at most 12 and max_handles in {1, 2, 3, 7, 12}: every section starts
on a multiple of 16, sections do not overlap, the order is plain / weighted / scene / update, and the total never exceeds what
m3_batch_create sizes a slot with for that max_handles.  Its mode `frozen` holds the one layout and the one capacity against a
transcription of the header as it stood with one function per generation of sections: all 8 combinations of the section bits,
every split of up to 12 handles, max_handles 1 .. 40, on the library's entry sizes.  Each mode is built and run once plain and
once under -fsanitize=address,undefined.  (The modes rt, sv and pr: tests/test_batch_panda_runtime_cpu.py,
test_batch_point_rollout_scenes_cpu.py, test_batch_prior_samples_cpu.py.)
"""
import os
import re
import subprocess

from tests.test_batch_panda_runtime_cpu import entry_sizes  # noqa: F401  (the fixture: sizeof the panda entries and UpdateArgs)

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(tmp, extra=("-O2",)):
    out = str(tmp / "batch_table_layout_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + list(extra) +
                          [os.path.join(HERE, "native", "batch_table_layout_host.cpp"), "-o", out])
    return out


SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _run(prog, mode=("sections",), env=None):
    r = subprocess.run([prog] + [str(x) for x in mode], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    m = re.fullmatch(r"(\d+) checks, 0 failures\n", r.stdout)
    assert m and int(m.group(1)) > 10000, r.stdout
    return r.stderr


def test_every_split_is_aligned_ordered_disjoint_and_fits_the_slot(tmp_path):
    _run(_build(tmp_path))


def _run_sanitized(tmp_path, mode):
    prog = _build(tmp_path, SANITIZE)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    err = _run(prog, mode, env=env)
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-2000:]


def test_the_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    _run_sanitized(tmp_path, ["sections"])


def test_the_one_layout_gives_the_offsets_and_slot_sizes_of_the_layout_per_generation(tmp_path, entry_sizes):
    _run(_build(tmp_path), ["frozen"] + entry_sizes)


def test_the_comparison_with_the_layout_per_generation_is_clean_under_asan_and_ubsan(tmp_path, entry_sizes):
    _run_sanitized(tmp_path, ["frozen"] + entry_sizes)
