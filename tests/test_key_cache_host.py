"""The key directory (csrc/key_cache.h) on the host: tests/c/key_cache_asan.cpp
drives the text the kernels compile, pass by pass as the header launch does,
over a directory of 16 cells and 12 slots so that probes collide.  The program
is built twice, plainly and with -fsanitize=address,undefined, and run as a
child process; nothing is loaded into Python and the environment is passed on
as it is.  Every check prints a line of its own, which the tests below look
for by name."""
import functools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")

CHECKS = [
    "layout",
    "layout_rejects",
    "insert_12",                          # 12 keys, each three times in the batch
    "lookup_12",
    "generation_distinct_count",          # the batch again: 12 first stamps, nothing built
    "distinct_of_this_batch",             # a sub-batch counts its own keys only
    "equal_hash_other_bytes_absent",
    "full_empties_and_reinserts",         # a 13th key: emptied, the batch's keys inserted again
    "emptied_forgets_the_rest",
    "equal_hash_kept_apart",
    "certificates_full_takes_new_only",
    "more_new_than_slots_not_inserted",
    "over_the_limit_inserts_nothing",
    "probe_cap",
]


@functools.lru_cache(maxsize=None)
def _run(target):
    subprocess.run(["make", "-C", CDIR, "-f", "Makefile.key_cache_asan", "build/" + target],
                   check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    return subprocess.run([os.path.join(CDIR, "build", target)], env=env, capture_output=True,
                          text=True, timeout=120)


@pytest.mark.parametrize("name", CHECKS)
def test_directory(name):
    r = _run("key_cache_host")
    assert "ok " + name in r.stdout.splitlines(), r.stdout + r.stderr


def test_every_check_is_listed_and_the_program_exits_clean():
    r = _run("key_cache_host")
    assert r.returncode == 0, r.stdout + r.stderr
    assert [ln.split()[1] for ln in r.stdout.splitlines()] == CHECKS


def test_directory_under_asan_ubsan():
    r = _run("key_cache_asan")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert [ln.split() for ln in r.stdout.splitlines()] == [["ok", c] for c in CHECKS]
