"""The per-key VRF tables (csrc/verify.h vrfkey_base / vrfkey_fill /
vrf_u_fixed_lane, csrc/tpraos.h hdr_u_shared) and the workspace arithmetic of
their launch (csrc/vrfkey_ws.h) under AddressSanitizer + UBSan, in a
stand-alone program with its own main (tests/c/vrfkey_asan.cpp): built here
with -fsanitize=address,undefined and run as a subprocess.  Every table,
window and workspace region is a heap block of exactly its size.  Nothing is
loaded into Python and the environment is passed on as it is; the program must
exit clean with no mismatch between the table chain's U and the doubling
chain's."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")


def test_vrfkey_tables_under_asan_ubsan():
    subprocess.run(["make", "-C", CDIR, "-f", "Makefile.vrfkey_asan", "build/vrfkey_asan"],
                   check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    r = subprocess.run([os.path.join(CDIR, "build", "vrfkey_asan")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    words = r.stdout.split()
    assert words[0] == "keys" and int(words[1]) == 8
    assert words[2] == "chains" and int(words[3]) == 8 * 16
    assert words[4] == "mismatches" and int(words[5]) == 0
    assert words[6] == "layouts" and int(words[7]) == 45
