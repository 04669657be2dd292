"""The host Byron block walker, in both passes, and the host hashes of the body
proof under AddressSanitizer + UBSan, in a stand-alone program with its own
main (tests/c/byron_block_asan.cpp): built here with
-fsanitize=address,undefined and run as a subprocess over a file of
length-prefixed cases -- the case set, every single-byte flip and every
truncation of the reference's golden Byron block.  Nothing is loaded into
Python and the environment is passed on as it is; the program must exit clean,
having sliced as many regular blocks as byron_block.parse_byron_block accepts
and folded the statuses, counts, bits, roots and messages this test restates
from the Python rule and hashlib."""
import hashlib
import os
import struct
import subprocess

import byron_block_cases as C
from ouroboros_network_amd import byron_block as BB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")


def _words(b: bytes):
    return [int.from_bytes(b[4 * k:4 * k + 4], "little") for k in range(len(b) // 4)]


def test_byron_block_walker_and_hashes_under_asan_ubsan(tmp_path):
    subprocess.run(["make", "-C", CDIR, "-f", "Makefile.byron_block_asan",
                    "build/byron_block_asan"], check=True, stdout=subprocess.DEVNULL)
    cases = list(C.case_set()["raws"]) + C.golden_flips() + C.golden_truncations()
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for r in cases:
            f.write(struct.pack("<I", len(r)))
            f.write(r)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    # (-1: each header's own magic, so the magic rule holds and the program's
    # verdict is the rule's with the signature taken as valid)
    r = subprocess.run([os.path.join(CDIR, "build", "byron_block_asan"), str(path), "-1"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    words = r.stdout.split()
    assert words[0] == "cases" and int(words[1]) == len(cases)
    fold, ok = [0] * 8, 0
    for c in cases:
        st, v, root = BB.byron_block_rule(c, "header", lambda sig, msg, key: True)
        _, ntx, gb, mb = BB.byron_block_counts(c, "header")
        x = [0] * 8
        if st == BB.PACK_OK:
            ok += 1
            b = BB.parse_byron_block(c)
            hm = hashlib.blake2b(b.message(-1), digest_size=32).digest()
            s = _words(b.sig)
            x = [p ^ q ^ k ^ s0 ^ s1 for p, q, k, s0, s1 in zip(
                _words(root), _words(hm), _words(b.delegate_xpub[:32]), s[:8], s[8:])]
        for k in range(8):
            fold[k] = (fold[k] * 1000003 + x[k] + st + 7 * ntx + 11 * gb + 13 * mb + 17 * v) \
                & 0xFFFFFFFF
    assert int(words[3]) == ok and ok > 500
    assert words[4] == "digest" and [int(w, 16) for w in words[5:13]] == fold
