"""The host Byron witness walker, in both passes, the host tx-id hash and the
message builder under AddressSanitizer + UBSan, in a stand-alone program with
its own main (tests/c/byron_witness_asan.cpp): built here with
-fsanitize=address,undefined and run as a subprocess over a file of
length-prefixed cases -- the case set, the magics, every single-byte flip and
every truncation of the reference's golden Byron block.  Nothing is loaded into
Python and the environment is passed on as it is; the program must exit clean,
having sliced as many blocks as byron_witness.parse_byron_witnesses accepts and
folded the statuses, counts, rows and messages this test restates from the
Python rule and hashlib."""
import hashlib
import os
import struct
import subprocess

import pytest

import byron_block_cases as C
import byron_witness_cases as WC
from ouroboros_network_amd import byron_witness as BW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")


def _words(b: bytes):
    return [int.from_bytes(b[4 * k:4 * k + 4], "little") for k in range(len(b) // 4)]


@pytest.mark.parametrize("magic", [-1, 24])
def test_byron_witness_walker_and_hashes_under_asan_ubsan(tmp_path, magic):
    subprocess.run(["make", "-C", CDIR, "-f", "Makefile.byron_witness_asan",
                    "build/byron_witness_asan"], check=True, stdout=subprocess.DEVNULL)
    cases = list(WC.case_set()["raws"]) + WC.magic_set()
    if magic < 0:
        cases += C.golden_flips() + C.golden_truncations()
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for r in cases:
            f.write(struct.pack("<I", len(r)))
            f.write(r)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    r = subprocess.run([os.path.join(CDIR, "build", "byron_witness_asan"), str(path), str(magic)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    words = r.stdout.split()
    assert words[0] == "cases" and int(words[1]) == len(cases)
    fold, ok = [0] * 8, 0
    for c in cases:
        st, ntx, nwit = BW.byron_witness_counts(c)
        x = [0] * 8
        if st == BW.PACK_OK:
            ok += 1
            b = BW.parse_byron_witnesses(c)
            ids = b.tx_ids(c)
            for w in b.witnesses:
                msg = BW.byron_witness_message(b.magic if magic < 0 else magic, w.kind, ids[w.tx])
                d = _words(hashlib.blake2b(msg, digest_size=32).digest())
                v, s = _words(w.vk64), _words(w.sig)
                x = [(x[k] * 31 + (d[k] ^ v[k] ^ v[8 + k] ^ s[k] ^ s[8 + k]) + w.kind + 3 * w.tx)
                     & 0xFFFFFFFF for k in range(8)]
        for k in range(8):
            fold[k] = (fold[k] * 1000003 + x[k] + st + 7 * ntx + 11 * nwit) & 0xFFFFFFFF
    assert int(words[3]) == ok and ok > 60
    assert words[4] == "digest" and [int(w, 16) for w in words[5:13]] == fold
