"""The host block slicer and the host streaming Blake2b under AddressSanitizer
+ UBSan, in a stand-alone program with its own main (tests/c/block_asan.cpp):
built here with -fsanitize=address,undefined and run as a subprocess over a
file of length-prefixed cases -- the golden blocks, every single-byte flip of
the case set, every truncation of the golden blocks, and the malformed shapes.
Nothing is loaded into Python and the environment is passed on as it is; the
program must exit clean, having sliced as many blocks as block.parse_block
accepts and folded the statuses and hashes this test computes itself."""
import os
import struct
import subprocess

import block_cases as BC
from ouroboros_network_amd import block as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")


def _cases():
    cs = BC.case_set()
    out = [r for r, k in zip(cs["raws"], cs["kinds"]) if k in ("golden", "byron")]
    out += [r for r, k in zip(cs["raws"], cs["kinds"]) if k.startswith("flip_") or k == "shape"]
    for b in BC.golden():                      # every truncation of every golden block
        raw = bytes.fromhex(b["raw"])
        out += [raw[:cut] for cut in range(len(raw))]
    small = [r for r, k in zip(cs["raws"], cs["kinds"]) if k == "synthetic" and len(r) < 3000]
    for raw in small[:6]:                      # every single-byte flip of a few small blocks
        for pos in range(0, len(raw)):
            r = bytearray(raw)
            r[pos] ^= 0x81
            out.append(bytes(r))
    return out


def test_block_slicer_and_blake2b_under_asan_ubsan(tmp_path):
    subprocess.run(["make", "-C", CDIR, "-f", "Makefile.block_asan", "build/block_asan"],
                   check=True, stdout=subprocess.DEVNULL)
    cases = _cases()
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for r in cases:
            f.write(struct.pack("<I", len(r)))
            f.write(r)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    r = subprocess.run([os.path.join(CDIR, "build", "block_asan"), str(path)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    words = r.stdout.split()
    assert words[0] == "cases" and int(words[1]) == len(cases)
    assert int(words[3]) == sum(B.block_status(c) == B.PACK_OK for c in cases)
    # the program's fold of every status, body hash and whole-case hash,
    # restated here from parse_block and hashlib
    fold = [0] * 8
    for c in cases:
        try:
            st, h = B.PACK_OK, B.parse_block(c).bb_hash(c)
        except B.BlockError as e:
            st, h = e.status, bytes(32)
        w = BC.b2b(c)
        for k in range(8):
            x = int.from_bytes(h[4 * k:4 * k + 4], "little") ^ int.from_bytes(w[4 * k:4 * k + 4],
                                                                             "little")
            fold[k] = (fold[k] * 1000003 + x + st) & 0xFFFFFFFF
    assert words[4] == "digest" and [int(x, 16) for x in words[5:13]] == fold
