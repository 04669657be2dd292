"""The host witness walker, in both passes, and the host streaming Blake2b
under AddressSanitizer + UBSan, in a stand-alone program with its own main
(tests/c/witness_asan.cpp): built here with -fsanitize=address,undefined and
run as a subprocess over a file of length-prefixed cases -- the case set,
every truncation of the golden blocks and every single-byte flip of a few
small blocks.  Nothing is loaded into Python and the environment is passed on
as it is; the program must exit clean, having sliced as many blocks as
witness.parse_witnesses accepts and folded the statuses, counts, tx ids and
rows this test restates from parse_witnesses and hashlib."""
import os
import struct
import subprocess

import block_cases as BC
import witness_cases as WC
from ouroboros_network_amd import block as B
from ouroboros_network_amd import witness as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")


def _cases():
    out = list(WC.case_set()["raws"])
    for b in BC.golden():                      # every truncation of every golden block
        raw = bytes.fromhex(b["raw"])
        out += [raw[:cut] for cut in range(len(raw))]
    small = [WC.small_block()] + [r for r, _ in WC.valid() if len(r) < 3000][:3]
    for raw in small:                          # every single-byte flip of a few small blocks
        for pos in range(len(raw)):
            r = bytearray(raw)
            r[pos] ^= 0x81
            out.append(bytes(r))
    return out


def _words(b: bytes):
    return [int.from_bytes(b[4 * k:4 * k + 4], "little") for k in range(len(b) // 4)]


def test_witness_walker_and_blake2b_under_asan_ubsan(tmp_path):
    subprocess.run(["make", "-C", CDIR, "-f", "Makefile.witness_asan", "build/witness_asan"],
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
    r = subprocess.run([os.path.join(CDIR, "build", "witness_asan"), str(path)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    words = r.stdout.split()
    assert words[0] == "cases" and int(words[1]) == len(cases)
    fold, ok = [0] * 8, 0
    for c in cases:
        x, st, ntx, nwit, extra = [0] * 8, B.PACK_OK, 0, 0, 0
        try:
            p = W.parse_witnesses(c)
        except B.BlockError as e:
            st = e.status
        else:
            ok += 1
            ntx, nwit = len(p.tx_spans), len(p.witnesses)
            for h in p.tx_ids(c):
                x = [a ^ b for a, b in zip(x, _words(h))]
            for w in p.witnesses:
                s = _words(w.sig)
                x = [a ^ b ^ c0 ^ c1 for a, b, c0, c1 in zip(x, _words(w.vk), s[:8], s[8:])]
                extra += 3 * w.tx + w.kind
        for k in range(8):
            fold[k] = (fold[k] * 1000003 + x[k] + st + 7 * ntx + 11 * nwit + extra) & 0xFFFFFFFF
    assert int(words[3]) == ok
    assert words[4] == "digest" and [int(v, 16) for v in words[5:13]] == fold
