"""The Byron ledger-view checks' host side (csrc/sha3.h, csrc/pbft_view.h, the
window fold and the host check entry of csrc/pbft_api.cpp) under
AddressSanitizer + UBSan, in a stand-alone program with its own main
(tests/c/pbft_asan.cpp): built here with -fsanitize=address,undefined and run
as a subprocess over a case file -- a three-entry schedule, an incoming window
and rows of every outcome, each array in a heap buffer of exactly its size.
Nothing is loaded into Python and the environment is passed on as it is; the
program must exit clean, and the digests it folds must be the ones this test
folds from hashlib and pbft.pbft_rule."""
import hashlib
import os
import struct
import subprocess

import numpy as np

import pbft_cases as PC
from ouroboros_network_amd import pbft as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")
M32 = 0xFFFFFFFF


class Fold:
    def __init__(self):
        self.x = 0

    def add(self, v):
        self.x = (self.x * 1000003 + (int(v) & M32)) & M32

    def words(self, b):
        for k in range(len(b) // 4):
            self.add(int.from_bytes(b[4 * k:4 * k + 4], "little"))


def test_host_side_under_asan_ubsan(tmp_path):
    subprocess.run(["make", "-C", CDIR, "-f", "Makefile.pbft_asan", "build/pbft_asan"],
                   check=True, stdout=subprocess.DEVNULL)
    v = PC.schedule(3, 3, 10, 3)
    vk, slot, status = PC.rows(340, 3, 3, 103)
    st0 = P.PBftState([(0, PC.gen_id(1)), (0, b"\x77" * 28), (1, PC.gen_id(0))])
    rec = struct.pack("<IQQ", len(v.entries), v.window, v.threshold)
    rec += v.first_slot.tobytes() + v.dlg_begin.tobytes()
    for r in range(v.rows):
        rec += v.delegate_id[r].tobytes() + v.genesis_id[r].tobytes()
    rec += struct.pack("<I", len(st0.signers))
    for s, g in st0.signers:
        rec += struct.pack("<Q", s) + g
    rec += struct.pack("<I", len(slot))
    for i in range(len(slot)):
        rec += vk[i].tobytes() + struct.pack("<QB", int(slot[i]), int(status[i]))
    path = tmp_path / "cases.bin"
    path.write_bytes(rec)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    r = subprocess.run([os.path.join(CDIR, "build", "pbft_asan"), str(path)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    lines = r.stdout.splitlines()
    f = Fold()
    for n in range(136):
        f.words(hashlib.sha3_256(bytes(n)).digest())
    assert lines[0] == "sha3 %08x" % f.x
    keys = [k.tobytes() for k in vk]
    bits, rows, cnt, after = P.pbft_rule(v, keys, slot.tolist(), status.tolist(), st0)
    f = Fold()
    for i in range(len(slot)):
        f.add(bits[i])
        f.add(rows[i])
        f.add(int(cnt[i]) & M32)
        f.add(int(cnt[i]) >> 32)
        f.words(P.key_hash(keys[i]))
    f.add(len(after.signers))
    for s, g in after.signers:
        f.add(s & M32)
        f.add(s >> 32)
        f.words(g)
    assert lines[1] == "rows %d fold %08x" % (len(slot), f.x)
    assert np.count_nonzero(bits) > 100
