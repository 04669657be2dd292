"""The host prover and the host leader schedule (csrc/forge.h, csrc/prove.h)
under AddressSanitizer + UBSan, in a stand-alone program with its own main
(tests/c/prove_asan.cpp): built here with -fsanitize=address,undefined and run
as a subprocess over a file of records -- certified VRFs over alphas of every
boundary length, each ending at the last byte of its allocation, and the
schedule's parameter sets with rows of exactly n items.  Nothing is loaded
into Python and the environment is passed on as it is; the program must exit
clean, and the digest it folds from every proof, output, class and index must
be the one this test folds from the oracle's."""
import os
import struct
import subprocess

import forge_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")
M32 = 0xFFFFFFFF
N_SCHED = 40


def _words(b: bytes):
    return [int.from_bytes(b[4 * k:4 * k + 4], "little") for k in range(len(b) // 4)]


def _records():
    """(bytes of the record, its expected contribution x[8])"""
    out = []
    ks = FC.keys()[:26]
    alphas, _, _, _ = FC.prove_inputs(len(ks), lens=FC.ALPHA_LENS, seed=9)
    for (_, sk), a in zip(ks, alphas):
        x = [0] * 8
        pi, beta = FC.oracle_prove(sk, a)
        for k, w in enumerate(_words(pi)):
            x[k & 7] ^= w
        for k, w in enumerate(_words(beta)):
            x[k & 7] = (x[k & 7] + w) & M32
        out.append((b"P" + sk + struct.pack("<I", len(a)) + a, x))
    sk = FC.pool_key()
    for name, ps in FC.param_sets(N_SCHED).items():
        L = ps["L"] & ((1 << 128) - 1)
        rec = b"S" + sk + struct.pack("<I", 0 if ps["eta0"] is None else 1)
        rec += ps["eta0"] or bytes(32)
        rec += struct.pack("<II", 1 if ps["f_is_one"] else 0, ps["ngen"])
        rec += struct.pack("<9Q", ps["epoch_first_slot"], ps["sigma"].numerator,
                           ps["sigma"].denominator, L & ((1 << 64) - 1), L >> 64,
                           ps["d"].numerator, ps["d"].denominator, ps["asc_inv"] or 1,
                           ps["first_slot"])
        rec += struct.pack("<I", N_SCHED)
        cls, gen, beta = FC.restate(sk, ps, N_SCHED)
        x = [0] * 8
        for i in range(N_SCHED):
            x[i & 7] = (x[i & 7] + int(cls[i]) * 0x9E3779B1 + int(gen[i])) & M32
            for k, w in enumerate(_words(bytes(beta[i]))):
                x[k & 7] ^= (w + i) & M32
        out.append((rec, x))
    return out


def test_prover_and_schedule_under_asan_ubsan(tmp_path):
    subprocess.run(["make", "-C", CDIR, "-f", "Makefile.prove_asan", "build/prove_asan"],
                   check=True, stdout=subprocess.DEVNULL)
    recs = _records()
    path = tmp_path / "records.bin"
    with open(path, "wb") as f:
        for r, _ in recs:
            f.write(r)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    r = subprocess.run([os.path.join(CDIR, "build", "prove_asan"), str(path)], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    words = r.stdout.split()
    assert words[0] == "records" and int(words[1]) == len(recs)
    fold = [0] * 8
    for _, x in recs:
        for k in range(8):
            fold[k] = (fold[k] * 1000003 + x[k]) & M32
    assert words[2] == "digest" and [int(v, 16) for v in words[3:11]] == fold
