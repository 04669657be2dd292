"""bench.py's command line: a plain run times the steps and prints the result
line only, --full adds the other legs, --dump-outputs writes what the last
timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# keys only a --full run may hold: each needs runs of its own
FULL_ONLY = ("ed25519", "vrf", "kes", "leader", "single_item", "e2e", "raw_cbor", "cbor_abi",
             "inproc_cbor", "integrity_cbor", "byron_cbor", "latency", "cpu_baseline", "inproc")


def test_dump_outputs_sample(tmp_path):
    """dump_outputs on host tensors: every verdict, and for more than
    DUMP_BETA_ROWS headers the same ascending sample of rows on every call."""
    import torch

    sys.path.insert(0, ROOT)
    import bench

    n = bench.DUMP_BETA_ROWS + 4321
    g = torch.Generator().manual_seed(5)
    v = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
    be = torch.randint(0, 256, (n * 64,), dtype=torch.uint8, generator=g)
    bl = torch.randint(0, 256, (n * 64,), dtype=torch.uint8, generator=g)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), v, be, bl)
    got = {k: np.load(tmp_path / "a" / (k + ".npy"))
           for k in ("verdict", "beta_rows", "beta_eta", "beta_leader")}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in got)
    for k, a in got.items():
        assert a.dtype == (np.float64 if k == "beta_rows" else np.float32)
        assert np.array_equal(a, np.load(tmp_path / "b" / (k + ".npy")))
    rows = got["beta_rows"].astype(np.int64)
    assert rows.shape == (bench.DUMP_BETA_ROWS,) and (np.diff(rows) > 0).all()
    assert rows[0] >= 0 and rows[-1] < n
    assert np.array_equal(got["verdict"], v.numpy())
    assert np.array_equal(got["beta_eta"], be.view(n, 64).numpy()[rows])
    assert np.array_equal(got["beta_leader"], bl.view(n, 64).numpy()[rows])
    # the files of the default 1,048,576-header run stay within 64 MB
    assert 4 * (1 << 20) + bench.DUMP_BETA_ROWS * (8 + 2 * 64 * 4) <= 64e6


@pytest.mark.gpu
def test_plain_run_and_dump(gpu_lib, tmp_path):
    """One plain run on 4,096 headers: --steps sets the timed steps, the line
    holds ms_per_step and no --full leg, and the dumped arrays are the header
    kernel's results on the same synthetic inputs."""
    import torch

    sys.path.insert(0, ROOT)
    import bench

    n, steps = 4096, 3
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", "1", "--headers", str(n), "--dump-outputs",
                        str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "headers/s" and d["higher_is_better"]
    assert d["steps"] == steps and d["all_valid"] is True
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(n / (d["ms_per_step"] * 1e-3), rel=1e-3)
    assert not [k for k in FULL_ONLY if k in d]
    assert d["roofline"]["peak"] is None and d["roofline"]["clock_ghz"] is None

    dev = torch.device("cuda:0")
    t, _ = bench.synth_headers(n, 1024, dev)
    hdr = bench.DeviceHeaders(t, n, dev)
    hdr.launch(torch.cuda.current_stream())
    torch.cuda.synchronize()
    want = {"verdict": hdr.verdict.cpu().numpy(),
            "beta_rows": np.arange(n),
            "beta_eta": hdr.beta_eta.cpu().numpy().reshape(n, 64),
            "beta_leader": hdr.beta_leader.cpu().numpy().reshape(n, 64)}
    assert ((want["verdict"] & 15) == 15).all()
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in want)
    for k, w in want.items():
        a = np.load(out / (k + ".npy"))
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a, w), k
