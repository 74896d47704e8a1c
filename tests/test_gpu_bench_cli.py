"""GPU: bench.py's plain line and --dump-outputs.  A plain run times the steps and prints the headline fields, nothing
else; --dump-outputs writes what the last timed step computed, the same arrays from run to run on the same arguments,
and those arrays are the path's real results (checked against the C oracle on a prefix)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 3000


def _bench(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--frames", str(F), "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    line = _bench(a)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "markers/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["full"] is False
    for k in ("parity", "cpu_baseline", "latency", "blob_stage", "configs", "ba"):
        assert k not in line, k                          # --full only
    _bench(b)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) == sorted(n + ".npy" for n in ("frames", "xyz", "err", "corr", "n_out", "status", "n_cand"))
    assert sum(os.path.getsize(a / n) for n in names) <= 64 << 20
    got = {n[:-4]: np.load(a / n) for n in names}
    for n in names:                                      # same inputs, same outputs, bit for bit
        assert got[n[:-4]].dtype in (np.float32, np.float64), n
        assert np.isfinite(got[n[:-4]]).all(), n
        assert np.array_equal(got[n[:-4]], np.load(b / n)), n
    assert np.array_equal(got["frames"], np.arange(F)) and (got["status"] == 0).all() and got["n_out"].shape == (F,)
    P = int(got["n_out"].sum())                           # the points of every frame, packed in frame order
    assert got["xyz"].shape == (P, 3) and got["err"].shape == (P,) and got["corr"].shape == (P, 8)

    # the dumped arrays are the path's results: rank 0's stream (seed 1) through the C oracle, first frames
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "low-cost-mocap_amd"))
    from mocap_core import synth
    from oracle import c_oracle
    rig = synth.ring_rig(8)
    blobs, counts, _ = synth.make_blob_stream(rig, F, 16, seed=1)
    n = 64
    ref = c_oracle.COracle(rig["K"], rig["R"], rig["t"]).match_triangulate(blobs[:n], counts[:n], gate_px=5.0, K_max=48)
    assert np.array_equal(got["n_out"][:n], ref["n_out"])
    vv = np.arange(48)[None, :] < ref["n_out"][:, None]
    p = int(ref["n_out"].sum())
    assert np.array_equal(got["corr"][:p], ref["corr"][vv])
    assert np.abs(got["xyz"][:p] - ref["xyz"][vv]).max() / np.abs(ref["xyz"][vv]).max() < 1e-5
