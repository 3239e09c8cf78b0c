"""bench.py without --full, as it is run for the headline: the timed steps alone, and --dump-outputs writing what the last timed
step handed back (small genome)."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    B = 100000
    # a child process (never an exec of this one, which may have touched the GPU)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--genome-size", "2.5e8", "--batch-pairs", str(B),
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:].decode(errors="replace")
    rec = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["value"] > 0 and rec["ms_per_step"] > 0
    assert abs(rec["value"] - 2 * B / rec["ms_per_step"] / 1e3) < 1e-3 * rec["value"] + 1e-3
    # what only --full measures is not in a plain run
    assert rec["cpu_baseline"] is None
    for k in ("resident_value", "resident_ms_per_step", "secondary", "realistic", "pecaller"):
        assert k not in rec
    m1, m2, mt = (np.load(out / (n + ".npy")) for n in ("m1", "m2", "mapping_type"))
    for x in (m1, m2, mt):
        assert x.dtype == np.float64 and x.shape == (B,) and np.array_equal(x, np.floor(x)) and (x >= 0).all()
    assert not (out / "pair_index.npy").exists()
    # the last step's mapped share is the run's (mapped_frac: over the 3 timed steps)
    assert abs(((m1 > 0).sum() + (m2 > 0).sum()) / (2.0 * B) - rec["mapped_frac"]) < 0.02
    assert mt.max() <= 8          # PEMAP_UNIQUE_MATE .. PEMAP_NEITHER_MAP
