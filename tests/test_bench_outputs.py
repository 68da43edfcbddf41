"""bench.py's plain run and --dump-outputs, on the CPU oracle at a size it
steps in about a second: the result line keeps its headline fields and leaves
the --full figures out, the dumped arrays are float64 files under the size cap,
and two runs with the same arguments dump the same arrays."""
import glob
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(REPO, "oracle", "_build", "libgossip_oracle.so")


def _bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--workload", "config3", "--peers", "100",
           "--steps", str(steps), "--warmup", "1", "--lib", ORACLE, "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [x for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    arrays = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(str(out_dir), "*.npy"))}
    return json.loads(lines[0]), arrays


def test_plain_line_and_dump(tmp_path):
    line, a = _bench(tmp_path / "a", 1)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    # one step = one round of 10 hops with 1000 messages published
    assert line["events_per_step"]["deliveries"] > 0
    for k in ("roofline", "rooflines_other", "cpu_baseline", "device_gib"):
        assert k not in line, k
    assert {"counters", "scores", "behaviour_penalty", "mesh_count", "mesh_topics", "topic_fmd"} <= set(a)
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64e6
    assert len(a["scores"]) == len(a["sample_edges"]) and np.isfinite(a["scores"]).all()
    assert a["mesh_count"].sum() > 0  # meshes formed and were read back
    _, b = _bench(tmp_path / "b", 1)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
