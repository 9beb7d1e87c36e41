"""bench.py's command line: a plain run prints the headline line alone, --full adds
the figures that take runs of their own, --dump-outputs writes what the last timed step
computed (checked against the oracle's tick on the same synthetic state)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "distributed-faas_amd"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

FULL_ONLY = ("cpu_baseline", "reference_python_value", "host_observed")
W, T, STEPS = 4096, 50000, 3


def test_dump_outputs_samples_large_arrays(tmp_path):
    """Up to the cap an array is written whole (shape kept); beyond it, the same sorted
    sample every time, float64; an empty array gets no file."""
    import bench
    big = np.arange(bench.DUMP_MAX_ELEMS + 12345, dtype=np.int64) * 3
    small = np.arange(12, dtype=np.int32).reshape(3, 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), dict(big=big, small=small, empty=np.zeros(0, np.uint8)))
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float64 and a.shape == (bench.DUMP_MAX_ELEMS,)
    assert np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and np.all(a % 3 == 0) and a.max() <= big.max()
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small)
    assert not (tmp_path / "a" / "empty.npy").exists()  # an empty output is left out


def _run(*extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
           "--workers", str(W), "--tasks", str(T), *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_headline_and_dump(tmp_path):
    from faasbal import synth
    from oracle import Oracle
    line = _run("--dump-outputs", str(tmp_path))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == STEPS and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0
    # the headline is the committed tick (value / ms_per_step carry the commit's delta)
    assert line["ms_per_step"] == line["committed"]["ms_per_step_with_commit"]
    assert line["value"] == line["committed"]["value_with_commit"]
    for k in FULL_ONLY:
        assert k not in line
    assert "kernels_avg_ms" not in line["tick"] and "frac" not in line["roofline"]
    # the dumped step against the oracle's tick on the same state
    st = synth.zipf_state(W=W, seed=0)
    o = Oracle(W, 2 * len(st["log"]) + T + 16, purge_mode=1)
    o.load(st["reg"], st["free"], st["hb"], st["epoch"], st["queue"], st["log"])
    ref = o.tick(1000.0, 10.0, [], [], [], [], [], T)
    for k in ("assign", "orphans", "evicted"):
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, np.asarray(ref[k], np.float64), err_msg=k)
    res = np.load(tmp_path / "result.npy")
    assert res[0] == len(ref["assign"]) == line["config"]["assigned_per_tick"]
    assert res[1] == len(ref["orphans"]) and res[4] == len(ref["evicted"])
    # every file holds something: an empty list is left out (its count is in the record)
    assert sorted(os.listdir(tmp_path)) == ["assign.npy", "evicted.npy", "orphans.npy", "result.npy"]
    assert all(np.load(tmp_path / f).size > 0 for f in os.listdir(tmp_path))


@pytest.mark.gpu
def test_full_run_adds_the_rest():
    line = _run("--full", "--cpu-budget", "0.2")
    for k in FULL_ONLY:
        assert k in line
    assert set(line["tick"]["kernels_avg_ms"]) and line["roofline"]["frac"] > 0
    assert line["steps"] == STEPS
    assert line["ms_per_step"] == line["committed"]["ms_per_step_with_commit"]
