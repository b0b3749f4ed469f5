"""bench.py's command line: a plain run prints the headline figure only, `--full` adds every other measurement and the
self-check, `--dump-outputs DIR` writes the last timed request's result as float64 arrays that are the same from run to
run (the synthetic data is seeded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("ms_per_request_latency", "ms_per_step_sequential", "roofline", "precomputed", "host_ms_per_request",
             "cpu_baseline", "checked", "check_errors")

TREE = {"hosts": {"sum_other_doc_count": 5, "buckets": [
    {"key": "host-0001", "doc_count": 3, "per_hour": {"buckets": [
        {"key": 0, "doc_count": 3, "rt": {"count": 3, "min": None, "sum": 4.5}}]}},
    {"key": "host-0002", "doc_count": 2, "per_hour": {"buckets": [
        {"key": 0, "doc_count": 2, "rt": {"count": 2, "min": 1.0, "sum": 4.5}},
        {"key": 3600000, "doc_count": 0, "rt": {"count": 0, "min": float("inf"), "sum": 0.0}}]}}]}}


def _bench():
    sys.path.insert(0, REPO)
    import bench
    return bench


def _load(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_one_float64_array_per_value_path(tmp_path):
    _bench().dump_outputs(str(tmp_path / "d"), TREE)
    got = _load(tmp_path / "d")
    assert all(a.dtype == np.float64 and a.ndim == 1 for a in got.values())
    assert sorted(got) == sorted(n + ".npy" for n in (
        "hosts.sum_other_doc_count", "hosts.buckets.key.crc32", "hosts.buckets.doc_count",
        "hosts.buckets.per_hour.buckets.key", "hosts.buckets.per_hour.buckets.doc_count",
        "hosts.buckets.per_hour.buckets.rt.count", "hosts.buckets.per_hour.buckets.rt.min",
        "hosts.buckets.per_hour.buckets.rt.sum"))
    assert got["hosts.buckets.doc_count.npy"].tolist() == [3.0, 2.0]
    assert got["hosts.buckets.per_hour.buckets.key.npy"].tolist() == [0.0, 0.0, 3600000.0]
    assert got["hosts.buckets.per_hour.buckets.rt.sum.npy"].tolist() == [4.5, 4.5, 0.0]
    mins = got["hosts.buckets.per_hour.buckets.rt.min.npy"]
    assert np.isnan(mins[0]) and mins[1] == 1.0 and np.isinf(mins[2])
    keys = got["hosts.buckets.key.crc32.npy"]
    assert keys[0] != keys[1] and all(k == int(k) and 0 <= k < 2 ** 32 for k in keys)


def test_dump_outputs_caps_its_size_with_a_fixed_sample(tmp_path, monkeypatch):
    bench = _bench()
    tree = {"h": {"buckets": [{"key": i, "doc_count": 2 * i} for i in range(1000)]}, "n": 7}
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 8 * 100)  # 3 arrays: 100 values each
    bench.dump_outputs(str(tmp_path / "a"), tree)
    bench.dump_outputs(str(tmp_path / "b"), tree)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= 3 * 8 * 100
    assert a["n.npy"].tolist() == [7.0]
    k, c = a["h.buckets.key.npy"], a["h.buckets.doc_count.npy"]
    assert len(k) == 100 and np.all(np.diff(k) > 0) and set(k) <= set(range(1000))  # positions kept in order
    assert np.array_equal(c, 2 * k)  # arrays of one level are cut at the same positions
    assert all(np.array_equal(a[f], b[f]) for f in a) and sorted(a) == sorted(b)  # the same sample every run


def _run(*extra):
    r = subprocess.run([sys.executable, "-s", os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--docs", str(1 << 20), *extra], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_repeatable_outputs(tmp_path):
    a = _run("--dump-outputs", str(tmp_path / "a"))
    b = _run("--dump-outputs", str(tmp_path / "b"))
    for line in (a, b):
        assert all(k in line for k in HEADLINE) and not any(k in line for k in FULL_ONLY)
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx((1 << 20) / (line["ms_per_step"] / 1e3))
    da, db = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(da) == sorted(db) and da
    for f in da:
        assert da[f].dtype == np.float64 and np.array_equal(da[f], db[f], equal_nan=True), f
    # every doc of the shard is in one of the ten terms or in sum_other_doc_count
    assert da["hosts.buckets.doc_count.npy"].sum() + da["hosts.sum_other_doc_count.npy"].sum() == 1 << 20
    assert da["hosts.buckets.per_hour.buckets.rt.count.npy"].sum() == da["hosts.buckets.doc_count.npy"].sum()


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements_and_the_self_check():
    line = _run("--full", "--cpu-docs", "200000", "--cpu-threads", "2", "--cpu-single-docs", "100000")
    assert all(k in line for k in HEADLINE + FULL_ONLY)
    assert line["checked"] is True and line["check_errors"] == []
    assert line["cpu_baseline"]["value"] > 0 and line["roofline"]["kernel_ms"] > 0
    assert line["ms_per_step_sequential"] > 0 and line["ms_per_request_latency"] > 0
