"""CPU: a plain bench.py run does the warm-up, the timed steps and the line only; verification, CPU baselines, the extra
roofline figures and the "also" configurations run with --full.  bench.main() is driven with a recording stand-in for
the engine context and for every workload, so the test sees each call the benchmark makes."""
import json
import sys

import numpy as np
import pytest

import bench


class FakeArray:
    ptr = 0

    def __init__(self, shape=(4, 3)):
        self.shape = shape

    def offset(self, n, shape):
        return FakeArray(shape)

    def upload(self, host):
        pass

    def to_host(self):
        return np.zeros(self.shape, np.float32)


class FakeCtx:
    def __init__(self, calls):
        self.calls = calls

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append(name)
            return {"prof_query": (3, 3.0), "device_info": {"name": "stand-in"}, "timer_stop": 1.0}.get(name)
        return call


def _run(monkeypatch, capfd, argv):
    calls = []

    class FakeWorkload:
        metric, unit, dtype, kernel = "entries/s", "entries/s", "int32 counts -> f32 PS", "ps_tile_v3_kernel"
        gen_s = 0.0

        def __init__(self, ctx, rank, n, s, block_rows=0):
            self.n, self.s = n or 10, s or 3
            self.units, self.alg_bytes = self.n * self.s, 8.0 * self.n * self.s
            self.d_counts, self.d_ps = FakeArray(), FakeArray()
            self.sample_counts = np.zeros((4, 3), np.int32)

        def step(self):
            calls.append("step")

        def outputs(self):
            return []

        def describe(self):
            return {"workload": "stand-in"}

        def verify(self):
            calls.append("verify")
            return True, 1

        def cpu_baseline(self, sample):
            calls.append("cpu_baseline")
            return {"value": 1.0}

    monkeypatch.setattr(bench, "Context", lambda device: FakeCtx(calls))
    monkeypatch.setattr(bench, "WORKLOADS", {k: FakeWorkload for k in bench.WORKLOADS})
    monkeypatch.setattr(bench, "cpu_baseline_all_cores", lambda workload: calls.append("all_cores"))
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    bench.main()
    out, _ = capfd.readouterr()
    return json.loads(out.strip().splitlines()[-1]), calls


def test_plain_run_does_the_steps_and_the_line_only(monkeypatch, capfd):
    line, calls = _run(monkeypatch, capfd, ["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert calls.count("step") == 7
    assert set(calls) == {"step", "sync", "prof_enable", "prof_reset", "prof_query", "device_info", "close"}
    assert line["steps"] == 5 and line["warmup"] == 2 and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(line["steps"] * 30 / (line["ms_per_step"] * line["steps"] * 1e-3))
    assert line["verify"] is None and line["cpu_baseline"] is None and "also" not in line
    assert "pcie" not in line["roofline"] and "copy_same_bytes_ms" not in line["roofline"]


def test_full_run_verifies_and_measures_the_rest(monkeypatch, capfd):
    line, calls = _run(monkeypatch, capfd, ["--gpus", "1", "--steps", "5", "--warmup", "2", "--full"])
    assert calls[0] == "all_cores" and "copy2d_dev" in calls
    assert line["verify"] == {"ok": True, "checked": 1} and line["cpu_baseline"]["all_cores"] is None
    assert "pcie" in line["roofline"] and "copy_same_bytes_ms" in line["roofline"]
    assert list(line["also"]) == [a[0] for a in bench.ALSO]
    assert calls.count("verify") == 1 + len(bench.ALSO)
    assert calls.count("cpu_baseline") == 1 + sum(1 for a in bench.ALSO if a[6])
