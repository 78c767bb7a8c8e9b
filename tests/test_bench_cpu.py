"""bench.py's command line on the torch-only rehearsal workload (CPU): --steps, ms_per_step, --dump-outputs, --full."""
import json
import sys

import numpy as np
import pytest


def _run(monkeypatch, capsys, *argv):
    import bench
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--workload", "rehearsal", "--gpus", "1", *argv])
    bench.main()
    return json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])


def test_plain_line_and_step_count(monkeypatch, capsys):
    import bench
    calls = []
    real = bench.TrainStep.step

    def counted(self, *a, **kw):
        calls.append(1)
        return real(self, *a, **kw)

    monkeypatch.setattr(bench.TrainStep, "step", counted)
    line = _run(monkeypatch, capsys, "--steps", "4", "--warmup", "2")
    assert len(calls) == 6   # a plain run: the warm-up and the timed steps, nothing else
    assert line["steps"] == 4 and line["warmup"] == 2
    assert line["unit"] == "image-tokens/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    tokens = 4 * line["config"]["global_batch"] * line["config"]["seq_len"]
    assert line["value"] == pytest.approx(tokens / (4 * line["ms_per_step"] * 1e-3), rel=1e-2)
    assert not line["roofline"] and not line["kernels"] and "secondary" not in line and "cpu_baseline" not in line


def test_dump_outputs_repeatable(monkeypatch, capsys, tmp_path):
    lines = [_run(monkeypatch, capsys, "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d))
             for d in ("a", "b")]
    a = {p.name: np.load(p) for p in sorted((tmp_path / "a").iterdir())}
    b = {p.name: np.load(p) for p in sorted((tmp_path / "b").iterdir())}
    assert sorted(a) == sorted(b) == ["loss.npy"]
    assert a["loss.npy"].dtype == np.float32 and a["loss.npy"].shape == (1,) and np.isfinite(a["loss.npy"]).all()
    np.testing.assert_array_equal(a["loss.npy"], b["loss.npy"])   # same seeded inputs, deterministic on the CPU
    assert float(a["loss.npy"][0]) == pytest.approx(lines[0]["loss"], abs=1e-5)


def test_full_option_accepted(monkeypatch, capsys):
    line = _run(monkeypatch, capsys, "--steps", "2", "--warmup", "1", "--full")
    assert line["steps"] == 2 and line["ms_per_step"] > 0
