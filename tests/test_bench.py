"""bench.py's command line: a plain run carries the headline figure only, --full the rest,
and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("kernel_ms", "landmark_ms", "roofline")


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("shd_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """A small table is written whole; above the size threshold both tables are written at
    the same seeded, sorted flat positions, the same ones from call to call."""
    import torch
    bench = _bench_module()
    rng = np.random.default_rng(3)
    lat = torch.from_numpy(rng.integers(1, 500, size=(8, 37)).astype(np.float64))  # (7 rows used of 8)
    rel = torch.from_numpy(rng.random((8, 37)))
    rmin = lat.min(dim=1).values
    dmin = rmin[:7].min().reshape(1)
    bench.dump_outputs(str(tmp_path / "w"), torch, 0, 1, 7, lat, rel, rmin, dmin)
    got = {n: np.load(tmp_path / "w" / f"{n}.npy") for n in ("lat", "rel", "row_min", "runahead_min")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["lat"], lat[:7].numpy().ravel())
    assert np.array_equal(got["rel"], rel[:7].numpy().ravel())
    assert np.array_equal(got["row_min"], rmin[:7].numpy()) and np.array_equal(got["runahead_min"], dmin.numpy())

    monkeypatch.setattr(bench, "DUMP_WHOLE_BYTES", 16 * 7 * 37 - 1)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 50)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), torch, 1, 2, 7, lat, rel, rmin, dmin)
    s_lat, s_rel = np.load(tmp_path / "s1" / "lat_rank1.npy"), np.load(tmp_path / "s1" / "rel_rank1.npy")
    assert s_lat.shape == s_rel.shape == (50,)
    flat_lat, flat_rel = lat[:7].numpy().ravel(), rel[:7].numpy().ravel()
    idx = np.sort(np.random.default_rng(2024).choice(7 * 37, size=50, replace=False))
    assert np.array_equal(s_lat, flat_lat[idx]) and np.array_equal(s_rel, flat_rel[idx])
    assert np.array_equal(s_lat, np.load(tmp_path / "s2" / "lat_rank1.npy"))
    assert np.load(tmp_path / "s1" / "row_min_rank1.npy").shape == (7,)


def _run(*argv):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2",
                          "--steps", "2", "--warmup", "1", *argv], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_lines_and_dumps(tmp_path):
    plain = _run("--dump-outputs", str(tmp_path / "a"))
    full = _run("--full", "--no-cpu-baseline", "--verify", "2", "--dump-outputs", str(tmp_path / "b"))
    for line in (plain, full):
        assert all(k in line for k in HEADLINE)
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["dtype"] == "f64"
        assert line["config"]["sources_total"] == 2000  # C2: every vertex a source, each step
        assert line["value"] == pytest.approx(2000 / (line["ms_per_step"] / 1e3))
    assert not any(k in plain for k in FULL_ONLY) and plain["verified_rows_vs_oracle"] is None
    assert all(k in full for k in FULL_ONLY) and full["verified_rows_vs_oracle"] is True
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["lat.npy", "rel.npy", "row_min.npy", "runahead_min.npy"] == sorted(os.listdir(tmp_path / "b"))
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64 and np.array_equal(a, b, equal_nan=True), n
    lat = np.load(tmp_path / "a" / "lat.npy")
    assert lat.shape == (3_000_000,)  # 2000 x 2000 x 16 B is above the whole-table threshold
    assert np.load(tmp_path / "a" / "row_min.npy").shape == (2000,)
    assert np.load(tmp_path / "a" / "runahead_min.npy")[0] == np.load(tmp_path / "a" / "row_min.npy").min()
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
