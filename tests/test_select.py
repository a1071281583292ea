"""The kernel selection on the host alone (no GPU): tests/select_main.cpp runs select_all() of
shadow_amd/csrc/select.hpp, built with the address and undefined-behaviour sanitizers, on every
case of tests/golden/select_info.json, and what shd_route_get_info would report of its decision
must equal what the engine reported on the GPU when the fixture was recorded."""
from __future__ import annotations

import json
import os
import subprocess

import pytest

from shadow_amd import build
from tests import select_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
WANT = json.load(open(os.path.join(HERE, "golden", "select_info.json")))
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover"]


@pytest.fixture(scope="session")
def select_main(tmp_path_factory):
    """The program, built once; skips where hipcc or the sanitizer runtime is absent."""
    if not os.path.exists(build.HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("select")
    hipcc = [build.HIPCC, f"--offload-arch={build.ARCH}", "-O1", "-g", "-std=c++17", *SAN]
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([*hipcc, "-o", str(d / "probe"), str(probe)], capture_output=True).returncode:
        pytest.skip("no sanitizer runtime")
    exe = d / "select_main"
    subprocess.run([*hipcc, "-o", str(exe), os.path.join(HERE, "select_main.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="session")
def graph_file(tmp_path_factory):
    d = tmp_path_factory.mktemp("select_graphs")
    made = {}

    def get(name):
        if name not in made:
            made[name] = str(d / f"{name}.txt")
            with open(made[name], "w") as f:
                f.write(sc.graph_text(sc.graph(name)))
        return made[name]
    return get


def info_of(line: str) -> dict:
    """What shd_route_get_info reports, from the program's line (engine.hip: shd_route_get_info,
    lat16_ok; device_bytes counts every upload(): the base graph arrays and the staged ones)."""
    tok = line.split()
    assert tok[0] == "select"
    f = {}
    for t in tok[1:]:
        k, v = t.split("=")
        if "[" not in k:
            f[k] = float(v) if k in ("min_w", "kf.delta", "kf.wscale") else int(v)
    n, nnz, sel = f["n"], f["nnz"], f["sel"]
    csr = 4 * (n + 1) + (4 + 8 + 8) * max(nnz, 1)           # row, col, w, r (an empty array takes one element)
    base = csr * (2 if f["directed"] else 1) + 3 * 8 * n + 4  # + vf, self_w, self_r, the error word
    return {
        "kernel": sel,
        "block": {0: f["f64.block"], 1: f["k32.block"], 2: f["kb.block"], 4: f["kd.block"], 5: f["kf.block"]}[sel],
        "reserved": {0: 0, 1: 0, 2: f["kb.fused"], 4: f["kd.delta"], 5: int(f["kf.wscale"])}[sel],
        "dist_bound": f["k32.bound"],
        "lat16": int(bool(f["integer_w"] and f["self16"] and 0 < f["k32.bound"] < 0xFFFF)),
        "lds_resident": int(bool((f["f64.lds"] or sel) and not f["kf.h"])),
        "device_bytes": f["upload_bytes"] + base,
        "integer_weights": f["integer_w"], "multigraph": f["multigraph"], "n_arcs": nnz,
        "min_edge_latency": f["min_w"],
    }


def test_cases_are_the_fixture():
    assert set(WANT) == set(sc.CASES)


def test_fixture_covers_every_kernel_and_block():
    have = {(i["kernel"], i["block"]) for i in WANT.values()}
    assert {k for k, _ in have} == {0, 1, 2, 4, 5}
    assert {(4, 256), (4, 1024), (5, 256), (5, 1024)} <= have


@pytest.mark.parametrize("name", sorted(WANT))
def test_selection_matches_recorded(select_main, graph_file, name):
    gname, env = sc.CASES[name]
    e = {k: v for k, v in os.environ.items() if not k.startswith("SHD_ROUTE_")}
    e.update(env)
    runs = [subprocess.run([select_main, graph_file(gname)], capture_output=True, text=True, env=e) for _ in range(2)]
    for r in runs:
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    got = info_of(runs[0].stdout)
    want = {k: WANT[name][k] for k in got}
    assert got == want
    assert runs[1].stdout == runs[0].stdout
