"""Census of the engine's environment knobs (CPU).

Every `SHD_*` variable the native code reads is an A/B switch that performance work flips
into a default sooner or later, and behind each sits code that is compiled into the product.
A knob that no test ever sets is code that no test ever runs.  So: every name read through
`getenv("SHD_...")`, `num("SHD_...")` or `off("SHD_...")` under shadow_amd/csrc/ must occur as
a string in some tests/*.py (set through monkeypatch.setenv or an environment dict), or be
listed in EXEMPT below with a reason.  A new knob without a test fails here, on the CPU,
before any GPU run.
"""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "shadow_amd", "csrc")

# knobs no test can set to any effect, each with its reason
EXEMPT = {
    "SHD_ROUTE_DFLAGS": "read only in builds with -DSHD_STAMPS (the stamp profiler); not compiled into the product",
    "SHD_ROUTE_PLAN_DEBUG": "prints the plan's shape to stderr; changes no plan, launch or result",
}

_READ = re.compile(r'\b(?:getenv|num|off)\(\s*"(SHD_[A-Z0-9_]+)"')
_QUOTED = re.compile(r'["\'](SHD_[A-Z0-9_]+)["\']')


def knobs_read():
    """name -> the csrc files that read it."""
    out = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not os.path.isfile(path):
            continue
        with open(path, errors="replace") as f:
            for name in _READ.findall(f.read()):
                out.setdefault(name, set()).add(os.path.basename(path))
    return out


def knobs_in_tests():
    """Every quoted SHD_* name in tests/*.py and tests/golden/*.py, this file left out (its
    EXEMPT table names the knobs it excuses)."""
    out = set()
    me = os.path.abspath(__file__)
    for path in glob.glob(os.path.join(HERE, "*.py")) + glob.glob(os.path.join(HERE, "golden", "*.py")):
        if os.path.abspath(path) == me:
            continue
        with open(path) as f:
            out.update(_QUOTED.findall(f.read()))
    return out


def test_census_finds_the_knobs():
    """The scan itself: it sees the three spellings (getenv in engine.hip and plan.hpp, off in
    plan.hpp, num in select.hpp) and a plausible number of knobs."""
    k = knobs_read()
    assert "SHD_ROUTE_FWRBLK" in k and "engine.hip" in k["SHD_ROUTE_FWRBLK"]  # getenv
    assert "SHD_ROUTE_LMSPREAD" in k and "plan.hpp" in k["SHD_ROUTE_LMSPREAD"]  # off
    assert "SHD_ROUTE_KBTCAP" in k and "select.hpp" in k["SHD_ROUTE_KBTCAP"]  # num
    assert "SHD_TOPOLOGY_LAT16" in k  # the front end's, in C
    assert len(k) >= 60, sorted(k)


def test_every_knob_is_set_by_some_test():
    read, used = knobs_read(), knobs_in_tests()
    missing = sorted(n for n in read if n not in used and n not in EXEMPT)
    assert not missing, f"knobs read by the engine that no test sets: {missing}"


def test_exemptions_are_current():
    """An exemption for a knob that is gone, or that a test sets after all, is stale."""
    read, used = knobs_read(), knobs_in_tests()
    assert sorted(n for n in EXEMPT if n not in read) == []
    assert sorted(n for n in EXEMPT if n in used) == []
    assert all(len(r) > 20 for r in EXEMPT.values())


# ---- the selection under the two creation-time knobs of tests/test_knobs_gpu.py ------------------

@pytest.fixture(scope="module")
def select_line(tmp_path_factory):
    """graph, environment -> the fields of tests/select_main.cpp's line (built once, host only)."""
    from shadow_amd import build
    from tests import select_cases as sc
    assert os.path.exists(build.HIPCC), "hipcc is needed to build tests/select_main.cpp"
    d = tmp_path_factory.mktemp("knobs")
    exe = str(d / "select_main")
    subprocess.run([build.HIPCC, f"--offload-arch={build.ARCH}", "-O1", "-std=c++17", "-o", exe,
                    os.path.join(HERE, "select_main.cpp")], check=True)
    files = {}

    def get(g, env):
        if g.name not in files:
            files[g.name] = str(d / f"{len(files)}.txt")
            with open(files[g.name], "w") as f:
                f.write(sc.graph_text(g))
        e = {k: v for k, v in os.environ.items() if not k.startswith("SHD_ROUTE_")}
        e.update(env)
        r = subprocess.run([exe, files[g.name]], capture_output=True, text=True, env=e)
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        tok = r.stdout.split()
        assert tok[0] == "select"
        return {k: int(v) for k, v in (t.split("=") for t in tok[1:] if "[" not in t) if v.lstrip("-").isdigit()}
    return get


@pytest.mark.parametrize("name,default", [("ba400", 384), ("c2", 1984)])
def test_kbtcap_sets_the_fused_rows_chunk(select_line, name, default):
    """SHD_ROUTE_KBTCAP on the graphs of test_knobs_gpu.py::test_kb_target_chunks: the fused KB
    rows stay selected and stage that many targets at a time (a multiple of 64, 64 at least)."""
    from tests.test_kb_gpu import _graph
    g = _graph(name)
    f = select_line(g, {})
    assert f["sel"] == 2 and f["kb.fused"] == 1 and f["kb.f_tcap"] == default == (g.n & ~63)
    for v, want in (("64", 64), ("128", 128), ("100", 64), ("1", 64), ("100000", default)):
        f = select_line(g, {"SHD_ROUTE_KBTCAP": v})
        assert f["sel"] == 2 and f["kb.fused"] == 1 and f["kb.f_tcap"] == want, (v, f["kb.f_tcap"])


def test_hub1024_off_keeps_the_contexts_block(select_line):
    """SHD_ROUTE_HUB1024=0 on lmonly3000 under KD at 256 threads: no 1024-thread hub form."""
    from tests.golden import make_plan_jobs as mk
    g = mk.graph("lmonly3000")
    env = {"SHD_ROUTE_KERNEL": "kd"}
    f = select_line(g, env)
    assert f["sel"] == 4 and f["kd.block"] == 256 and f["kd.hub_block"] == 1024
    f0 = select_line(g, {**env, "SHD_ROUTE_HUB1024": "0"})
    assert f0["sel"] == 4 and f0["kd.block"] == 256 and f0["kd.hub_block"] == 0
    assert f0["kd.slots"] == f["kd.slots"] and f0["kd.lds"] == f["kd.lds"]
    assert select_line(g, {**env, "SHD_ROUTE_HUB1024": "1"})["kd.hub_block"] == 1024


# ---- tests/plan_check.py itself -----------------------------------------------------------------

def _jobs(rows):
    """JOB_DTYPE records from (row, s, store, [(seed, u, wr), ...])."""
    from shadow_amd.route import JOB_DTYPE
    out = np.zeros(len(rows), JOB_DTYPE)
    for j, (row, s, store, seeds) in zip(out, rows):
        j["row"], j["s"], j["store"], j["nseed"] = row, s, store, len(seeds)
        for k, (slot, u, wr) in enumerate(seeds):
            j["seed"][k], j["u"][k], j["wr"][k] = slot, u, wr
    return out


def _path_dist(s):
    return np.abs(np.arange(6) - s).astype(np.float64) * 2.0     # a path of 6 vertices, latency 2


def test_plan_check_accepts_a_valid_plan():
    from tests import plan_check
    src = np.arange(6)
    # slot 0 <- row of 2; slots 1, 2: landmark rows of the vertices 5 and 0
    good = _jobs([(2, 2, 0, []), (1, 1, -1, [(0, 2, 2), (2, 0, 2)]), (3, 3, 0, [(0, 2, 2)]), (4, 4, -1, [(0, 3, 3), (1, 5, 2)]),
                  (0, 0, -1, [(2, 0, 0)]), (5, 5, -1, [(1, 5, 0), (0, 3, 4), (2, 0, 0xFFFF)])])
    s = plan_check.validate(good, src, np.arange(6), _path_dist)
    assert s["unseeded"] == 1 and s["row_seeds"] == 4 and s["landmark_seeds"] == 5 and s["landmarks"] == 2
    # helper rows (no output row): one kept for a later job, one computed for nothing
    more = _jobs([(-1, 4, 3, []), (0, 0, -1, [(3, 4, 8)]), (1, 1, -1, []), (-1, 5, -1, [(3, 4, 2)])])
    s = plan_check.validate(more, src, np.arange(2), _path_dist)
    assert s["helpers"] == 2 and s["idle_helpers"] == 1


@pytest.mark.parametrize("what", ["order", "vertex", "short", "wide", "twice", "missing", "nseed", "landmark",
                                  "landmark_slot", "source"])
def test_plan_check_refuses(what):
    from tests import plan_check
    src = np.arange(6)
    pos = np.arange(3)
    ok = [(0, 0, 0, []), (1, 1, -1, [(0, 0, 2)]), (2, 2, -1, [(0, 0, 4), (1, 5, 6)])]
    plan_check.validate(_jobs(ok), src, pos, _path_dist)
    bad = {
        "order": [ok[1], ok[0], ok[2]],                                  # the seed's row comes later
        "vertex": [ok[0], (1, 1, -1, [(0, 3, 4)]), ok[2]],               # slot 0 holds the row of 0, not of 3
        "short": [ok[0], (1, 1, -1, [(0, 0, 1)]), ok[2]],                # wr below d(1, 0) = 2
        "wide": [ok[0], (1, 1, -1, [(0, 0, 0x10000)]), ok[2]],
        "twice": [ok[0], ok[1], ok[2], ok[1]],
        "missing": ok[:2],
        "nseed": None,                                                   # (set below: four seeds)
        "landmark": [ok[0], (1, 1, -1, [(1, 4, 6)]), ok[2]],             # landmark slot 1: vertex 4, then 5
        "landmark_slot": [(0, 0, 3, []), ok[1][:2] + (-1, [(3, 0, 2)]), (2, 2, -1, [(3, 0, 4), (1, 5, 6)])],
        "source": [ok[0], (1, 2, -1, [(0, 0, 4)]), ok[2]],               # row 1 belongs to source 1
    }[what]
    with pytest.raises(plan_check.PlanError):
        if what == "nseed":
            j = _jobs(ok)
            j["nseed"][2] = 4
            plan_check.validate(j, src, pos, _path_dist)
        else:
            plan_check.validate(_jobs(bad), src, pos, _path_dist)
