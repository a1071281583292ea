"""The host stages of the path calls on the host alone (no GPU): tests/path_host_main.cpp runs
shadow_amd/csrc/path_host.hpp, built with the address and undefined-behaviour sanitizers, and
what it prints -- the arcs the hops and ties upload, the pairs of a call grouped by source, the
source chunks of the row scratch and the launch form of each state kernel -- must equal a few
lines of numpy over the same inputs."""
from __future__ import annotations

import itertools
import os
import subprocess

import numpy as np
import pytest

from shadow_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover"]
KNOBS = {"hops": "SHD_ROUTE_HOPS_LDS", "loads": "SHD_ROUTE_LOADS_LDS", "ties": "SHD_ROUTE_TIES_LDS"}


@pytest.fixture(scope="session")
def path_host_main(tmp_path_factory):
    """The program, built once; skips where hipcc or the sanitizer runtime is absent."""
    if not os.path.exists(build.HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("path_host")
    hipcc = [build.HIPCC, f"--offload-arch={build.ARCH}", "-O1", "-g", "-std=c++17", *SAN]
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([*hipcc, "-o", str(d / "probe"), str(probe)], capture_output=True).returncode:
        pytest.skip("no sanitizer runtime")
    exe = d / "path_host_main"
    subprocess.run([*hipcc, "-o", str(exe), os.path.join(HERE, "path_host_main.cpp")], check=True)
    return str(exe)


def run(exe, *args, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("SHD_ROUTE_")}
    e.update(env or {})
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=e)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return r.stdout


def arrays(out: str) -> dict:
    got = {}
    for ln in out.splitlines():
        name, _, vals = ln.partition(":")
        got[name] = [float(v) if name in ("in.w", "in.r", "out.w") else int(v) for v in vals.split()]
    return got


def fields(out: str) -> dict:
    return {k: int(v) for k, v in (t.split("=") for t in out.split())}


# ---- the arcs ----
# edges (src, dst, latency, loss); vertex 2 has two self-loops (edges 3 and 6: the first counts),
# 0 -> 1 and 3 -> 1 are parallel pairs, 1 -> 0 runs against one of them
MULTI = [(0, 1, 5.0, 0.0), (1, 0, 7.0, 0.25), (0, 1, 5.0, 0.5), (2, 2, 1.0, 0.125), (1, 2, 2.5, 0.0),
         (2, 3, 4.0, 0.0625), (2, 2, 9.0, 0.0), (3, 1, 3.0, 0.0), (3, 1, 3.0, 0.75), (3, 0, 11.0, 0.0),
         (0, 0, 2.0, 0.5)]
ARC_CASES = {"directed_multi": (4, True, MULTI), "undirected_multi": (4, False, MULTI), "one_vertex": (1, False, [])}


def want_arcs(n, directed, edges):
    head, tail, eid, self_e = [], [], [], [-1] * n
    for e, (a, b, _, _) in enumerate(edges):
        if a == b:
            if self_e[a] < 0:
                self_e[a] = e
            continue
        head.append(b); tail.append(a); eid.append(e)
        if not directed:
            head.append(a); tail.append(b); eid.append(e)
    head, tail, eid = (np.array(x, dtype=np.int64) for x in (head, tail, eid))
    lat = np.array([w for _, _, w, _ in edges], dtype=np.float64)
    rel = 1.0 - np.array([p for _, _, _, p in edges], dtype=np.float64)
    want = {"self": self_e}
    for name, rows, cols in (("in", head, tail), ("out", tail, head)):
        o = np.lexsort((eid, cols, rows))  # by row, then column, then edge id
        want[f"{name}.row"] = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n)))).tolist()
        want[f"{name}.col"] = cols[o].tolist()
        want[f"{name}.eid"] = eid[o].tolist()
        want[f"{name}.w"] = lat[eid[o]].tolist()
        if name == "in":
            want["in.r"] = rel[eid[o]].tolist()
    return want


@pytest.mark.parametrize("name", sorted(ARC_CASES))
def test_arcs(path_host_main, tmp_path, name):
    n, directed, edges = ARC_CASES[name]
    f = tmp_path / "graph.txt"
    f.write_text(f"{n} {len(edges)} {int(directed)}\n" + "".join(f"{a} {b} {w!r} {p!r}\n" for a, b, w, p in edges) +
                 " ".join(["nan"] * n) + "\n")
    got = arrays(run(path_host_main, "arcs", f))
    want = want_arcs(n, directed, edges)
    assert got == want
    if edges:  # the cases are what they claim: parallel arcs kept, self-loops dropped, both ways when undirected
        loops = sum(a == b for a, b, _, _ in edges)
        assert len(got["in.col"]) == (len(edges) - loops) * (1 if directed else 2)
        assert got["self"][2] == 3 and got["self"][1] == -1
        assert any(got["in.col"][q] == got["in.col"][q + 1] and got["in.eid"][q] < got["in.eid"][q + 1]
                   for r in range(n) for q in range(got["in.row"][r], got["in.row"][r + 1] - 1))


# ---- pairs grouped by source ----
PAIR_CASES = {
    "unsorted": [(5, 1), (2, 9), (7, 0), (2, 3), (0, 4), (5, 5)],
    "repeated": [(3, 1), (1, 2), (3, 1), (3, 1), (1, 2), (0, 0), (1, 2)],
    "one_source": [(4, 7), (4, 1), (4, 7), (4, 0)],
    "empty": [],
}


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", sorted(PAIR_CASES))
def test_pairs(path_host_main, tmp_path, name, weighted):
    pairs = PAIR_CASES[name]
    wt = [(1 << 40) + 17 * k for k in range(len(pairs))]
    f = tmp_path / "pairs.txt"
    f.write_text(f"{len(pairs)} {int(weighted)}\n" +
                 "".join(f"{s} {t}" + (f" {wt[k]}" if weighted else "") + "\n" for k, (s, t) in enumerate(pairs)))
    got = arrays(run(path_host_main, "pairs", f))
    src = np.array([s for s, _ in pairs], dtype=np.int64)
    tgt = np.array([t for _, t in pairs], dtype=np.int64)
    order = np.lexsort((np.arange(len(pairs)), src))  # by source, the caller's order within one
    us, first, gsi = np.unique(src[order], return_index=True, return_inverse=True)
    assert got == {"order": order.tolist(), "us": us.tolist(), "first": first.tolist() + [len(pairs)],
                   "gsi": gsi.tolist(), "gt": tgt[order].tolist(),
                   "gw": np.array(wt, dtype=object)[order].tolist() if weighted else []}


# ---- source chunks of the row scratch ----
@pytest.mark.parametrize("hrow", [0, 1])
@pytest.mark.parametrize("what,n,count,mult", [("below_one_source", 60, 12, 0.5), ("exact_multiple", 60, 12, 3),
                                               ("one_byte_short", 60, 12, 3 - 1 / 960), ("fewer_sources", 60, 2, 5),
                                               ("past_2_31", 70000, 40000, 40000)])
def test_chunks(path_host_main, what, n, count, mult, hrow):
    per = n * (16 if hrow else 12)  # f64 distances, u32 parents, i32 hops
    budget = int(per * mult)
    got = fields(run(path_host_main, "chunks", n, count, budget, hrow))
    chunk = max(1, min(count, budget // per))
    assert got == {"chunk": chunk, "bytes": per * chunk, "par_off": 8 * n * chunk, "hrow_off": 12 * n * chunk}
    assert chunk == {"below_one_source": 1, "exact_multiple": 3, "one_byte_short": 2, "fewer_sources": 2,
                     "past_2_31": 40000}[what]


# ---- the form of the state kernels ----
def a16(x):
    return (x + 15) & ~15


# family -> (LDS bytes beside the state, state bytes of element width t, LDS budget, default slot budget)
FAMILIES = {
    "hops": (16, lambda n, t: 4 * a16(t * n), 160 * 1024, 256 << 20),             # path_hops.hpp
    "loads": (96, lambda n, t: 2 * a16(8 * n) + a16(4 * (n + 1)) + a16(t * n), 160 * 1024, (1 << 30) // 4),  # link_loads.hpp
    "ties": (16, lambda n, t: 3 * a16(8 * n) + a16(4 * n) + 2 * a16(t * n), 160 * 1024, (1 << 30) // 4),  # ties_layout.hpp
}


def largest_lds_n(family):
    small, state, budget, _ = FAMILIES[family]
    n = max(n for n in range(1, 65536) if small + state(n, 2) <= budget)
    assert small + state(n + 1, 2) > budget and n + 1 <= 65535
    return n


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_state_form(path_host_main, family):
    small, state, budget, slot_budget = FAMILIES[family]
    nfit = largest_lds_n(family)
    seen = set()
    ns = (nfit, nfit + 1, 65535, 65536)
    for knob, mode, (k, sb) in itertools.product((None, "", "0", "1"), (0, 1, 2),
                                                 ((2000, slot_budget), (5, slot_budget), (2000, 1000))):
        env = {} if knob is None else {KNOBS[family]: knob}
        lines = run(path_host_main, "form", family, mode, k, sb, *ns, env=env).splitlines()
        assert len(lines) == len(ns)
        for n, ln in zip(ns, lines):
            got = fields(ln)
            if mode == 2:
                want = {"form": 0, "grid": min(k, 1024), "lds": small, "stride": 0, "slots": 0}
            elif n <= 65535 and small + state(n, 2) <= budget and knob != "0":
                want = {"form": 1, "grid": min(k, 1024), "lds": small + state(n, 2), "stride": 0, "slots": 0}
            else:
                stride = a16(state(n, 2 if n <= 65535 else 4))
                slots = max(16, min(512, sb // stride))
                want = {"form": 2 if n <= 65535 else 3, "grid": min(k, slots), "lds": small, "stride": stride,
                        "slots": slots}
            assert got == want, (n, knob, mode, k, sb)
            seen.add((got["form"], n))
    # every form is reached, the LDS form ends exactly at nfit and u16 state at 65535
    assert {f for f, _ in seen} == {0, 1, 2, 3}
    assert (1, nfit) in seen and (1, nfit + 1) not in seen and (2, 65535) in seen and (3, 65536) in seen
