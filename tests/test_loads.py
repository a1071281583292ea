"""CPU: the link loads interface is declared through every layer, and the link line
formatter (shadow_amd/csrc/link_fmt.c) as a stand-alone program under the host sanitizers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_SYMS = ("shd_route_loads_async", "shd_route_loads", "shd_route_pair_loads")
TOPO_SYMS = ("shd_topology_link_loads", "shd_topology_dump_link_loads", "shd_topology_link_line")


def _declared(header, pattern):
    text = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(pattern, text))


def test_declarations():
    import ctypes
    from shadow_amd import build, route, topology
    build.build()
    assert set(ROUTE_SYMS) <= _declared("shd_route.h", r"\b(shd_route_[a-z_]+)\s*\(")
    assert set(TOPO_SYMS) <= _declared("shd_topology.h", r"\b(shd_(?:topology|graphml|attach)_[a-z_]+)\s*\(")
    assert set(ROUTE_SYMS) <= set(route.EXPORTS) and set(TOPO_SYMS) <= set(topology.EXPORTS)
    eng, front = ctypes.CDLL(route.LIB_PATH), ctypes.CDLL(topology.LIB_PATH)
    for sym in ROUTE_SYMS:
        assert hasattr(eng, sym), sym
    for sym in TOPO_SYMS:
        assert hasattr(front, sym), sym
    for name in ("loads", "loads_async", "pair_loads"):
        assert callable(getattr(route.RouteEngine, name))
    for name in ("link_loads", "dump_link_loads"):
        assert callable(getattr(topology.Topology, name))
    assert route.LOADS_ADD == 0x400
    assert re.search(r"#define\s+SHD_ROUTE_LOADS_ADD\s+0x400u", open(os.path.join(ROOT, "include", "shd_route.h")).read())


def _line(names, edge, a, b, lat, loss, packets, directed):
    nm = (lambda v: names[v]) if names else (lambda v: "%d" % v)
    sep = "-->" if directed else "<-->"
    return "link %s%s%s (%i%s%i) edge %i is %f ms with %f loss, %d packets" % (
        nm(a), sep, nm(b), a, sep, b, edge, lat, loss, packets)


def test_link_formatter_standalone_sanitized(tmp_path):
    """link_fmt.c with tests/link_fmt_main.c, built with -fsanitize=address,undefined and run
    as its own process: an undirected line, a directed line with a missing id, 40-character
    names with a packet count above 2^32 (the buffer grows from 64 bytes) and the largest
    count, against strings built here with %f."""
    cc = shutil.which("gcc")
    if not cc:
        pytest.skip("no gcc")
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    # the runtimes linked statically where gcc has them (the program then starts whatever
    # else the process environment loads), else the shared ones
    for extra in (["-static-libasan", "-static-libubsan"], []):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover", *extra]
        if subprocess.run([cc, *san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip("gcc lacks the sanitizer runtime")
    exe = tmp_path / "link_fmt_test"
    subprocess.run([cc, "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", *san, "-o", str(exe),
                    os.path.join(ROOT, "tests", "link_fmt_main.c"),
                    os.path.join(ROOT, "shadow_amd", "csrc", "link_fmt.c")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    names = ["vertex-%033d" % q for q in range(12)]
    want = [
        _line(None, 7, 3, 17, 12.0, 0.01, 42, False),
        _line(["poi-1", "poi-2", "2", "poi-9"], 0, 3, 2, 20.25, 0.125, 1, True),
        _line(names, 2147483647, 11, 4, 1.5, 0.0, 2 ** 40 + 3, False),
        _line(None, 5, 9, 9, 7.0, 0.75, 2 ** 64 - 1, False),
    ]
    assert len(names[0]) == 40 and len(want[2]) > 128
    assert got == want
    assert want[0] == "link 3<-->17 (3<-->17) edge 7 is 12.000000 ms with 0.010000 loss, 42 packets"
    assert want[1] == "link poi-9-->2 (3-->2) edge 0 is 20.250000 ms with 0.125000 loss, 1 packets"
    assert want[2].endswith("1099511627779 packets")
