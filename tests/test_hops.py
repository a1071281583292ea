"""CPU: the path hops interface is declared through every layer, and the route line
formatter (shadow_amd/csrc/route_fmt.c) as a stand-alone program under the host sanitizers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTE_SYMS = ("shd_route_hops_async", "shd_route_hops", "shd_route_paths")
TOPO_SYMS = ("shd_topology_get_path", "shd_topology_format_path", "shd_topology_dump_routes",
             "shd_topology_route_line")


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
    for name in ("hops", "hops_async", "paths"):
        assert callable(getattr(route.RouteEngine, name))
    for name in ("get_path", "format_path", "dump_routes"):
        assert callable(getattr(topology.Topology, name))
    assert callable(route.path_edge_offsets)


def _line(names, vert, hop_lat, hop_rel, lat, rel, directed):
    nm = (lambda v: names[v]) if names else (lambda v: "%d" % v)
    sep = "-->" if directed else "<-->"
    s = "shortest path %s%s%s (%i%s%i) is %f ms with %f loss, path: %s" % (
        nm(vert[0]), sep, nm(vert[-1]), vert[0], sep, vert[-1], lat, 1 - rel, nm(vert[0]))
    for q in range(1, len(vert)):
        s += "%s[%f,%f]-->%s" % ("--" if directed else "<--", hop_lat[q - 1], 1.0 - hop_rel[q - 1], nm(vert[q]))
    return s


def test_formatter_standalone_sanitized(tmp_path):
    """route_fmt.c with tests/route_fmt_main.c, built with -fsanitize=address,undefined and
    run as its own process: a one-hop undirected path, a directed path, a 600-hop path with
    40-character names (the buffer grows from 64 bytes to tens of KiB) and the [s, s] self
    entry, against strings built here with %f."""
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
    exe = tmp_path / "route_fmt_test"
    subprocess.run([cc, "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", *san, "-o", str(exe),
                    os.path.join(ROOT, "tests", "route_fmt_main.c"),
                    os.path.join(ROOT, "shadow_amd", "csrc", "route_fmt.c")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    K = 600
    names = ["vertex-%033d" % q for q in range(K + 1)]
    hl = [1.0 + 0.125 * q for q in range(K)]
    hr = [1.0 - q / 1024.0 for q in range(K)]
    lat = 0.0
    for x in hl:
        lat += x
    want = [
        _line(None, [3, 17], [12.0], [0.99], 12.0, 0.99, False),
        _line(["poi-1", "poi-2", "relay", "poi-9"], [2, 0, 3, 1], [1.5, 20.25, 3.0], [1.0, 0.875, 0.5], 24.75, 0.4375,
              True),
        _line(names, [K - q for q in range(K + 1)], hl, hr, lat, 0.25, False),
        _line(None, [5, 5], [7.0], [0.75], 7.0, 0.75, False),
    ]
    assert len(names[0]) == 40 and len(want[2]) > 30000
    assert got == want
    assert want[0] == ("shortest path 3<-->17 (3<-->17) is 12.000000 ms with 0.010000 loss, "
                       "path: 3<--[12.000000,0.010000]-->17")
