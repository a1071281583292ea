"""Several live contexts (CPU part): the pairs of graphs tests/test_contexts_gpu.py keeps alive
together, one pair per kernel function whose dynamic-LDS limit a context sets for itself
(hipFuncSetAttribute in engine.hip apply_selection, shd_route_create, fw_prepare; path_calls.hpp
ensure_hops).
The limit belongs to the function, not to the context, so the second context of a pair moves
it under the first one's feet.  For that to be tried, the two must ask for different amounts:
here, without a GPU, every pair is held to

    large >= 2 x small, and large > 64 KiB where the kernel's form can get there

with the sizes read from tests/select_main.cpp's line (select_all() on the host), or from the
header's formulas for the hops (path_hops.hpp) and K4 (engine.hip fw_prepare).

The graphs are those of shape_graphs.SUITE (range_graphs.SUITE has no two graphs of different
vertex counts for one kernel: its KF graphs all have 389 vertices or 5); a forced
SHD_ROUTE_KERNEL=kf takes the sized graphs (integer latencies, about 100 reliabilities).

Where 64 KiB is out of a form's reach, the reason is the selection's own limit:
  k32_256   256-thread K32 ends at 4096 vertices (58 KiB); the 512- and 1024-thread forms are
            other kernel functions, and SIZES has no two graphs in either
  attr      the K2 pass runs behind KB only, which ends at about 4096 vertices (41 KiB)
  kd_256    256-thread KD ends at 16384 vertices: 64272 bytes
  kf_256    256-thread KF ends at 2688 vertices (40 KiB)
  k4_rows   K4 reaches 64 KiB from about 6000 vertices, where the dense host tables and the
            table itself cost seconds; its 8-source parent kernel is past 64 KiB at 4097
"""
from __future__ import annotations

import os
import subprocess

import pytest

from shadow_amd import build
from tests import select_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
KIB64 = 64 * 1024
LDS_BUDGET = 160 * 1024


def a16(x):
    return (x + 15) & ~15


def hops_lds(f):
    """path_hops.hpp: kHpSmall + hp_state_bytes<uint16_t>(n)."""
    return 16 + 4 * a16(2 * f["n"])


def k4_rows_lds(f):
    """engine.hip fw_prepare / shd_route_fw_rows_async: rel f64 + order u16 per vertex + the buckets."""
    return a16(8 * f["n"]) + a16(2 * f["n"]) + a16(4 * (f["k32.bound"] + 2))


def k4_parent8_lds(f):
    """fw_parent8_kernel: 16 bytes per padded vertex (FW_T = 64)."""
    return 16 * ((f["n"] + 63) // 64 * 64)


# name -> (creation environment, large graph, small graph, {what: key of select_main's line or a
# formula}, the sizes that must pass 64 KiB, fields that must agree between the two: the same
# kernel function)
PAIRS = {
    "k32_256": ({"SHD_ROUTE_KERNEL": "k32"}, "sized2689", "sized63", {"k32": "k32.lds"}, (), ("sel", "k32.block")),
    "kb_plain": ({"SHD_ROUTE_KERNEL": "kb"}, "sized2689", "sized63", {"kb": "kb.lds", "attr": "attr.lds"}, ("kb",),
                 ("sel", "kb.fused")),
    "kb_fused": ({}, "sized2048", "sized255", {"kb_fused": "kb.f_lds"}, ("kb_fused",), ("sel", "kb.fused")),
    "kd_256": ({"SHD_ROUTE_KERNEL": "kd"}, "sized11212", "sized63", {"kd": "kd.lds"}, (), ("sel", "kd.block")),
    "kd_1024": ({"SHD_ROUTE_KERNEL": "kd", "SHD_ROUTE_KDBLOCK": "1024"}, "sized16385", "sized63", {"kd": "kd.lds"},
                ("kd",), ("sel", "kd.block")),
    "kd_hub": ({"SHD_ROUTE_KERNEL": "kd", "SHD_ROUTE_LANDMARKS": "64"}, "sized11212", "sized63",
               {"hub": "kd.hub_lds"}, ("hub",), ("sel", "kd.block", "kd.hub_block")),
    "kf_256": ({"SHD_ROUTE_KERNEL": "kf"}, "sized2688", "sized63", {"kf": "kf.lds"}, (), ("sel", "kf.block", "kf.h")),
    "kf_1024": ({"SHD_ROUTE_KERNEL": "kf"}, "sized11212", "sized2689", {"kf": "kf.lds"}, ("kf",),
                ("sel", "kf.block", "kf.h")),
    "kfh": ({"SHD_ROUTE_KERNEL": "kf", "SHD_ROUTE_KFH": "1"}, "sized16385", "sized63", {"kf": "kf.lds"}, ("kf",),
            ("sel", "kf.block", "kf.h")),
    "f64": ({"SHD_ROUTE_KERNEL": "f64"}, "sized4097", "sized63", {"f64": "f64.bytes"}, ("f64",), ("sel", "f64.lds")),
    "hops": ({}, "sized11212", "sized63", {"hops": hops_lds}, ("hops",), ()),
    "k4": ({}, "sized4097", "sized63", {"rows": k4_rows_lds, "parent8": k4_parent8_lds}, ("parent8",), ()),
}
# what the kernel behind each pair must be (select_main's fields)
KERNEL_OF = {"k32_256": {"sel": 1, "k32.block": 256}, "kb_plain": {"sel": 2, "kb.fused": 0},
             "kb_fused": {"sel": 2, "kb.fused": 1}, "kd_256": {"sel": 4, "kd.block": 256},
             "kd_1024": {"sel": 4, "kd.block": 1024}, "kd_hub": {"sel": 4, "kd.block": 256, "kd.hub_block": 1024},
             "kf_256": {"sel": 5, "kf.block": 256, "kf.h": 0}, "kf_1024": {"sel": 5, "kf.block": 1024, "kf.h": 0},
             "kfh": {"sel": 5, "kf.block": 1024, "kf.h": 1}, "f64": {"sel": 0, "f64.lds": 1}, "hops": {}, "k4": {}}


@pytest.fixture(scope="module")
def selection(tmp_path_factory):
    """name, environment -> the fields of select_main's line (the program is built once, plain)."""
    assert os.path.exists(build.HIPCC), "hipcc is needed to build tests/select_main.cpp"
    d = tmp_path_factory.mktemp("contexts")
    exe = str(d / "select_main")
    subprocess.run([build.HIPCC, f"--offload-arch={build.ARCH}", "-O1", "-std=c++17", "-o", exe,
                    os.path.join(HERE, "select_main.cpp")], check=True)
    files, seen = {}, {}

    def get(gname, env):
        key = (gname, tuple(sorted(env.items())))
        if key not in seen:
            if gname not in files:
                files[gname] = str(d / f"{gname}.txt")
                with open(files[gname], "w") as f:
                    f.write(sc.graph_text(sc.graph(gname)))
            e = {k: v for k, v in os.environ.items() if not k.startswith("SHD_ROUTE_")}
            e.update(env)
            r = subprocess.run([exe, files[gname]], capture_output=True, text=True, env=e)
            assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
            tok = r.stdout.split()
            assert tok[0] == "select"
            seen[key] = {k: float(v) if "." in v or "e" in v or "n" in v else int(v)
                         for k, v in (t.split("=") for t in tok[1:] if "[" not in t)}
        return seen[key]
    return get


def sizes(selection, name):
    """{what: (large bytes, small bytes)} of a pair."""
    env, big, small, what, _, _ = PAIRS[name]
    fb, fs = selection(big, env), selection(small, env)
    val = lambda f, k: k(f) if callable(k) else f[k]
    return {w: (val(fb, k), val(fs, k)) for w, k in what.items()}


def test_every_per_context_kernel_has_a_pair():
    assert set(PAIRS) == set(KERNEL_OF)
    have = {w for p in PAIRS.values() for w in p[3]}
    assert have == {"k32", "kb", "attr", "kb_fused", "kd", "hub", "kf", "f64", "hops", "rows", "parent8"}


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_pair_asks_for_different_amounts(selection, name):
    env, big, small, what, past64, same = PAIRS[name]
    fb, fs = selection(big, env), selection(small, env)
    for k, v in KERNEL_OF[name].items():
        assert fb[k] == v and fs[k] == v, (k, fb[k], fs[k])        # the same kernel function on both
    for k in same:
        assert fb[k] == fs[k], k
    got = sizes(selection, name)
    print(name, got)
    for w, (lb, ls) in got.items():
        assert 0 < ls and lb >= 2 * ls, (w, lb, ls)
        assert lb <= LDS_BUDGET
        assert (lb > KIB64) == (w in past64), (w, lb)
    if name in ("hops", "k4"):
        # both graphs take the LDS forms: the hops state and K4's eligibility (engine.hip fw_eligible)
        for f in (fb, fs):
            assert f["n"] <= 65535 and hops_lds(f) <= LDS_BUDGET
            assert name == "hops" or (f["integer_w"] == 1 and f["multigraph"] == 0 and 0 < f["k32.bound"] < 0xFFFF
                                      and k4_rows_lds(f) <= LDS_BUDGET)
