"""CPU: the C-ABI library loads and exports every symbol include/shd_route.h declares
(no compute calls: there is no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, "include", "shd_route.h")).read()
    return sorted(set(re.findall(r"\b(shd_route_[a-z_]+)\s*\(", text)))


def test_header_matches_binding_exports():
    from shadow_amd import route
    assert sorted(route.EXPORTS) == header_symbols()


def test_library_exports_all_symbols():
    from shadow_amd import build, route
    if not os.path.exists(route.LIB_PATH):
        build.build()
    lib = ctypes.CDLL(route.LIB_PATH)
    for sym in header_symbols():
        assert hasattr(lib, sym), sym
    # pure host function: safe without a GPU
    route.load_library()
    assert route.strerror(route.ENOEDGE).startswith("path hop")
    assert route.strerror(0) == "success"


def test_no_cpu_fallback_when_missing(tmp_path, monkeypatch):
    from shadow_amd import route
    monkeypatch.setattr(route, "LIB_PATH", str(tmp_path / "missing.so"))
    monkeypatch.setattr(route, "_lib", None)
    with pytest.raises(RuntimeError, match="not built"):
        route.load_library()


def test_product_does_not_import_oracle():
    """Only tests/, smoke() and bench.py's cpu_baseline may touch oracle/."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "shadow_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".c", ".cpp", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("oracle/", "").lower() or f == "__init__.py", f


def test_front_end_exports():
    import re
    from shadow_amd import build, topology
    build.build()
    text = open(os.path.join(ROOT, "include", "shd_topology.h")).read()
    declared = sorted(set(re.findall(r"\b(shd_(?:topology|graphml|attach)_[a-z_]+)\s*\(", text)))
    assert sorted(topology.EXPORTS) == declared
    lib = ctypes.CDLL(topology.LIB_PATH)
    for sym in declared:
        assert hasattr(lib, sym), sym


def _dyn_exports(path, prefix):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith(prefix)})


def test_cmake_hip_target(tmp_path):
    """integration/CMakeLists.txt (enable_language(HIP), CMAKE_HIP_ARCHITECTURES gfx950) the
    way Shadow's build would take it (reference src/main/CMakeLists.txt:103-108): configure
    and build out of tree; the engine carries a gfx950 code object and exports exactly the
    C-ABI of include/shd_route.h, the front end that of include/shd_topology.h."""
    import shutil
    import subprocess
    from shadow_amd import route, topology
    if not shutil.which("cmake") or not os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        pytest.skip("cmake or the ROCm clang is not installed")
    b = tmp_path / "cmake"
    subprocess.run(["cmake", "-S", os.path.join(ROOT, "integration"), "-B", str(b)], check=True,
                   capture_output=True)
    subprocess.run(["cmake", "--build", str(b), "-j8"], check=True, capture_output=True)
    eng, front = str(b / "libshd_route.so"), str(b / "libshd_topology.so")
    assert _dyn_exports(eng, "shd_route_") == sorted(route.EXPORTS)
    assert _dyn_exports(front, "shd_") == sorted(topology.EXPORTS)
    assert b"gfx950" in open(eng, "rb").read()
    assert os.path.exists(b / "glue_test") or not os.path.exists("/opt/conda/lib/libglib-2.0.so")


def test_host_wait_unregistered_chunk_not_fatal(monkeypatch):
    """a 256 MiB chunk the runtime refuses to register stays pageable and usable,
    so shd_route_host_wait reports success and shd_route_host_unpinned counts the chunk.
    Chunk 1 of three is forced to fail; without a GPU every registration fails, and the
    buffer is still fully usable memory."""
    import torch
    from shadow_amd import route
    monkeypatch.setenv("SHD_ROUTE_REGFAIL_CHUNK", "1")
    mib = 1 << 20
    buf = route.PinnedBuffer(520 * mib, lazy=True)
    try:
        buf.wait()  # must not raise
        un = buf.unpinned()
        if torch.cuda.is_available():
            assert un == 256 * mib
        else:
            assert un >= 256 * mib
        a = buf.array()
        a[:: 4096] = 1.0
        assert float(a[:: 4096].sum()) == len(a[:: 4096])
    finally:
        buf.close()


def test_plan_scheduler_standalone_sanitized(tmp_path):
    """The planner's list scheduler (shadow_amd/csrc/plan_sched.hpp: pure host code) with
    tests/plan_sched_main.cpp, built with -fsanitize=address,undefined and run as its own
    process: 900 random seed DAGs (1 to ~2000 jobs; 1, 7 and 256 workgroup slots); every
    order is a permutation with each job after its non-landmark seeds, the same on a second
    call, and the identity with the schedule off."""
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked statically where g++ has them (the program then starts whatever
    # else the process environment loads), else the shared ones
    for extra in (["-static-libasan", "-static-libubsan"], []):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover", *extra]
        if subprocess.run([cxx, *san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip("g++ lacks the sanitizer runtime")
    exe = tmp_path / "plan_sched_test"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *san, "-o", str(exe),
                    os.path.join(ROOT, "tests", "plan_sched_main.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stdout.strip() == "ok 900 schedules", r.stdout


def test_fill_schedule_standalone_sanitized(tmp_path):
    """The schedule of shd_route_fill_triangle (shadow_amd/csrc/fill_sched.hpp: pure host code)
    with tests/fill_sched_main.cpp, built with -fsanitize=address,undefined and run as its own
    process: 1080 random rank shares (na 1 to ~3000, world 1 to 8, both layouts, stages from one
    row to everything, host chunks of 0, 2 and 6 MiB) against a brute-force byte map of the
    triangle, and the default constants at the C3 and C4 sizes, whose chunk, buffer-reuse and
    copy-piece counts the output line puts on record (C4, one rank: 38 chunks interleaved, 25
    compact -- 36 and 23 packs of a staging buffer that was copied out before)."""
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for extra in (["-static-libasan", "-static-libubsan"], []):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover", *extra]
        if subprocess.run([cxx, *san, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip("g++ lacks the sanitizer runtime")
    exe = tmp_path / "fill_sched_test"
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *san, "-o", str(exe),
                    os.path.join(ROOT, "tests", "fill_sched_main.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr)
    print(r.stdout.strip())
    m = re.fullmatch(r"ok 1088 schedules; c3 interleaved 2 chunks 0 reuses \d+ pieces compact 1 chunks 0 reuses \d+ pieces "
                     r"world2 .*, c4 interleaved 38 chunks 36 reuses \d+ pieces compact 25 chunks 23 reuses \d+ pieces "
                     r"world8 interleaved (\d+) chunks (\d+) reuses \d+ pieces world8 compact (\d+) chunks (\d+) reuses \d+ pieces",
                     r.stdout.strip())
    assert m, r.stdout
    assert int(m.group(1)) - 2 == int(m.group(2)) >= 1 and int(m.group(3)) - 2 == int(m.group(4)) >= 1
