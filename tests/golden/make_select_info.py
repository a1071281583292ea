#!/usr/bin/env python3
"""Record the kernel selection of shd_route_create (tests/golden/select_info.json).  Needs the GPU.

Every rows kernel is bit-exact against the oracle, so the parity tests pass on whichever kernel
a context was given: a change that moves a graph across a limit (from KD to f64, say) shows in no
row.  This fixture can tell: for each case of tests/select_cases.py (a graph and a creation-time
SHD_ROUTE_* environment) it holds what RouteEngine.info reported.  It is DATA recorded from the
engine as it stood before the selection became select.hpp; tests/test_select.py compares the
host-only selection with it and tests/test_select_gpu.py the created context.  A refactor of
the selection must leave this file alone: a mismatch is a bug in the refactor.

  make_select_info.py           create every case twice, write the cases whose two contexts
                                agree, name the others
  make_select_info.py --check   create every recorded case again and compare with the file
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "select_info.json")


def record(name) -> dict:
    """Create the case's context in its own SHD_ROUTE_* environment (every other SHD_ROUTE_*
    variable is unset) and return the recorded fields of its info."""
    from shadow_amd import route
    from tests import select_cases as sc
    gname, env = sc.CASES[name]
    for k in [k for k in os.environ if k.startswith("SHD_ROUTE_")]:
        del os.environ[k]
    os.environ.update(env)
    eng = route.RouteEngine(sc.graph(gname))
    info = {k: eng.info[k] for k in sc.FIELDS}
    eng.close()
    return info


def coverage(cases: dict) -> list:
    """What the file must contain and does not: every selectable kernel, every KD and KF block."""
    have = {(i["kernel"], i["block"]) for i in cases.values()}
    need = [(0, 256), (1, None), (2, None), (4, 256), (4, 1024), (5, 256), (5, 1024)]
    return [(k, b) for k, b in need if not any(hk == k and (b is None or hb == b) for hk, hb in have)]


if __name__ == "__main__":
    import torch
    torch.cuda.init()  # (torch's HIP runtime before the engine's, as tests/conftest.py)
    from tests.select_cases import CASES
    if "--check" in sys.argv:
        want = json.load(open(OUT))
        bad = [n for n in want if record(n) != want[n]]
        print(f"{len(want) - len(bad)} of {len(want)} recorded cases reproduced; differing: {bad}", flush=True)
        sys.exit(1 if bad else 0)
    first = {n: record(n) for n in CASES}
    second = {n: record(n) for n in CASES}
    unstable = [n for n in CASES if first[n] != second[n]]
    for n in unstable:
        print(f"not deterministic, left out: {n}\n  {first[n]}\n  {second[n]}", flush=True)
    kept = {n: first[n] for n in CASES if n not in unstable}
    json.dump(kept, open(OUT, "w"), indent=1)
    print(f"wrote {len(kept)} cases to {OUT}; (kernel, block) not covered: {coverage(kept)}", flush=True)
