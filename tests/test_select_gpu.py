"""GPU: shd_route_create decides for every case of tests/golden/select_info.json what it decided
when the fixture was recorded (the rows are bit-exact on whichever kernel a context gets, so only
the context's info can tell that a graph moved to another kernel, block or bucket width)."""
from __future__ import annotations

import json
import os

import pytest

from tests import select_cases as sc

pytestmark = pytest.mark.gpu

WANT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "select_info.json")))


@pytest.mark.parametrize("name", sorted(WANT))
def test_info_matches_recorded(monkeypatch, name):
    from shadow_amd import route
    gname, env = sc.CASES[name]
    for k in [k for k in os.environ if k.startswith("SHD_ROUTE_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = route.RouteEngine(sc.graph(gname))
    try:
        assert {k: eng.info[k] for k in sc.FIELDS} == WANT[name]
    finally:
        eng.close()
