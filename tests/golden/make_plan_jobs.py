#!/usr/bin/env python3
"""Record the seeded-row planner's output (tests/golden/plan_jobs.json).  Needs the GPU.

Every row of a planned launch is bit-exact against the oracle whatever the plan is, so the
rows cannot tell whether a change to the planner moved a seed choice or the queue order.
This fixture can: for each case below it holds the plan's info, a digest of its positions
and a digest of its job array (shd_route_plan_jobs, queue order).  It is DATA recorded from
the planner as it stood when the accessor was added; tests/test_seed_gpu.py
(test_plan_jobs_match_recorded) rebuilds every plan and compares.  A refactor of the
planner must leave this file alone: a mismatch is a bug in the refactor.

  make_plan_jobs.py           build every case twice (fresh engines), write the cases whose
                              two builds agree, name the others
  make_plan_jobs.py --check   build every recorded case again and compare with the file
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "plan_jobs.json")

KD7 = {"SHD_ROUTE_KERNEL": "kd", "SHD_ROUTE_KDGRID": "7"}  # tests/test_seed_gpu.py's kd fixture
KD = {"SHD_ROUTE_KERNEL": "kd"}                             # the context's own grid


def _cases():
    """name -> (graph, environment, world, rank)."""
    c = {}
    # neighbour-seeded, one rank
    for tag, env in (("default", {}), ("seeds1", {"SHD_ROUTE_SEEDS": "1"}), ("hostchoice", {"SHD_ROUTE_GPUCHOICE": "0"}),
                     ("hostchoice_nopipe", {"SHD_ROUTE_GPUCHOICE": "0", "SHD_ROUTE_PIPE": "0"}),
                     ("nosched", {"SHD_ROUTE_SCHED": "0"}), ("no2hop", {"SHD_ROUTE_SEED2HOP": "0"}),
                     ("nolandmarks", {"SHD_ROUTE_LANDMARKS": "0"}), ("depth2", {"SHD_ROUTE_SEED_DEPTH": "2"})):
        c[f"ba400-{tag}"] = ("ba400", {**KD7, **env}, 1, 0)
    c["ties-default"] = ("ties", dict(KD7), 1, 0)
    c["chain-default"] = ("chain", dict(KD7), 1, 0)
    # forest partition: helper rows, two seeds per row
    for r in range(3):
        c[f"ba400-w3r{r}"] = ("ba400", dict(KD7), 3, r)
        c[f"ba400-w3r{r}-hostchoice"] = ("ba400", {**KD7, "SHD_ROUTE_GPUCHOICE": "0"}, 3, r)
    # landmark-seeded roots: every row is a root, so the grid size cannot change the plan
    c["roots300-default"] = ("roots300", dict(KD), 1, 0)
    c["roots300-lm64"] = ("roots300", {**KD, "SHD_ROUTE_LANDMARKS": "64"}, 1, 0)
    # landmark-only plans (the default is built on the device)
    for wtag, world, rank in (("w1", 1, 0), ("w3r1", 3, 1)):
        for tag, env in (("default", {}), ("plandev0", {"SHD_ROUTE_PLANDEV": "0"}),
                         ("hostchoice", {"SHD_ROUTE_GPUCHOICE": "0"}), ("lm2_64", {"SHD_ROUTE_LM2": "64"}),
                         ("lmbias0", {"SHD_ROUTE_LMBIAS": "0"}), ("lmorder0", {"SHD_ROUTE_LMORDER": "0"})):
            c[f"lmonly3000-{wtag}-{tag}"] = ("lmonly3000", {**KD, **env}, world, rank)
    # fallback: a directed graph's plan is unseeded (no job array)
    c["dir-fallback"] = ("dir", dict(KD7), 1, 0)
    return c


def _knob_cases():
    """The planner knob values no default reaches (tests/test_knobs_gpu.py runs their rows): one
    case per value, on the graph, rank and base environment where it moves the plan.  The list
    schedule's costs move a plan only when fewer roots than workgroup slots start at tick 0,
    hence SHD_ROUTE_SEED_ROOTS beside them; SHD_ROUTE_HOPDEG above its default needs a vertex of
    more than 256 neighbours (hub300).  name -> (graph, environment, world, rank), and
    KNOB_OF[name] = the variable the case is about."""
    c, of = {}, {}

    def add(gname, base, world, rank, knob, value):
        tag = gname + ("" if world == 1 else f"-w{world}r{rank}")
        name = f"{tag}-{knob[10:].lower()}{value}"
        c[name] = (gname, {**base, knob: value}, world, rank)
        of[name] = knob

    for knob, value in (("SHD_ROUTE_LMSEEDS", "1"), ("SHD_ROUTE_LMSEEDS", "2"), ("SHD_ROUTE_SEEDALPHA", "0"),
                        ("SHD_ROUTE_SEEDALPHA", "10"), ("SHD_ROUTE_HOPDEG", "1"), ("SHD_ROUTE_SEED_ROOTS", "0"),
                        ("SHD_ROUTE_SEED_ROOTS", "1"), ("SHD_ROUTE_SEED_ROOTS", "1000000"), ("SHD_ROUTE_STORE_SYNC", "1"),
                        ("SHD_ROUTE_FLAGAT", "1")):
        add("ba400", KD7, 1, 0, knob, value)
    add("hub300", KD7, 1, 0, "SHD_ROUTE_HOPDEG", "100000")
    for knob, value in (("SHD_ROUTE_TOPCAP", "1"), ("SHD_ROUTE_TOPCAP", "64")):
        add("ba400", KD7, 3, 1, knob, value)
    for knob, value in (("SHD_ROUTE_ROOTCOST", "0.1"), ("SHD_ROUTE_ROOTCOST", "50"), ("SHD_ROUTE_FLAGAT", "0")):
        add("ba400", {**KD7, "SHD_ROUTE_SEED_ROOTS": "0"}, 1, 0, knob, value)     # one unseeded root
    for knob, value in (("SHD_ROUTE_LMCOST", "0.1"), ("SHD_ROUTE_LMCOST", "50")):
        add("ba400", {**KD7, "SHD_ROUTE_SEED_ROOTS": "1"}, 1, 0, knob, value)     # one landmark-seeded root
    for knob, value in (("SHD_ROUTE_LMSPREAD", "0"), ("SHD_ROUTE_LMALL_SMALL", "0")):
        add("lmonly3000", KD, 1, 0, knob, value)
    return c, of


KNOB_CASES, KNOB_OF = _knob_cases()
CASES = {**_cases(), **KNOB_CASES}


def _hub300():
    """shape_graphs.star(300) with a self-loop on every vertex: the hub has 299 neighbours, more
    than the default SHD_ROUTE_HOPDEG lets a two-hop seed pass through."""
    import dataclasses
    from tests import shape_graphs
    g = shape_graphs.star(300)
    lv = np.setdiff1d(np.arange(g.n), g.src[g.src == g.dst]).astype(np.int32)
    return dataclasses.replace(g, src=np.concatenate([g.src, lv]), dst=np.concatenate([g.dst, lv]),
                               latency=np.concatenate([g.latency, np.full(len(lv), 2.0)]),
                               packetloss=np.concatenate([g.packetloss, np.zeros(len(lv))]), name="hub300")


def graph(name):
    from shadow_amd.graph import internet_like
    from tests.test_kd_gpu import _graph
    if name == "roots300":
        return internet_like(300, 2, seed=340, name="ba300")
    if name == "lmonly3000":
        return internet_like(3000, 3, seed=77, name="ba3000")
    if name == "hub300":
        return _hub300()
    return _graph(name)


def case_env(name):
    """The case's whole SHD_ROUTE_* environment (every other SHD_ROUTE_* variable is unset)."""
    return dict(CASES[name][1])


def jobs_digest(jobs) -> str | None:
    """sha256 over row, s, store, nseed and the first nseed entries of seed, u, wr, rec of every
    job, in queue order (padding and unused seed entries stay out of it)."""
    if jobs is None:
        return None
    h = hashlib.sha256()
    for j in jobs:
        k = int(j["nseed"])
        h.update(np.array([j["row"], j["s"], j["store"], k], "<i4").tobytes())
        for f in ("seed", "u", "wr", "rec"):
            h.update(np.ascontiguousarray(j[f][:k], "<i4").tobytes())
    return h.hexdigest()


def record(name) -> dict:
    """Build the case's plan on a fresh engine, in the environment already set for it."""
    from shadow_amd import route
    gname, _, world, rank = CASES[name]
    g = graph(gname)
    eng = route.RouteEngine(g)
    plan = eng.plan(g.targets(), world, rank)
    jobs = plan.jobs()
    out = dict(info={k: int(v) for k, v in plan.info.items()},
               positions=hashlib.sha256(np.ascontiguousarray(plan.positions, "<i4").tobytes()).hexdigest(),
               njobs=None if jobs is None else len(jobs), jobs=jobs_digest(jobs))
    plan.close()
    eng.close()
    return out


def _record_in_env(name):
    for k in [k for k in os.environ if k.startswith("SHD_ROUTE_")]:
        del os.environ[k]
    os.environ.update(case_env(name))
    return record(name)


if __name__ == "__main__":
    import torch
    torch.cuda.init()  # (torch's HIP runtime before the engine's, as tests/conftest.py)
    if "--check" in sys.argv:
        want = json.load(open(OUT))
        bad = [n for n in want if _record_in_env(n) != want[n]]
        print(f"{len(want) - len(bad)} of {len(want)} recorded cases reproduced; differing: {bad}", flush=True)
        sys.exit(1 if bad else 0)
    first = {n: _record_in_env(n) for n in CASES}
    second = {n: _record_in_env(n) for n in CASES}
    unstable = [n for n in CASES if first[n] != second[n]]
    for n in unstable:
        print(f"not deterministic, left out: {n}\n  {first[n]}\n  {second[n]}", flush=True)
    json.dump({n: first[n] for n in CASES if n not in unstable}, open(OUT, "w"), indent=1)
    print(f"wrote {len(CASES) - len(unstable)} cases to {OUT}", flush=True)
