"""Host validation of a seeded plan's job records (shd_route_plan_jobs), in plain Python.

A planned rows launch takes its jobs from a queue: a workgroup that dequeues a seeded job waits
for the ready flag of each seed's store slot, which the job that computes that row sets.  The
rows are bit-exact against the oracle under any valid plan, so the rows cannot show a bad plan;
and a plan whose queue order puts a row ahead of the row it seeds from makes a workgroup wait
for a flag nobody sets.  So the tests that run a plan nobody has run before (tests/
test_knobs_gpu.py) hold its job array to the rules below first, and launch only what passes.

    validate(jobs, sources, positions, dist, landmarks=None)

  jobs       RoutePlan.jobs(): JOB_DTYPE records in queue order
  sources    the source list the plan was made over; positions = RoutePlan.positions
  dist       dist(s) -> the exact latencies of source s to every vertex (the oracle's row;
             NaN = unreachable)
  landmarks  RoutePlan.landmarks() (a device-built landmark-only plan), else None

Rules, over the array in queue order:
  1. the jobs with row >= 0 write every output row of the plan once, and job.s is that row's
     source; a job with row < 0 is a helper row, kept for others to seed from (one without a
     store slot is computed for nothing: counted as an idle helper, not refused)
  2. 0 <= nseed <= 3
  3. for each used seed k the latest earlier job with store == seed[k] exists and has
     s == u[k].  A slot that no job of the array writes is a landmark-store slot: every job that
     names it must name the same vertex, two such slots hold two vertices, and they lie after
     every slot the array writes (a device-built landmark-only plan: below landmarks["nland"],
     and no job writes a slot)
  4. wr[k] is an integer in [d(s, u[k]), 0xFFFF] (an upper bound of the seed's distance in the
     store's u16 units; below the exact distance the row would come out too short)
(A slot that is written twice serves each reader its latest earlier row, which rule 3 holds
to the vertex the reader names.)

Returns a summary dict (counts by kind) for the caller's own assertions."""
from __future__ import annotations

import numpy as np

KD_SEEDS = 3


class PlanError(AssertionError):
    pass


def _fail(q, job, what):
    raise PlanError(f"job {q} (row {int(job['row'])}, s {int(job['s'])}, store {int(job['store'])}, "
                    f"nseed {int(job['nseed'])}, seed {job['seed'].tolist()}, u {job['u'].tolist()}, "
                    f"wr {job['wr'].tolist()}): {what}")


def validate(jobs, sources, positions, dist, landmarks=None):
    sources = np.asarray(sources)
    positions = np.asarray(positions)
    nrows = len(positions)
    if jobs is None:
        raise PlanError("no job array (an unseeded plan)")
    for f in ("row", "s", "store", "nseed", "seed", "u", "wr"):
        if not np.issubdtype(jobs.dtype[f].base, np.integer):
            raise PlanError(f"field {f} is not an integer")
    written = set(int(x) for x in jobs["store"] if x >= 0)      # every slot some job writes
    seen_rows = np.zeros(nrows, np.int64)
    writer = {}          # slot -> (queue index, source) of its latest writer so far
    landmark = {}        # landmark slot -> vertex
    summary = dict(jobs=len(jobs), helpers=0, idle_helpers=0, unseeded=0, landmark_seeds=0, row_seeds=0, slots=len(written))
    for q, J in enumerate(jobs):
        row, s, store, k = int(J["row"]), int(J["s"]), int(J["store"]), int(J["nseed"])
        if row >= 0:
            if row >= nrows:
                _fail(q, J, f"output row past the plan's {nrows} rows")
            seen_rows[row] += 1
            if s != int(sources[positions[row]]):
                _fail(q, J, f"row {row} belongs to source {int(sources[positions[row]])}")
        else:
            summary["helpers"] += 1
            summary["idle_helpers"] += store < 0
        if not 0 <= k <= KD_SEEDS:
            _fail(q, J, "nseed outside 0..3")
        if k == 0:
            summary["unseeded"] += 1
        drow = dist(s) if k else None
        for i in range(k):
            slot, u, wr = int(J["seed"][i]), int(J["u"][i]), int(J["wr"][i])
            if slot < 0:
                _fail(q, J, f"seed {i}: negative store slot")
            if slot in writer:
                if writer[slot][1] != u:
                    _fail(q, J, f"seed {i}: slot {slot} holds the row of {writer[slot][1]} (job {writer[slot][0]}), not of {u}")
                summary["row_seeds"] += 1
            elif slot in written:
                _fail(q, J, f"seed {i}: slot {slot} is written only by a later job: the row would wait for ever")
            else:
                if landmark.setdefault(slot, u) != u:
                    _fail(q, J, f"seed {i}: landmark slot {slot} was vertex {landmark[slot]} before")
                if landmarks is not None and slot >= landmarks["nland"]:
                    _fail(q, J, f"seed {i}: landmark slot {slot} past the store's {landmarks['nland']}")
                summary["landmark_seeds"] += 1
            d = 0.0 if u == s else float(drow[u])
            if not (d == d):
                _fail(q, J, f"seed {i}: {u} is unreachable from {s}")
            if not (d <= wr <= 0xFFFF):
                _fail(q, J, f"seed {i}: wr {wr} outside [d(s, u) = {d}, 0xFFFF]")
        if store >= 0:
            writer[store] = (q, s)
    if not np.all(seen_rows == 1):
        bad = np.flatnonzero(seen_rows != 1)
        raise PlanError(f"output rows not written exactly once: {bad[:16].tolist()} (counts {seen_rows[bad[:16]].tolist()})")
    if len(set(landmark.values())) != len(landmark):
        raise PlanError("two landmark slots hold the same vertex")
    if landmark and written and min(landmark) <= max(written):
        raise PlanError(f"landmark slot {min(landmark)} inside the kept rows' slots (up to {max(written)})")
    if landmarks is not None and written:
        raise PlanError("a device-built landmark-only plan keeps no rows, yet a job has a store slot")
    summary["landmarks"] = len(landmark)
    return summary
