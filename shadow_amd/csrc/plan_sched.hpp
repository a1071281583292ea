// plan_sched.hpp -- the seeded-row planner's list scheduler (plan.hpp): the queue order of the
// one KD launch from the seed DAG.  Pure host code: no HIP and no engine types, so that
// tests/plan_sched_main.cpp checks it under the host sanitizers without a GPU.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <numeric>
#include <vector>

namespace shd {

constexpr int PLAN_SCHED_SEEDS = 3;  // seeds per job at most (KD_SEEDS)
using SeedIdx = std::array<int, PLAN_SCHED_SEEDS>;

// estimated row times, in seeded rows: an unseeded root, a landmark-seeded root, and the
// share of a kept row's time after which its ready flag is up
struct SchedCosts {
    double root = 3.4, lm = 2.0, flag_at = 0.7;
};

// The seed DAG of nj jobs: job j has nsd[j] seeds, seed k the job seedjob[j][k] (always of a
// smaller index) unless lmseed[j][k] >= 0 (a landmark row: complete before the launch).
// Dependants of each job as one CSR (job j's in [dbeg[j], dbeg[j + 1])); left[j]: the seeds
// job j waits for.
struct SeedDeps {
    std::vector<int> left, dbeg, dep;
};

inline SeedDeps seed_dependants(int nj, const int* nsd, const SeedIdx* seedjob, const SeedIdx* lmseed) {
    SeedDeps D;
    D.left.assign(nj, 0);
    D.dbeg.assign(nj + 1, 0);
    for (int j = 0; j < nj; j++)
        for (int k = 0; k < nsd[j]; k++)
            if (lmseed[j][k] < 0) { D.dbeg[seedjob[j][k] + 1]++; D.left[j]++; }
    for (int j = 0; j < nj; j++) D.dbeg[j + 1] += D.dbeg[j];
    D.dep.resize(D.dbeg[nj]);
    std::vector<int> fill(D.dbeg.begin(), D.dbeg.end() - 1);
    for (int j = 0; j < nj; j++)
        for (int k = 0; k < nsd[j]; k++)
            if (lmseed[j][k] < 0) D.dep[fill[seedjob[j][k]]++] = j;
    return D;
}

// Queue order: list scheduling of the seed DAG over the launch's W workgroups with
// estimated row times (a root ~3.4x a seeded row; a kept row's flag at ~0.7 of it): each
// workgroup, when free, takes the row whose seeds' flags are estimated earliest.  A row
// still follows all of its seeds in the queue (no deadlock), but rows no longer wait at
// every level boundary for seeds just started.  Returns the jobs in queue order (sched
// false: plain job order, the A/B); *ticks: the last bucket reached (-1: none).
inline std::vector<int> list_schedule(int nj, const int* nsd, const SeedIdx* lmseed, SeedDeps D, int W,
                                      const SchedCosts& cost, bool sched, long long* ticks = nullptr) {
    std::vector<int> order;
    order.reserve(nj);
    std::vector<int>& left = D.left;
    const std::vector<int>&dbeg = D.dbeg, &dep = D.dep;
    // times in integer ticks of 1/100 row: the ready queue is a bucket queue (a row
    // becomes ready strictly after the start of the row that releases it, so the
    // queue's minimum only grows and every bucket is complete when it is reached;
    // within a bucket, rows in job order).  A binary heap of (double, job) pairs took
    // ~6 ms at C4.
    auto tk = [](double x) { return (long long)std::llround(x * 100.0); };
    const long long t_root = tk(cost.root), t_lm = tk(cost.lm), t_one = 100;
    // buckets as singly linked lists through one array (no allocation per bucket): a
    // bucket's rows are sorted by job when it is reached
    std::vector<long long> ready(nj, 0);
    std::vector<int> bhead(1024, -1), bnext(nj, -1), cur_b;
    auto push = [&](long long t, int j) {
        if ((size_t)t >= bhead.size()) bhead.resize(std::max((size_t)t + 1, 2 * bhead.size()), -1);
        bnext[j] = bhead[t];
        bhead[t] = j;
    };
    size_t bq_n = 0;  // rows queued
    for (int j = nj - 1; j >= 0; j--) if (!left[j]) { push(0, j); bq_n++; }
    // free walker slots: a second bucket queue over ticks (a slot frees at its row's
    // start + cost >= the current minimum, so this minimum only grows too); it replaced
    // a binary heap of (tick, slot) pairs, 11.4 -> 7.4 ms for C4's schedule on the host
    std::vector<int> fhead(1024, -1), fnext(W, -1);
    auto fpush = [&](long long t, int w) {
        if ((size_t)t >= fhead.size()) fhead.resize(std::max((size_t)t + 1, 2 * fhead.size()), -1);
        fnext[w] = fhead[t];
        fhead[t] = w;
    };
    for (int w = W - 1; w >= 0; w--) fpush(0, w);
    long long fcur = 0;
    long long cur = -1;
    size_t pos = 0;
    if (!sched) {  // A/B: plain rank order
        order.resize(nj);
        std::iota(order.begin(), order.end(), 0);
        bq_n = 0;
    }
    while (bq_n) {
        while (pos >= cur_b.size()) {  // next non-empty bucket
            cur++;
            cur_b.clear();
            pos = 0;
            if ((size_t)cur < bhead.size())
                for (int j = bhead[cur]; j >= 0; j = bnext[j]) cur_b.push_back(j);
            if (cur_b.size() > 1) std::sort(cur_b.begin(), cur_b.end());
        }
        const int j = cur_b[pos++];
        bq_n--;
        while (fhead[fcur] < 0) fcur++;
        const int fw = fhead[fcur];
        fhead[fcur] = fnext[fw];
        const long long t = !nsd[j] ? t_root : lmseed[j][0] >= 0 ? t_lm : t_one;
        const long long start = std::max(fcur, cur);
        fpush(start + t, fw);
        order.push_back(j);
        const long long rel = start + std::max(1ll, tk(cost.flag_at * (double)t / 100.0));
        for (int e = dbeg[j]; e < dbeg[j + 1]; e++) {
            const int d = dep[e];
            ready[d] = std::max(ready[d], rel);
            if (--left[d] == 0) { push(ready[d], d); bq_n++; }
        }
    }
    if (ticks) *ticks = cur;
    return order;
}

}  // namespace shd
