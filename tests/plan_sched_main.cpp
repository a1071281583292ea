// Stand-alone driver of shadow_amd/csrc/plan_sched.hpp (the seeded-row planner's list
// scheduler) for tests/test_library.py: random seed DAGs -- parents always of a smaller index,
// 0 to 3 seeds per job, some of them landmark rows -- at 1 to ~2000 jobs and 1, 7 and 256
// workgroup slots.  Built with the host sanitizers and run as its own process.  Every order
// must be a permutation in which a job follows all of its non-landmark seeds, the same on a
// second call, and the identity with the schedule off.  Prints one line; exit status 0 = pass.
#include <cstdint>
#include <cstdio>
#include <numeric>

#include "../shadow_amd/csrc/plan_sched.hpp"

using namespace shd;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {  // xorshift64*: the same DAGs on every run
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n;
}

static int check(int nj, int W, int near) {
    std::vector<int> nsd(nj);
    std::vector<SeedIdx> seedjob(nj), lmseed(nj);
    for (int j = 0; j < nj; j++) {
        seedjob[j].fill(0);
        lmseed[j].fill(-1);
        nsd[j] = (int)rnd(PLAN_SCHED_SEEDS + 1);
        const bool lm = rnd(8) == 0;  // a landmark-seeded root: every seed a landmark row
        if (j == 0 && !lm) nsd[j] = 0;
        for (int k = 0; k < nsd[j]; k++) {
            if (lm || rnd(16) == 0) lmseed[j][k] = (int)rnd(64);
            else seedjob[j][k] = near ? j - 1 - (int)rnd((uint32_t)std::min(j, near)) : (int)rnd((uint32_t)j);
        }
    }
    SchedCosts cost;
    if (rnd(4) == 0) { cost.root = 0.1 + rnd(100) / 10.0; cost.lm = 0.1 + rnd(50) / 10.0; cost.flag_at = rnd(11) / 10.0; }
    auto run = [&](bool sched, long long* ticks) {
        return list_schedule(nj, nsd.data(), lmseed.data(), seed_dependants(nj, nsd.data(), seedjob.data(), lmseed.data()),
                             W, cost, sched, ticks);
    };
    long long t1 = -2, t2 = -2, t0 = -2;
    const std::vector<int> order = run(true, &t1);
    if ((int)order.size() != nj) return 1;
    std::vector<int> at(nj, -1);
    for (int q = 0; q < nj; q++) {
        if (order[q] < 0 || order[q] >= nj || at[order[q]] >= 0) return 2;  // a permutation
        at[order[q]] = q;
    }
    for (int j = 0; j < nj; j++)
        for (int k = 0; k < nsd[j]; k++)
            if (lmseed[j][k] < 0 && at[seedjob[j][k]] >= at[j]) return 3;  // after its seeds
    if (run(true, &t2) != order || t1 != t2 || t1 < 0) return 4;  // deterministic
    std::vector<int> id(nj);
    std::iota(id.begin(), id.end(), 0);
    if (run(false, &t0) != id || t0 != -1) return 5;  // schedule off: job order
    return 0;
}

int main() {
    const int Ws[3] = {1, 7, 256};
    int cases = 0;
    for (int rep = 0; rep < 300; rep++) {
        const int nj = rep < 8 ? rep + 1 : rep % 10 == 0 ? 1500 + (int)rnd(600) : 1 + (int)rnd(400);
        const int near = rep % 3 == 0 ? 0 : 1 + (int)rnd(40);  // (near: seeds among the last few jobs, long chains)
        for (int W : Ws) {
            const int rc = check(nj, W, near);
            if (rc) { std::printf("FAIL %d: rep %d nj %d W %d\n", rc, rep, nj, W); return rc; }
            cases++;
        }
    }
    std::printf("ok %d schedules\n", cases);
    return 0;
}
