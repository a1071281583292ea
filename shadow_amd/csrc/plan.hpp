// plan.hpp -- seeded planning (shd_route_plan_*): which row seeds which, how a multi-GPU
// rank's rows are partitioned, and the queue order of the one KD launch.  Part of engine.hip's
// translation unit: included there once struct shd_route, HostPool, DevBuf, kd_args,
// kd_launch, take_err and hip_check are defined.  The planner's kernels come first, then
// struct shd_route_plan, the options (every environment knob, read in one place), the hub /
// landmark rows, the stages of a plan in the order shd_route_plan_create runs them, and the
// entry points.  The list scheduler is plan_sched.hpp (pure host code).
#pragma once

#include <array>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <thread>

#include "plan_sched.hpp"

namespace {
// The planner's seed choices on the device (shd_route_plan_create): one thread per source
// row, the same rule as the host's choose() -- the kseeds neighbours u of smaller closeness
// rank (and with a row in the plan) by (w(s,u) + alpha * closeness(u), u), then, if short,
// two-hop rows s -> x -> u (deg x <= hop_deg) by (w(s,x) + w(x,u) + closeness(u), u, record).
// Arcs from the packed out-records (u | w << 16 | ridx << 24).  Entries [0, m) are
// neighbour seeds, [m, m + nh) two-hop seeds (w = w(s,x) + w(x,u), record (x,u)).
// Up to PC_CAND neighbour candidates are listed in order (ncand of them asked for), so
// that the sequential pass, whose usable set is a subset of `avail` (the seed-chain depth
// cap), finds the exact top-kseeds usable ones in the list instead of rescanning the CSR
// row on the host (C3: 928 host recomputations, ~2 ms of the 4.1 ms plan).
constexpr int PC_CAND = 6;
struct PlanChoice {
    int m, nh;
    int u[PC_CAND], w[PC_CAND];
    uint32_t rec[PC_CAND];
    int pad[2];
};
static_assert(KD_SEEDS <= 3 && 2 * KD_SEEDS <= PC_CAND, "PlanChoice holds the candidates");

// A root's landmark seeds on the device (shd_route_plan_create): one wave per root row s, the
// host rule -- the klm landmarks nearest s by (d_L(s), landmark index) (undirected graphs:
// d_L(s) = d(s, L)), each with the record of L's own vertex in s's tree: the last arc (x, L)
// of the s -> L path in L's tree, found by walking L's parent records up from s.
constexpr int LM_DIV_K = 16;  // spread landmark seeds: up to 64 x 16 = 1024 landmarks per row's wave
struct LmChoice {
    int m;
    int l[3], d[3];
    uint32_t rec[3];
    int pad[2];
};
// (bias, device-built landmark-only plans, round 6: a landmark's pick key is d(s, L) + bias[L],
// bias = half L's mean distance to the first 16 landmarks, so that of two landmarks about as
// near to s the more central one seeds the row: its row bounds more of s's paths.  Offline on C3
// (tools/landmark_choice.py, 300 sampled rows, exact distances): the share of vertices a row
// improves on its bound 15.9% -> 13.1%; weights 0.375-0.625 measure the same, 0.25 13.5%, 1.0 15.3%)
__device__ inline LmChoice lm_pick(const uint16_t* __restrict__ drow, const uint32_t* __restrict__ prow, long long rs,
                                   const int* __restrict__ lmv, int nland, int s, int klm, int n, int lane,
                                   const uint16_t* __restrict__ bias = nullptr, int spread = 0) {
    LmChoice o;
    o.m = 0; o.pad[0] = o.pad[1] = 0;
    for (int k = 0; k < 3; k++) { o.l[k] = 0; o.d[k] = 0; o.rec[k] = 0u; }
    // L's own record in s's tree: the last arc (x, L) of L's tree path from s
    auto rec_of = [&](int l) __attribute__((always_inline)) {
        const int L = lmv[l];
        uint32_t rec = KD_SRC_MARK;
        if (L != s) {
            const uint32_t* lp = prow + (long long)l * rs;
            int x = s;
            for (int hop = 0; hop < n && (int)(lp[x] & 0xFFFFu) != L; hop++) x = (int)(lp[x] & 0xFFFFu);
            rec = (uint32_t)x | (lp[x] & 0xFFFF0000u);
        }
        return rec;
    };
    if (bias && spread && nland <= 64 * LM_DIV_K) {
        // Spread seeds (round 6): each next landmark minimises d(s, L) + bias[L] - d(L', L) / 2
        // over the landmarks not picked, L' the nearest already-picked one (its row gives
        // d(L', L) at L's vertex), so the seeds bound s's paths from different sides.  Offline
        // on C3 (tools/landmark_choice.py, 300 rows): improved share 13.5% (central-biased
        // nearest) -> 9.3%; separation weights 3/8-5/8 the same, 3/4 10.6%, 1 14.1%.
        int dl[LM_DIV_K], sc[LM_DIV_K];
#pragma unroll
        for (int j = 0; j < LM_DIV_K; j++) {
            const int l = lane + 64 * j;
            const unsigned d = l < nland ? drow[(long long)l * rs + s] : 0xFFFFu;
            dl[j] = (int)d;
            sc[j] = (l < nland && d != 0xFFFFu) ? (int)d + (int)bias[l] : 0x7FFFFFFF;
        }
        int sep[LM_DIV_K];
#pragma unroll
        for (int j = 0; j < LM_DIV_K; j++) sep[j] = 0x7FFFFFFF;
        for (int k = 0; k < klm && k < 3; k++) {
            // the wave's minimum of (score, l) over the landmarks not yet picked
            unsigned long long best = ~0ull;
#pragma unroll
            for (int j = 0; j < LM_DIV_K; j++) {
                if (sc[j] == 0x7FFFFFFF) continue;
                const int x = k == 0 ? sc[j] : sc[j] - sep[j] / 2;
                const unsigned long long key = ((unsigned long long)(unsigned)(x + 0x40000000) << 32) |
                                               (unsigned)(lane + 64 * j);
                best = min(best, key);
            }
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long y = ((unsigned long long)(unsigned)__shfl_xor((int)(best >> 32), off) << 32) |
                                             (unsigned)__shfl_xor((int)(unsigned)best, off);
                best = min(best, y);
            }
            if (best == ~0ull) break;
            const int l = (int)(unsigned)best;
            int dpick = 0;  // (register arrays indexed by unrolled constants only: no scratch)
#pragma unroll
            for (int j = 0; j < LM_DIV_K; j++)
                if (j == (l >> 6)) {
                    if ((l & 63) == lane) sc[j] = 0x7FFFFFFF;  // (picked)
                    dpick = dl[j];
                }
            // separations to the picked landmark: its row at every landmark's vertex
            if (k + 1 < klm) {
                const uint16_t* lr = drow + (long long)l * rs;
#pragma unroll
                for (int j = 0; j < LM_DIV_K; j++) {
                    const int q = lane + 64 * j;
                    if (q < nland) sep[j] = min(sep[j], (int)lr[lmv[q]]);
                }
            }
            o.l[k] = l; o.d[k] = __shfl(dpick, l & 63); o.rec[k] = rec_of(l);
            o.m = k + 1;
        }
        return o;
    }
    // each lane's three smallest keys (d << 16 | l) over its landmarks l = lane + 64 j, read
    // once; the wave's k-th pick is then the minimum over the lanes' lists past the (k-1)-th
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    uint32_t c0 = NONE, c1 = NONE, c2 = NONE;
    for (int l0 = 0; l0 < nland; l0 += 64 * 8) {
        uint32_t d8[8];
#pragma unroll
        for (int h = 0; h < 8; h++) {
            const int l = l0 + 64 * h + lane;
            d8[h] = l < nland ? drow[(long long)l * rs + s] : 0xFFFFu;
        }
        if (bias) {
#pragma unroll
            for (int h = 0; h < 8; h++) {
                const int l = l0 + 64 * h + lane;
                if (l < nland && d8[h] != 0xFFFFu) d8[h] = min(0xFFFEu, d8[h] + (uint32_t)bias[l]);
            }
        }
#pragma unroll
        for (int h = 0; h < 8; h++) {
            const uint32_t key = (d8[h] << 16) | (uint32_t)(l0 + 64 * h + lane);
            if (d8[h] == 0xFFFFu) continue;
            if (key < c2) {
                c2 = key;
                if (c2 < c1) { const uint32_t t = c1; c1 = c2; c2 = t; }
                if (c1 < c0) { const uint32_t t = c0; c0 = c1; c1 = t; }
            }
        }
    }
    for (int k = 0; k < klm && k < 3; k++) {
        uint32_t best = c0;
        for (int off = 32; off > 0; off >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, off));
        if (best == NONE) break;
        if (c0 == best) { c0 = c1; c1 = c2; c2 = NONE; }  // (keys are unique: one lane owns it)
        const int l = (int)(best & 0xFFFFu);
        // (with a bias the key is not the distance: the offset is read back)
        o.l[k] = l; o.d[k] = bias ? (int)drow[(long long)l * rs + s] : (int)(best >> 16); o.rec[k] = rec_of(l);
        o.m = k + 1;
    }
    return o;
}

__global__ void plan_landmark_kernel(const uint16_t* __restrict__ drow, const uint32_t* __restrict__ prow, long long rs,
                                     const int* __restrict__ lmv, int nland, const int* __restrict__ srcq, int nq, int klm,
                                     int n, LmChoice* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (q >= nq) return;  // the whole wave
    const LmChoice o = lm_pick(drow, prow, rs, lmv, nland, srcq[q], klm, n, lane);
    if (lane == 0) out[q] = o;
}

// Landmark-only plans built on the device (round 5): the queue order and the job records
// without a host round trip.  The order is the host rule's: descending (closeness, vertex,
// position), closeness = the sum of the first nclose hub rows' distances (unreached: the
// largest key).  Keys are unique, so a job's queue slot is the number of larger keys (a rank
// sort: every workgroup holds all keys in LDS, nq <= PLAN_DEV_MAXJ; ~20 us at C3, where a
// one-workgroup bitonic sort took ~0.3 ms).
constexpr int PLAN_DEV_MAXJ = 16384;
__global__ void plan_lmall_keys_kernel(const uint16_t* __restrict__ drow, long long rs, int nclose,
                                       const int* __restrict__ srcq, int nq, unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const int s = srcq[i];
    unsigned sum = 0;
    bool unr = false;
    for (int q = 0; q < nclose; q++) {
        const unsigned d = drow[(long long)q * rs + s];
        unr = unr || d == 0xFFFFu;
        sum += d;
    }
    if (unr) sum = (1u << 20) - 1;  // (16 finite distances sum below it)
    keys[i] = ((unsigned long long)sum << 40) | ((unsigned long long)s << 24) | (unsigned long long)i;
}
__global__ __launch_bounds__(256) void plan_lmall_rank_kernel(const unsigned long long* __restrict__ keys, int nq,
                                                              int* __restrict__ slot) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long rkeys[];
    for (int j = threadIdx.x; j < nq; j += blockDim.x) rkeys[j] = keys[j];
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const unsigned long long k = rkeys[i];
    int r = 0;
    for (int j = 0; j < nq; j++) r += rkeys[j] > k;  // (same j across the wave: an LDS broadcast)
    slot[i] = r;
}

// one wave per job i (jobs in position order, so that a workgroup's waves read neighbouring
// columns of the landmark rows, and consecutive workgroups on one XCD: blockIdx.x % 8 picks
// the XCD, which takes one contiguous eighth of the jobs), the landmark seeds of the row
// (lm_pick) written as its KDJob at its queue slot.  row = the position's index in this
// rank's rows, seeds = landmark slots (the borrowed store holds the landmark rows only).
// nroots counts the jobs left unseeded (no landmark reaches s).
__global__ void plan_lmall_jobs_kernel(const uint16_t* __restrict__ drow, const uint32_t* __restrict__ prow, long long rs,
                                       const int* __restrict__ lmv, int nland, const int* __restrict__ srcq,
                                       const int* __restrict__ slot, int nq, int klm, int n, KDJob* __restrict__ out,
                                       int* __restrict__ nroots, int hub_base = -1,
                                       const uint16_t* __restrict__ bias = nullptr, int spread = 0) {
    const int lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    const int per = gridDim.x / 8;  // (the grid is a multiple of 8 workgroups)
    const int b = (int)(blockIdx.x % 8) * per + (int)(blockIdx.x / 8);  // (XCD-contiguous block order)
    const int i = b * wpb + (threadIdx.x >> 6);
    if (i >= nq) return;  // the whole wave
    const int s = srcq[i];
    const LmChoice o = lm_pick(drow, prow, rs, lmv, nland, s, klm, n, lane, bias, spread);
    if (lane == 0) {
        // (hub_base >= 0: a second-level landmark row of the plan's own hub launch, kept in
        // store slot hub_base + i, no output row)
        KDJob J;
        J.row = hub_base >= 0 ? -1 : i; J.s = s; J.store = hub_base >= 0 ? hub_base + i : -1; J.nseed = o.m;
        for (int k = 0; k < KD_SEEDS; k++) {
            const bool on = k < o.m;
            J.seed[k] = on ? o.l[k] : 0;
            J.u[k] = on ? lmv[o.l[k]] : 0;
            J.wr[k] = on ? o.d[k] : 0;
            J.rec[k] = on ? (int)o.rec[k] : 0;
        }
        out[slot ? slot[i] : i] = J;
        if (o.m == 0 && nroots) atomicAdd(nroots, 1);
    }
}

// each landmark's pick bias (lm_pick): half its mean distance to the first nclose landmarks,
// rounded, from the landmark rows (unreached: the largest bias)
__global__ void plan_lmall_bias_kernel(const uint16_t* __restrict__ drow, long long rs, int nclose,
                                       const int* __restrict__ lmv, int nland, uint16_t* __restrict__ bias) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nland) return;
    const int v = lmv[l];
    unsigned sum = 0;
    bool unr = false;
    for (int q = 0; q < nclose; q++) {
        const unsigned d = drow[(long long)q * rs + v];
        unr = unr || d == 0xFFFFu;
        sum += d;
    }
    bias[l] = unr ? (uint16_t)0x7FFF : (uint16_t)min(0x7FFFu, (sum + (unsigned)nclose) / (2u * (unsigned)nclose));
}

// lexicographic minimum of (x, u, t) over the wave (t: a tie-breaking key, arc or record)
__device__ inline void wave_min3(double& x, int& u, uint32_t& t) {
    for (int o = 32; o > 0; o >>= 1) {
        const double x2 = __shfl_xor(x, o);
        const int u2 = __shfl_xor(u, o);
        const uint32_t t2 = __shfl_xor(t, o);
        if (x2 < x || (x2 == x && (u2 < u || (u2 == u && t2 < t)))) { x = x2; u = u2; t = t2; }
    }
}

// one wave per source row: each pick is the wave's minimum key over the arcs whose head is
// not picked yet, which is the host's top-k of the per-head best keys (duplicate heads of a
// multigraph keep their best arc, the first one on a full tie)
__global__ void plan_choice_kernel(const int* __restrict__ row, const uint32_t* __restrict__ orec,
                                   const double* __restrict__ close, const int* __restrict__ rk,
                                   const uint8_t* __restrict__ avail, const int* __restrict__ srcq, int nq, int kseeds,
                                   int two_hop, int hop_deg, double alpha, int ncand, PlanChoice* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (q >= nq) return;  // the whole wave
    const int s = srcq[q], rks = rk[s], a0 = row[s], a1 = row[s + 1];
    int su[PC_CAND], sw[PC_CAND];
    uint32_t sr[PC_CAND];
#pragma unroll
    for (int k = 0; k < PC_CAND; k++) { su[k] = -1; sw[k] = 0; sr[k] = 0u; }
    auto picked = [&](int u) {
        bool p = false;
#pragma unroll
        for (int k = 0; k < PC_CAND; k++) p = p || u == su[k];
        return p;
    };
    ncand = max(kseeds, min(ncand, PC_CAND));
    int m = 0;
    for (; m < ncand; m++) {
        double bx = INFINITY;
        int bu = INT_MAX;
        uint32_t ba = UINT_MAX;
        for (int a = a0 + lane; a < a1; a += 64) {
            const uint32_t r = orec[a];
            const int u = (int)(r & 0xFFFFu);
            if (u == s || picked(u) || !avail[u] || rk[u] >= rks) continue;
            const double x = (double)((r >> 16) & 0xFFu) + alpha * close[u];
            if (x < bx || (x == bx && (u < bu || (u == bu && (uint32_t)a < ba)))) { bx = x; bu = u; ba = (uint32_t)a; }
        }
        wave_min3(bx, bu, ba);
        if (ba == UINT_MAX) break;
        const uint32_t r = orec[ba];
        su[m] = bu;
        sw[m] = (int)((r >> 16) & 0xFFu);
        sr[m] = (uint32_t)s | ((r >> 24) << 16) | ((r >> 16 & 0xFFu) << 24);
    }
    int nh = 0;
    if (two_hop && m < kseeds) {
        const int need = kseeds - m;
        int hu[3] = {-1, -1, -1};
        for (; nh < need; nh++) {
            double bx = INFINITY;
            int bu = INT_MAX;
            uint32_t br = UINT_MAX;
            int bo = 0;
            for (int a = a0; a < a1; a++) {
                const uint32_t ra = orec[a];
                const int x = (int)(ra & 0xFFFFu);
                if (x == s || row[x + 1] - row[x] > hop_deg) continue;
                const int wa = (int)((ra >> 16) & 0xFFu);
                for (int b = row[x] + lane; b < row[x + 1]; b += 64) {
                    const uint32_t rb = orec[b];
                    const int u = (int)(rb & 0xFFFFu);
                    if (u == s || u == x || rk[u] >= rks || !avail[u]) continue;
                    if (picked(u) || u == hu[0] || u == hu[1] || u == hu[2]) continue;
                    const int wb = (int)((rb >> 16) & 0xFFu);
                    const double cost = (double)wa + (double)wb + close[u];
                    const uint32_t rec = (uint32_t)x | ((rb >> 24) << 16) | ((uint32_t)wb << 24);
                    if (cost < bx || (cost == bx && (u < bu || (u == bu && rec < br)))) { bx = cost; bu = u; br = rec; bo = wa + wb; }
                }
            }
            const double x0 = bx;
            const int u0 = bu;
            const uint32_t r0 = br;
            wave_min3(bx, bu, br);
            if (br == UINT_MAX && bu == INT_MAX) break;
            // the winning lane's w(s,x) + w(x,u)
            const bool mine = x0 == bx && u0 == bu && r0 == br;
            const unsigned long long bal = __ballot(mine);
            bo = __shfl(bo, __ffsll((long long)bal) - 1);
            hu[nh] = bu;
            su[m + nh] = bu;
            sw[m + nh] = bo;
            sr[m + nh] = br;
        }
    }
    if (lane == 0) {
        PlanChoice o;
        o.m = m; o.nh = nh;
        o.pad[0] = o.pad[1] = 0;
        for (int k = 0; k < PC_CAND; k++) {
            const bool v = k < m + nh;
            o.u[k] = v ? su[k] : 0; o.w[k] = v ? sw[k] : 0; o.rec[k] = v ? sr[k] : 0u;
        }
        out[q] = o;
    }
}
}  // namespace

struct shd_route_plan {
    shd_route* c = nullptr;
    int world = 1, rank = 0, ns_all = 0;
    int seeded = 0, nroots = 0, nhelpers = 0, nslots = 0;
    int delta = 1;                 // bucket width of the rows (<= the context's kd_delta)
    int nland = 0;                 // landmark seed rows after the kept rows' slots (flags preset)
    std::vector<int32_t> row_pos;  // caller-list position of each output row of this rank
    std::vector<int> lvl_off;      // jobs of launch k: [lvl_off[k], lvl_off[k + 1])
    KDJob* d_jobs = nullptr;
    int* d_next = nullptr;         // the launch's job-queue counter + one ready flag per kept row
    int32_t* d_src = nullptr;      // unseeded plans: the source vertex of each row
    uint16_t* d_drow = nullptr;    // row store
    uint32_t* d_prow = nullptr;
    uint64_t store_bytes = 0;
    // Landmark-only plans built on the device (round 6: their landmark rows are part of every
    // launch): shd_route_rows_planned_async first recomputes the nhub landmark rows into the
    // plan's own store (one hub-row launch, jobs d_hjobs, ready flags d_hdone), then the queue
    // order and the job records from them (plan_lmall_* kernels over d_sq / d_lv / d_key /
    // d_slot), then the rows: every SSSP the table needs runs inside the launch sequence.
    bool lm_step = false;
    int nhub = 0, hub_grid = 0, klm = 0;
    bool hub1024 = false;
    // multi-GPU landmark-only plans: this rank's share of the landmark rows (slots
    // [lm_first, lm_first + lm_count), equal shares), the rest all-gathered from the other
    // ranks by the caller (shd_route_plan_refresh_async with SHD_ROUTE_REFRESH_MINE, then the
    // exchange into the store, then SHD_ROUTE_REFRESH_JOBS)
    int lm_first = 0, lm_count = 0;
    int lm2 = 0;                   // > 0: landmark rows in two levels (SHD_ROUTE_LM2, lm_refresh)
    bool order_fixed = false;      // the queue order (d_slot) is computed; refreshes keep it
    uint16_t* d_bias = nullptr;    // the landmarks' pick biases (lm_pick; null: nearest first)
    int spread = 1;                // seeds picked spread apart (lm_pick; SHD_ROUTE_LMSPREAD=0: nearest-biased)
    KDJob* d_hjobs2 = nullptr;     // (the second level's jobs, written on the device)
    bool store_external = false;   // d_drow / d_prow are the caller's (shd_route_plan_bind_store)
    KDJob* d_hjobs = nullptr;
    int* d_hdone = nullptr;
    int* d_sq = nullptr;
    int* d_lv = nullptr;
    int* d_slot = nullptr;
    unsigned long long* d_key = nullptr;
    ~shd_route_plan() {
        for (void* q : {(void*)d_jobs, (void*)d_next, (void*)d_src, (void*)d_hjobs, (void*)d_hjobs2, (void*)d_bias,
                        (void*)d_hdone, (void*)d_sq, (void*)d_lv, (void*)d_slot, (void*)d_key})
            if (q) (void)hipFree(q);
        if (!store_external)
            for (void* q : {(void*)d_drow, (void*)d_prow})
                if (q) (void)hipFree(q);
    }
};

namespace {

static_assert(KD_SEEDS == PLAN_SCHED_SEEDS, "plan_sched.hpp holds KD_SEEDS seeds per job");

// landmark-only plans: at most this many rows per workgroup slot, and their landmark count
constexpr double PLAN_LMALL_RPS = 1.5;
// (round 5, hub rows outside the step: C3 1 GPU 256 / 512 / 1024 / 2048 landmarks 2.49 / 2.30 /
//  2.18 / 2.07 ms of rows.  Round 6, the landmark rows inside every step: 512 / 768 / 1024 give
//  2.677 / 2.69 / 2.77 ms per step (rows 2.14 / 2.05 / 1.99 + landmark rows and job records
//  0.55 / 0.65 / 0.79), two runs each on one box)
constexpr int PLAN_LMALL_COUNT = 448;

std::mutex g_pool_mu, g_pool_use;
std::unique_ptr<HostPool> g_pool;

// host threads of a plan (the box's CPU quota is 16)
int plan_threads() {
    int nth = std::max(1, std::min(16, (int)std::thread::hardware_concurrency()));
    if (const char* e = getenv("SHD_ROUTE_PLAN_THREADS")) nth = std::max(1, std::min(64, atoi(e)));
    return nth;
}
// the process-wide planner workers (created once; none when one host thread is asked for)
HostPool* host_pool() {
    std::lock_guard<std::mutex> l(g_pool_mu);
    if (!g_pool && plan_threads() > 1) g_pool.reset(new HostPool(plan_threads() - 1));
    return g_pool.get();
}

// Every environment knob of the planner, read once at the top of shd_route_plan_create (per
// call: tests and A/B runs change the environment between two plans of one context) and
// nowhere else; SHD_ROUTE_PLAN_THREADS alone stays with plan_threads().
struct PlanOptions {
    // SHD_ROUTE_SEED=0: plain rows
    bool seed = true;
    // SHD_ROUTE_PLAN_DELTA: bucket width of the plan's rows: any width up to the context's is
    // exact (the light in-CSR holds every in-arc below the context's width).  Round 5 read its
    // builds as "split ranks prefer the 12th percentile (30 on C4)"; the direct A/B on one box
    // with this per-plan width says otherwise (C4 8-way emulated, shared context, two runs
    // each: 30 -> 8.95 / 8.97 ms max, 38 -> 8.73 / 8.72 ms), so every plan keeps the
    // context's; the knob narrows it (tests, A/B runs)
    int delta = 1;
    // Landmark-only plans (round 5): when a rank has few rows per workgroup slot, seed chains
    // make its time a few serial row latencies (C3 8-way: 1.2 rows per slot, 3-4 levels, 28% of
    // linear); every row then seeds from its 3 nearest of PLAN_LMALL_COUNT landmark rows
    // instead (all at level 0: no waits, no chains).  Multi-GPU ranks with chains take 256
    // landmarks for their roots (C4 8-way 9.08 -> 8.77 ms with 3 landmark seeds each; 256 hub
    // rows cost the plan what 16 do: one unseeded row per CU, in parallel).
    // SHD_ROUTE_LMALL: rows per slot at most; SHD_ROUTE_LMALL_SMALL (256-thread contexts,
    // n <= 16384: PLAN_LMALL_COUNT landmarks are >= 3% of the vertices, and the 3 nearest bound
    // a row better than its neighbour rows: C3 1 GPU 2.51 -> 2.30 ms with 512, 8-way 1.12 ->
    // 0.65 ms)
    bool lm_all = false;
    // SHD_ROUTE_LANDMARKS: landmark rows: 16 for 1024-thread plans, 64 for 256-thread ones
    // (computed in the same device launch as the closeness rows, ensure_hub_rows),
    // PLAN_LMALL_COUNT for landmark-only plans, 256 for the other multi-GPU ranks
    int nland = 0;
    // SHD_ROUTE_GPUCHOICE=0: the partition forest, the seed choices and the roots' landmark
    // seeds by the host scans instead of the device kernels
    bool gpu_choice = true;
    // SHD_ROUTE_LMALL_REV=0: a landmark-only plan's rows in rank order (default: the peripheral
    // rows, the costliest to bound from landmarks, go first, so the launch ends on cheap
    // central ones: C3 2.18 -> 2.12 ms, 8-way 0.63 -> 0.61 ms)
    bool lmall_rev = true;
    // SHD_ROUTE_PLANDEV=0: a landmark-only plan's jobs on the host (build_device_lm_plan)
    bool plan_dev = true;
    // SHD_ROUTE_LMSEEDS: landmark seeds of a root row: three (C4 8-way roots 9.08 -> 8.83 ms
    // with 64 landmarks; landmark-only C3 plans 0.79 -> 0.70 ms at 8-way)
    int klm = KD_SEEDS;
    // device-built landmark-only plans: SHD_ROUTE_LM2=k the landmark rows in two levels (the
    // first k >= 16 unseeded), SHD_ROUTE_LMBIAS=0 no pick bias, SHD_ROUTE_LMSPREAD=0
    // nearest-biased seeds instead of spread ones (lm_pick), SHD_ROUTE_LMORDER=0 the queue
    // order recomputed in every refresh
    int lm2 = 0;
    bool lm_bias = true, lm_spread = true, lm_order_fixed = true;
    // SHD_ROUTE_SEEDALPHA: seed score w(s,u) + alpha * closeness(u)
    double alpha = 1.0;
    // SHD_ROUTE_TOPCAP: the forest's top rows are those whose subtree holds more than
    // 1 / top_cap of a rank's share
    int top_cap = 4;
    // SHD_ROUTE_SEEDS: seeds per row (1..KD_SEEDS): three, C4 48.6 -> 48.1 ms; on 256-thread
    // rows, whose init pass costs relatively more, two measured better in round 2 (C3 3.00 vs
    // 3.07 ms) and three since the streamed init of round 3 (round 4: C3 2.74 -> 2.67 ms).
    // Multi-GPU ranks: two; a rank's third candidates are mostly two-hop rows, and the extra
    // init pass costs more than they save: 8-way C4 rank 9.6 vs 9.4 ms with three
    int kseeds = KD_SEEDS;
    // SHD_ROUTE_SEED_ROOTS: the `roots` most central rows start unseeded (default, -1: one per
    // workgroup slot, so the launch starts full and the seed chains below them are short: C4
    // 1 GPU 52.9 -> 51.0 ms, an 8-way rank 12.8 -> 10.0 ms, C3 4.0 -> 3.4 ms; every row of a
    // landmark-only plan)
    int seed_roots = -1;
    // SHD_ROUTE_SEED_DEPTH: seed chains are at most `depth` rows long (default, 0: about half
    // the rows each workgroup slot runs in turn, so that seed chains are shorter than a slot's
    // queue, and at least 8 (C4: 195 rows per slot, no cap in effect; C3: 9 per slot, cap 8:
    // 3.5 -> 3.1 ms against cap 4))
    int seed_depth = 0;
    // SHD_ROUTE_SEED2HOP=0: no two-hop seeds; SHD_ROUTE_HOPDEG: largest degree of a two-hop
    // row's middle vertex x
    bool two_hop = true;
    int hop_deg = 256;
    // SHD_ROUTE_PIPE=0 (A/B): choices first, then the sequential pass
    bool pipe = true;
    // SHD_ROUTE_STORE_SYNC=1: the row store's allocation after the schedule, on the planning
    // thread -- an A/B of the schedule's time with and without the allocating thread beside it
    bool store_sync = false;
    // SHD_ROUTE_ROOTCOST / SHD_ROUTE_LMCOST / SHD_ROUTE_FLAGAT: the list schedule's estimates
    SchedCosts cost;
    // SHD_ROUTE_SCHED=0 (A/B): plain rank order
    bool sched = true;
    // SHD_ROUTE_PLAN_DEBUG: stage times and plan shape on stderr (tools/plan_debug.py)
    bool debug = false;

    int roots(const shd_route* c, int nj) const {
        return seed_roots >= 0 ? seed_roots : lm_all && nland > 0 ? nj : c->kd.slots;
    }
    int depth(const shd_route* c, int nj) const {
        return seed_depth > 0 ? seed_depth : std::max(8, nj / std::max(1, 2 * c->kd.slots));
    }
};

PlanOptions plan_options(const shd_route* c, int ns, int world) {
    PlanOptions o;
    const int n = c->n;
    auto off = [](const char* k) { const char* e = getenv(k); return e && atoi(e) == 0; };
    o.seed = !off("SHD_ROUTE_SEED");
    o.delta = c->kd.delta;
    if (const char* e = getenv("SHD_ROUTE_PLAN_DELTA")) o.delta = std::max(1, std::min(c->kd.delta, atoi(e)));
    double lmall_rps = PLAN_LMALL_RPS;
    if (const char* e = getenv("SHD_ROUTE_LMALL")) lmall_rps = atof(e);
    int lmall_small = 1;
    if (const char* e = getenv("SHD_ROUTE_LMALL_SMALL")) lmall_small = atoi(e);
    // (the multigraph terms below, like the duplicate-head notes at plan_choice_kernel and at the
    // host's candidate order, never decide anything: a seeded plan needs KD (shd_route_plan_create:
    // sel == 4), and select_inrows gives a multigraph no integer kernel, so its plans are plain
    // rows before any of these options is read -- tests/test_multi_gpu.py test_plans_fall_back)
    o.lm_all = !c->multigraph && c->kd.slots > 0 &&
               ((lmall_small && c->kd.block < 1024 && n >= 2048) ||
                (double)ns / world <= lmall_rps * (double)c->kd.slots);
    o.nland = c->multigraph ? 0 : std::min(c->kd.block >= 1024 ? 16 : 64, n);
    if (o.lm_all) o.nland = std::min(n, PLAN_LMALL_COUNT);
    else if (world > 1 && !c->multigraph) o.nland = std::min(n, 256);
    if (const char* e = getenv("SHD_ROUTE_LANDMARKS")) o.nland = c->multigraph ? 0 : std::max(0, std::min(atoi(e), n));
    o.gpu_choice = !off("SHD_ROUTE_GPUCHOICE");
    o.lmall_rev = !off("SHD_ROUTE_LMALL_REV");
    o.plan_dev = !off("SHD_ROUTE_PLANDEV");
    if (const char* e = getenv("SHD_ROUTE_LMSEEDS")) o.klm = std::max(1, std::min(KD_SEEDS, atoi(e)));
    if (const char* e = getenv("SHD_ROUTE_LM2")) o.lm2 = atoi(e);
    o.lm_bias = !off("SHD_ROUTE_LMBIAS");
    o.lm_spread = !off("SHD_ROUTE_LMSPREAD");
    o.lm_order_fixed = !off("SHD_ROUTE_LMORDER");
    if (const char* e = getenv("SHD_ROUTE_SEEDALPHA")) o.alpha = atof(e);
    if (const char* e = getenv("SHD_ROUTE_TOPCAP")) o.top_cap = std::max(1, atoi(e));
    o.kseeds = std::min(KD_SEEDS, world == 1 ? 3 : 2);
    if (const char* e = getenv("SHD_ROUTE_SEEDS")) o.kseeds = std::max(1, std::min(KD_SEEDS, atoi(e)));
    if (const char* e = getenv("SHD_ROUTE_SEED_ROOTS")) o.seed_roots = std::max(0, atoi(e));
    if (const char* e = getenv("SHD_ROUTE_SEED_DEPTH")) o.seed_depth = std::max(1, atoi(e));
    if (const char* e = getenv("SHD_ROUTE_SEED2HOP")) o.two_hop = atoi(e) != 0;
    if (const char* e = getenv("SHD_ROUTE_HOPDEG")) o.hop_deg = std::max(1, atoi(e));
    o.pipe = !off("SHD_ROUTE_PIPE");
    if (const char* e = getenv("SHD_ROUTE_STORE_SYNC")) o.store_sync = atoi(e) != 0;
    if (const char* e = getenv("SHD_ROUTE_LMCOST")) o.cost.lm = std::max(0.1, atof(e));
    if (const char* e = getenv("SHD_ROUTE_ROOTCOST")) o.cost.root = std::max(0.1, atof(e));
    if (const char* e = getenv("SHD_ROUTE_FLAGAT")) o.cost.flag_at = std::max(0.0, std::min(1.0, atof(e)));
    o.sched = !off("SHD_ROUTE_SCHED");
    o.debug = getenv("SHD_ROUTE_PLAN_DEBUG") != nullptr;
    return o;
}

// SHD_ROUTE_PLAN_DEBUG stage times: seconds since the plan's start (or a duration), by name
struct StageTimes {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    struct Mark { const char* name; double t; } v[16];
    int n = 0;
    double since() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
    void mark(const char* name) { mark(name, since()); }
    void mark(const char* name, double t) { if (n < 16) v[n++] = Mark{name, t}; }
    double ms(const char* name) const {  // (0 for a stage the plan did not run)
        for (int k = 0; k < n; k++) if (!strcmp(v[k].name, name)) return 1e3 * v[k].t;
        return 0;
    }
};

// the hub-row launch's grid for k rows: up to 256 in 1024-thread workgroups (one per CU) where
// the context's are smaller, more in the context's own
inline bool hub_big(const shd_route* c, int k) { return c->kd.hub_block > 0 && k <= 256; }
inline int hub_grid(const shd_route* c, int k) { return std::min(k, hub_big(c, k) ? 256 : std::max(256, c->kd.slots)); }

// the job records of a hub-row launch: no output row (row -1), row q kept in store slot q
std::vector<KDJob> hub_jobs(const std::vector<int>& verts) {
    std::vector<KDJob> jobs(verts.size());
    for (size_t q = 0; q < verts.size(); q++) {
        std::memset(&jobs[q], 0, sizeof(KDJob));
        jobs[q].row = -1; jobs[q].s = verts[q]; jobs[q].store = (int)q; jobs[q].nseed = 0;
    }
    return jobs;
}

// the hub-row launches' per-workgroup scratch, grown to `bytes` (kept: a free costs a sync)
int ensure_hub_ws(shd_route* c, size_t bytes) {
    if (c->hub_ws_bytes >= bytes) return SHD_ROUTE_OK;
    if (c->d_hub_ws) (void)hipFree(c->d_hub_ws);
    c->d_hub_ws = nullptr; c->hub_ws_bytes = 0;
    if (hipMalloc((void**)&c->d_hub_ws, bytes) != hipSuccess) { c->d_hub_ws = nullptr; return SHD_ROUTE_ENOMEM; }
    c->hub_ws_bytes = bytes;
    return SHD_ROUTE_OK;
}

// Exact rows of `verts` on the device for the planner: one unplanned KD launch whose jobs
// write no output row (row -1) but keep their row in store slot k, the format seeded rows
// read (u16 distances, 0xFFFF = unreached, and the engine tie-rule parent record
// `parent | ridx << 16 | w << 24` of every vertex).  The store stays in dd / dp (device) and
// is copied back into d_out / p_out.  Blocks: the planner runs once per context, before any
// planned launch.
int device_store_rows(shd_route* c, const std::vector<int>& verts, DevBuf& dd, DevBuf& dp, std::vector<uint16_t>& hd,
                      int ncopy, bool debug) {
    const int k = (int)verts.size(), n = c->n;
    if (k == 0) return SHD_ROUTE_OK;
    StageTimes T;
    const long long rs = kd_row_stride(n);
    const std::vector<KDJob> jobs = hub_jobs(verts);
    // one round of workgroups for all k rows (each row is unseeded: k rows on fewer
    // workgroups take k / grid row latencies): up to 256 rows in 1024-thread workgroups, one
    // per CU, and more in the context's own (256-thread contexts: four per CU, each row only
    // ~25% slower: C3's 512 hub rows 1.0 ms in two rounds of 1024-thread rows).  The launch
    // has its own per-workgroup scratch: the context's is left to its rows launches, so none
    // of those can share it even if one is still in flight.
    const bool hub1024 = hub_big(c, k);
    const int grid = hub_grid(c, k);
    DevBuf dj, dn;
    if (dj.alloc(sizeof(KDJob) * k) || dd.alloc(sizeof(uint16_t) * (size_t)rs * k) ||
        dp.alloc(sizeof(uint32_t) * (size_t)rs * k) || dn.alloc(sizeof(int) * (1 + (size_t)k)))
        return SHD_ROUTE_ENOMEM;
    int rc = ensure_hub_ws(c, c->kd.stride * (size_t)grid);
    if (rc) return rc;
    // (errors of earlier launches are reported by their own sync, not by this plan)
    if (hipDeviceSynchronize() != hipSuccess) return SHD_ROUTE_EDEVICE;
    if ((rc = take_err(c))) return rc;
    T.mark("alloc");
    if (hipMemcpy(dj.p, jobs.data(), sizeof(KDJob) * k, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(dn.p, 0, sizeof(int) * (1 + (size_t)k)) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    DevDelta g = kd_args(c);
    g.jobs = (const KDJob*)dj.p;
    g.drow = (const uint16_t*)dd.p; g.drow_out = (uint16_t*)dd.p; g.prow = (uint32_t*)dp.p; g.rstride = rs;
    g.done = (int*)dn.p + 1;
    if ((rc = kd_launch(c, g, (int*)dn.p, nullptr, k, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, true,
                        c->d_hub_ws, grid, hub1024)))
        return rc;
    if (hipDeviceSynchronize() != hipSuccess) return SHD_ROUTE_EDEVICE;
    if ((rc = take_err(c))) return rc;
    T.mark("launch");
    // only the rows the host reads (the closeness rows' distances): the landmark rows stay on
    // the device, where the plan's landmark-seed kernel reads them (copying 512 rows of C3 to
    // pageable memory took 6 ms); ensure_lm_host copies them for the host fallback
    ncopy = std::min(ncopy, k);
    hd.resize((size_t)rs * ncopy);
    if (ncopy && hipMemcpy(hd.data(), dd.p, sizeof(uint16_t) * hd.size(), hipMemcpyDeviceToHost) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    T.mark("copy");
    if (debug)
        fprintf(stderr, "hub rows (%d): alloc+sync %.2f, launch done %.2f, copies done %.2f ms\n", k, T.ms("alloc"),
                T.ms("launch"), T.ms("copy"));
    return SHD_ROUTE_OK;
}

// The planner's device rows, once per context, in one launch: the rows of the k highest-degree
// vertices (the hubs of a BA-like topology; ties by id).  The first 16 give every vertex's
// closeness estimate (its mean distance to them); all k are the landmark rows that seed the
// plans' roots, kept on the device in the row-store format (a plan copies them device to
// device).  (Before round 3: 16 pseudo-random closeness rows, then the 16 (64) most central
// vertices' rows in a second launch.)
// the k highest-degree vertices (ties by id): the hub / landmark rows
std::vector<int> hub_vertices(const shd_route* c, int k) {
    const int n = c->n;
    std::vector<int> ord(n);
    std::iota(ord.begin(), ord.end(), 0);
    auto deg = [&](int v) { return c->h_row.empty() ? 0 : c->h_row[v + 1] - c->h_row[v]; };
    std::partial_sort(ord.begin(), ord.begin() + k, ord.end(), [&](int a, int b) {
        return deg(a) != deg(b) ? deg(a) > deg(b) : a < b;
    });
    return std::vector<int>(ord.begin(), ord.begin() + k);
}

int ensure_hub_rows(shd_route* c, int k, bool debug, bool host_close = true) {
    const int n = c->n;
    k = std::min(n, std::max(k, 16));
    const int L = std::min(n, 16);  // the closeness rows: the first 16 hub rows
    const long long rs = kd_row_stride(n);
    std::vector<uint16_t> hd;
    if ((int)c->lm_v.size() < k) {
        std::vector<int> lv = hub_vertices(c, k);
        DevBuf dd, dp;
        int rc = device_store_rows(c, lv, dd, dp, hd, host_close ? L : 0, debug);
        if (rc) return rc;
        // (no plan keeps a pointer to these rows -- a plan copies them into its own store --
        // so the previous ones are freed; hipFree waits for work still reading them)
        if (c->d_lm_drow) (void)hipFree(c->d_lm_drow);
        if (c->d_lm_prow) (void)hipFree(c->d_lm_prow);
        c->d_lm_drow = (uint16_t*)dd.p; dd.p = nullptr;
        c->d_lm_prow = (uint32_t*)dp.p; dp.p = nullptr;
        c->lm_v = lv;
        c->lm_hd.clear();  // (host copies on demand: ensure_lm_host)
        c->lm_hp.clear();
        c->lm_rs = rs;
        c->close.clear();
        if (!host_close) return SHD_ROUTE_OK;
    } else {
        if (!host_close || (int)c->close.size() == n) return SHD_ROUTE_OK;
        hd.resize((size_t)rs * L);  // (rows computed by a device-built plan: their closeness now)
        if (hipMemcpy(hd.data(), c->d_lm_drow, sizeof(uint16_t) * hd.size(), hipMemcpyDeviceToHost) != hipSuccess)
            return SHD_ROUTE_EDEVICE;
    }
    c->close.assign(n, 0.0);
    for (int v = 0; v < n; v++) {
        double sum = 0;
        for (int q = 0; q < L; q++) {
            const uint16_t x = hd[(size_t)q * rs + v];
            sum += x == 0xFFFFu ? INFINITY : (double)x;
        }
        c->close[v] = sum / L;
    }
    return SHD_ROUTE_OK;
}

// the landmark rows on the host (the plan's host fallback for landmark seeds)
int ensure_lm_host(shd_route* c) {
    const size_t cnt = (size_t)c->lm_rs * c->lm_v.size();
    if (c->lm_hd.size() == cnt && c->lm_hp.size() == cnt) return SHD_ROUTE_OK;
    c->lm_hd.resize(cnt);
    c->lm_hp.resize(cnt);
    if (hipMemcpy(c->lm_hd.data(), c->d_lm_drow, sizeof(uint16_t) * cnt, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(c->lm_hp.data(), c->d_lm_prow, sizeof(uint32_t) * cnt, hipMemcpyDeviceToHost) != hipSuccess) {
        c->lm_hd.clear(); c->lm_hp.clear();
        return SHD_ROUTE_EDEVICE;
    }
    return SHD_ROUTE_OK;
}

// A device-built landmark-only plan's in-launch work (shd_route_plan::lm_step), enqueued on
// st: the landmark rows into the plan's store, then the queue order and the job records
// from them.  No host synchronisation: errors surface at the next shd_route_sync.
int lm_refresh(shd_route* c, const shd_route_plan* P, uint32_t what, hipStream_t st) {
    const int n = c->n, nj = (int)P->row_pos.size();
    const long long rs = kd_row_stride(n);
    if (!what) what = SHD_ROUTE_REFRESH_ALL | SHD_ROUTE_REFRESH_JOBS;
    if ((what & SHD_ROUTE_REFRESH_ALL) && P->lm2 > 0) {
        // two levels: the first lm2 landmark rows unseeded in 1024-thread workgroups (one per
        // CU), then the others seeded from their three nearest of those (the main rows' seeding
        // rule, as the plan_lmall_jobs_kernel writes it), in the context's workgroups
        const int k0 = P->lm2, k1 = P->nhub - P->lm2;
        if (!c->d_hub_ws || c->hub_ws_bytes < c->kd.stride * (size_t)std::max(hub_grid(c, k0), hub_grid(c, k1)))
            return SHD_ROUTE_EINVAL;
        if (hipMemsetAsync(P->d_hdone, 0, sizeof(int) * (1 + (size_t)P->nhub), st) != hipSuccess) return SHD_ROUTE_EDEVICE;
        DevDelta g = kd_args(c);
        g.jobs = P->d_hjobs;
        g.drow = P->d_drow; g.drow_out = P->d_drow; g.prow = P->d_prow; g.rstride = rs;
        g.done = P->d_hdone + 1;
        int rc = kd_launch(c, g, P->d_hdone, nullptr, k0, nullptr, 0, 0, nullptr, nullptr, nullptr, st, true,
                           c->d_hub_ws, hub_grid(c, k0), hub_big(c, k0));
        if (rc) return rc;
        hipLaunchKernelGGL(plan_lmall_jobs_kernel, dim3(8 * (((k1 + 15) / 16 + 7) / 8)), dim3(1024), 0, st, P->d_drow,
                           P->d_prow, rs, P->d_lv, k0, P->d_lv + k0, (const int*)nullptr, k1, P->klm, n, P->d_hjobs2,
                           (int*)nullptr, k0);
        if (hipMemsetAsync(P->d_hdone, 0, sizeof(int), st) != hipSuccess) return SHD_ROUTE_EDEVICE;  // (queue only)
        g.jobs = P->d_hjobs2;
        rc = kd_launch(c, g, P->d_hdone, nullptr, k1, nullptr, 0, 0, nullptr, nullptr, nullptr, st, true,
                       c->d_hub_ws, std::min(k1, c->kd.slots), false);
        if (rc) return rc;
    } else if ((what & SHD_ROUTE_REFRESH_ALL) || (what & SHD_ROUTE_REFRESH_MINE)) {
        const bool all = (what & SHD_ROUTE_REFRESH_ALL) != 0;
        const int q0 = all ? 0 : P->lm_first, k = all ? P->nhub : P->lm_count;
        // (the hub-row launch's scratch: the context's, grown at plan creation to this grid)
        if (!c->d_hub_ws || c->hub_ws_bytes < c->kd.stride * (size_t)hub_grid(c, k)) return SHD_ROUTE_EINVAL;
        if (hipMemsetAsync(P->d_hdone, 0, sizeof(int) * (1 + (size_t)P->nhub), st) != hipSuccess) return SHD_ROUTE_EDEVICE;
        DevDelta g = kd_args(c);
        g.jobs = P->d_hjobs + q0;  // (a job's store slot is its global landmark index)
        g.drow = P->d_drow; g.drow_out = P->d_drow; g.prow = P->d_prow; g.rstride = rs;
        g.done = P->d_hdone + 1;
        const int rc = kd_launch(c, g, P->d_hdone, nullptr, k, nullptr, 0, 0, nullptr, nullptr, nullptr, st, true,
                                 c->d_hub_ws, hub_grid(c, k), hub_big(c, k));
        if (rc) return rc;
    }
    if (!(what & SHD_ROUTE_REFRESH_JOBS)) return SHD_ROUTE_OK;
    // the queue order (peripheral rows first, by the closeness the first 16 landmark rows
    // give) is the plan's schedule: fixed when the plan is made, like a neighbour-seeded
    // plan's list schedule (the rank sort took 0.13 ms of every C3 step); the job records --
    // each row's nearest landmarks, its offsets d(s, L) and L's record in s's tree -- are
    // derived from the landmark rows in every refresh
    if (!P->order_fixed) {
        if (hipMemsetAsync(P->d_next, 0, sizeof(int), st) != hipSuccess) return SHD_ROUTE_EDEVICE;  // (root count)
        const int nb = (nj + 255) / 256;
        hipLaunchKernelGGL(plan_lmall_keys_kernel, dim3(nb), dim3(256), 0, st, P->d_drow, rs, std::min(n, 16), P->d_sq,
                           nj, P->d_key);
        hipLaunchKernelGGL(plan_lmall_rank_kernel, dim3(nb), dim3(256), 8 * nj, st, P->d_key, nj, P->d_slot);
    }
    if (P->d_bias)
        hipLaunchKernelGGL(plan_lmall_bias_kernel, dim3((P->nhub + 255) / 256), dim3(256), 0, st, P->d_drow, rs,
                           std::min(P->nhub, 16), P->d_lv, P->nhub, P->d_bias);
    hipLaunchKernelGGL(plan_lmall_jobs_kernel, dim3(8 * (((nj + 15) / 16 + 7) / 8)), dim3(1024), 0, st, P->d_drow,
                       P->d_prow, rs, P->d_lv, P->nhub, P->d_sq, P->d_slot, nj, P->klm, n, P->d_jobs,
                       P->order_fixed ? (int*)nullptr : P->d_next, -1, (const uint16_t*)P->d_bias, P->spread);
    return hip_check(hipGetLastError());
}

// -----------------------------------------------------------------------------
// The stages of a plan, in the order shd_route_plan_create runs them
// -----------------------------------------------------------------------------
// what the stages share: the request, the plan being filled and the per-job state
struct PlanBuild {
    shd_route* c;
    const int32_t* src;
    int ns, world, rank;
    const PlanOptions& o;
    shd_route_plan* P;
    StageTimes T;
    bool want = false;             // seeding is possible and asked for
    std::vector<int> rk;           // closeness rank of every vertex: a row may only be seeded by rows of smaller rank
    std::vector<int> job_pos, job_row;  // each job's position in the caller's list, its output row (-1: a helper)
    std::vector<int> first;        // first job of each source vertex
    // per job, in rank order (assign_seeds): level in the seed DAG, the row-store slot it is
    // kept in (-1: not kept), its seeds -- their jobs, or their landmark index (lmseed >= 0) --
    // and its record (store and landmark slots final only in queue_jobs)
    std::vector<int> lvl, slot, nsd;
    std::vector<SeedIdx> seedjob, lmseed;
    std::unique_ptr<KDJob[]> byjob;
    int nlev = 1;
    int n_recomp = 0, n_direct[KD_SEEDS + 1] = {0}, n_twohop = 0;  // SHD_ROUTE_PLAN_DEBUG: seed kinds
};

// A landmark-only plan built on the device (round 5): the hub rows without their host
// closeness, then one kernel for the queue order and one for the job records, and one
// sync at the end.  C3: plan 2.6 -> ~1.3 ms.  The host stages stay for SHD_ROUTE_GPUCHOICE=0 /
// SHD_ROUTE_LMALL_REV=0 / SHD_ROUTE_PLANDEV=0 and larger ranks.
// Round 6: the landmark rows are computed inside every launch sequence of the plan
// (lm_refresh), into the plan's own store; creating the plan runs that sequence once
// (for the root count and to surface errors now), the rows launch reads its results.
int build_device_lm_plan(PlanBuild& B) {
    shd_route* c = B.c;
    shd_route_plan* P = B.P;
    const PlanOptions& o = B.o;
    const int n = c->n, world = B.world, rank = B.rank;
    const int nh = std::min(n, std::max(o.nland, 16));
    const std::vector<int> lv = hub_vertices(c, nh);
    B.T.mark("close");
    std::vector<int> sq;
    sq.reserve((B.ns - rank + world - 1) / world);
    for (int p = rank; p < B.ns; p += world) { P->row_pos.push_back(p); sq.push_back(B.src[p]); }
    const int nj = (int)sq.size();
    P->klm = o.klm;
    const long long rs = kd_row_stride(n);
    P->nhub = nh;
    P->hub1024 = hub_big(c, nh);
    P->hub_grid = hub_grid(c, nh);
    // a rank's share of the landmark rows (equal shares; the last rank's is the rest)
    P->lm_count = (nh + world - 1) / world;
    P->lm_first = std::min(nh, rank * P->lm_count);
    P->lm_count = std::max(0, std::min(nh, P->lm_first + P->lm_count) - P->lm_first);
    const std::vector<KDJob> hj = hub_jobs(lv);
    if (o.lm2 >= 16 && o.lm2 < nh) P->lm2 = o.lm2;
    if (!o.lm_spread) P->spread = 0;
    if ((o.lm_bias && hipMalloc((void**)&P->d_bias, sizeof(uint16_t) * (size_t)nh) != hipSuccess) ||
        (P->lm2 && hipMalloc((void**)&P->d_hjobs2, sizeof(KDJob) * (size_t)(nh - P->lm2)) != hipSuccess) ||
        hipMalloc((void**)&P->d_sq, sizeof(int) * nj) != hipSuccess ||
        hipMalloc((void**)&P->d_lv, sizeof(int) * nh) != hipSuccess ||
        hipMalloc((void**)&P->d_slot, sizeof(int) * nj) != hipSuccess ||
        hipMalloc((void**)&P->d_key, sizeof(unsigned long long) * nj) != hipSuccess ||
        hipMalloc((void**)&P->d_hjobs, sizeof(KDJob) * nh) != hipSuccess ||
        hipMalloc((void**)&P->d_hdone, sizeof(int) * (1 + (size_t)nh)) != hipSuccess ||
        hipMalloc((void**)&P->d_drow, sizeof(uint16_t) * (size_t)rs * nh) != hipSuccess ||
        hipMalloc((void**)&P->d_prow, sizeof(uint32_t) * (size_t)rs * nh) != hipSuccess ||
        hipMalloc((void**)&P->d_jobs, sizeof(KDJob) * (size_t)nj) != hipSuccess ||
        hipMalloc((void**)&P->d_next, sizeof(int) * (1 + (size_t)nh)) != hipSuccess)
        return SHD_ROUTE_ENOMEM;
    int rc = ensure_hub_ws(c, c->kd.stride * (size_t)std::max(std::max(P->hub_grid, hub_grid(c, std::max(1, P->lm_count))),
                                                              P->lm2 ? std::max(hub_grid(c, P->lm2), std::min(nh - P->lm2, c->kd.slots)) : 0));
    if (rc) return rc;
    if (hipMemcpy(P->d_sq, sq.data(), sizeof(int) * nj, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(P->d_lv, lv.data(), sizeof(int) * nh, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(P->d_hjobs, hj.data(), sizeof(KDJob) * nh, hipMemcpyHostToDevice) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    if ((rc = hip_check(hipFuncSetAttribute((const void*)plan_lmall_rank_kernel,
                                            hipFuncAttributeMaxDynamicSharedMemorySize, 8 * nj))))
        return rc;
    P->row_pos.shrink_to_fit();
    // (errors of earlier launches are reported by their own sync, not by this plan)
    if (hipDeviceSynchronize() != hipSuccess) return SHD_ROUTE_EDEVICE;
    if ((rc = take_err(c))) return rc;
    if ((rc = lm_refresh(c, P, 0, nullptr))) return rc;
    int nroots = 0;
    if (hipMemcpy(&nroots, P->d_next, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return SHD_ROUTE_EDEVICE;
    if ((rc = take_err(c))) return rc;
    P->lm_step = true;
    P->order_fixed = o.lm_order_fixed;
    P->nslots = 0; P->nland = nh; P->store_bytes = (uint64_t)nh * (uint64_t)rs * 6u; P->nroots = nroots;
    P->seeded = 1;
    P->lvl_off = {0, nj};
    if (o.debug)
        fprintf(stderr, "plan world %d rank %d: jobs %d levels 1, device-built landmark-only plan (%d landmarks, "
                "%d unseeded), landmark rows in every launch: setup %.2f ms, plan total %.2f ms\n", world, rank, nj, nh, nroots,
                B.T.ms("close"), 1e3 * B.T.since());
    return SHD_ROUTE_OK;
}

// rank by (closeness, vertex).  closeness is a mean of L integer distances, so L times
// it is an exact integer sum: a counting sort over the sums, vertices ascending within
// one (an std::sort of (double, int) pairs took ~3 ms at C4)
std::vector<int> closeness_ranks(const shd_route* c) {
    const int n = c->n;
    std::vector<int> rk(n);
    const double L = (double)std::min(n, 16);
    bool integral = true;
    long long smax = 0;
    for (int v = 0; v < n && integral; v++) {
        const double x = c->close[v] * L;
        integral = x >= 0 && x < 1e8 && x == std::floor(x);
        if (integral) smax = std::max(smax, (long long)x);
    }
    if (integral) {
        std::vector<int> cnt((size_t)smax + 2, 0);
        for (int v = 0; v < n; v++) cnt[(size_t)(c->close[v] * L) + 1]++;
        for (long long x = 0; x <= smax; x++) cnt[x + 1] += cnt[x];
        for (int v = 0; v < n; v++) rk[v] = cnt[(size_t)(c->close[v] * L)]++;
    } else {
        std::vector<std::pair<double, int>> ord(n);
        for (int v = 0; v < n; v++) ord[v] = {c->close[v], v};
        std::sort(ord.begin(), ord.end());
        for (int q = 0; q < n; q++) rk[ord[q].second] = q;
    }
    return rk;
}

// positions by (vertex rank, position): counting sort
void positions_by_rank(const PlanBuild& B, std::vector<int>& v) {
    const int n = B.c->n;
    std::vector<int> cnt(n + 1, 0), tmp(v.size());
    std::vector<int> sv(v);
    if (!std::is_sorted(sv.begin(), sv.end())) std::sort(sv.begin(), sv.end());
    for (int p : sv) cnt[B.rk[B.src[p]] + 1]++;
    for (int x = 0; x < n; x++) cnt[x + 1] += cnt[x];
    for (int p : sv) tmp[cnt[B.rk[B.src[p]]]++] = p;
    v.swap(tmp);
}

// the best seeds of source s among the vertices avail(u) says have a usable row: neighbours
// of smaller rank by w(s,u) + closeness(u), then vertex.  One pass keeping the k best in
// order (what a full sort of the candidates would list first; a multigraph's repeated u
// keeps its best arc, the first arc on a full tie): hubs have thousands of neighbours, k is
// at most 3.
template <typename Avail>
inline int best_seeds(const shd_route* c, const int* rk, int s, double alpha, Avail avail, int k, int* arc_out) {
    double sc[KD_SEEDS];
    int m = 0;
    for (int a = c->h_row[s]; a < c->h_row[s + 1]; a++) {
        const int u = c->h_col[a];
        if (u == s || !avail(u) || rk[u] >= rk[s]) continue;
        const double x = c->h_w[a] + alpha * c->close[u];
        int dq = -1;
        for (int q = 0; q < m; q++) if (c->h_col[arc_out[q]] == u) dq = q;
        if (dq >= 0) {
            if (!(x < sc[dq])) continue;
            for (int q = dq; q + 1 < m; q++) { sc[q] = sc[q + 1]; arc_out[q] = arc_out[q + 1]; }
            m--;
        }
        auto before = [&](int q) { return x != sc[q] ? x < sc[q] : u < c->h_col[arc_out[q]]; };
        if (m == k && !before(m - 1)) continue;
        int q = m < k ? m++ : k - 1;
        for (; q > 0 && before(q - 1); q--) { sc[q] = sc[q - 1]; arc_out[q] = arc_out[q - 1]; }
        sc[q] = x;
        arc_out[q] = a;
    }
    return m;
}

// A row's seeds: its best kseeds available neighbour rows, then (if short) its best
// two-hop rows (s -> x -> u, x of degree <= 256), each list in the order a full sort
// of the candidates would give.  avail(u): u's row is a usable seed.
// A row with fewer such neighbours (a multi-GPU rank holds only its own rows) takes
// two-hop seeds s -> x -> u (u one of this rank's rows, x any neighbour of degree
// <= 256): D0 = w(s,x) + w(x,u) + d_u(.) is as consistent as a neighbour's, and u's
// own record is the arc (x,u), tight whenever u keeps D0.
// (the chosen arcs' head, weight and record are kept in the choice: the sequential
// pass then reads no CSR array, whose random reads cost ~5 ms at C4)
struct Hop { double cost; int u, off; uint32_t rec; };
struct Choice { int m, nh; int arcs[KD_SEEDS]; int u[KD_SEEDS], w[KD_SEEDS]; uint32_t rec[KD_SEEDS]; Hop hop[KD_SEEDS]; };

template <typename Avail>
inline void choose_seeds(const shd_route* c, const int* rk, int s, const PlanOptions& o, Avail avail, Choice& C) {
    const int kseeds = o.kseeds, hop_deg = o.hop_deg;
    C.m = best_seeds(c, rk, s, o.alpha, avail, kseeds, C.arcs);
    for (int k = 0; k < C.m; k++) {
        const int a = C.arcs[k];
        C.u[k] = c->h_col[a];
        C.w[k] = (int)c->h_w[a];
        C.rec[k] = (uint32_t)s | ((uint32_t)c->h_ridx[a] << 16) | ((uint32_t)c->h_w[a] << 24);
    }
    C.nh = 0;
    if (!o.two_hop || C.m >= kseeds) return;
    const int need = kseeds - C.m;
    auto before = [](const Hop& x, const Hop& y) {
        return x.cost != y.cost ? x.cost < y.cost : x.u != y.u ? x.u < y.u : x.rec < y.rec;
    };
    for (int a = c->h_row[s]; a < c->h_row[s + 1]; a++) {
        const int x = c->h_col[a];
        if (x == s || c->h_row[x + 1] - c->h_row[x] > hop_deg) continue;
        for (int b = c->h_row[x]; b < c->h_row[x + 1]; b++) {
            const int u = c->h_col[b];
            if (u == s || u == x || rk[u] >= rk[s] || !avail(u)) continue;
            bool dup = false;
            for (int k = 0; k < C.m; k++) dup = dup || C.u[k] == u;
            if (dup) continue;
            const Hop h{c->h_w[a] + c->h_w[b] + c->close[u], u, (int)(c->h_w[a] + c->h_w[b]),
                        (uint32_t)x | ((uint32_t)c->h_ridx[b] << 16) | ((uint32_t)c->h_w[b] << 24)};
            int dq = -1;
            for (int q = 0; q < C.nh; q++) if (C.hop[q].u == u) dq = q;
            if (dq >= 0) {
                if (!before(h, C.hop[dq])) continue;
                for (int q = dq; q + 1 < C.nh; q++) C.hop[q] = C.hop[q + 1];
                C.nh--;
            }
            if (C.nh == need && !before(h, C.hop[C.nh - 1])) continue;
            int q = C.nh < need ? C.nh++ : need - 1;
            for (; q > 0 && before(h, C.hop[q - 1]); q--) C.hop[q] = C.hop[q - 1];
            C.hop[q] = h;
        }
    }
}

// The seed choices of the rows sq[0, nq) on the device, one wave per row (plan_choice_kernel:
// the host rule of choose_seeds, against the vertices with first[v] >= 0): closeness, rank
// and availability up, the candidate lists back.  false: take the host scan instead.
bool device_seed_choices(const PlanBuild& B, const std::vector<int>& first, const int* sq, int nq, int k, int two_hop,
                         int hop_deg, int cand, std::vector<PlanChoice>& out) {
    const shd_route* c = B.c;
    const int n = c->n;
    std::vector<uint8_t> av(n);
    for (int v = 0; v < n; v++) av[v] = first[v] >= 0;
    DevBuf dcl, drk, dav, dsq, dout;
    if (dcl.alloc(sizeof(double) * n) || drk.alloc(sizeof(int) * n) || dav.alloc(n) ||
        dsq.alloc(sizeof(int) * nq) || dout.alloc(sizeof(PlanChoice) * nq))
        return false;
    if (hipMemcpy(dcl.p, c->close.data(), sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(drk.p, B.rk.data(), sizeof(int) * n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dav.p, av.data(), n, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dsq.p, sq, sizeof(int) * nq, hipMemcpyHostToDevice) != hipSuccess)
        return false;
    hipLaunchKernelGGL(plan_choice_kernel, dim3((nq + 3) / 4), dim3(256), 0, 0, c->d_row, c->kd.d_orec,
                       (const double*)dcl.p, (const int*)drk.p, (const uint8_t*)dav.p, (const int*)dsq.p, nq,
                       k, two_hop, hop_deg, B.o.alpha, cand, (PlanChoice*)dout.p);
    out.resize(nq);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpy(out.data(), dout.p, sizeof(PlanChoice) * nq, hipMemcpyDeviceToHost) != hipSuccess) {
        out.clear();
        return false;
    }
    return true;
}

// Multi-GPU: partition the seed forest (each row's best seed) so that a rank holds
// whole subtrees: every seed a row needs is then on its own rank.  The forest's
// top levels (T) are computed on every rank (helper rows where not output there);
// the subtrees hanging below T go to ranks by size (largest first, least loaded).
void partition_forest(PlanBuild& B) {
    const shd_route* c = B.c;
    const int32_t* src = B.src;
    const int n = c->n, ns = B.ns, world = B.world, rank = B.rank;
    shd_route_plan* P = B.P;
    std::vector<int> first(n, -1), pos(ns);
    for (int p = 0; p < ns; p++) if (first[src[p]] < 0) first[src[p]] = p;
    std::iota(pos.begin(), pos.end(), 0);
    positions_by_rank(B, pos);
    std::vector<int> fpar(ns, -1), flvl(ns, 0), sub(ns, 1);
    // each row's best seed (the forest's parent): on the device, one wave per row (the
    // plan's seed-choice kernel with k = 1: ~1 ms with the copies at C4, against ~6 ms
    // of host CSR scans on every rank); SHD_ROUTE_GPUCHOICE=0 keeps the host scan
    std::vector<int> bu(ns, -1);
    std::vector<PlanChoice> ho;
    if (B.o.gpu_choice && c->kd.d_orec != nullptr && device_seed_choices(B, first, src, ns, 1, 0, 0, 1, ho)) {
        for (int p = 0; p < ns; p++) bu[p] = ho[p].m > 0 ? ho[p].u[0] : -1;
    } else {
        for (int p = 0; p < ns; p++) {
            int a;
            bu[p] = best_seeds(c, B.rk.data(), src[p], B.o.alpha, [&](int u) { return first[u] >= 0; }, 1, &a) ? c->h_col[a] : -1;
        }
    }
    for (int p : pos)
        if (bu[p] >= 0) {
            fpar[p] = first[bu[p]];
            flvl[p] = flvl[fpar[p]] + 1;
        }
    for (int q = ns - 1; q >= 0; q--) if (fpar[pos[q]] >= 0) sub[fpar[pos[q]]] += sub[pos[q]];
    // T = the rows whose subtree holds more than a quarter of a rank's share (the
    // forest's skeleton near its roots); every other row hangs in a subtree of at most
    // that size whose head's parent is in T (or which is a whole small tree)
    const int cap = std::max(1, ns / (B.o.top_cap * world));
    std::vector<int> top, heads;
    for (int p : pos) {
        if (sub[p] > cap) top.push_back(p);
        else if (fpar[p] < 0 || sub[fpar[p]] > cap) heads.push_back(p);
    }
    std::stable_sort(heads.begin(), heads.end(), [&](int a, int b) { return sub[a] > sub[b]; });
    std::vector<int> owner(ns, -1);
    std::vector<long long> load(world, 0);
    auto least = [&]() { return (int)(std::min_element(load.begin(), load.end()) - load.begin()); };
    for (int h : heads) { const int r = least(); owner[h] = r; load[r] += sub[h]; }
    for (int p : top) { const int r = least(); owner[p] = r; load[r] += 1; }
    for (int p : pos) if (owner[p] < 0 && fpar[p] >= 0) owner[p] = owner[fpar[p]];  // (rank order: parent first)
    // rows of this rank: its share of T, then its subtrees, in rank order; helpers: T
    for (int p : pos)
        if (owner[p] == rank) { B.job_row.push_back((int)P->row_pos.size()); P->row_pos.push_back(p); B.job_pos.push_back(p); }
    for (int p : top)
        if (owner[p] != rank) { B.job_pos.push_back(p); B.job_row.push_back(-1); P->nhelpers++; }
}

// which positions this rank computes: output rows + helper rows
void partition_rows(PlanBuild& B) {
    const int ns = B.ns, world = B.world, rank = B.rank;
    shd_route_plan* P = B.P;
    if (B.want && world > 1 && B.o.lm_all) {
        // landmark-only plans seed from no other row: a rank takes every world-th position
        // (row costs vary with the vertex's place in the graph: a stride spreads them), no
        // helper rows
        for (int p = rank; p < ns; p += world) {
            B.job_row.push_back((int)P->row_pos.size()); P->row_pos.push_back(p); B.job_pos.push_back(p);
        }
    } else if (!B.want || world == 1) {
        // a contiguous block of the caller's list (world 1: all of it)
        const int blk = (ns + world - 1) / world, lo = std::min(ns, rank * blk), hi = std::min(ns, lo + blk);
        for (int p = lo; p < hi; p++) { P->row_pos.push_back(p); B.job_pos.push_back(p); B.job_row.push_back(p - lo); }
    } else {
        partition_forest(B);
    }
}

// jobs renumbered in rank order (a job's seeds, of smaller rank, are settled before
// it), so that the later passes walk every per-job array in sequence
void order_jobs(PlanBuild& B) {
    const int nj = (int)B.job_pos.size(), n = B.c->n;
    std::vector<int> jpos_of(B.ns, -1);
    for (int j = 0; j < nj; j++) jpos_of[B.job_pos[j]] = j;
    std::vector<int> order(B.job_pos);
    positions_by_rank(B, order);
    std::vector<int> jr(nj);
    for (int q = 0; q < nj; q++) jr[q] = B.job_row[jpos_of[order[q]]];
    B.job_pos.swap(order);
    B.job_row.swap(jr);
    // (landmark-only plans have no seed order to keep: the peripheral rows go first,
    // PlanOptions::lmall_rev)
    if (B.o.lm_all && B.o.lmall_rev) {
        std::reverse(B.job_pos.begin(), B.job_pos.end());
        std::reverse(B.job_row.begin(), B.job_row.end());
    }
    B.first.assign(n, -1);
    for (int j = 0; j < nj; j++) if (B.first[B.src[B.job_pos[j]]] < 0) B.first[B.src[B.job_pos[j]]] = j;
}

// the first nr0 rows' (the roots') landmark seeds on the device (a host loop over the landmark
// rows took ~2 us per root: strided distance reads and a parent walk per landmark seed);
// empty: take the host fallback
std::vector<LmChoice> device_landmark_choices(const PlanBuild& B, int nr0) {
    const shd_route* c = B.c;
    const int nland = B.o.nland;
    std::vector<LmChoice> lmc;
    std::vector<int> sq(nr0);
    for (int i = 0; i < nr0; i++) sq[i] = B.src[B.job_pos[i]];
    std::vector<int> lv(c->lm_v.begin(), c->lm_v.begin() + nland);
    DevBuf dsq, dlv, dout;
    bool ok = !dsq.alloc(sizeof(int) * nr0) && !dlv.alloc(sizeof(int) * nland) && !dout.alloc(sizeof(LmChoice) * nr0) &&
              hipMemcpy(dsq.p, sq.data(), sizeof(int) * nr0, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(dlv.p, lv.data(), sizeof(int) * nland, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(plan_landmark_kernel, dim3((nr0 + 3) / 4), dim3(256), 0, 0, c->d_lm_drow, c->d_lm_prow,
                           (long long)c->lm_rs, (const int*)dlv.p, nland, (const int*)dsq.p, nr0, B.o.klm, c->n,
                           (LmChoice*)dout.p);
        lmc.resize(nr0);
        ok = hipGetLastError() == hipSuccess &&
             hipMemcpy(lmc.data(), dout.p, sizeof(LmChoice) * nr0, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (!ok) lmc.clear();
    return lmc;
}

// a root's landmark seeds on the host (the fallback of device_landmark_choices): the nearest
// landmarks by d(s, L) (undirected: d_L(s)), up to klm; returns how many
int host_landmark_seeds(const shd_route* c, int s, int nland, int klm, int* su, int* wr, int* srec, int* lmseed) {
    std::vector<std::pair<double, int>> lc;
    for (int l = 0; l < nland; l++) {
        const uint16_t dls = c->lm_hd[(size_t)l * c->lm_rs + s];
        if (dls != 0xFFFFu) lc.push_back({(double)dls, l});
    }
    std::sort(lc.begin(), lc.end());
    int mk = 0;
    for (const auto& pr : lc) {
        if (mk == klm) break;
        const int l = pr.second, L = c->lm_v[l];
        uint32_t rec = KD_SRC_MARK;
        if (L != s) {
            // the last arc (x, L) of the shortest s -> L path in L's tree
            int x = s;
            const uint32_t* lp = c->lm_hp.data() + (size_t)l * c->lm_rs;
            while ((int)(lp[x] & 0xFFFFu) != L) x = (int)(lp[x] & 0xFFFFu);
            const uint32_t px = lp[x];  // L | ridx(x,L) << 16 | w << 24
            rec = (uint32_t)x | (px & 0xFFFF0000u);
        }
        su[mk] = L; wr[mk] = (int)pr.first; srec[mk] = (int)rec; lmseed[mk] = l;
        mk++;
    }
    return mk;
}

// A row's choice from the device's ordered candidate list o, given the rows usable now
// (fl[u] >= 0): the first kseeds usable entries are the host rule's choice over the usable
// rows, when the list held kseeds usable ones or every available neighbour (o.m < PC_CAND);
// a two-hop fill stands when every listed neighbour was usable (same exclusions, same
// count) and so are its picks.  false: not exact, the row is rescanned on the host.
inline bool choice_from_candidates(const PlanChoice& o, const std::vector<int>& fl, const PlanOptions& opt, Choice& ch) {
    const int kseeds = opt.kseeds;
    int got = 0;
    bool direct_all = true;
    for (int k = 0; k < o.m && got < kseeds; k++) {
        if (fl[o.u[k]] >= 0) { ch.u[got] = o.u[k]; ch.w[got] = o.w[k]; ch.rec[got] = o.rec[k]; got++; }
        else direct_all = false;
    }
    ch.m = got;
    bool exact = got == kseeds || o.m < PC_CAND;
    if (exact && got < kseeds && opt.two_hop) {
        bool hop_ok = o.m < kseeds && direct_all;
        for (int k = 0; k < o.nh && hop_ok; k++) hop_ok = fl[o.u[o.m + k]] >= 0;
        if (hop_ok) {
            ch.nh = o.nh;
            for (int k = 0; k < o.nh; k++) ch.hop[k] = Hop{0.0, o.u[o.m + k], o.w[o.m + k], o.rec[o.m + k]};
        } else exact = false;
    }
    return exact;
}

// Seeds of each job, in one sequential pass over the jobs in rank order: the kseeds
// neighbours u (jobs of this rank, smaller rank, level below the cap) with the smallest
// w(s,u) + closeness(u), i.e. the likely gateways of most shortest paths from s.
// The roots (the rows that would start unseeded) seed from landmark rows instead:
// D0 = d(s, L) + d_L(.) is consistent for any landmark L, and L's own record is the last arc
// (x, L) of a shortest s -> L path (tight whenever L keeps D0).  C3 roots are a ninth of the
// rows and cost ~3.4 seeded rows each unseeded.
// (C3, 1024 roots over 256-thread rows: 16/32/64/256 landmarks 2.90/2.89/2.80/2.76 ms;
// C4's 256 roots are 0.5% of its rows: 16 and 64 measure the same, and each landmark
// is a host Dijkstra of the plan (~40 ms at C4))
int assign_seeds(PlanBuild& B) {
    shd_route* c = B.c;
    shd_route_plan* P = B.P;
    const PlanOptions& o = B.o;
    const int32_t* src = B.src;
    const int n = c->n, nj = (int)B.job_pos.size(), nland = o.nland, kseeds = o.kseeds;
    const int nroot_min = o.roots(c, nj), depth = o.depth(c, nj);
    const int* rk = B.rk.data();
    const std::vector<int>&order = B.job_pos, &first = B.first;
    B.lvl.assign(nj, 0); B.slot.assign(nj, -1); B.nsd.assign(nj, 0);
    B.seedjob.resize(nj);
    B.lmseed.resize(nj);  // landmark index of seed k, or -1
    for (auto& a : B.lmseed) a.fill(-1);
    std::vector<int>&lvl = B.lvl, &slot = B.slot, &nsd = B.nsd;
    std::vector<int> fl(n, -1);  // first job of a vertex, once its level is below the cap
    // Choices precomputed on host threads against a superset of the usable rows (every
    // row of an earlier source: the sequential pass below only withholds rows past the
    // seed-chain depth cap); the sequential pass keeps a precomputed choice when every
    // row in it is usable -- then it is exactly the choice over the usable rows -- and
    // recomputes the row otherwise.
    // (not value-initialised: the worker threads first-touch their own pages)
    std::unique_ptr<Choice[]> pre(new Choice[order.size()]);
    // The worker threads take chunks of 256 choices in order and mark each one done; the
    // sequential pass below runs concurrently, consuming the chunks as they complete (and
    // taking a chunk itself while the one it needs is not done), so it hides behind the
    // choices instead of following them (C4: ~1.4 ms).
    const int nq = (int)order.size(), CH = 256;
    const int nchunk = nq > nroot_min ? (nq - nroot_min + CH - 1) / CH : 0;
    std::unique_ptr<std::atomic<int>[]> chunk_done(new std::atomic<int>[std::max(1, nchunk)]);
    for (int k = 0; k < nchunk; k++) chunk_done[k].store(0, std::memory_order_relaxed);
    std::atomic<int> nextq{nroot_min};
    auto take_chunk = [&]() {
        if (nextq.load(std::memory_order_relaxed) >= nq) return false;  // (no unbounded fetch_add)
        const int q0 = nextq.fetch_add(CH);
        if (q0 >= nq) return false;
        const int q1 = std::min(nq, q0 + CH);
        for (int qq = q0; qq < q1; qq++) {
            // the rows come in rank order, i.e. at random places of the CSR: prefetch the
            // row offsets 8 sources ahead and the arcs 4 ahead (choices ~30% faster)
            if (qq + 8 < q1) __builtin_prefetch(&c->h_row[src[order[qq + 8]]]);
            if (qq + 4 < q1) {
                const int s4 = src[order[qq + 4]], a0 = c->h_row[s4], a1 = c->h_row[s4 + 1];
                for (int a = a0; a < a1; a += 16) __builtin_prefetch(&c->h_col[a]);
                for (int a = a0; a < a1; a += 8) __builtin_prefetch(&c->h_w[a]);
            }
            choose_seeds(c, rk, src[order[qq]], o, [&](int u) { return first[u] >= 0; }, pre[qq]);
        }
        chunk_done[(q0 - nroot_min) / CH].store(1, std::memory_order_release);
        return true;
    };
    // the choices on the device by default (one wave per row, ~1 ms with the copies at C4;
    // on the host workers they took 3.7-8 ms depending on the box's host load: C4 plans
    // 8.5-8.9 against 13.2 ms on one box); SHD_ROUTE_GPUCHOICE=0 keeps them on the host
    const double th0 = B.T.since();
    bool dev_choice = nchunk > 0 && o.gpu_choice;
    std::vector<PlanChoice> dch;  // device candidate lists of the seedable rows, in queue order
    if (dev_choice) {
        std::vector<int> sq(nq - nroot_min);
        for (int i = 0; i < nq - nroot_min; i++) sq[i] = src[order[nroot_min + i]];
        dev_choice = device_seed_choices(B, first, sq.data(), nq - nroot_min, kseeds, o.two_hop ? 1 : 0, o.hop_deg, PC_CAND, dch);
        if (dev_choice) {
            nextq.store(nq);
            for (int k = 0; k < nchunk; k++) chunk_done[k].store(1, std::memory_order_relaxed);
        }
    }
    std::vector<LmChoice> lmc;
    if (nland > 0 && nroot_min > 0 && c->d_lm_drow && o.gpu_choice) lmc = device_landmark_choices(B, std::min(nroot_min, nq));
    HostPool* pool = dev_choice ? nullptr : host_pool();
    std::unique_lock<std::mutex> lease(g_pool_use, std::try_to_lock);
    std::unique_ptr<HostPool> own;  // the shared workers are busy with another plan
    if (pool && !lease.owns_lock()) {
        own.reset(new HostPool(plan_threads() - 1));
        pool = own.get();
    }
    struct PoolWait {
        HostPool* p;
        bool on;
        void operator()() { if (on) { p->wait(); on = false; } }
        ~PoolWait() { (*this)(); }
    } pool_wait{pool, pool && nchunk > 0};
    if (pool_wait.on) pool->run([&]() { while (take_chunk()) {} });
    if (!o.pipe) {  // A/B: choices first, then the pass
        while (take_chunk()) {}
        pool_wait();
    }
    int q = 0;
    B.byjob.reset(new KDJob[nj]);
    B.T.mark("loop0");
    for (int j = 0; j < nj; j++) {
        const int p = B.job_pos[j], s = src[p];
        const int qi = q;
        const bool seedable = q++ >= nroot_min;
        if (seedable && (qi - nroot_min) % CH == 0) {
            std::atomic<int>& dn = chunk_done[(qi - nroot_min) / CH];
            while (!dn.load(std::memory_order_acquire))
                if (!take_chunk()) std::this_thread::yield();
        }
        auto usable = [&](int u) { return fl[u] >= 0; };
        Choice ch;
        ch.m = ch.nh = 0;
        if (seedable && dev_choice) {
            if (!choice_from_candidates(dch[qi - nroot_min], fl, o, ch)) {
                ch.m = ch.nh = 0;
                choose_seeds(c, rk, s, o, usable, ch);
                B.n_recomp++;
            }
        } else if (seedable) {
            bool ok = true;
            const Choice& pc = pre[qi];
            for (int k = 0; k < pc.m; k++) ok = ok && fl[pc.u[k]] >= 0;
            for (int k = 0; k < pc.nh; k++) ok = ok && fl[pc.hop[k].u] >= 0;
            if (ok) ch = pc;
            else { choose_seeds(c, rk, s, o, usable, ch); B.n_recomp++; }
        }
        int m = ch.m;
        int su[KD_SEEDS] = {0}, wr[KD_SEEDS] = {0}, srec[KD_SEEDS] = {0};  // seed vertex, offset, record
        if (seedable) { B.n_direct[std::min(ch.m, KD_SEEDS)]++; if (ch.nh) B.n_twohop++; }
        if (!seedable && nland > 0 && qi < (int)lmc.size()) {
            const LmChoice& lo = lmc[qi];
            for (int k = 0; k < lo.m; k++) {
                su[k] = c->lm_v[lo.l[k]]; wr[k] = lo.d[k]; srec[k] = (int)lo.rec[k]; B.lmseed[j][k] = lo.l[k];
            }
            nsd[j] = lo.m;
        } else if (!seedable && nland > 0) {
            if (ensure_lm_host(c)) return SHD_ROUTE_EDEVICE;
            nsd[j] = host_landmark_seeds(c, s, nland, o.klm, su, wr, srec, B.lmseed[j].data());
        }
        for (int k = 0; k < m; k++) { su[k] = ch.u[k]; wr[k] = ch.w[k]; srec[k] = (int)ch.rec[k]; }
        for (int q2 = 0; q2 < ch.nh; q2++, m++) {
            su[m] = ch.hop[q2].u; wr[m] = ch.hop[q2].off; srec[m] = (int)ch.hop[q2].rec;
        }
        for (int k = 0; k < m; k++) {
            const int sj = first[su[k]];
            B.seedjob[j][k] = sj;
            lvl[j] = std::max(lvl[j], lvl[sj] + 1);
            if (slot[sj] < 0) slot[sj] = P->nslots++;
        }
        if (seedable || nland == 0) nsd[j] = m;
        if (!nsd[j]) P->nroots++;
        B.nlev = std::max(B.nlev, lvl[j] + 1);
        if (first[src[p]] == j && lvl[j] + 1 < depth) fl[src[p]] = p;
        // the job record, in job order (queue_jobs copies it into queue order: one cache
        // line per job instead of five scattered per-job arrays); its own store slot and
        // landmark slots (-1 - l: after every kept row's slot) are final only after this pass
        KDJob& J = B.byjob[j];
        std::memset(&J, 0, sizeof(J));
        J.row = B.job_row[j]; J.s = s; J.store = -1; J.nseed = nsd[j];
        for (int k = 0; k < nsd[j]; k++) {
            J.seed[k] = B.lmseed[j][k] >= 0 ? -1 - B.lmseed[j][k] : slot[B.seedjob[j][k]];
            J.u[k] = su[k]; J.wr[k] = wr[k]; J.rec[k] = srec[k];
        }
    }
    pool_wait();
    B.T.mark("hop", B.T.since() - th0);
    B.T.mark("seeds");
    return SHD_ROUTE_OK;
}

// The row store's allocation and the landmark rows' device copies (they run on a second host
// thread while the planning thread builds the schedule: C4 ~0.5 ms of hipMalloc and copies),
// then the job array and the launch's queue counter + ready flags.
void alloc_plan_store(shd_route* c, shd_route_plan* P, int nj, int ntot, bool* ok) {
    const long long rs = kd_row_stride(c->n);
    bool r = hipSetDevice(c->device) == hipSuccess &&
             hipMalloc((void**)&P->d_drow, sizeof(uint16_t) * (size_t)rs * ntot) == hipSuccess &&
             hipMalloc((void**)&P->d_prow, sizeof(uint32_t) * (size_t)rs * ntot) == hipSuccess;
    if (r && P->nland)
        // landmark rows into the slots after the kept rows' (the rows are in the store
        // format already, pads included)
        r = hipMemcpy(P->d_drow + (size_t)rs * P->nslots, c->d_lm_drow,
                      sizeof(uint16_t) * (size_t)rs * P->nland, hipMemcpyDeviceToDevice) == hipSuccess &&
            hipMemcpy(P->d_prow + (size_t)rs * P->nslots, c->d_lm_prow,
                      sizeof(uint32_t) * (size_t)rs * P->nland, hipMemcpyDeviceToDevice) == hipSuccess;
    r = r && hipMalloc((void**)&P->d_jobs, sizeof(KDJob) * (size_t)nj) == hipSuccess &&
        hipMalloc((void**)&P->d_next, sizeof(int) * (1 + (size_t)ntot)) == hipSuccess;
    *ok = r;
}

// The launch's job array: the jobs' level offsets, the list schedule (plan_sched.hpp) over the
// launch's workgroup slots, and each job's record copied in that order, its own store slot
// and its landmark seeds' slots (after every kept row's) now final.
std::vector<KDJob> queue_jobs(PlanBuild& B) {
    const int nj = (int)B.job_pos.size();
    shd_route_plan* P = B.P;
    std::vector<int> cnt(B.nlev + 1, 0);
    for (int j = 0; j < nj; j++) cnt[B.lvl[j] + 1]++;
    for (int k = 0; k < B.nlev; k++) cnt[k + 1] += cnt[k];
    P->lvl_off = cnt;
    SeedDeps deps = seed_dependants(nj, B.nsd.data(), B.seedjob.data(), B.lmseed.data());
    B.T.mark("deps");
    std::vector<KDJob> jobs(nj);
    B.T.mark("jobs");
    long long ticks = -1;
    const std::vector<int> order = list_schedule(nj, B.nsd.data(), B.lmseed.data(), std::move(deps),
                                                 std::max(1, B.c->kd.slots), B.o.cost, B.o.sched, &ticks);
    for (int qi = 0; qi < nj; qi++) {
        KDJob& J = jobs[qi];
        J = B.byjob[order[qi]];
        J.store = B.slot[order[qi]];
        for (int k = 0; k < J.nseed; k++)
            if (J.seed[k] < 0) J.seed[k] = P->nslots + (-1 - J.seed[k]);
    }
    B.T.mark("sched");
    if (B.o.debug) fprintf(stderr, "  schedule: job array ready %.2f ms (%d jobs, ticks to %lld)\n", B.T.ms("jobs"), nj, ticks);
    return jobs;
}

// SHD_ROUTE_PLAN_DEBUG: the plan's shape and stage times (tools/plan_debug.py reads the lines)
void report_plan(const PlanBuild& B) {
    const int nj = (int)B.job_pos.size();
    const StageTimes& T = B.T;
    int hist[KD_SEEDS + 1] = {0};
    for (int j = 0; j < nj; j++) hist[B.nsd[j]]++;
    fprintf(stderr, "plan world %d rank %d: jobs %d levels %d seeds:", B.world, B.rank, nj, B.nlev);
    for (int k = 0; k <= KD_SEEDS; k++) fprintf(stderr, " %d:%d", k, hist[k]);
    fprintf(stderr, "  closeness rows %.2f ms, rank sort done %.2f, order sort done %.2f, landmark rows %.2f ms, "
            "seed choices (threads, overlapping the pass) %.2f ms, seeds done %.2f, schedule done %.2f ms\n",
            T.ms("close"), T.ms("rk"), T.ms("order"), T.ms("land"), T.ms("hop"), T.ms("seeds"), T.ms("sched"));
    fprintf(stderr, "  seq loop start %.2f (recomputed %d), store thread started %.2f, deps done %.2f\n", T.ms("loop0"), B.n_recomp,
            T.ms("alloc"), T.ms("deps"));
    int nlm = 0;
    for (int j = 0; j < nj; j++) nlm += B.nsd[j] > 0 && B.lmseed[j][0] >= 0;
    fprintf(stderr, "  seed kinds: landmark-seeded roots %d; neighbour-seeded rows by direct seeds:", nlm);
    for (int k = 0; k <= KD_SEEDS; k++) fprintf(stderr, " %d:%d", k, B.n_direct[k]);
    fprintf(stderr, " (with two-hop seeds %d; at most one direct seed: %.1f%% of the other rows)\n", B.n_twohop,
            100.0 * (B.n_direct[0] + B.n_direct[1]) / std::max(1, nj - nlm));
}

// Seeds, row store and queue order of the jobs (at least two): the plan is seeded when some
// row is kept or landmark rows are used and the store could be allocated; `jobs` is then the
// launch's job array.
int seed_and_schedule(PlanBuild& B, std::vector<KDJob>& jobs) {
    shd_route* c = B.c;
    shd_route_plan* P = B.P;
    const int nj = (int)B.job_pos.size();
    order_jobs(B);
    B.T.mark("order");
    if (B.o.nland > 0) {
        const double t0 = B.T.since();
        const int rc = ensure_hub_rows(c, B.o.nland, B.o.debug);
        if (rc) return rc;
        B.T.mark("land", B.T.since() - t0);
    }
    const int rc = assign_seeds(B);
    if (rc) return rc;
    bool uses_lm = false;
    for (int j = 0; j < nj && !uses_lm; j++) uses_lm = B.nsd[j] > 0 && B.lmseed[j][0] >= 0;
    P->nland = uses_lm ? B.o.nland : 0;
    const int ntot = P->nslots + P->nland;
    P->store_bytes = (uint64_t)ntot * (uint64_t)kd_row_stride(c->n) * 6u;
    bool store_ok = false;
    std::thread store_th;
    if (ntot > 0 && !B.o.store_sync) store_th = std::thread(alloc_plan_store, c, P, nj, ntot, &store_ok);
    struct JoinOne { std::thread& t; ~JoinOne() { if (t.joinable()) t.join(); } } join_store{store_th};
    B.T.mark("alloc");
    if (ntot > 0) {
        jobs = queue_jobs(B);
        if (B.o.debug) report_plan(B);
    }
    if (store_th.joinable()) store_th.join();
    if (ntot > 0 && B.o.store_sync) alloc_plan_store(c, P, nj, ntot, &store_ok);
    B.T.mark("store");
    if (store_ok) {
        P->seeded = 1;
    } else {
        for (void** q : {(void**)&P->d_drow, (void**)&P->d_prow, (void**)&P->d_jobs, (void**)&P->d_next})
            if (*q) { (void)hipFree(*q); *q = nullptr; }
        P->nslots = 0; P->nroots = 0; P->nland = 0; P->store_bytes = 0;
    }
    return SHD_ROUTE_OK;
}

// plain rows (the helpers of an unseeded multi-GPU plan are not needed)
int finish_unseeded(PlanBuild& B) {
    shd_route_plan* P = B.P;
    const int nr = (int)P->row_pos.size();
    P->nhelpers = 0;
    std::vector<int32_t> sv(std::max(nr, 1), 0);
    for (int r = 0; r < nr; r++) sv[r] = B.src[P->row_pos[r]];
    if (hipMalloc((void**)&P->d_src, sizeof(int32_t) * sv.size()) != hipSuccess) return SHD_ROUTE_ENOMEM;
    if (hipMemcpy(P->d_src, sv.data(), sizeof(int32_t) * sv.size(), hipMemcpyHostToDevice) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    P->nroots = nr;
    return SHD_ROUTE_OK;
}

}  // namespace

extern "C" {

int shd_route_plan_create(shd_route_t* c, const int32_t* src, int32_t ns, int32_t world, int32_t rank,
                          shd_route_plan_t** out) {
    if (!c || !out || ns < 0 || (ns && !src) || world < 1 || rank < 0 || rank >= world) return SHD_ROUTE_EINVAL;
    *out = nullptr;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    for (int p = 0; p < ns; p++) if (src[p] < 0 || src[p] >= c->n) return SHD_ROUTE_EINVAL;
    const PlanOptions o = plan_options(c, ns, world);
    auto P = std::make_unique<shd_route_plan>();
    P->c = c; P->world = world; P->rank = rank; P->ns_all = ns;
    P->delta = o.delta;
    PlanBuild B{c, src, ns, world, rank, o, P.get()};
    B.want = o.seed && c->sel == 4 && c->kd.fused && !c->complete && !c->prefer_direct && ns >= 2 && !c->h_row.empty();
    int rc;
    const int nmine = ns > rank ? (ns - rank + world - 1) / world : 0;
    if (B.want && o.lm_all && o.nland > 0 && nmine >= 2 && nmine <= PLAN_DEV_MAXJ && o.gpu_choice && o.lmall_rev &&
        o.plan_dev) {
        if ((rc = build_device_lm_plan(B))) return rc;
        *out = P.release();
        return SHD_ROUTE_OK;
    }
    if (B.want) {
        if ((rc = ensure_hub_rows(c, o.nland, o.debug))) return rc;
        B.T.mark("close");
        B.rk = closeness_ranks(c);
        B.T.mark("rk");
    }
    partition_rows(B);
    std::vector<KDJob> jobs;
    if (B.want && B.job_pos.size() >= 2 && (rc = seed_and_schedule(B, jobs))) return rc;
    if (P->seeded) {
        if (hipMemcpy(P->d_jobs, jobs.data(), sizeof(KDJob) * jobs.size(), hipMemcpyHostToDevice) != hipSuccess)
            return SHD_ROUTE_EDEVICE;
    } else if ((rc = finish_unseeded(B))) {
        return rc;
    }
    if (o.debug) fprintf(stderr, "  store thread joined %.2f, plan total %.2f ms\n", B.T.ms("store"), 1e3 * B.T.since());
    *out = P.release();
    return SHD_ROUTE_OK;
}

void shd_route_plan_destroy(shd_route_plan_t* P) {
    if (!P) return;
    (void)hipSetDevice(P->c->device);
    delete P;
}

int shd_route_plan_get_info(const shd_route_plan_t* P, shd_route_plan_info_t* info) {
    if (!P || !info) return SHD_ROUTE_EINVAL;
    info->rows = (int32_t)P->row_pos.size();
    info->seeded = P->seeded;
    // (landmark-only: hub rows, [landmark biases,] the job records [+ order keys and ranks], rows)
    info->launches = P->lm_step ? (P->order_fixed ? 3 : 5) + (P->d_bias ? 1 : 0) : 1;
    info->levels = P->seeded ? (int32_t)P->lvl_off.size() - 1 : 1;
    info->roots = P->nroots;
    info->helpers = P->nhelpers;
    info->stored_rows = P->nslots;
    info->world = P->world;
    info->rank = P->rank;
    info->store_bytes = P->store_bytes;
    info->delta = P->seeded ? P->delta : P->c->kd.delta;
    info->pad_ = 0;
    return SHD_ROUTE_OK;
}

int shd_route_plan_rows(const shd_route_plan_t* P, int32_t* pos_out) {
    if (!P || !pos_out) return SHD_ROUTE_EINVAL;
    std::copy(P->row_pos.begin(), P->row_pos.end(), pos_out);
    return SHD_ROUTE_OK;
}

int shd_route_plan_refresh_async(shd_route_t* c, const shd_route_plan_t* P, uint32_t what, void* stream) {
    if (!c || !P || P->c != c || (what & ~(SHD_ROUTE_REFRESH_ALL | SHD_ROUTE_REFRESH_MINE | SHD_ROUTE_REFRESH_JOBS)))
        return SHD_ROUTE_EINVAL;
    if (!P->lm_step) return SHD_ROUTE_OK;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    return lm_refresh(c, P, what, (hipStream_t)stream);
}

int shd_route_plan_landmarks(const shd_route_plan_t* P, int32_t* nland, int32_t* first, int32_t* count,
                             int64_t* row_stride) {
    if (!P || !nland || !first || !count || !row_stride) return SHD_ROUTE_EINVAL;
    if (!P->lm_step) return SHD_ROUTE_EUNSUPPORTED;
    *nland = P->nhub; *first = P->lm_first; *count = P->lm_count;
    *row_stride = kd_row_stride(P->c->n);
    return SHD_ROUTE_OK;
}

int shd_route_plan_bind_store(shd_route_t* c, shd_route_plan_t* P, uint16_t* d_drow, uint32_t* d_prow) {
    if (!c || !P || P->c != c || !d_drow || !d_prow) return SHD_ROUTE_EINVAL;
    if (!P->lm_step) return SHD_ROUTE_EUNSUPPORTED;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    const size_t cells = (size_t)kd_row_stride(c->n) * P->nhub;
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(d_drow, P->d_drow, sizeof(uint16_t) * cells, hipMemcpyDeviceToDevice) != hipSuccess ||
        hipMemcpy(d_prow, P->d_prow, sizeof(uint32_t) * cells, hipMemcpyDeviceToDevice) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    if (!P->store_external) {
        (void)hipFree(P->d_drow);
        (void)hipFree(P->d_prow);
    }
    P->d_drow = d_drow; P->d_prow = d_prow; P->store_external = true;
    return SHD_ROUTE_OK;
}

int shd_route_rows_planned_async(shd_route_t* c, const shd_route_plan_t* P, const int32_t* d_tgt, int32_t nt,
                                 int64_t ld, uint32_t flags, double* d_lat, double* d_rel, double* d_row_min,
                                 void* stream) {
    if (!c || !P || P->c != c || nt < 0 || (nt && !d_tgt) || ld < nt) return SHD_ROUTE_EINVAL;
    const int nr = (int)P->row_pos.size();
    if (!P->seeded) return shd_route_rows_async(c, P->d_src, nr, d_tgt, nt, ld, flags, d_lat, d_rel, d_row_min, stream);
    hipStream_t st = (hipStream_t)stream;
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    if (P->lm_step && !(flags & SHD_ROUTE_PLAN_REUSE)) {
        const int rc = lm_refresh(c, P, 0, st);  // the landmark rows and the jobs, on this stream
        if (rc) return rc;
    }
    // one launch: jobs in level order from one queue; a seeded job waits for its seed's
    // ready flag (set once the kept row is complete, before that row's phase C)
    if (hipMemsetAsync(P->d_next, 0, sizeof(int) * (1 + (size_t)P->nslots), st) != hipSuccess) return SHD_ROUTE_EDEVICE;
    if (P->nland && hipMemsetD32Async((hipDeviceptr_t)(P->d_next + 1 + P->nslots), 1, (size_t)P->nland, st) != hipSuccess)
        return SHD_ROUTE_EDEVICE;  // landmark rows: complete before the launch
    DevDelta k = kd_args(c);
    k.delta = P->delta;
    k.drow = P->d_drow; k.drow_out = P->d_drow; k.prow = P->d_prow; k.rstride = kd_row_stride(c->n);
    k.jobs = P->d_jobs;
    k.done = P->d_next + 1;
    return kd_launch(c, k, P->d_next, nullptr, P->lvl_off.back(), d_tgt, nt, ld, d_lat, d_rel, d_row_min, st);
}

// Diagnostics: the plan's job records in queue order (include/shd_route.h)
int shd_route_plan_jobs(shd_route_t* c, const shd_route_plan_t* P, int32_t* njobs, void* out, int64_t out_bytes) {
    if (!c || !P || P->c != c || !njobs) return SHD_ROUTE_EINVAL;
    if (!P->seeded) return SHD_ROUTE_EUNSUPPORTED;
    const int nj = P->lvl_off.back();
    *njobs = nj;
    if (!out) return SHD_ROUTE_OK;
    if (out_bytes < (int64_t)sizeof(KDJob) * nj) return SHD_ROUTE_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return SHD_ROUTE_EDEVICE;
    if (nj && hipMemcpy(out, P->d_jobs, sizeof(KDJob) * (size_t)nj, hipMemcpyDeviceToHost) != hipSuccess)
        return SHD_ROUTE_EDEVICE;
    return SHD_ROUTE_OK;
}

}  // extern "C"

namespace {
// shd_route_rows through a seeded plan: every row in one device table (EUNSUPPORTED when
// the plan is not seeded or the table does not fit, so the caller takes the chunked path)
int planned_host_rows(shd_route* c, const int32_t* src, int32_t ns, const int32_t* tgt, int32_t nt,
                      uint32_t flags, double* lat_out, double* rel_out, double* row_min_out) {
    if (hipSetDevice(c->device) != hipSuccess) return SHD_ROUTE_EDEVICE;
    const size_t table = sizeof(double) * (size_t)ns * (size_t)nt;
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess || 2 * table + ((size_t)ns << 20) > fr / 2) return SHD_ROUTE_EUNSUPPORTED;
    shd_route_plan_t* P = nullptr;
    int rc = shd_route_plan_create(c, src, ns, 1, 0, &P);
    if (rc == SHD_ROUTE_ENOMEM) return SHD_ROUTE_EUNSUPPORTED;  // the chunked rows need far less
    if (rc) return rc;
    std::unique_ptr<shd_route_plan, void (*)(shd_route_plan*)> guard(P, shd_route_plan_destroy);
    if (!P->seeded) return SHD_ROUTE_EUNSUPPORTED;
    DevBuf dtgt, dlat, drel, dmin;
    if (dtgt.alloc(sizeof(int32_t) * nt) || dlat.alloc(table) || drel.alloc(table) || dmin.alloc(sizeof(double) * ns))
        return SHD_ROUTE_EUNSUPPORTED;
    if (hipMemcpy(dtgt.p, tgt, sizeof(int32_t) * nt, hipMemcpyHostToDevice) != hipSuccess) return SHD_ROUTE_EDEVICE;
    // (the plan was made just now: its landmark rows, if any, are current)
    rc = shd_route_rows_planned_async(c, P, (const int32_t*)dtgt.p, nt, nt, flags | SHD_ROUTE_PLAN_REUSE, (double*)dlat.p, (double*)drel.p,
                                      (double*)dmin.p, nullptr);
    if (rc) return rc;
    const int soft = shd_route_sync(c, nullptr);
    if (soft && soft != SHD_ROUTE_ENOEDGE && soft != SHD_ROUTE_EUNREACH) return soft;
    if ((lat_out && hipMemcpy(lat_out, dlat.p, table, hipMemcpyDeviceToHost) != hipSuccess) ||
        (rel_out && hipMemcpy(rel_out, drel.p, table, hipMemcpyDeviceToHost) != hipSuccess) ||
        (row_min_out && hipMemcpy(row_min_out, dmin.p, sizeof(double) * ns, hipMemcpyDeviceToHost) != hipSuccess))
        return SHD_ROUTE_EDEVICE;
    return soft;
}
}  // namespace
