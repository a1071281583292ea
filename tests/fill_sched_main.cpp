// Stand-alone driver of shadow_amd/csrc/fill_sched.hpp (the schedule of shd_route_fill_triangle)
// for tests/test_library.py.  Built with the host sanitizers and run as its own process.
//
// Random inputs: na from 1 to ~3000; world 1 to 8 with a random partition of the rows (row by
// row, or in runs as a forest partition gives them), this rank's rows in ascending or in random
// order; both layouts; stage sizes from one row (SHD_ROUTE_FILL_STAGE=1 through the knob's own
// parser) to everything, and raw ones below a row; host chunks of 0, 2 MiB and 6 MiB with the
// triangle at a random 2 MiB multiple inside the mapping.  Against a brute-force byte map of the
// triangle, built here from plain prefix sums:
//   1  every byte of every owned row (compact: of its lines, pad included) is the destination of
//      exactly one piece and no other byte is
//   2  a piece's source range lies inside one staging buffer of the effective size and is the
//      packed position of the rows it carries (off[r] - off[r0], plus the offset in the row)
//   3  no piece crosses a host chunk boundary, none is empty
//   4  chunks are consecutive, non-empty and as long as the stage allows, buffers alternate, none
//      exceeds the stage except a single row, and the pieces of a chunk are its own
//   5  the default constants at C3 (na 9337; world 1, 2) and C4 (na 50000; world 1, 8) give the
//      chunk counts the sizes give: ceil(total / stage) <= chunks <= total / (stage - longest
//      row) + 1, and exactly 2 / 1 (C3) and 38 / 25 (C4) for one rank, interleaved / compact
// Prints one line with the C3 and C4 counts; exit status 0 = pass.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>

#include "../shadow_amd/csrc/fill_sched.hpp"

using namespace shd;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {  // xorshift64*: the same inputs on every run
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n;
}

// this rank's rows: by = 0 each row to a random rank, else runs of 1 .. by rows
static std::vector<int> share(int na, int world, int rank, int by, bool shuffle) {
    std::vector<int> pos;
    for (int i = 0; i < na;) {
        const int len = by ? 1 + (int)rnd((uint32_t)by) : 1;
        const int owner = (int)rnd((uint32_t)world);
        for (int k = 0; k < len && i < na; k++, i++)
            if (owner == rank) pos.push_back(i);
    }
    if (shuffle)
        for (size_t k = pos.size(); k > 1; k--) std::swap(pos[k - 1], pos[rnd((uint32_t)k)]);
    return pos;
}

struct Counts {
    long long chunks = 0, pieces = 0;
};

// checks 1 to 4; bytemap false (the C3 / C4 sizes): the byte map is replaced by the sum of
// the pieces' bytes and their pairwise order within a row
static int check(int na, const std::vector<int>& pos, bool l16, long long stage_units, long long stage_bytes,
                 size_t host_chunk, size_t host_off, bool bytemap, Counts* out) {
    const int nr = (int)pos.size();
    const long long unit = l16 ? 64 : 16;
    auto units = [&](long long i) { return l16 ? (na - i + 5) / 6 : na - i; };
    std::vector<long long> start((size_t)na + 1, 0);  // the triangle, row by row
    for (int i = 0; i < na; i++) start[i + 1] = start[i] + units(i);
    const long long total = unit * start[na];
    if (l16 && start[na] != fill_tri16_line(na, na)) return 10;
    std::vector<long long> pk((size_t)nr + 1, 0);     // the packed rows, in plan order
    std::vector<int> at((size_t)na, -1);
    for (int r = 0; r < nr; r++) {
        pk[r + 1] = pk[r] + units(pos[r]);
        at[pos[r]] = r;
    }
    const FillSchedule S = fill_schedule(na, pos.data(), nr, l16, stage_units, host_chunk, host_off);
    if (S.pk != pk) return 11;
    if (out) { out->chunks = (long long)S.chunks.size(); out->pieces = (long long)S.pieces.size(); }
    // 4: the chunks
    int r_next = 0, p_next = 0;
    for (size_t k = 0; k < S.chunks.size(); k++) {
        const FillChunk& c = S.chunks[k];
        if (c.r0 != r_next || c.r1 <= c.r0 || c.r1 > nr) return 40;
        if (c.buf != (int)(k & 1)) return 41;
        if (pk[c.r1] - pk[c.r0] > stage_units && c.r1 - c.r0 != 1) return 42;
        if (c.r1 < nr && pk[c.r1 + 1] - pk[c.r0] <= stage_units) return 43;  // (the next row fitted)
        if (c.p0 != p_next || c.p1 <= c.p0 || c.p1 > (int)S.pieces.size()) return 44;
        r_next = c.r1;
        p_next = c.p1;
    }
    if (r_next != nr || p_next != (int)S.pieces.size()) return 45;
    // 1, 2, 3: the pieces
    std::vector<uint8_t> cnt(bytemap ? (size_t)total : 0, 0);
    long long sum = 0;
    for (const FillChunk& c : S.chunks)
        for (int q = c.p0; q < c.p1; q++) {
            const FillPiece& p = S.pieces[q];
            if (p.bytes <= 0 || p.dst < 0 || p.dst + p.bytes > total) return 30;
            if (p.src < 0 || p.src + p.bytes > stage_bytes) {
                // (a single row longer than a raw stage: only then may the source run past it)
                if (!(c.r1 - c.r0 == 1 && pk[c.r1] - pk[c.r0] > stage_units) || p.src < 0) return 20;
            }
            if (host_chunk && (host_off + (size_t)p.dst) / host_chunk != (host_off + (size_t)(p.dst + p.bytes - 1)) / host_chunk)
                return 31;
            // row by row through the piece: the row is this chunk's and sits where the pack
            // kernels put it
            for (long long d = p.dst, left = p.bytes; left;) {
                const int i = (int)(std::upper_bound(start.begin(), start.end(), d / unit) - start.begin()) - 1;
                if (i < 0 || i >= na) return 21;
                const int r = at[i];
                if (r < c.r0 || r >= c.r1) return 22;
                const long long within = d - unit * start[i];
                if (p.src + (d - p.dst) != unit * (pk[r] - pk[c.r0]) + within) return 23;
                const long long nb = std::min(left, unit * units(i) - within);
                d += nb;
                left -= nb;
            }
            sum += p.bytes;
            if (bytemap) {  // no byte of it marked before; mark them
                if (std::memchr(cnt.data() + p.dst, 1, (size_t)p.bytes)) return 12;
                std::memset(cnt.data() + p.dst, 1, (size_t)p.bytes);
            }
        }
    if (sum != unit * pk[nr]) return 13;
    if (bytemap)
        for (int i = 0; i < na; i++)  // an owned row: no byte unmarked; another's: none marked
            if (std::memchr(cnt.data() + unit * start[i], at[i] >= 0 ? 0 : 1, (size_t)(unit * units(i)))) return 14;
    return 0;
}

int main() {
    // the knobs' parsers
    if (fill_stage_pairs(nullptr, 100, false) != FILL_STAGE_PAIRS || fill_stage_pairs("", 100, true) != FILL_STAGE_PAIRS ||
        fill_stage_pairs("x", 100, false) != FILL_STAGE_PAIRS || fill_stage_pairs("-5", 100, false) != FILL_STAGE_PAIRS ||
        fill_stage_pairs("0", 100, false) != FILL_STAGE_PAIRS || fill_stage_pairs("1", 101, false) != 104 ||
        fill_stage_pairs("1", 101, true) != 68 || fill_stage_pairs("1", 6, true) != 4 || fill_stage_pairs("1", 7, true) != 8 ||
        fill_stage_pairs("1001", 7, false) != 1004 || fill_stage_units(1004, true) != 251 || fill_stage_units(1004, false) != 1004) {
        std::printf("FAIL: SHD_ROUTE_FILL_STAGE parsing\n");
        return 1;
    }
    const size_t mib = (size_t)1 << 20;
    if (fill_host_chunk(nullptr) != 256 * mib || fill_host_chunk("") != 256 * mib || fill_host_chunk("abc") != 256 * mib ||
        fill_host_chunk("0") != 256 * mib || fill_host_chunk("-1") != 256 * mib || fill_host_chunk("1") != 2 * mib ||
        fill_host_chunk("2097152") != 2 * mib || fill_host_chunk("2097153") != 4 * mib || fill_host_chunk("6291456") != 6 * mib) {
        std::printf("FAIL: SHD_ROUTE_HOST_CHUNK parsing\n");
        return 1;
    }
    int cases = 0;
    for (int rep = 0; rep < 360; rep++) {
        const int na = rep < 12 ? rep + 1 : rep % 40 == 20 ? 1500 + (int)rnd(1500) : rep % 20 == 10 ? 400 + (int)rnd(600)
                                                                                                      : 1 + (int)rnd(400);
        const int world = 1 + (int)rnd(8), rank = (int)rnd((uint32_t)world);
        const bool l16 = rep & 1;
        const std::vector<int> pos = share(na, world, rank, rep % 3 == 0 ? 0 : 1 + (int)rnd(20), rep % 4 >= 2);
        long long all = 0;  // the rank's pairs
        for (int i : pos) all += na - i;
        // the stage: the knob at its minimum, somewhere between, everything; or raw units that
        // are less than the first row (a single row may then exceed the stage)
        const int how = rep % 5;
        long long stage_units, stage_bytes;
        if (how == 4) {
            stage_units = 1 + (long long)rnd((uint32_t)std::max(1, (l16 ? (na + 5) / 6 : na)));
            stage_bytes = (l16 ? 64 : 16) * stage_units;
        } else {
            const std::string env = how == 0 ? "1" : how == 1 ? std::to_string(1 + rnd((uint32_t)std::max(1ll, 8ll * na)))
                                             : how == 2 ? std::to_string(1 + rnd((uint32_t)(all + 1))) : std::to_string(all + 7);
            const long long pairs = fill_stage_pairs(env.c_str(), na, l16);
            if (pairs % 4 || pairs < (l16 ? 4 * ((na + 5) / 6) : na)) { std::printf("FAIL: stage %lld na %d\n", pairs, na); return 1; }
            stage_units = fill_stage_units(pairs, l16);
            stage_bytes = 16 * pairs;
        }
        const size_t chunks[3] = {0, 2 * mib, 6 * mib};
        for (size_t hc : chunks) {
            const size_t off = hc ? 2 * mib * rnd(12) : 0;
            Counts n;
            const int rc = check(na, pos, l16, stage_units, stage_bytes, hc, off, true, &n);
            if (rc) {
                std::printf("FAIL %d: rep %d na %d world %d rank %d rows %zu l16 %d stage %lld chunk %zu off %zu\n", rc, rep, na,
                            world, rank, pos.size(), (int)l16, stage_units, hc, off);
                return rc;
            }
            if (how == 3 && n.chunks != (pos.empty() ? 0 : 1)) { std::printf("FAIL: everything in %lld chunks\n", n.chunks); return 1; }
            cases++;
        }
    }
    // 5: the default constants at C3 and C4
    std::string line;
    const int sizes[2] = {9337, 50000}, worlds[2] = {2, 8};
    for (int s = 0; s < 2; s++) {
        const int na = sizes[s];
        line += s ? ", c4" : "c3";
        for (int w = 0; w < 2; w++) {
            const int world = w ? worlds[s] : 1;
            for (int l16 = 0; l16 < 2; l16++) {
                const std::vector<int> pos = share(na, world, 0, w ? 64 : 0, false);
                const long long pairs = fill_stage_pairs(nullptr, na, l16);
                const long long su = fill_stage_units(pairs, l16);
                Counts n;
                const int rc = check(na, pos, l16, su, 16 * pairs, fill_host_chunk(nullptr), 0, false, &n);
                if (rc) { std::printf("FAIL %d: na %d world %d l16 %d\n", rc, na, world, l16); return rc; }
                long long total = 0, longest = 0;
                for (int i : pos) {
                    const long long u = l16 ? (na - i + 5) / 6 : na - i;
                    total += u;
                    longest = std::max(longest, u);
                }
                const long long lo = (total + su - 1) / su, hi = total / (su - longest) + 1;
                if (n.chunks < lo || n.chunks > hi) { std::printf("FAIL: na %d world %d: %lld chunks, not in [%lld, %lld]\n", na, world, n.chunks, lo, hi); return 1; }
                if (!w) {
                    const long long want = s ? (l16 ? 25 : 38) : (l16 ? 1 : 2);
                    if (n.chunks != want || lo != want) { std::printf("FAIL: na %d l16 %d: %lld chunks\n", na, l16, n.chunks); return 1; }
                }
                line += std::string(" ") + (w ? "world" + std::to_string(world) + " " : "") + (l16 ? "compact " : "interleaved ") +
                        std::to_string(n.chunks) + " chunks " + std::to_string(std::max(0ll, n.chunks - 2)) + " reuses " +
                        std::to_string(n.pieces) + " pieces";
                cases++;
            }
        }
    }
    std::printf("ok %d schedules; %s\n", cases, line.c_str());
    return 0;
}
