// fill_sched.hpp -- the schedule of shd_route_fill_triangle (engine.hip): which plan rows go
// into which staging buffer, and the device-to-host copies that take each packed chunk to the
// host triangle, already cut at the registration boundaries of lazily pinned memory.  Pure
// host code: no HIP and no engine types, so that tests/fill_sched_main.cpp checks it under the
// host sanitizers without a GPU.  The engine keeps the events, the waits and the launches and
// walks this schedule.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <vector>

namespace shd {

constexpr long long FILL_STAGE_PAIRS = 32ll << 20;        // 512 MiB of (lat, rel) per staging buffer
constexpr size_t FILL_HOST_CHUNK = (size_t)256 << 20;     // one registration of lazily pinned memory
constexpr size_t FILL_HUGE_PAGE = (size_t)2 << 20;        // the mapping's alignment

// first 64-byte line of row i of the compact triangle (shd_route_tri16_line of shd_route.h)
inline long long fill_tri16_line(long long na, long long i) {
    long long pad = (i / 6) * 15;
    for (long long t = 0; t < i % 6; t++) pad += (6 - (na - t) % 6) % 6;
    return (i * na - i * (i - 1) / 2 + pad) / 6;
}

// SHD_ROUTE_FILL_STAGE (tests: many stage chunks on a small triangle): the pairs per staging
// buffer.  NULL, empty, non-numeric or <= 0: the default.  Never below one whole row (na
// pairs; ceil(na / 6) lines of 4 pairs' bytes in the compact layout), and a multiple of 4,
// so that the compact layout's line count 16 * pairs / 64 is exact.
inline long long fill_stage_pairs(const char* env, int na, bool l16) {
    long long v = env ? std::atoll(env) : 0;
    if (v <= 0) v = FILL_STAGE_PAIRS;
    const long long row = l16 ? 4 * (((long long)na + 5) / 6) : (long long)na;
    v = std::max(v, row);
    return (v + 3) & ~3ll;
}

// the same in packed units: 64-byte lines (compact) or pairs (interleaved)
inline long long fill_stage_units(long long stage_pairs, bool l16) { return l16 ? stage_pairs / 4 : stage_pairs; }

// SHD_ROUTE_HOST_CHUNK (tests: registration boundaries inside a small triangle): the bytes
// per chunk of shd_route_host_alloc / _lazy, a multiple of the 2 MiB huge page and at least
// one.  NULL, empty, non-numeric or <= 0: the default.
inline size_t fill_host_chunk(const char* env) {
    const long long v = env ? std::atoll(env) : 0;
    if (v <= 0) return FILL_HOST_CHUNK;
    return ((size_t)v + FILL_HUGE_PAGE - 1) & ~(FILL_HUGE_PAGE - 1);
}

// one device-to-host copy: bytes from `src` of the chunk's staging buffer to `dst` of the
// triangle (byte offsets)
struct FillPiece {
    long long dst, src, bytes;
};

// plan rows [r0, r1) packed into staging buffer `buf`, copied out by pieces [p0, p1)
struct FillChunk {
    int r0, r1, buf, p0, p1;
};

struct FillSchedule {
    std::vector<FillChunk> chunks;
    std::vector<FillPiece> pieces;
    std::vector<long long> pk;  // packed offset of each plan row in units (nr + 1 entries): the
                                // pack kernels' off[], row r of a chunk at pk[r] - pk[r0]
};

// The rank's rows row_pos[0 .. nr) (attached positions, in plan order) of a triangle over na
// vertices.  Rows are taken in plan order while they fit stage_units (a single longer row
// still makes a chunk of its own); the buffers alternate.  Of each chunk, consecutive rows
// that are consecutive in the triangle too go out as one piece, and a piece is cut wherever
// host_off + dst crosses a multiple of host_chunk (host_chunk 0: memory without
// registration boundaries, no cuts) -- a copy must not span two registrations.
inline FillSchedule fill_schedule(int na, const int* row_pos, int nr, bool l16, long long stage_units,
                                  size_t host_chunk, size_t host_off) {
    FillSchedule S;
    const long long unit = l16 ? 64 : 16;  // bytes per line / per pair
    auto row_units = [&](int r) { return l16 ? ((long long)na - row_pos[r] + 5) / 6 : (long long)na - row_pos[r]; };
    auto tri_unit = [&](int r) {  // where row r starts in the triangle
        const long long i = row_pos[r];
        return l16 ? fill_tri16_line(na, i) : i * (long long)na - i * (i - 1) / 2;
    };
    S.pk.assign((size_t)nr + 1, 0);
    for (int r = 0; r < nr; r++) S.pk[r + 1] = S.pk[r] + row_units(r);
    int buf = 0;
    for (int r0 = 0; r0 < nr; buf ^= 1) {
        int r1 = r0;
        while (r1 < nr && S.pk[r1 + 1] - S.pk[r0] <= stage_units) r1++;
        if (r1 == r0) r1 = r0 + 1;
        FillChunk c{r0, r1, buf, (int)S.pieces.size(), 0};
        for (int a = r0; a < r1;) {
            int b = a + 1;
            while (b < r1 && tri_unit(b) == tri_unit(b - 1) + row_units(b - 1)) b++;
            long long dst = unit * tri_unit(a), src = unit * (S.pk[a] - S.pk[r0]), bytes = unit * (S.pk[b] - S.pk[a]);
            while (bytes) {
                long long nb = bytes;
                if (host_chunk) {
                    const size_t o = host_off + (size_t)dst;
                    nb = (long long)std::min<size_t>((size_t)nb, (o / host_chunk + 1) * host_chunk - o);
                }
                S.pieces.push_back({dst, src, nb});
                dst += nb; src += nb; bytes -= nb;
            }
            a = b;
        }
        c.p1 = (int)S.pieces.size();
        S.chunks.push_back(c);
        r0 = r1;
    }
    return S;
}

}  // namespace shd
