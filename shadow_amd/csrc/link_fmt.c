/*
 * link_fmt.c -- the line shd_topology_dump_link_loads writes per edge, in the style of the
 * route line (route_fmt.c):
 *   link A<-->B (i<-->j) edge E is L ms with P loss, N packets
 * No reference equivalent: Shadow 1.14 counts packets per cached Path (path.c:57-60), not per
 * link.  A pure host function over plain values (no engine, no topology object), so it
 * builds and runs without a GPU.  The text grows in a caller-owned malloc buffer.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/shd_topology.h"

int64_t shd_topology_link_line(char** buf, size_t* cap, char* const* names, int32_t edge, int32_t a, int32_t b,
                               double latency, double loss, uint64_t packets, int directed) {
    if (!buf || !cap || edge < 0 || a < 0 || b < 0) return -1;
    char ta[16], tb[16];
    const char* na = names && names[a] ? names[a] : NULL;
    const char* nb = names && names[b] ? names[b] : NULL;
    if (!na) { snprintf(ta, sizeof ta, "%d", (int)a); na = ta; }
    if (!nb) { snprintf(tb, sizeof tb, "%d", (int)b); nb = tb; }
    const char* sep = directed ? "-->" : "<-->";
    if (!*buf) *cap = 0;
    for (;;) {
        const int k = snprintf(*buf, *cap, "link %s%s%s (%i%s%i) edge %i is %f ms with %f loss, %llu packets", na, sep,
                               nb, (int)a, sep, (int)b, (int)edge, latency, loss, (unsigned long long)packets);
        if (k < 0) return -1;
        if ((size_t)k < *cap) return (int64_t)k;
        size_t nc = *cap ? *cap * 2 : 64;
        while (nc < (size_t)k + 1) nc *= 2;
        char* ns = realloc(*buf, nc);
        if (!ns) return -1;
        *buf = ns;
        *cap = nc;
    }
}
