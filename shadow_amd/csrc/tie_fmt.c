/*
 * tie_fmt.c -- the lines shd_topology_dump_ties writes, in the style of the route line
 * (route_fmt.c): one per pair whose reliability depends on the tie rule,
 *   tie A<-->B (i<-->j) has N shortest paths, reliability LO to HI, spread S
 * and the summary that closes the dump,
 *   ties: P pairs, T tied, S sensitive, U saturated, max spread X at (i<-->j) with N paths
 * No reference equivalent: Shadow 1.14 keeps the one path igraph returns.  Reliabilities and
 * spreads are printed with %.17g (they round-trip); a count that saturated at 2^64 - 1 ends
 * in '+'.  Pure host functions over plain values (no engine, no topology object), so they
 * build and run without a GPU.  The text grows in a caller-owned malloc buffer.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/shd_topology.h"

/* room for k + 1 bytes in *buf: 0, or -1 when realloc fails */
static int tie_grow(char** buf, size_t* cap, size_t k) {
    size_t nc = *cap ? *cap * 2 : 64;
    while (nc < k + 1) nc *= 2;
    char* ns = realloc(*buf, nc);
    if (!ns) return -1;
    *buf = ns;
    *cap = nc;
    return 0;
}

int64_t shd_topology_tie_line(char** buf, size_t* cap, char* const* names, int32_t a, int32_t b, uint64_t count,
                              double rel_lo, double rel_hi, int directed) {
    if (!buf || !cap || a < 0 || b < 0) return -1;
    char ta[16], tb[16];
    const char* na = names && names[a] ? names[a] : NULL;
    const char* nb = names && names[b] ? names[b] : NULL;
    if (!na) { snprintf(ta, sizeof ta, "%d", (int)a); na = ta; }
    if (!nb) { snprintf(tb, sizeof tb, "%d", (int)b); nb = tb; }
    const char* sep = directed ? "-->" : "<-->";
    const double spread = rel_hi > 0.0 ? (rel_hi - rel_lo) / rel_hi : 0.0;
    if (!*buf) *cap = 0;
    for (;;) {
        const int k = snprintf(*buf, *cap, "tie %s%s%s (%i%s%i) has %llu%s shortest paths, reliability %.17g to %.17g, "
                               "spread %.17g", na, sep, nb, (int)a, sep, (int)b, (unsigned long long)count,
                               count == UINT64_MAX ? "+" : "", rel_lo, rel_hi, spread);
        if (k < 0) return -1;
        if ((size_t)k < *cap) return (int64_t)k;
        if (tie_grow(buf, cap, (size_t)k)) return -1;
    }
}

int64_t shd_topology_tie_summary_line(char** buf, size_t* cap, const shd_tie_stats_t* st, int directed) {
    if (!buf || !cap || !st) return -1;
    const char* sep = directed ? "-->" : "<-->";
    if (!*buf) *cap = 0;
    for (;;) {
        const int k = snprintf(*buf, *cap, "ties: %llu pairs, %llu tied, %llu sensitive, %llu saturated, max spread %.17g "
                               "at (%i%s%i) with %llu%s paths", (unsigned long long)st->pairs,
                               (unsigned long long)st->tied, (unsigned long long)st->sensitive,
                               (unsigned long long)st->saturated, st->max_spread, (int)st->worst_src, sep,
                               (int)st->worst_dst, (unsigned long long)st->worst_count,
                               st->worst_count == UINT64_MAX ? "+" : "");
        if (k < 0) return -1;
        if ((size_t)k < *cap) return (int64_t)k;
        if (tie_grow(buf, cap, (size_t)k)) return -1;
    }
}
