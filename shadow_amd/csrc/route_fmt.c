/*
 * route_fmt.c -- the line _topology_computeSourcePaths logs for every path it computes
 * (reference topology.c:1829-1834), with the path string _topology_computePathProperties
 * assembles hop by hop (topology.c:1449, 1502-1503):
 *   shortest path A<-->B (i<-->j) is L ms with P loss, path: A<--[lat,loss]-->X<--[lat,loss]-->B
 * A pure host function over arrays (no engine, no topology object), so it builds and runs
 * without a GPU.  The text grows in a caller-owned malloc buffer.
 */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/shd_topology.h"

typedef struct {
    char* s;
    size_t cap, len;
    int failed;
} fbuf;

static void fb_printf(fbuf* b, const char* fmt, ...) {
    if (b->failed) return;
    for (;;) {
        va_list ap;
        va_start(ap, fmt);
        const int k = vsnprintf(b->s ? b->s + b->len : NULL, b->s ? b->cap - b->len : 0, fmt, ap);
        va_end(ap);
        if (k < 0) { b->failed = 1; return; }
        if (b->s && (size_t)k < b->cap - b->len) { b->len += (size_t)k; return; }
        size_t nc = b->cap ? b->cap * 2 : 64;
        while (nc < b->len + (size_t)k + 1) nc *= 2;
        char* ns = realloc(b->s, nc);
        if (!ns) { b->failed = 1; return; }
        b->s = ns;
        b->cap = nc;
    }
}

/* the name the reference prints for a vertex: its graphml id, or the decimal index */
static const char* vname(char* const* names, int32_t v, char tmp[16]) {
    if (names && names[v]) return names[v];
    snprintf(tmp, 16, "%d", (int)v);
    return tmp;
}

int64_t shd_topology_route_line(char** buf, size_t* cap, char* const* names, const int32_t* vert, int32_t nv,
                                const double* hop_lat, const double* hop_rel, double lat, double rel, int directed) {
    if (!buf || !cap || !vert || nv < 1 || (nv > 1 && (!hop_lat || !hop_rel))) return -1;
    fbuf b = { *buf, *buf ? *cap : 0, 0, 0 };
    char ta[16], tb[16];
    const char* sep = directed ? "-->" : "<-->";
    fb_printf(&b, "shortest path %s%s%s (%i%s%i) is %f ms with %f loss, path: %s", vname(names, vert[0], ta), sep,
              vname(names, vert[nv - 1], tb), (int)vert[0], sep, (int)vert[nv - 1], lat, 1 - rel,
              vname(names, vert[0], ta));
    for (int32_t q = 1; q < nv; q++)
        fb_printf(&b, "%s[%f,%f]-->%s", directed ? "--" : "<--", hop_lat[q - 1], 1.0 - hop_rel[q - 1],
                  vname(names, vert[q], ta));
    *buf = b.s;
    *cap = b.cap;
    return b.failed ? -1 : (int64_t)b.len;
}
