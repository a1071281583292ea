/* Stand-alone driver of shadow_amd/csrc/route_fmt.c for tests/test_hops.py: formats four
 * paths and prints one line each.  Built with the host sanitizers and run as its own
 * process; the expected strings are rebuilt in Python from the same formulas. */
#include <stdio.h>
#include <stdlib.h>

#include "../include/shd_topology.h"

#define LONG_HOPS 600

int main(void) {
    char* buf = NULL;
    size_t cap = 0;
    int64_t k;

    /* 1: one hop, undirected, decimal vertex names */
    {
        const int32_t v[2] = { 3, 17 };
        const double hl[1] = { 12.0 }, hr[1] = { 0.99 };
        k = shd_topology_route_line(&buf, &cap, NULL, v, 2, hl, hr, 12.0, 0.99, 0);
        if (k < 0) return 1;
        printf("%s\n", buf);
    }
    /* 2: three hops, directed, graphml ids */
    {
        char* names[4] = { "poi-1", "poi-2", "relay", "poi-9" };
        const int32_t v[4] = { 2, 0, 3, 1 };
        const double hl[3] = { 1.5, 20.25, 3.0 }, hr[3] = { 1.0, 0.875, 0.5 };
        k = shd_topology_route_line(&buf, &cap, names, v, 4, hl, hr, 24.75, 0.4375, 1);
        if (k < 0) return 2;
        printf("%s\n", buf);
    }
    /* 3: LONG_HOPS hops with 40-character names: the buffer grows several times */
    {
        char** names = malloc(sizeof(char*) * (LONG_HOPS + 1));
        int32_t* v = malloc(sizeof(int32_t) * (LONG_HOPS + 1));
        double* hl = malloc(sizeof(double) * LONG_HOPS);
        double* hr = malloc(sizeof(double) * LONG_HOPS);
        double lat = 0.0;
        for (int q = 0; q <= LONG_HOPS; q++) {
            names[q] = malloc(41);
            snprintf(names[q], 41, "vertex-%033d", q);
            v[q] = LONG_HOPS - q;
        }
        for (int q = 0; q < LONG_HOPS; q++) {
            hl[q] = 1.0 + 0.125 * q;
            hr[q] = 1.0 - q / 1024.0;
            lat += hl[q];
        }
        free(buf);  /* a fresh buffer: every growth step from the first 64 bytes */
        buf = NULL; cap = 0;
        k = shd_topology_route_line(&buf, &cap, names, v, LONG_HOPS + 1, hl, hr, lat, 0.25, 0);
        if (k < 0 || cap < (size_t)k + 1 || cap < 4096) return 3;
        printf("%s\n", buf);
        for (int q = 0; q <= LONG_HOPS; q++) free(names[q]);
        free(names); free(v); free(hl); free(hr);
    }
    /* 4: the [s, s] self entry (one self-loop hop), into the grown buffer */
    {
        const int32_t v[2] = { 5, 5 };
        const double hl[1] = { 7.0 }, hr[1] = { 0.75 };
        k = shd_topology_route_line(&buf, &cap, NULL, v, 2, hl, hr, 7.0, 0.75, 0);
        if (k < 0) return 4;
        printf("%s\n", buf);
    }
    /* bad arguments are refused */
    if (shd_topology_route_line(&buf, &cap, NULL, NULL, 2, NULL, NULL, 0, 0, 0) != -1) return 5;
    free(buf);
    return 0;
}
