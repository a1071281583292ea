/* Stand-alone driver of shadow_amd/csrc/link_fmt.c for tests/test_loads.py: formats four
 * link lines and prints one line each.  Built with the host sanitizers and run as its own
 * process; the expected strings are rebuilt in Python from the same formulas. */
#include <stdio.h>
#include <stdlib.h>

#include "../include/shd_topology.h"

#define NAMES 12

int main(void) {
    char* buf = NULL;
    size_t cap = 0;
    int64_t k;

    /* 1: undirected, decimal vertex names */
    k = shd_topology_link_line(&buf, &cap, NULL, 7, 3, 17, 12.0, 0.01, 42, 0);
    if (k < 0 || cap < (size_t)k + 1) return 1;
    printf("%s\n", buf);
    /* 2: directed, graphml ids, one id missing (the decimal index stands in) */
    {
        char* names[4] = { "poi-1", "poi-2", NULL, "poi-9" };
        k = shd_topology_link_line(&buf, &cap, names, 0, 3, 2, 20.25, 0.125, 1, 1);
        if (k < 0) return 2;
        printf("%s\n", buf);
    }
    /* 3: 40-character names and a packet count above 2^32, into a fresh buffer: every growth
     * step from the first 64 bytes */
    {
        char* names[NAMES];
        for (int q = 0; q < NAMES; q++) {
            names[q] = malloc(41);
            snprintf(names[q], 41, "vertex-%033d", q);
        }
        free(buf);
        buf = NULL; cap = 0;
        k = shd_topology_link_line(&buf, &cap, names, 2147483647, 11, 4, 1.5, 0.0, (1ull << 40) + 3, 0);
        if (k < 0 || cap < (size_t)k + 1 || cap < 128) return 3;
        printf("%s\n", buf);
        for (int q = 0; q < NAMES; q++) free(names[q]);
    }
    /* 4: a self-loop and the largest count, into the grown buffer */
    k = shd_topology_link_line(&buf, &cap, NULL, 5, 9, 9, 7.0, 0.75, 18446744073709551615ull, 0);
    if (k < 0) return 4;
    printf("%s\n", buf);
    /* bad arguments are refused */
    if (shd_topology_link_line(NULL, &cap, NULL, 0, 0, 0, 0, 0, 0, 0) != -1) return 5;
    if (shd_topology_link_line(&buf, &cap, NULL, -1, 0, 0, 0, 0, 0, 0) != -1) return 6;
    free(buf);
    return 0;
}
