/* Stand-alone driver of shadow_amd/csrc/tie_fmt.c for tests/test_ties.py: formats four tie
 * lines and two summary lines and prints one line each.  Built with the host sanitizers and
 * run as its own process; the expected strings are literals in the test. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/shd_topology.h"

#define NAMES 12

int main(void) {
    char* buf = NULL;
    size_t cap = 0;
    int64_t k;

    /* 1: undirected, decimal vertex names */
    k = shd_topology_tie_line(&buf, &cap, NULL, 3, 17, 2, 0.5, 0.75, 0);
    if (k < 0 || cap < (size_t)k + 1) return 1;
    printf("%s\n", buf);
    /* 2: directed, graphml ids, one id missing (the decimal index stands in) */
    {
        char* names[4] = { "poi-1", "poi-2", NULL, "poi-9" };
        k = shd_topology_tie_line(&buf, &cap, names, 3, 2, 6, 0.98999999999999999, 0.99, 1);
        if (k < 0) return 2;
        printf("%s\n", buf);
    }
    /* 3: 40-character names and a saturated count, into a fresh buffer: every growth step
     * from the first 64 bytes */
    {
        char* names[NAMES];
        for (int q = 0; q < NAMES; q++) {
            names[q] = malloc(41);
            snprintf(names[q], 41, "vertex-%033d", q);
        }
        free(buf);
        buf = NULL; cap = 0;
        k = shd_topology_tie_line(&buf, &cap, names, 11, 4, 18446744073709551615ull, 0.125, 0.25, 0);
        if (k < 0 || cap < (size_t)k + 1 || cap < 128) return 3;
        printf("%s\n", buf);
        for (int q = 0; q < NAMES; q++) free(names[q]);
    }
    /* 4: both bounds zero (no spread to divide), into the grown buffer */
    k = shd_topology_tie_line(&buf, &cap, NULL, 0, 1, 3, 0.0, 0.0, 0);
    if (k < 0) return 4;
    printf("%s\n", buf);
    /* 5, 6: the summary, with a worst pair and without one */
    {
        shd_tie_stats_t st;
        memset(&st, 0, sizeof st);
        st.pairs = 4950; st.tied = 321; st.sensitive = 17; st.saturated = 1; st.max_spread = 0.25;
        st.worst_src = 5; st.worst_dst = 77; st.worst_count = 18446744073709551615ull; st.worst_lo = 0.75; st.worst_hi = 1.0;
        k = shd_topology_tie_summary_line(&buf, &cap, &st, 0);
        if (k < 0) return 5;
        printf("%s\n", buf);
        memset(&st, 0, sizeof st);
        st.pairs = 276; st.worst_src = st.worst_dst = -1;
        free(buf);
        buf = NULL; cap = 0;
        k = shd_topology_tie_summary_line(&buf, &cap, &st, 1);
        if (k < 0 || cap < (size_t)k + 1) return 6;
        printf("%s\n", buf);
    }
    /* bad arguments are refused */
    if (shd_topology_tie_line(NULL, &cap, NULL, 0, 0, 0, 0, 0, 0) != -1) return 7;
    if (shd_topology_tie_line(&buf, &cap, NULL, -1, 0, 0, 0, 0, 0) != -1) return 8;
    if (shd_topology_tie_summary_line(&buf, &cap, NULL, 0) != -1) return 9;
    free(buf);
    return 0;
}
