// A job with a mapped column (UnitCol::map, pccm_reduce_map_*) has no lean kernel: for every stride / cfg / defer of kLeanShapes
// (open_pcc_metric_amd/csrc/pccm_reduce_shape.h) the job of that shape keeps its row while its maps are 0, and goes to the general
// kernel -- the only one that applies a map -- with any nonzero map on a column it reduces.  One line per job, read by
// tests/test_chamfer_host.py.  Host code only; built with the host sanitizers and run as a process of its own.
#include <cstdio>

#include "pccm_reduce_shape.h"

using namespace pccm;

static UnitJob job_of(const ReduceShape &s)
{
    UnitJob J = {};
    J.stride = s.stride;
    J.defer = s.defer;
    J.ncols = s.cfg == 0 ? 2 : 1;
    if (s.cfg == 0) {
        J.c[1].off = 1;
        J.c[1].square = 1;
    } else if (s.cfg == 2) {
        J.c[0].off = 1;
        J.c[0].square = 1;
    }
    if (J.ncols == 1) J.c[1] = J.c[0];      // (as slot_prepare fills a one-column job)
    return J;
}

int main()
{
    int bad = 0, lines = 0;
    for (int row = 0; row < kLeanCount; ++row) {
        const ReduceShape s = kLeanShapes[row];
        for (int m0 = 0; m0 <= 3; ++m0)
            for (int m1 = 0; m1 <= 3; ++m1) {
                UnitJob J = job_of(s);
                J.c[0].map = m0;
                J.c[0].cap = 0.25;
                J.c[1].map = m1;
                J.c[1].cap = 4.0;
                const bool reduced1 = J.ncols == 2;            // column 1 of a one-column job is not reduced: its map is not read
                const bool mapped = m0 != 0 || (reduced1 && m1 != 0);
                const int got = lean_index(reduce_shape(J)), want = mapped ? -1 : row;
                printf("stride %d cfg %d defer %d maps %d %d: %s\n", s.stride, s.cfg, s.defer, m0, m1,
                       got < 0 ? "general" : got == row ? "lean" : "another row");
                bad += got != want;
                ++lines;
            }
    }
    static_assert(sizeof(UnitJobs) <= 4096, "UnitJobs must fit the kernel-argument limit");
    printf("sizeof(UnitJobs) %zu\n", sizeof(UnitJobs));
    return bad == 0 && lines == 16 * kLeanCount ? 0 : 1;
}
