// A job with a density map (PCCM_MAP_DENSITY, pccm_reduce_density_*) has no lean kernel: for every stride / cfg / defer of
// kLeanShapes (open_pcc_metric_amd/csrc/pccm_reduce_shape.h) the job of that shape keeps its row while its maps are 0, and goes
// to the general kernel -- the only one that gathers the match counts -- with the density map, with or without the root in front
// of it, on a column it reduces.  Also: the density map's slot key is its alpha, and a job with the rows' source and the counts
// still fits the kernel arguments.  One line per job, read by tests/test_dcd_host.py.  Host code only; built with the host
// sanitizers and run as a process of its own.
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
    static const uint32_t counts[4] = {1, 1, 1, 1};
    static const int32_t rows[4] = {0, 1, 2, 3};
    const int maps[3] = {0, PCCM_MAP_DENSITY, PCCM_MAP_DENSITY | PCCM_MAP_ROOT};
    int bad = 0, lines = 0;
    for (int row = 0; row < kLeanCount; ++row) {
        const ReduceShape s = kLeanShapes[row];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                UnitJob J = job_of(s);
                J.c[0].map = maps[a];
                J.c[0].alpha = 40.0;
                J.c[1].map = maps[b];
                J.c[1].alpha = 5.0;
                J.rows = s.stride == 1 ? rows : nullptr;
                J.cnt = counts;
                J.cnt_rows = 4;
                const bool reduced1 = J.ncols == 2;            // column 1 of a one-column job is not reduced: its map is not read
                const bool mapped = maps[a] != 0 || (reduced1 && maps[b] != 0);
                const int got = lean_index(reduce_shape(J)), want = mapped ? -1 : row;
                printf("stride %d cfg %d defer %d maps %d %d: %s\n", s.stride, s.cfg, s.defer, maps[a], maps[b],
                       got < 0 ? "general" : got == row ? "lean" : "another row");
                bad += got != want;
                ++lines;
            }
    }
    // the slot key of a density map is the bit pattern of its alpha; the root bit is part of the map, so the squared and the
    // unsquared request at one alpha are two slots; a plain root still has no second key word
    const bool keys = map_cap_bits(PCCM_MAP_DENSITY, 40.0) != map_cap_bits(PCCM_MAP_DENSITY, 5.0) &&
                      map_cap_bits(PCCM_MAP_DENSITY, 40.0) == map_cap_bits(PCCM_MAP_DENSITY | PCCM_MAP_ROOT, 40.0) &&
                      map_cap_bits(PCCM_MAP_DENSITY, 0.0) == 0 && map_cap_bits(PCCM_MAP_ROOT, 40.0) == 0 &&
                      map_cap_bits(PCCM_MAP_CLAMP, 0.25) != 0;
    printf("keys %s\n", keys ? "ok" : "bad");
    static_assert(sizeof(UnitJobs) <= 4096, "UnitJobs must fit the kernel-argument limit");
    printf("sizeof(UnitJobs) %zu\n", sizeof(UnitJobs));
    return bad == 0 && keys && lines == 9 * kLeanCount ? 0 : 1;
}
