// The workspace of pccm_voxel_occupancy (occupancy_layout, open_pcc_metric_amd/csrc/pccm_internal.h) for clouds of n1 and n2 rows:
// the table's capacity is a power of two, at least 64 and at least 2 (n1 + n2) -- the probe sequences end on an empty slot --;
// the table, the seen words and the three 64-bit tallies follow one another without overlap inside the total; the tallies lie
// on an 8-byte boundary; and the part one memset clears (seen and the tallies) is exactly what lies behind the table.  One line
// per pair of sizes, read by tests/test_occupancy_host.py.  Host code only; built with the host sanitizers and run as a process
// of its own.
#include <cstdio>

#include "pccm_internal.h"

using namespace pccm;

static bool check(int64_t n1, int64_t n2)
{
    const OccupancyLayout L = occupancy_layout(n1, n2);
    const uint64_t n = (uint64_t)n1 + (uint64_t)n2;
    bool ok = true;
    ok = ok && L.cap >= 64 && (L.cap & (L.cap - 1)) == 0;                          // a power of two, with its floor
    ok = ok && L.cap >= 2 * n && (L.cap == 64 || L.cap / 2 < 2 * n);               // the smallest that holds 2 (n1 + n2)
    ok = ok && L.table == 0 && L.table + L.cap <= L.seen;                          // table | seen
    ok = ok && L.seen + (uint64_t)n1 <= L.tally;                                   // seen | tallies
    ok = ok && L.tally - (L.seen + (uint64_t)n1) <= 1;                             // (at most the one word of padding)
    ok = ok && (L.tally * sizeof(uint32_t)) % 8 == 0;                              // 64-bit atomics need their alignment
    ok = ok && L.tally + 3 * (sizeof(unsigned long long) / sizeof(uint32_t)) == L.words;
    ok = ok && L.bytes() == L.words * sizeof(uint32_t) && L.bytes() % 8 == 0;      // (what follows the layout stays aligned)
    printf("n1 %lld n2 %lld: cap %llu seen %zu tally %zu words %zu %s\n", (long long)n1, (long long)n2, (unsigned long long)L.cap,
           L.seen, L.tally, L.words, ok ? "ok" : "bad");
    return ok;
}

int main()
{
    const int64_t sizes[5] = {1, 63, 64, 65, 1000};
    int bad = 0, lines = 0;
    for (int64_t n1 : sizes)
        for (int64_t n2 : sizes) {
            bad += !check(n1, n2);
            ++lines;
        }
    // the largest clouds the entry point takes: n1 + n2 = 2^32 - 2 rows (0xffffffff is the empty slot), and uneven neighbours
    const int64_t half = (int64_t)1 << 31;
    bad += !check(half - 1, half - 1);
    bad += !check(half - 2, half - 1);
    bad += !check(half + 5, half - 7);
    lines += 3;
    printf("kOccupancyMax %d\n", kOccupancyMax);
    return bad == 0 && lines == 28 ? 0 : 1;
}
