// Host check of the filed tails' capture rule (open_pcc_metric_amd/csrc/pccm_tail_wave.h, its host half: no GPU, no HIP call;
// tests/test_tailfile_host.py builds it with the host sanitizers and runs it).  The binning of a tail list by blocks of 4096 rows
// against a count made here another way, and tail_filing_allowed on the facts that decide it: a flagged query, a block one over
// the capacity, the switch, a direction that was not searched.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <vector>

#include "pccm_tail_wave.h"

using namespace pccm;

static int g_failed = 0, g_checked = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        ++g_checked;                                                   \
        if (!(cond)) {                                                 \
            ++g_failed;                                                \
            printf("FAILED line %d: %s\n", __LINE__, #cond);          \
        }                                                              \
    } while (0)

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t next_u64()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return g_state;
}

static TailFacts facts(bool searched, int64_t flagged, int64_t block_max)
{
    TailFacts f;
    f.searched = searched;
    f.flagged = flagged;
    f.block_max = block_max;
    return f;
}

int main()
{
    static_assert(kTailBlockShift == 12 && kTailBlockCap == 32, "a block is one reduction workgroup's 4096 rows; its list holds 32 queries");

    // ---- binning -----------------------------------------------------------------------------------------------------------
    for (int64_t nrows : {1ll, 4095ll, 4096ll, 4097ll, 60000ll, 50000ll, 1000000ll}) {
        const int64_t nblocks = (nrows + 4095) / 4096;
        for (int rep = 0; rep < 4; ++rep) {
            const int64_t n = rep == 0 ? 0 : (int64_t)(next_u64() % (uint64_t)(nrows < 3000 ? nrows + 1 : 3000));
            std::vector<int32_t> rows((size_t)n);
            std::map<int64_t, int64_t> by_block;
            int64_t want = 0;
            for (auto &r : rows) {
                r = (int32_t)(next_u64() % (uint64_t)nrows);
                want = ++by_block[r / 4096] > want ? by_block[r / 4096] : want;
            }
            std::vector<int64_t> per;
            EXPECT(tail_block_max(rows.data(), n, nrows, &per) == want);
            EXPECT(tail_block_max(rows.data(), n, nrows) == want);
            EXPECT((int64_t)per.size() == nblocks);
            int64_t total = 0;
            for (int64_t b = 0; b < nblocks; ++b) {
                EXPECT(per[(size_t)b] == (by_block.count(b) ? by_block[b] : 0));
                total += per[(size_t)b];
            }
            EXPECT(total == n);
        }
    }
    {   // the first row, and the last row of a partial last block
        const int32_t rows[] = {0, 59999, 59999 - 4096, 57344, 57343};
        std::vector<int64_t> per;
        EXPECT(tail_block_max(rows, 5, 60000, &per) == 2);
        EXPECT(per.size() == 15 && per[0] == 1 && per[14] == 2 && per[13] == 2);
        EXPECT(tail_block_max(rows, 0, 60000, &per) == 0);
    }
    {   // rows that are not the shard's
        const int32_t over[] = {5, 60000}, under[] = {-1};
        EXPECT(tail_block_max(over, 2, 60000) == -1);
        EXPECT(tail_block_max(over, 1, 60000) == 1);
        EXPECT(tail_block_max(under, 1, 60000) == -1);
    }
    {   // one block with exactly the capacity, then one more
        std::vector<int32_t> rows;
        for (int k = 0; k < kTailBlockCap; ++k) rows.push_back(3 * 4096 + 17 * k);
        rows.push_back(4 * 4096);
        EXPECT(tail_block_max(rows.data(), (int64_t)rows.size(), 60000) == kTailBlockCap);
        rows.push_back(3 * 4096 + 4095);
        EXPECT(tail_block_max(rows.data(), (int64_t)rows.size(), 60000) == kTailBlockCap + 1);
    }

    // ---- the rule ------------------------------------------------------------------------------------------------------------
    {
        const TailFacts ok[2] = {facts(true, 0, 5), facts(true, 0, kTailBlockCap)};
        EXPECT(tail_filing_allowed(ok, 2, true));
        EXPECT(!tail_filing_allowed(ok, 2, false));                      // PCCM_TAIL_FILED=0
        const TailFacts over[2] = {facts(true, 0, 5), facts(true, 0, kTailBlockCap + 1)};
        EXPECT(!tail_filing_allowed(over, 2, true));
        const TailFacts over0[2] = {facts(true, 0, kTailBlockCap + 1), facts(true, 0, 0)};
        EXPECT(!tail_filing_allowed(over0, 2, true));
        const TailFacts flagged[2] = {facts(true, 1, 5), facts(true, 0, 5)};
        EXPECT(!tail_filing_allowed(flagged, 2, true));
        const TailFacts flagged1[2] = {facts(true, 0, 5), facts(true, 1, 5)};
        EXPECT(!tail_filing_allowed(flagged1, 2, true));
        const TailFacts foreign[2] = {facts(true, 0, -1), facts(true, 0, 5)};   // a list with rows of another shard
        EXPECT(!tail_filing_allowed(foreign, 2, true));
        const TailFacts none[2] = {facts(false, 0, 0), facts(false, 0, 0)};
        EXPECT(!tail_filing_allowed(none, 2, true));
        // a direction that was not searched has no say in the rule: its stale counts are not looked at (and a capture that
        // searches it all the same files nothing: pccm_ctx::TailFile::fact_dirs, tests/test_gpu_tail_filed.py)
        const TailFacts one[2] = {facts(true, 0, 0), facts(false, 7, 99)};
        EXPECT(tail_filing_allowed(one, 2, true));
        const TailFacts empty[2] = {facts(true, 0, 0), facts(true, 0, 0)};      // no tails at all: nothing to settle, nothing to launch
        EXPECT(tail_filing_allowed(empty, 2, true));
    }
    if (g_failed) {
        printf("tailfile host: %d of %d checks FAILED\n", g_failed, g_checked);
        return 1;
    }
    printf("tailfile host ok: %d checks\n", g_checked);
    return 0;
}
