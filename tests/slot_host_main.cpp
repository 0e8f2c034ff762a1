// Host check of open_pcc_metric_amd/csrc/pccm_slot.h and the slot structs of pccm_internal.h (tests/test_slot_host.py builds and
// runs it; no GPU, no HIP call).  slot_host COLUMN N WORLD...: COLUMN holds N raw little-endian float64 values.  For every WORLD
// the ranks' rows come from shard_of, each rank's pinned host buffer is filled through SlotView with what the reduction kernels
// would leave there, and the consumers' answers are printed as bit patterns; the caller compares them with NumPy.  What needs no
// NumPy is asserted here.  Linked against libpccm.so for the public finishers and lengths.
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

#include "pccm_internal.h"

using namespace pccm;

static int g_failed = 0, g_checked = 0;
static char g_case[96] = "";
#define EXPECT(cond)                                                              \
    do {                                                                          \
        ++g_checked;                                                              \
        if (!(cond)) {                                                            \
            ++g_failed;                                                           \
            printf("FAILED [%s] line %d: %s\n", g_case, __LINE__, #cond);        \
        }                                                                         \
    } while (0)

static unsigned long long bits(double x)
{
    unsigned long long u;
    memcpy(&u, &x, sizeof(u));
    return u;
}

// what k_unit_jobs leaves in a slot's host buffer for rows [s.begin, s.end) of col
static void kernel_fill(const SlotShape &s, const SlotView &v, const double *col)
{
    for (int64_t u = 0; u < s.nunits; ++u) {
        const int64_t r0 = s.begin + u * kLeaf, cnt = s.end - r0 < kLeaf ? s.end - r0 : kLeaf;
        double mm[2];
        fold_minmax(col + r0, col + r0, cnt, mm);
        v.usum[u] = np_pairwise_sum(col + r0, cnt);
        v.umin[u] = mm[0];
        v.umax[u] = mm[1];
    }
    for (int64_t b = 0; b < s.nblocks; ++b) {
        const int64_t u0 = b * kLeavesPerBlock, cnt = s.nunits - u0 < kLeavesPerBlock ? s.nunits - u0 : kLeavesPerBlock;
        const bool whole = cnt == kLeavesPerBlock && s.begin + (u0 + cnt) * kLeaf <= s.end;
        // a partial last block: only its min / max are ever read
        v.bsum[b] = whole ? leaf_tree(v.usum + u0, kLeavesPerBlock) : std::numeric_limits<double>::quiet_NaN();
        double mm[2];
        fold_minmax(v.umin + u0, v.umax + u0, cnt, mm);
        v.bmin[b] = mm[0];
        v.bmax[b] = mm[1];
    }
    for (int64_t k = 0; k < s.tail_n; ++k) v.tail[k] = col[s.t0 + k];
}

static void run_world(const std::vector<double> &col, int world)
{
    const int64_t n = (int64_t)col.size();
    snprintf(g_case, sizeof(g_case), "n %lld, world %d", (long long)n, world);
    std::vector<SlotShape> shape;
    std::vector<std::vector<double>> host;
    int64_t at = 0;
    bool all_aligned = true;
    for (int r = 0; r < world; ++r) {
        int64_t b, e;
        shard_of(n, r, world, &b, &e);
        // (a) the ranks' rows tile [0, n): a rank without rows may say [0, 0) or [n, n)
        EXPECT(b <= e && (b == e || b == at));
        if (e > b) at = e;
        const SlotShape s = slot_shape(n, b, e);
        EXPECT(s.n_iter == n && s.begin == b && s.end == e && s.ns == e - b);
        EXPECT(s.nunits == (s.ns + kLeaf - 1) / kLeaf && s.nblocks == (s.nunits + 31) / 32);
        EXPECT(s.tail_n >= 0 && s.tail_n <= s.ns && (s.tail_n == 0 || (s.t0 >= b && s.t0 + s.tail_n == e && s.t0 >= s.full_rows())));
        EXPECT(b % kLeaf == 0);
        all_aligned = all_aligned && s.chunk_aligned();
        // (c) the seven regions: in order, back to back, ending one double before the buffer does
        host.emplace_back((size_t)s.host_doubles(), 0.0);
        double *h = host.back().data();
        const SlotView v(s, h);
        EXPECT(v.usum == h && v.umin == v.usum + s.nunits && v.umax == v.umin + s.nunits && v.bsum == v.umax + s.nunits);
        EXPECT(v.bmin == v.bsum + s.nblocks && v.bmax == v.bmin + s.nblocks && v.tail == v.bmax + s.nblocks);
        EXPECT(v.tail + s.tail_n == h + s.host_doubles() - 1);
        // (d) the lengths are the public functions'
        EXPECT(s.xvec_len() == pccm_xvec_len(n) && s.cvec_len() == pccm_cvec_len(n));
        // the kernels are told the same shape, and the same places
        UnitJob U;
        UnitCol c;
        bind_shape(U, s);
        bind_outputs(c, v, false);
        EXPECT(U.ns == s.ns && U.nunits == s.nunits && U.nblocks == s.nblocks && U.tail_first == s.t0 - b && U.tail_n == s.tail_n);
        EXPECT(c.out_units == nullptr && c.out_blocks == v.bsum && c.out_tail == v.tail);
        bind_outputs(c, v, true);
        EXPECT(c.out_units == v.usum);
        kernel_fill(s, v, col.data());
        shape.push_back(s);
    }
    EXPECT(at == n);
    // (b) every rank has whole chunks exactly when there are as many chunks as ranks -- or when one rank owns the column from its
    // first row to its last: there is one rank, or one leaf
    EXPECT(all_aligned == (n >= (int64_t)world * kChunk || world == 1 || n <= kLeaf));
    printf("world %d aligned %d\n", world, all_aligned ? 1 : 0);

    double sum = 0.0, mm[2], fold[2] = {INFINITY, -INFINITY};
    if (world == 1) {
        double out[3];
        slot_total(shape[0], SlotView(shape[0], host[0].data()), out);
        printf("world %d total %016llx %016llx %016llx\n", world, bits(out[0]), bits(out[1]), bits(out[2]));
    }
    if (all_aligned) {
        std::vector<double> acc((size_t)pccm_cvec_len(n) + 1, 0.0), part(acc.size());
        for (int r = 0; r < world; ++r) {
            slot_fill_cvec(shape[r], SlotView(shape[r], host[r].data()), part.data(), mm);
            for (int64_t k = 0; k < shape[r].cvec_len(); ++k) acc[k] += part[k];
        }
        EXPECT(pccm_finish_chunks(acc.data(), n, &sum) == PCCM_OK);
        printf("world %d chunks %016llx\n", world, bits(sum));
    }
    std::vector<double> acc((size_t)pccm_xvec_len(n) + 1, 0.0), part(acc.size());
    for (int r = 0; r < world; ++r) {
        slot_fill_xvec(shape[r], SlotView(shape[r], host[r].data()), part.data(), mm);
        for (int64_t k = 0; k < shape[r].xvec_len(); ++k) acc[k] += part[k];
        fold[0] = mm[0] < fold[0] ? mm[0] : fold[0];
        fold[1] = mm[1] > fold[1] ? mm[1] : fold[1];
    }
    EXPECT(pccm_finish_sum(acc.data(), n, &sum) == PCCM_OK);
    printf("world %d leaves %016llx\n", world, bits(sum));
    printf("world %d minmax %016llx %016llx\n", world, bits(fold[0]), bits(fold[1]));
}

// (e) the free-slot policy, over keys alone: generation 5 is current for every direction
static void test_pick_free()
{
    snprintf(g_case, sizeof(g_case), "pick_free");
    const uint64_t gen[3] = {5, 5, 5};
    auto live = [] { SlotKey k; k.pending = true; k.gen = 5; return k; };
    auto stale = [] { SlotKey k; k.pending = true; k.gen = 4; return k; };
    SlotKey *const *none = nullptr;
    {
        SlotKey s[4] = {live(), stale(), SlotKey(), live()};              // an idle slot before a stale one, wherever they are
        EXPECT(pick_free(s, none, 0, gen) == &s[2]);
        s[2] = live();                                                    // a stale one before a live one
        EXPECT(pick_free(s, none, 0, gen) == &s[1]);
        s[1].dir = 2;                                                     // (stale by ITS direction's generation: here it is not)
        s[3] = stale();
        const uint64_t gen2[3] = {5, 5, 4};
        EXPECT(pick_free(s, none, 0, gen2) == &s[3]);
    }
    {
        SlotKey s[3] = {live(), live(), live()};                          // all live: never a member of the batch being assembled
        SlotKey *fresh[3] = {&s[0], &s[2], &s[1]};
        EXPECT(pick_free(s, fresh, 0, gen) == &s[0]);
        EXPECT(pick_free(s, fresh, 1, gen) == &s[1]);
        EXPECT(pick_free(s, fresh, 2, gen) == &s[1]);
        EXPECT(pick_free(s, fresh, 3, gen) == nullptr);                   // ... and null when every slot is
    }
    {
        SelectSlot q[2];                                                  // the same template serves both slot types
        q[0].pending = true; q[0].gen = 5;
        SelectSlot *const *no_sel = nullptr;
        EXPECT(pick_free(q, no_sel, 0, gen) == &q[1]);
        ReduceSlot r[2];
        r[0].pending = true; r[0].gen = 5;
        r[1].pending = true; r[1].gen = 5;
        ReduceSlot *fresh[1] = {&r[0]};
        EXPECT(pick_free(r, fresh, 1, gen) == &r[1]);
    }
    // one comparison finds both kinds of slot: the mode only where it enters the column; units / rank on top
    ReduceSlot r;
    r.pending = true; r.dir = 1; r.metric = PCCM_METRIC_D1; r.mode = PCCM_NORMAL_ROW; r.gen = 5;
    EXPECT(r.matches(1, PCCM_METRIC_D1, PCCM_NORMAL_NEIGHBOUR, 5, false) && !r.matches(1, PCCM_METRIC_D1, PCCM_NORMAL_ROW, 5, true));
    EXPECT(!r.matches(0, PCCM_METRIC_D1, PCCM_NORMAL_ROW, 5, false) && !r.matches(1, PCCM_METRIC_D1, PCCM_NORMAL_ROW, 6, false));
    r.metric = PCCM_METRIC_D2;
    r.has_units = true;
    EXPECT(r.matches(1, PCCM_METRIC_D2, PCCM_NORMAL_ROW, 5, true) && !r.matches(1, PCCM_METRIC_D2, PCCM_NORMAL_NEIGHBOUR, 5, true));
    r.pending = false;
    EXPECT(!r.matches(1, PCCM_METRIC_D2, PCCM_NORMAL_ROW, 5, false));
    SelectSlot q;
    q.pending = true; q.metric = PCCM_METRIC_D1; q.gen = 5; q.k = 9;
    EXPECT(q.matches(0, PCCM_METRIC_D1, PCCM_NORMAL_NEIGHBOUR, 5, 9) && !q.matches(0, PCCM_METRIC_D1, PCCM_NORMAL_ROW, 5, 8));
}

// (f) a replay puts back everything that describes the reduction and nothing the slot owns
static void test_restore()
{
    snprintf(g_case, sizeof(g_case), "restore");
    static double buf_a[4], buf_b[4], dev_a[4], dev_b[4];
    ReduceSlot was;                                                       // the slot at capture time
    was.pending = true; was.dir = 1; was.metric = PCCM_METRIC_D2; was.mode = PCCM_NORMAL_NEIGHBOUR; was.gen = 11;
    was.wait_ev = (hipEvent_t)buf_a; was.wait_seq = 3;
    static_cast<SlotShape &>(was) = slot_shape(28673, 8192, 28673);
    was.has_units = was.has_job = true;
    memset(&was.job, 0, sizeof(was.job));
    was.job.val = dev_a; was.job.stride = 2; was.job.ncols = 1;
    bind_shape(was.job, was);
    was.val.p = dev_a; was.val.bytes = 64; was.host = buf_a; was.host_cap = 32;
    const SlotSnap<ReduceWhat> snap = snapshot(was);

    ReduceSlot now;                                                       // the same slot later: another column, buffers regrown
    now.dir = 0; now.metric = PCCM_METRIC_D1; now.gen = 12; now.wait_ev = (hipEvent_t)buf_b; now.wait_seq = 40;
    static_cast<SlotShape &>(now) = slot_shape(1000, 0, 1000);
    memset(&now.job, 0, sizeof(now.job));
    now.job.val = dev_b; now.job.stride = 1;
    bind_shape(now.job, now);
    now.val.p = dev_b; now.val.bytes = 128; now.host = buf_b; now.host_cap = 4096;
    restore(now, snap);

    EXPECT(now.val.p == dev_b && now.val.bytes == 128 && now.host == buf_b && now.host_cap == 4096);
    EXPECT(now.pending && now.dir == 1 && now.metric == PCCM_METRIC_D2 && now.mode == PCCM_NORMAL_NEIGHBOUR && now.gen == 11);
    EXPECT(now.wait_ev == (hipEvent_t)buf_a && now.wait_seq == 3);
    EXPECT(now.n_iter == 28673 && now.begin == 8192 && now.end == 28673 && now.ns == 20481 && now.nunits == 161 && now.nblocks == 6);
    EXPECT(now.t0 == 24576 && now.tail_n == 4097 && now.has_units && now.has_job);
    EXPECT(now.job.val == dev_a && now.job.stride == 2 && now.job.ncols == 1 && now.job.ns == 20481 && now.job.nunits == 161);
    EXPECT(now.job.nblocks == 6 && now.job.tail_first == 16384 && now.job.tail_n == 4097);
    // every byte of the snapshot is one of the two parts: a field added to either travels without a line written for it
    static_assert(sizeof(SlotSnap<ReduceWhat>) == sizeof(SlotKey) + sizeof(ReduceWhat), "the snapshot is the key and the description");
    static_assert(sizeof(SlotSnap<SelectWhat>) == sizeof(SlotKey) + sizeof(SelectWhat), "... in the selection table");
    static_assert(sizeof(SlotSnap<MapWhat>) == sizeof(SlotKey) + sizeof(MapWhat), "... and in the mapped reductions'");

    pccm_ctx *ctx = new pccm_ctx();                                       // (plain host memory until something is allocated)
    ctx->batch_ev = (hipEvent_t)dev_a;
    ctx->batches_issued = 100;
    rearm(now, ctx, snap.key.wait_seq);
    EXPECT(now.wait_ev == (hipEvent_t)dev_a && now.wait_seq == 103);
    rearm(now, ctx, 0);                                                   // no counter: the event only
    EXPECT(now.wait_seq == 0);
    delete ctx;
}

// ... in the other two tables as well
static void test_restore_select_and_map()
{
    snprintf(g_case, sizeof(g_case), "restore select / map");
    static double buf_a[4], buf_b[4];
    SelectSlot qwas;
    qwas.pending = true; qwas.dir = 1; qwas.metric = PCCM_METRIC_D2; qwas.mode = PCCM_NORMAL_NEIGHBOUR; qwas.gen = 11;
    qwas.wait_ev = (hipEvent_t)buf_a; qwas.wait_seq = 3;
    qwas.kind = kSlotCount; qwas.k = 0x3ff0000000000000ll;
    const SlotSnap<SelectWhat> qsnap = snapshot(qwas);
    SelectSlot q;
    q.dir = 0; q.metric = PCCM_METRIC_D1; q.gen = 12; q.wait_ev = (hipEvent_t)buf_b; q.wait_seq = 40; q.kind = kSlotSelect; q.k = 7;
    restore(q, qsnap);
    EXPECT(q.pending && q.dir == 1 && q.metric == PCCM_METRIC_D2 && q.mode == PCCM_NORMAL_NEIGHBOUR && q.gen == 11);
    EXPECT(q.wait_ev == (hipEvent_t)buf_a && q.wait_seq == 3 && q.kind == kSlotCount && q.k == 0x3ff0000000000000ll);

    MapSlot mwas;
    mwas.pending = true; mwas.dir = 1; mwas.metric = PCCM_METRIC_D2; mwas.mode = PCCM_NORMAL_NEIGHBOUR; mwas.gen = 11;
    mwas.wait_ev = (hipEvent_t)buf_a; mwas.wait_seq = 3;
    mwas.shape = slot_shape(28673, 0, 28673);
    mwas.shape.nunits = 0;
    mwas.map = PCCM_MAP_CLAMP | PCCM_MAP_ROOT; mwas.cap_bits = map_cap_bits(mwas.map, 0.25);
    mwas.host = buf_a; mwas.host_cap = 32;
    const SlotSnap<MapWhat> map_snap = snapshot(mwas);
    MapSlot m;
    m.dir = 0; m.metric = PCCM_METRIC_D1; m.gen = 12; m.wait_ev = (hipEvent_t)buf_b; m.wait_seq = 40;
    m.shape = slot_shape(1000, 0, 1000);
    m.map = PCCM_MAP_ROOT; m.cap_bits = 0;
    m.host = buf_b; m.host_cap = 4096;
    restore(m, map_snap);
    EXPECT(m.host == buf_b && m.host_cap == 4096);
    EXPECT(m.pending && m.dir == 1 && m.metric == PCCM_METRIC_D2 && m.mode == PCCM_NORMAL_NEIGHBOUR && m.gen == 11);
    EXPECT(m.wait_ev == (hipEvent_t)buf_a && m.wait_seq == 3);
    EXPECT(m.shape.n_iter == 28673 && m.shape.begin == 0 && m.shape.end == 28673 && m.shape.ns == 28673 && m.shape.nunits == 0);
    EXPECT(m.shape.nblocks == 8 && m.shape.t0 == 24576 && m.shape.tail_n == 4097);
    EXPECT(m.map == (PCCM_MAP_CLAMP | PCCM_MAP_ROOT) && m.cap_bits == 0x3fd0000000000000ull);
}

// (g) one search finds the pending slot of a request in any table
static void test_find_pending()
{
    snprintf(g_case, sizeof(g_case), "find_pending");
    const uint64_t gen[3] = {5, 6, 7};
    const int ROW = PCCM_NORMAL_ROW, NB = PCCM_NORMAL_NEIGHBOUR, D1 = PCCM_METRIC_D1, D2 = PCCM_METRIC_D2;
    auto key = [](SlotKey &k, int dir, int metric, int mode, uint64_t g) { k.pending = true; k.dir = dir; k.metric = metric; k.mode = mode; k.gen = g; };
    {
        ReduceSlot r[4];
        key(r[0], 0, D1, ROW, 5);
        key(r[1], 1, D2, ROW, 6);
        key(r[2], 1, D2, NB, 6);
        r[2].has_units = true;
        key(r[3], 0, D2, ROW, 4);                                         // (of an earlier search)
        EXPECT(find_pending(r, gen, 0, D1, ROW) == &r[0] && find_pending(r, gen, 0, D1, NB) == &r[0]);      // D1 ignores the mode
        EXPECT(find_pending(r, gen, 1, D2, ROW) == &r[1] && find_pending(r, gen, 1, D2, NB) == &r[2]);      // D2 does not
        EXPECT(find_pending(r, gen, 1, D2, ROW, true) == nullptr && find_pending(r, gen, 1, D2, NB, true) == &r[2]);   // need_units
        EXPECT(find_pending(r, gen, 0, D1, ROW, true) == nullptr && find_pending(r, gen, 1, D1, ROW) == nullptr);
        EXPECT(find_pending(r, gen, 0, D2, ROW) == nullptr);              // stale by its direction's generation
        r[0].pending = false;
        EXPECT(find_pending(r, gen, 0, D1, ROW) == nullptr);
    }
    {
        SelectSlot q[3];
        key(q[0], 0, D1, ROW, 5); q[0].kind = kSlotSelect; q[0].k = 9;
        key(q[1], 0, D1, ROW, 5); q[1].kind = kSlotCount; q[1].k = 9;     // a count whose threshold has a rank's bits: another request
        key(q[2], 1, D2, NB, 6); q[2].kind = kSlotSelect; q[2].k = 9;
        EXPECT(find_pending(q, gen, 0, D1, NB, (int64_t)9) == &q[0] && find_pending(q, gen, 0, D1, NB, (int64_t)9, kSlotSelect) == &q[0]);
        EXPECT(find_pending(q, gen, 0, D1, ROW, (int64_t)9, kSlotCount) == &q[1] && find_pending(q, gen, 0, D1, ROW, (int64_t)8) == nullptr);
        EXPECT(find_pending(q, gen, 1, D2, NB, (int64_t)9) == &q[2] && find_pending(q, gen, 1, D2, ROW, (int64_t)9) == nullptr);
        EXPECT(find_pending(q, gen, 1, D2, NB, (int64_t)9, kSlotCount) == nullptr);
    }
    {
        const int CL = PCCM_MAP_CLAMP, RT = PCCM_MAP_ROOT;
        MapSlot m[4];
        key(m[0], 0, D1, ROW, 5); m[0].map = CL; m[0].cap_bits = map_cap_bits(CL, 0.0);
        key(m[1], 0, D1, ROW, 5); m[1].map = CL; m[1].cap_bits = map_cap_bits(CL, -0.0);
        key(m[2], 0, D1, ROW, 5); m[2].map = RT; m[2].cap_bits = map_cap_bits(RT, 3.0);
        key(m[3], 1, D2, NB, 6); m[3].map = CL | RT; m[3].cap_bits = map_cap_bits(CL | RT, 0.5);
        EXPECT(map_cap_bits(CL, 0.0) != map_cap_bits(CL, -0.0) && map_cap_bits(RT, 3.0) == 0 && map_cap_bits(RT, -1.0) == 0);
        EXPECT(find_pending(m, gen, 0, D1, NB, CL, map_cap_bits(CL, 0.0)) == &m[0]);          // 0.0 and -0.0: two keys
        EXPECT(find_pending(m, gen, 0, D1, NB, CL, map_cap_bits(CL, -0.0)) == &m[1]);
        EXPECT(find_pending(m, gen, 0, D1, ROW, RT, map_cap_bits(RT, 8.0)) == &m[2]);         // no clamp: the cap is no part of the key
        EXPECT(find_pending(m, gen, 0, D1, ROW, CL | RT, map_cap_bits(CL | RT, 0.0)) == nullptr);
        EXPECT(find_pending(m, gen, 1, D2, NB, CL | RT, map_cap_bits(CL | RT, 0.5)) == &m[3]);
        EXPECT(find_pending(m, gen, 1, D2, ROW, CL | RT, map_cap_bits(CL | RT, 0.5)) == nullptr);
        EXPECT(find_pending(m, gen, 1, D2, NB, CL | RT, map_cap_bits(CL | RT, 0.25)) == nullptr);
    }
}

// (h) which requests of a call are enqueued, and on which columns
struct Req {
    int dir, metric, mode;
    int64_t key;
    double x;                                                             // (maps: the cap)
};
static bool groups_are(const std::vector<Req> &reqs, bool maps, const std::vector<int> &enqueued, const std::vector<int> &todo,
                       const std::vector<int> &col_of, const std::vector<Req> &cols)
{
    int dirs[8], metrics[8], modes[8];
    int64_t key[8];
    uint64_t key2[8];
    const int n = (int)reqs.size();
    for (int i = 0; i < n; ++i) {
        dirs[i] = reqs[i].dir; metrics[i] = reqs[i].metric; modes[i] = reqs[i].mode; key[i] = reqs[i].key;
        key2[i] = map_cap_bits((int)reqs[i].key, reqs[i].x);
    }
    const RequestGroups g = group_requests(n, dirs, metrics, modes, key, maps ? key2 : nullptr, [&](int i) {
        for (int e : enqueued)
            if (e == i) return true;
        return false;
    });
    bool ok = g.ntodo == (int)todo.size() && g.ncols == (int)cols.size() && todo.size() == col_of.size();
    for (int j = 0; ok && j < g.ntodo; ++j) ok = g.todo[j] == todo[j] && g.col_of[j] == col_of[j];
    for (int c = 0; ok && c < g.ncols; ++c) ok = g.dir[c] == cols[c].dir && g.metric[c] == cols[c].metric && g.mode[c] == cols[c].mode;
    return ok;
}

static void test_group_requests()
{
    snprintf(g_case, sizeof(g_case), "group_requests");
    const int ROW = PCCM_NORMAL_ROW, NB = PCCM_NORMAL_NEIGHBOUR, D1 = PCCM_METRIC_D1, D2 = PCCM_METRIC_D2;
    const int CL = PCCM_MAP_CLAMP, RT = PCCM_MAP_ROOT;
    std::vector<Req> eight;
    for (int i = 0; i < 8; ++i) eight.push_back({0, D1, ROW, 10 + i, 0.0});
    EXPECT(groups_are(eight, false, {}, {0, 1, 2, 3, 4, 5, 6, 7}, {0, 0, 0, 0, 0, 0, 0, 0}, {{0, D1, ROW}}));          // eight on one column
    EXPECT(groups_are(eight, false, {0, 1, 2, 3, 4, 5, 6, 7}, {}, {}, {}));                                            // all enqueued already
    EXPECT(groups_are(eight, false, {0, 2, 7}, {1, 3, 4, 5, 6}, {0, 0, 0, 0, 0}, {{0, D1, ROW}}));
    EXPECT(groups_are({{1, D2, ROW, 5}, {1, D2, ROW, 5}}, false, {}, {0}, {0}, {{1, D2, ROW}}));                       // the same request twice
    EXPECT(groups_are({{0, D1, ROW, 5}, {0, D1, NB, 5}, {0, D1, NB, 6}}, false, {}, {0, 2}, {0, 0}, {{0, D1, ROW}}));  // D1: one column under two modes
    EXPECT(groups_are({{0, D2, ROW, 5}, {0, D2, NB, 5}, {0, D2, ROW, 6}}, false, {}, {0, 1, 2}, {0, 1, 0}, {{0, D2, ROW}, {0, D2, NB}}));   // D2: two
    EXPECT(groups_are({{1, D1, ROW, 1}, {0, D1, ROW, 1}, {1, D2, ROW, 1}, {0, D1, ROW, 2}, {1, D1, ROW, 2}, {0, D2, ROW, 1}}, false, {},
                      {0, 1, 2, 3, 4, 5}, {0, 1, 2, 1, 0, 3}, {{1, D1, ROW}, {0, D1, ROW}, {1, D2, ROW}, {0, D2, ROW}}));   // first-seen order
    EXPECT(groups_are({{1, D1, ROW, 1}, {0, D1, ROW, 1}, {1, D1, ROW, 2}}, false, {0}, {1, 2}, {0, 1}, {{0, D1, ROW}, {1, D1, ROW}}));
    // maps: the cap is part of the key exactly when the map clamps
    EXPECT(groups_are({{0, D1, ROW, CL, 0.5}, {0, D1, ROW, CL, 0.25}}, true, {}, {0, 1}, {0, 0}, {{0, D1, ROW}}));
    EXPECT(groups_are({{0, D1, ROW, CL, 0.0}, {0, D1, ROW, CL, -0.0}, {0, D1, ROW, CL, 0.0}}, true, {}, {0, 1}, {0, 0}, {{0, D1, ROW}}));
    EXPECT(groups_are({{0, D1, ROW, RT, 0.5}, {0, D1, ROW, RT, 0.25}}, true, {}, {0}, {0}, {{0, D1, ROW}}));
    EXPECT(groups_are({{0, D1, ROW, CL, 0.5}, {0, D1, ROW, CL | RT, 0.5}, {1, D1, NB, CL, 0.5}}, true, {}, {0, 1, 2}, {0, 0, 1},
                      {{0, D1, ROW}, {1, D1, NB}}));
}

int main(int argc, char **argv)
{
    if (argc < 4) {
        fprintf(stderr, "usage: %s COLUMN N WORLD...\n", argv[0]);
        return 2;
    }
    const int64_t n = atoll(argv[2]);
    std::vector<double> col((size_t)n);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(col.data(), sizeof(double), (size_t)n, f) != (size_t)n) {
        fprintf(stderr, "cannot read %lld doubles from %s\n", (long long)n, argv[1]);
        return 2;
    }
    fclose(f);
    for (int a = 3; a < argc; ++a) run_world(col, atoi(argv[a]));
    test_pick_free();
    test_restore();
    test_restore_select_and_map();
    test_find_pending();
    test_group_requests();
    printf("%d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
