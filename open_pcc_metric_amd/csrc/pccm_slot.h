// A reduction slot's shape, the layout of its pinned host buffer and NumPy's summation order over what the kernels leave there:
// each decided here and nowhere else ("A reduction slot: shape, host layout, summation order").  What the three slot
// tables (reductions, selections and counts, mapped reductions) share is here too: the key, the snapshot a captured graph keeps,
// the search for a pending slot, the grouping of a call's requests by column and the free-slot policy.  Host-only: no HIP call, no
// allocation; pccm_internal.h includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "pccm.h"

namespace pccm {

// ---- reduction geometry: NumPy's pairwise sum (numpy/_core/src/umath/loops_utils.h.src) --
constexpr int kLeaf = 128;          // PW_BLOCKSIZE
constexpr int kChunk = 8192;        // NumPy's default ufunc buffer size in elements
constexpr int kLeavesPerChunk = kChunk / kLeaf;
constexpr int kLeavesPerBlock = kLeavesPerChunk / 2;   // a block: the half-chunk tree the reduction kernels finish

// The rows [*b, *e) of an n-row iterating cloud that rank `rank` of `world` owns.
inline void shard_of(int64_t n, int rank, int world, int64_t *b, int64_t *e)
{
    if (world <= 0) {                     // this context owns no rows of the direction
        *b = 0;
        *e = 0;
        return;
    }
    // shards start on whole 8192-row chunks of NumPy's sum whenever every rank can have one (the ranks then exchange
    // one number per chunk: pccm_reduce_chunks_many), else on 128-row leaves (pccm_reduce's per-leaf exchange vector)
    const int64_t unit = n >= (int64_t)world * kChunk ? kChunk : kLeaf;
    const int64_t units = (n + unit - 1) / unit;
    int64_t u0 = units * rank / world, u1 = units * (rank + 1) / world;
    int64_t lo = u0 * unit, hi = u1 * unit;
    *b = lo < n ? lo : n;
    *e = hi < n ? hi : n;
}

// What a reduction over rows [begin, end) of an n_iter-row column leaves on the host: one result per 128-row leaf (nunits) and
// per 32-leaf block (nblocks), counted from `begin`, and the raw values of the rows that fall into the column's last, partial
// chunk (tail_n of them, from row t0).
struct SlotShape {
    int64_t n_iter = 0, begin = 0, end = 0, ns = 0, nunits = 0, nblocks = 0, t0 = 0, tail_n = 0;

    int64_t nfull() const { return n_iter / kChunk; }           // whole chunks of the column
    int64_t full_rows() const { return nfull() * kChunk; }
    // the rows start and end on whole chunks (a shard without rows does): the block results are chunk halves, so the ranks
    // exchange the chunk vector; otherwise the per-leaf vector, for which the per-leaf results must cross to the host
    bool chunk_aligned() const { return ns <= 0 || (begin % kChunk == 0 && (end % kChunk == 0 || end == n_iter)); }
    int64_t host_doubles() const { return 3 * nunits + 3 * nblocks + tail_n + 1; }
    // exchange vectors of the whole column: a number per leaf (xvec) or per chunk (cvec) of the full chunks, then the tail's rows
    int64_t xvec_len() const { return n_iter <= 0 ? 0 : nfull() * kLeavesPerChunk + n_iter % kChunk; }
    int64_t cvec_len() const { return n_iter <= 0 ? 0 : nfull() + n_iter % kChunk; }
};

inline SlotShape slot_shape(int64_t n_iter, int64_t begin, int64_t end)
{
    SlotShape s;
    s.n_iter = n_iter; s.begin = begin; s.end = end;
    s.ns = end - begin;
    s.nunits = s.ns > 0 ? (s.ns + kLeaf - 1) / kLeaf : 0;
    s.nblocks = (s.nunits + kLeavesPerBlock - 1) / kLeavesPerBlock;
    s.t0 = begin > s.full_rows() ? begin : s.full_rows();
    s.tail_n = s.t0 < end ? end - s.t0 : 0;
    return s;
}

// The pinned host buffer of a slot: [3][nunits] leaf sums / minima / maxima | [3][nblocks] block trees / minima / maxima |
// tail_n raw values (| one spare double).
struct SlotView {
    double *usum, *umin, *umax, *bsum, *bmin, *bmax, *tail;
    SlotView(const SlotShape &s, double *host)
        : usum(host), umin(usum + s.nunits), umax(umin + s.nunits), bsum(umax + s.nunits), bmin(bsum + s.nblocks),
          bmax(bmin + s.nblocks), tail(bmax + s.nblocks)
    {
    }
};

// NumPy's DOUBLE pairwise sum over one contiguous run of at most kChunk values.
inline double np_pairwise_sum(const double *a, int64_t n)
{
    if (n < 8) {
        double res = 0.0;
        for (int64_t i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= kLeaf) {
        double r[8];
        for (int k = 0; k < 8; ++k) r[k] = a[k];
        int64_t i;
        for (i = 8; i < n - (n % 8); i += 8)
            for (int k = 0; k < 8; ++k) r[k] += a[i + k];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

// ... and its tree over cnt (a power of two) finished leaves
inline double leaf_tree(const double *l, int cnt)
{
    if (cnt == 1) return l[0];
    return leaf_tree(l, cnt / 2) + leaf_tree(l + cnt / 2, cnt / 2);
}

// np.sum of a column: the full chunks one after the other (chunk_value(c): chunk c's pairwise sum), then the pairwise sum of
// the partial chunk's tail_n raw values; the first term is taken as it is, not added to 0.0
template <class ChunkValue>
inline double np_chunked_sum(int64_t nfull, ChunkValue chunk_value, const double *tail, int64_t tail_n)
{
    double s = 0.0;
    bool first = true;
    for (int64_t c = 0; c < nfull; ++c) {
        const double cs = chunk_value(c);
        s = first ? cs : s + cs;
        first = false;
    }
    if (tail_n > 0) {
        const double ts = np_pairwise_sum(tail, tail_n);
        s = first ? ts : s + ts;
    }
    return s;
}

inline void fold_minmax(const double *mins, const double *maxs, int64_t count, double minmax[2])
{
    double mn = INFINITY, mx = -INFINITY;
    for (int64_t k = 0; k < count; ++k) {
        mn = mins[k] < mn ? mins[k] : mn;
        mx = maxs[k] > mx ? maxs[k] : mx;
    }
    minmax[0] = mn;
    minmax[1] = mx;
}

// The whole column's {sum, min, max} (begin = 0, end = n_iter): each chunk = NumPy's pairwise tree = (tree of its first 32
// leaves) + (tree of its last 32 leaves), and the GPU already finished both halves.
inline void slot_total(const SlotShape &s, const SlotView &v, double out[3])
{
    out[0] = np_chunked_sum(s.nfull(), [&](int64_t c) { return v.bsum[2 * c] + v.bsum[2 * c + 1]; }, v.tail, s.tail_n);
    fold_minmax(v.bmin, v.bmax, s.nblocks, out + 1);
}

// The shard's part of the column's per-leaf vector [xvec_len()] (zero elsewhere) and its min / max; needs the per-leaf results.
inline void slot_fill_xvec(const SlotShape &s, const SlotView &v, double *xvec, double minmax[2])
{
    memset(xvec, 0, (size_t)s.xvec_len() * sizeof(double));
    for (int64_t u = 0; u < s.nunits; ++u) {
        const int64_t row = s.begin + u * kLeaf;    // shard boundaries are multiples of kLeaf
        if (row < s.full_rows()) xvec[row / kLeaf] = v.usum[u];
    }
    fold_minmax(v.umin, v.umax, s.nunits, minmax);
    if (s.tail_n > 0)   // raw values of the last, partial 8192-row chunk that fall into this shard
        memcpy(xvec + s.nfull() * kLeavesPerChunk + (s.t0 - s.full_rows()), v.tail, (size_t)s.tail_n * sizeof(double));
}

// The shard's part of the column's chunk vector [cvec_len()] (zero elsewhere) and its min / max: a number per full chunk the
// shard owns + the raw values of the partial chunk.  For chunk_aligned() shapes.
inline void slot_fill_cvec(const SlotShape &s, const SlotView &v, double *cvec, double minmax[2])
{
    memset(cvec, 0, (size_t)s.cvec_len() * sizeof(double));
    const int64_t c0 = s.begin / kChunk;
    const int64_t owned = s.ns > 0 ? ((s.end < s.full_rows() ? s.end : s.full_rows()) - s.begin) / kChunk : 0;
    for (int64_t c = 0; c < owned; ++c) cvec[c0 + c] = v.bsum[2 * c] + v.bsum[2 * c + 1];
    if (s.tail_n > 0) memcpy(cvec + s.nfull() + (s.t0 - s.full_rows()), v.tail, (size_t)s.tail_n * sizeof(double));
    fold_minmax(v.bmin, v.bmax, s.nblocks, minmax);
}

// ---- what the slot tables share ----------------------------------------------------------------------------------------------

// normal_mode enters the column: the projection on a normal of the searched cloud and its square, nothing else
inline bool normal_mode_enters(int metric) { return metric == PCCM_METRIC_D2 || metric == PCCM_METRIC_PROJ; }

struct SlotKey {                    // which column an enqueued result belongs to, and what says that it is on the host
    bool pending = false;
    int dir = 0, metric = 0, mode = 0;
    uint64_t gen = 0;               // nn generation of `dir` it was computed from
    hipEvent_t wait_ev = nullptr;   // the context's batch event (one record serves every slot of a call / of a graph replay;
                                    // waiting on a later record of it only waits longer)
    uint64_t wait_seq = 0;          // ... or, sooner, the context's completion counter reaching this value (0: the event only;
                                    // in a GraphOp's snapshot: the batch's ordinal within the captured sequence)

    bool matches(int d, int m, int normal_mode, uint64_t gen_now) const
    {
        return pending && dir == d && metric == m && (!normal_mode_enters(m) || mode == normal_mode) && gen == gen_now;
    }
};

// A slot of any table is three parts: SlotKey, a `What` struct (Slot::What, a base of the slot) that describes the enqueued result,
// and what the slot owns.  A captured graph keeps the first two -- whole, so a new field travels too -- and its replay puts them back.
template <class What>
struct SlotSnap {
    SlotKey key;
    What what;
};
template <class Slot>
inline SlotSnap<typename Slot::What> snapshot(const Slot &s) { return {s, s}; }
template <class Slot>
inline void restore(Slot &s, const SlotSnap<typename Slot::What> &snap)
{
    static_cast<SlotKey &>(s) = snap.key;
    static_cast<typename Slot::What &>(s) = snap.what;
}

// the pending slot of a table that answers a request (rest: what the table's matches() asks on top of the column), or null
template <class Slot, size_t N, class... Rest>
inline Slot *find_pending(Slot (&slots)[N], const uint64_t *nn_gen, int dir, int metric, int normal_mode, Rest... rest)
{
    for (auto &s : slots)
        if (s.matches(dir, metric, normal_mode, nn_gen[dir], rest...)) return &s;
    return nullptr;
}

// the cap of a mapped reduction as a slot key: its bit pattern (0.0 and -0.0 are two keys), and nothing where the map does not
// clamp; of a density map: the bit pattern of its alpha; of a moment map: of its inlier bound
inline uint64_t map_cap_bits(int map, double x)
{
    uint64_t b = 0;
    if (map & (PCCM_MAP_CLAMP | PCCM_MAP_DENSITY | PCCM_MAP_MOMENT)) memcpy(&b, &x, sizeof b);
    return b;
}

// Which of a call's n <= 8 requests it still has to enqueue, and the distinct columns they read, in first-seen order.  A request
// is a column (D1 ignores the normal mode) and a key (a selection's rank, the bits of a count's threshold, a map) of one word or,
// with key2, two (a map's cap bits).  Left out: what enqueued(i) says is pending, and a repeat of an earlier request of the call.
struct RequestGroups {
    int ntodo = 0, ncols = 0;
    int todo[8] = {}, col_of[8] = {};                // todo[j]: a request to enqueue; col_of[j]: the column it reads
    int dir[8] = {}, metric[8] = {}, mode[8] = {};   // the columns
};
template <class Enqueued>
inline RequestGroups group_requests(int n, const int *dirs, const int *metrics, const int *normal_modes, const int64_t *key,
                                    const uint64_t *key2, Enqueued enqueued)
{
    RequestGroups g;
    auto same_column = [&](int d, int m, int mode, int i) {
        return d == dirs[i] && m == metrics[i] && (!normal_mode_enters(m) || mode == normal_modes[i]);
    };
    for (int i = 0; i < n; ++i) {
        if (enqueued(i)) continue;
        bool dup = false;
        for (int j = 0; j < g.ntodo; ++j) {
            const int t = g.todo[j];
            dup = dup || (same_column(dirs[t], metrics[t], normal_modes[t], i) && key[t] == key[i] && (!key2 || key2[t] == key2[i]));
        }
        if (dup) continue;
        int c = 0;
        while (c < g.ncols && !same_column(g.dir[c], g.metric[c], g.mode[c], i)) ++c;
        if (c == g.ncols) { g.dir[c] = dirs[i]; g.metric[c] = metrics[i]; g.mode[c] = normal_modes[i]; g.ncols++; }
        g.col_of[g.ntodo] = c;
        g.todo[g.ntodo++] = i;
    }
    return g;
}

// A slot for a new request: an idle one, then a stale one (nn_gen: the directions' generations now); failing that, a pending one
// that does NOT belong to the batch being assembled (`fresh`): its unconsumed result is given up (a later consumer recomputes
// it) -- never a slot of the current batch, whose host outputs an earlier job of the same launch is about to write.
template <class Slot, size_t N>
inline Slot *pick_free(Slot (&slots)[N], Slot *const *fresh, int nfresh, const uint64_t *nn_gen)
{
    for (auto &s : slots)
        if (!s.pending) return &s;
    for (auto &s : slots)
        if (s.gen != nn_gen[s.dir]) return &s;
    for (auto &s : slots) {
        bool mine = false;
        for (int k = 0; k < nfresh; ++k) mine = mine || fresh[k] == &s;
        if (!mine) return &s;
    }
    return nullptr;
}

}  // namespace pccm
