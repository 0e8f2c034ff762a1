// The passes of pccm_carry_normals and pccm_merge_duplicates: one kernel per pass, each a launch of its own over whole waves of
// rows (the launchers pad the row counts to multiples of 64; a kernel's first line drops the rest of the last workgroup).
//
// pccm_carry_normals averages the source cloud's normals over the rows that matched each target row, in ascending row order
// (integer atomics only: where a list lands is arbitrary, the order it is summed in is not).  k_carry_count (rows: n_from)
// counts; k_carry_place (n_to) gives every list of 1..kCarryLong rows a segment of `list` and queues the longer ones;
// k_carry_scatter_walk fills the segments (its first n_from rows, padded) and, in the waves behind them, sums one queued list per
// wave by walking nn_F in row order; k_carry_sum (n_to) sums the short lists and copies the fallback rows.
//
// pccm_merge_duplicates runs the same passes for its colour averages -- nn_F := rep (every row's group representative),
// n_from = n_to = n, src := the colours, nn_G null: a row that no row names (m = 0: not a representative) is then skipped -- and
// these of its own: k_merge_probe<false> (rows: n) puts every row into the open-addressed table of group representatives;
// k_merge_probe<true> (n) reads rep[i] back and notes per wave which rows are representatives (a 64-bit mask and its count);
// k_merge_scan_waves (one lane per wave of rows) and k_merge_scan_top (one wave) turn the counts into exclusive prefixes -- the
// ordered scan -- and leave n' in head[0]; k_merge_gather (n) writes map[i] = the position of rep[i] and, for a representative, its
// merged row.  A reflectance column is averaged by the same passes over rows of one double (CarryView::nc).
//
// pccm_voxel_occupancy runs the two k_merge_probe launches alone, in their occupancy mode (MergeArgs::voxel != 0, uniform over a
// launch): the table over the rows of BOTH clouds, keyed by a row's voxel, and three integer tallies instead of rep / bits / wpre.
#include "pccm_internal.h"

namespace pccm {

// Lists of up to kCarryLong rows are summed by one lane that picks the next larger row kCarryLong times over (<= kCarryLong^2
// loads of a segment the L2 holds); longer ones cost one wave a walk over all n_from rows each, and there are at most
// n_from / kCarryLong of them.  128: the lane's worst case stays at 16 K loads, the walks' at n_from^2 / 8192 row reads.
constexpr int kCarryLong = 128;
constexpr uint32_t kMergeEmpty = 0xffffffffu;      // an empty slot of the table (no cloud has that many rows)

__host__ __device__ constexpr int64_t whole_waves(int64_t rows) { return (rows + 63) / 64 * 64; }

// What a carry pass works on.  The workspace (uint32 words): head[0] segment cursor, head[1] queue length, head[2..3] -, then
// cnt[n_to], fill[n_to], base[n_to], list[n_from], queue[n_from / (kCarryLong + 1) + 1]
struct CarryView {
    const int32_t *nn_f, *nn_g;     // nn_F [n_from]: matched rows of the direction that iterates the source cloud; nn_G [n_to] or null
    const double *rec;              // the count pass alone (launch_match_counts): nn_F null -- the rows are read in place from
    int rec_stride;                 // these result records (matched_row, pccm_internal.h)
    const double *src;              // the source rows [n_from][nc]: normals or colours (nc 3), or a scalar column (nc 1)
    double *out;                    // the target rows [n_to][nc]
    int nc;
    int64_t n_from, n_to;
    uint32_t *head, *cnt, *fill, *base, *list, *queue;
};

static CarryView carry_view(const int32_t *nn_f, const int32_t *nn_g, const double *src, double *out, uint32_t *ws, int64_t n_from,
                            int64_t n_to, int nc)
{
    CarryView V;
    V.nc = nc;
    V.nn_f = nn_f;
    V.nn_g = nn_g;
    V.rec = nullptr;
    V.rec_stride = 0;
    V.src = src;
    V.out = out;
    V.n_from = n_from;
    V.n_to = n_to;
    V.head = ws;
    V.cnt = V.head + 4;
    V.fill = V.cnt + V.n_to;
    V.base = V.fill + V.n_to;
    V.list = V.base + V.n_to;
    V.queue = V.list + V.n_from;
    return V;
}

size_t carry_ws_bytes(int64_t n_from, int64_t n_to)
{
    return (size_t)(4 + 3 * n_to + n_from + n_from / (kCarryLong + 1) + 1) * sizeof(uint32_t);
}

__device__ __forceinline__ double lane_value(double v, int lane)      // v of `lane` (wave-uniform), in every lane
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// one row of the source / of the target: three doubles, of which a scalar column (nc 1) holds the first -- the other two are
// zeros that every sum carries along and nobody stores
__device__ __forceinline__ void carry_load(const CarryView &V, int64_t row, double &a0, double &a1, double &a2)
{
    const double *p = V.src + V.nc * row;
    a0 = p[0];
    a1 = a2 = 0.0;
    if (V.nc == 3) { a1 = p[1]; a2 = p[2]; }
}
__device__ __forceinline__ void carry_store(const CarryView &V, int64_t row, double s0, double s1, double s2)
{
    double *o = V.out + V.nc * row;
    o[0] = s0;
    if (V.nc == 3) { o[1] = s1; o[2] = s2; }
}

__device__ __forceinline__ void carry_count(const CarryView &V, int64_t i, int lane)
{
    // one atomic per distinct target in the wave, not one per row: a target cloud of a few points would otherwise put
    // every row's add on the same few words
    int32_t j = -1;
    if (i < V.n_from) {
        j = matched_row(V.nn_f, V.rec, V.rec_stride, i);
        if (j < 0 || (int64_t)j >= V.n_to) j = -1;                  // (no search writes such a row)
    }
    unsigned long long todo = __ballot(j >= 0);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int32_t jl = __builtin_amdgcn_readlane(j, lead);
        const unsigned long long same = __ballot(j == jl);
        if (lane == lead) atomicAdd(&V.cnt[jl], (uint32_t)__popcll(same));
        todo &= ~same;
    }
}

__device__ __forceinline__ void carry_place(const CarryView &V, int64_t i, int lane)
{
    // segments for the lists of 1..kCarryLong rows: the wave's lengths are scanned, one lane moves the cursor
    const uint32_t m = i < V.n_to ? V.cnt[i] : 0u;
    const uint32_t len = m <= (uint32_t)kCarryLong ? m : 0u;
    const uint32_t incl = wave_incl_scan_u32(len, lane);
    const uint32_t total = __shfl(incl, 63);
    uint32_t start = 0;
    if (lane == 0 && total) start = atomicAdd(&V.head[0], total);
    start = __shfl(start, 0);
    if (i < V.n_to) V.base[i] = start + incl - len;
    if (m > (uint32_t)kCarryLong) V.queue[atomicAdd(&V.head[1], 1u)] = (uint32_t)i;
}

__device__ __forceinline__ void carry_scatter(const CarryView &V, int64_t i)
{
    if (i >= V.n_from) return;
    const int32_t j = V.nn_f[i];
    if (j < 0 || (int64_t)j >= V.n_to) return;
    const uint32_t m = V.cnt[j];
    if (m > (uint32_t)kCarryLong) return;                           // (the walk finds these rows itself)
    const uint32_t p = atomicAdd(&V.fill[j], 1u);
    if (p < m) V.list[V.base[j] + p] = (uint32_t)i;
}

__device__ __forceinline__ void carry_sum(const CarryView &V, int64_t i)
{
    if (i >= V.n_to) return;
    const uint32_t m = V.cnt[i];
    if (m > (uint32_t)kCarryLong) return;
    double s0, s1, s2;
    if (m == 0) {                                                   // nobody's nearest neighbour: its own nearest row's normal
        if (!V.nn_g) return;                                        // (pccm_merge_duplicates: not a representative, no row of its own)
        int64_t r = V.nn_g[i];
        r = r < 0 ? 0 : (r >= V.n_from ? V.n_from - 1 : r);
        carry_load(V, r, s0, s1, s2);
        carry_store(V, i, s0, s1, s2);
        return;
    }
    const uint32_t *seg = V.list + V.base[i];
    if (m <= 2) {                                                   // (a two-term sum is the same either way round)
        carry_load(V, (int64_t)seg[0], s0, s1, s2);
        if (m == 2) {
            double b0, b1, b2;
            carry_load(V, (int64_t)seg[1], b0, b1, b2);
            s0 = __dadd_rn(s0, b0); s1 = __dadd_rn(s1, b1); s2 = __dadd_rn(s2, b2);
        }
    } else {
        // ascending rows without a private array: the smallest row above the last one, m times
        int64_t last = -1;
        s0 = s1 = s2 = 0.0;
        for (uint32_t r = 0; r < m; ++r) {
            int64_t next = INT64_MAX;
            for (uint32_t t = 0; t < m; ++t) {
                const int64_t v = (int64_t)seg[t];
                next = (v > last && v < next) ? v : next;
            }
            if (next == INT64_MAX) break;                           // (rows of a list are distinct: never taken)
            double a0, a1, a2;
            carry_load(V, next, a0, a1, a2);
            if (r == 0) { s0 = a0; s1 = a1; s2 = a2; }
            else { s0 = __dadd_rn(s0, a0); s1 = __dadd_rn(s1, a1); s2 = __dadd_rn(s2, a2); }
            last = next;
        }
    }
    const double dm = (double)m;
    carry_store(V, i, __ddiv_rn(s0, dm), __ddiv_rn(s1, dm), __ddiv_rn(s2, dm));
}

// wave i / 64 takes one queued target and walks nn_F in row order, 64 rows a step (four steps' rows are loaded ahead); the lanes
// whose row matched hold its normal, and the sum takes them in lane order -- ascending rows -- in every lane alike.  It reads
// neither the lists nor anything the sum writes (the sum leaves the queued rows alone), so it rides with the scatter
__device__ __forceinline__ void carry_walk(const CarryView &V, int64_t i, int lane)
{
    const int64_t w = i >> 6;
    if (w >= (int64_t)V.head[1]) return;                                // (wave-uniform)
    const int32_t j = (int32_t)V.queue[w];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    bool first = true;
    for (int64_t r0 = 0; r0 < V.n_from; r0 += 256) {                   // four steps' rows in flight, then two steps' normals at a time
        int32_t got[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t r = r0 + 64 * c + lane;
            got[c] = r < V.n_from ? V.nn_f[r] : -1;                     // (j >= 0: a row past the end never matches)
        }
#pragma unroll
        for (int h = 0; h < 4; h += 2) {
            if (!__ballot(got[h] == j || got[h + 1] == j)) continue;
            double a[2][3];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int64_t r = r0 + 64 * (h + c) + lane;
                a[c][0] = a[c][1] = a[c][2] = 0.0;
                if (got[h + c] == j) carry_load(V, r, a[c][0], a[c][1], a[c][2]);
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                unsigned long long mask = __ballot(got[h + c] == j);
                if (mask == ~0ull && !first) {
#pragma unroll
                    for (int b = 0; b < 64; ++b) {
                        s0 = __dadd_rn(s0, lane_value(a[c][0], b)); s1 = __dadd_rn(s1, lane_value(a[c][1], b)); s2 = __dadd_rn(s2, lane_value(a[c][2], b));
                    }
                    continue;
                }
                while (mask) {
                    const int b = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    const double v0 = lane_value(a[c][0], b), v1 = lane_value(a[c][1], b), v2 = lane_value(a[c][2], b);
                    if (first) { s0 = v0; s1 = v1; s2 = v2; first = false; }
                    else { s0 = __dadd_rn(s0, v0); s1 = __dadd_rn(s1, v1); s2 = __dadd_rn(s2, v2); }
                }
            }
        }
    }
    if (lane == 0) {
        const double dm = (double)V.cnt[j];
        carry_store(V, (int64_t)j, __ddiv_rn(s0, dm), __ddiv_rn(s1, dm), __ddiv_rn(s2, dm));
    }
}

__global__ __launch_bounds__(256) void k_carry_count(CarryView V)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < whole_waves(V.n_from)) carry_count(V, i, threadIdx.x & 63);
}

__global__ __launch_bounds__(256) void k_carry_place(CarryView V)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < whole_waves(V.n_to)) carry_place(V, i, threadIdx.x & 63);
}

__global__ __launch_bounds__(256) void k_carry_scatter_walk(CarryView V)      // the first waves scatter, the ones behind them walk
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, rows = whole_waves(V.n_from);
    if (i < rows) carry_scatter(V, i);
    else carry_walk(V, i - rows, threadIdx.x & 63);
}

__global__ __launch_bounds__(256) void k_carry_sum(CarryView V)
{
    carry_sum(V, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// pccm_carry_normals on the stream: counts and cursors zeroed, then count | place | scatter + walk | sum
int launch_carry(pccm_ctx *ctx, const int32_t *nn_f, const int32_t *nn_g, const double *n_from64, int64_t n_from, int64_t n_to,
                 uint32_t *ws, double *out, int nc)
{
    ProfScope ps(ctx, PCCM_K_POINT);
    PCCM_HIP(hipMemsetAsync(ws, 0, (size_t)(4 + 2 * n_to) * sizeof(uint32_t), ctx->stream));     // header, cnt, fill
    const CarryView V = carry_view(nn_f, nn_g, n_from64, out, ws, n_from, n_to, nc);
    const int64_t walk_lanes = (n_from / (kCarryLong + 1)) * 64;       // one wave per list that can be long
    auto blocks = [](int64_t lanes) { return dim3((unsigned)((lanes + 255) / 256)); };
    PCCM_LAUNCH(ctx, k_carry_count, blocks(whole_waves(n_from)), dim3(256), 0, ctx->stream, V);
    PCCM_LAUNCH(ctx, k_carry_place, blocks(whole_waves(n_to)), dim3(256), 0, ctx->stream, V);
    PCCM_LAUNCH(ctx, k_carry_scatter_walk, blocks(whole_waves(n_from) + walk_lanes), dim3(256), 0, ctx->stream, V);
    PCCM_LAUNCH(ctx, k_carry_sum, blocks(whole_waves(n_to)), dim3(256), 0, ctx->stream, V);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

// A direction's match counts (pccm_match_counts, the density map of k_unit_jobs): the count pass above on its own -- cnt zeroed on
// the stream, then k_carry_count over the shard's rows padded to whole waves.  Of the view only the rows' source, the two row
// counts and cnt are read.
int launch_match_counts(pccm_ctx *ctx, const int32_t *idx, const double *rec, int stride, int64_t ns, int64_t n_to, uint32_t *cnt)
{
    if (n_to <= 0) return PCCM_OK;
    ProfScope ps(ctx, PCCM_K_POINT);
    PCCM_HIP(hipMemsetAsync(cnt, 0, (size_t)n_to * sizeof(uint32_t), ctx->stream));
    if (ns <= 0) return PCCM_OK;
    CarryView V = {};
    V.nn_f = idx;
    V.rec = rec;
    V.rec_stride = stride;
    V.n_from = ns;
    V.n_to = n_to;
    V.cnt = cnt;
    PCCM_LAUNCH(ctx, k_carry_count, dim3((unsigned)((whole_waves(ns) + 255) / 256)), dim3(256), 0, ctx->stream, V);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

// ------------------------------------------------------------------------------------------
// pccm_merge_duplicates.  Rows with equal coordinates (== per component) end in one slot of an open-addressed table, whose value
// after the insert launch is the smallest of them whatever the arrival order: a slot is claimed once and never emptied, every row
// of a key walks the same probe sequence, and the only writes are compare-and-swap on an empty slot and atomicMin.  No loop waits
// for another lane: a probe sequence ends after at most `cap` slots (then the device error word says so).  The colour averages are
// the carry's passes above.
// ------------------------------------------------------------------------------------------
struct MergeArgs {
    const double *x;                // the points [n][3]
    const double *nrm, *rgb;        // the normals / the colours to keep per representative [n][3], or null
    double *out;                    // the merged rows (written): points [n][3], then normals [n][3], then colours [n][3]
    const double *refl;             // the reflectance to keep per representative [n], or null
    double *refl_out;               // the merged reflectance [n] (written)
    uint32_t *ws;                   // the uint32 words of the workspace (MergeLayout)
    int32_t *map;                   // [n] (written)
    uint32_t *err;                  // the device error word, or null
    int64_t n;
    // occupancy mode (voxel != 0; launch-uniform): the joint rows 0 .. n-1 are x's n1 rows, then x2's n - n1; ws is an
    // OccupancyLayout, whose table has cap slots and whose seen [n1] and tally [3] these are.  voxel 0: pccm_merge_duplicates,
    // none of the others read.  voxel stands next to n: the kernels read both in their first load of the arguments, and the
    // merge's path does not wait for a second one before it starts
    double voxel;
    const double *x2;
    int64_t n1;
    uint64_t cap;
    uint32_t *seen;
    unsigned long long *tally;      // |A u B|, |A|, |A n B| in voxels
};

__device__ __forceinline__ uint32_t merge_hash(double x, double y, double z)
{
    const double k[3] = {x == 0.0 ? 0.0 : x, y == 0.0 ? 0.0 : y, z == 0.0 ? 0.0 : z};     // (-0.0 == +0.0: one key, one hash)
    uint32_t h = 0x9e3779b9u;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        uint32_t w = (uint32_t)((a & 1) ? __double2hiint(k[a >> 1]) : __double2loint(k[a >> 1]));
        w *= 0xcc9e2d51u;
        w = (w << 15) | (w >> 17);
        w *= 0x1b873593u;
        h ^= w;
        h = (h << 13) | (h >> 19);
        h = h * 5u + 0xe6546b64u;
    }
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// Occupancy mode of k_merge_probe (pccm_voxel_occupancy): the same table over the joint rows of both clouds, keyed by a row's
// voxel floor(c / voxel) + 0.0 -- three doubles compared with ==, the correctly rounded fp64 quotient (never a product with a
// reciprocal: 0.3 / 0.1 floors to 2), -0.0 folded onto 0.0.  After the insert a slot holds the smallest joint row of its voxel, so
// a voxel holds a point of cloud 0 exactly when that row is < n1.  The find tallies, per wave and in integer atomics alone: the
// rows that are their voxel's representative (|A u B|), those of them in cloud 0 (|A|), and -- one row of cloud 1 per voxel whose
// representative is in cloud 0, the one whose exchange on seen[r] finds it unset -- |A n B|.
__device__ __forceinline__ void occupancy_key(const MergeArgs &A, int64_t row, double k[3])
{
    const double *p = row < A.n1 ? A.x + 3 * row : A.x2 + 3 * (row - A.n1);
    const double v = A.voxel;
    k[0] = floor(p[0] / v) + 0.0;
    k[1] = floor(p[1] / v) + 0.0;
    k[2] = floor(p[2] / v) + 0.0;
}

template <bool FIND>
__device__ __forceinline__ void occupancy_probe(const MergeArgs &A, int64_t i)
{
    const int64_t n = A.n, n1 = A.n1;
    uint32_t *tab = A.ws;                                           // (OccupancyLayout::table is 0; the host hands its cap in)
    int64_t r = -1;
    if (i < n) {
        double k[3];
        occupancy_key(A, i, k);
        const uint64_t cap = A.cap, mask = cap - 1;
        uint64_t slot = (uint64_t)merge_hash(k[0], k[1], k[2]) & mask;
        bool done = false;
        for (uint64_t probe = 0; probe < cap; ++probe, slot = (slot + 1) & mask) {
            uint32_t cur = __hip_atomic_load(&tab[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == kMergeEmpty) {
                if (FIND) break;
                cur = atomicCAS(&tab[slot], kMergeEmpty, (uint32_t)i);
                if (cur == kMergeEmpty) { done = true; break; }
            }
            if ((int64_t)cur >= n) break;
            double o[3];
            occupancy_key(A, (int64_t)cur, o);
            if (o[0] == k[0] && o[1] == k[1] && o[2] == k[2]) {
                if (!FIND) { if (cur > (uint32_t)i) atomicMin(&tab[slot], (uint32_t)i); }
                else r = (int64_t)cur;
                done = true;
                break;
            }
        }
        if (!done) {
            if (A.err) atomicOr(A.err, kErrMergeTable);
            r = i;
        }
    }
    if (!FIND) return;
    const bool own = i < n && r == i;
    bool first = false;
    // (the word only ever goes from 0 to 1: a lane that reads 1 has nothing to claim, and a coarse lattice, where a million rows
    // meet a few voxels, is spared a million exchanges on a few addresses)
    if (i < n && i >= n1 && r >= 0 && r < n1 && __hip_atomic_load(&A.seen[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
        first = atomicExch(&A.seen[r], 1u) == 0u;
    const unsigned long long m_union = __ballot(own), m_a = __ballot(own && i < n1), m_both = __ballot(first);
    if ((threadIdx.x & 63) == 0) {
        if (m_union) atomicAdd(&A.tally[0], (unsigned long long)__popcll(m_union));
        if (m_a) atomicAdd(&A.tally[1], (unsigned long long)__popcll(m_a));
        if (m_both) atomicAdd(&A.tally[2], (unsigned long long)__popcll(m_both));
    }
}

// FIND false: the insert.  FIND true: rep[i] (a row, stored in a uint32 word) and the waves' representative masks and counts
template <bool FIND>
__global__ __launch_bounds__(256) void k_merge_probe(MergeArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, n = A.n;
    if (i >= whole_waves(n)) return;
    if (A.voxel != 0.0) {                                           // (launch-uniform)
        occupancy_probe<FIND>(A, i);
        return;
    }
    const MergeLayout L = merge_layout(n);
    uint32_t *tab = A.ws + L.table;
    int32_t r = -1;
    if (i < n) {
        const double *x = A.x;
        const double kx = x[3 * i], ky = x[3 * i + 1], kz = x[3 * i + 2];
        const uint64_t mask = L.cap - 1;
        uint64_t slot = (uint64_t)merge_hash(kx, ky, kz) & mask;
        bool done = false;
        for (uint64_t probe = 0; probe < L.cap; ++probe, slot = (slot + 1) & mask) {
            uint32_t cur = __hip_atomic_load(&tab[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == kMergeEmpty) {
                if (FIND) break;                                    // (its own insert filled a slot on the way: never taken)
                cur = atomicCAS(&tab[slot], kMergeEmpty, (uint32_t)i);
                if (cur == kMergeEmpty) { done = true; break; }     // claimed
            }
            if ((int64_t)cur >= n) break;                           // (only rows are ever stored)
            const double *o = x + 3 * (int64_t)cur;
            if (o[0] == kx && o[1] == ky && o[2] == kz) {
                // (the slot only ever gets smaller: a row above its value has nothing to add)
                if (!FIND) { if (cur > (uint32_t)i) atomicMin(&tab[slot], (uint32_t)i); }
                else r = (int32_t)cur;
                done = true;
                break;
            }
        }
        if (!done) {
            if (A.err) atomicOr(A.err, kErrMergeTable);
            r = (int32_t)i;
        }
        if (FIND) A.ws[L.rep + i] = (uint32_t)r;
    }
    if (!FIND) return;
    const unsigned long long keep = __ballot(i < n && (int64_t)r == i);
    if ((threadIdx.x & 63) == 0) {
        const int64_t w = i >> 6;
        uint32_t *bits = A.ws + L.bits;
        bits[2 * w] = (uint32_t)keep;
        bits[2 * w + 1] = (uint32_t)(keep >> 32);
        A.ws[L.wpre + w] = (uint32_t)__popcll(keep);
    }
}

__global__ __launch_bounds__(256) void k_merge_scan_waves(MergeArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const MergeLayout L = merge_layout(A.n);
    if (i >= whole_waves(L.nw)) return;
    uint32_t *wpre = A.ws + L.wpre, *spre = A.ws + L.spre;
    const uint32_t c = i < L.nw ? wpre[i] : 0u;
    const uint32_t incl = wave_incl_scan_u32(c, threadIdx.x & 63);
    if (i < L.nw) wpre[i] = incl - c;
    if ((threadIdx.x & 63) == 63) spre[i >> 6] = incl;
}

__global__ __launch_bounds__(256) void k_merge_scan_top(MergeArgs A)        // one wave: a run of spre per lane
{
    if (blockIdx.x != 0 || threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const MergeLayout L = merge_layout(A.n);
    uint32_t *spre = A.ws + L.spre;
    const int64_t per = (L.nsw + 63) / 64, b = lane * per, e = b + per < L.nsw ? b + per : L.nsw;
    uint32_t sum = 0;
    for (int64_t k = b; k < e; ++k) sum += spre[k];
    const uint32_t incl = wave_incl_scan_u32(sum, lane);
    uint32_t run = incl - sum;
    for (int64_t k = b; k < e; ++k) {
        const uint32_t c = spre[k];
        spre[k] = run;
        run += c;
    }
    if (lane == 63) A.ws[0] = incl;
}

__global__ __launch_bounds__(256) void k_merge_gather(MergeArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, n = A.n;
    if (i >= n) return;
    const MergeLayout L = merge_layout(n);
    const uint32_t *bits = A.ws + L.bits;
    const int64_t r = (int32_t)A.ws[L.rep + i], w = r >> 6;
    const unsigned long long m64 = (unsigned long long)bits[2 * w] | ((unsigned long long)bits[2 * w + 1] << 32);
    const int64_t p = (int64_t)A.ws[L.spre + (w >> 6)] + A.ws[L.wpre + w] + __popcll(m64 & ((1ull << (r & 63)) - 1ull));
    A.map[i] = (int32_t)p;
    if (r != i) return;
    const double *x = A.x, *nrm = A.nrm, *rgb = A.rgb;
    double *o = A.out + 3 * p;
    o[0] = x[3 * i]; o[1] = x[3 * i + 1]; o[2] = x[3 * i + 2];
    if (nrm) { o += 3 * n; o[0] = nrm[3 * i]; o[1] = nrm[3 * i + 1]; o[2] = nrm[3 * i + 2]; o -= 3 * n; }
    if (rgb) { o += 6 * n; o[0] = rgb[3 * i]; o[1] = rgb[3 * i + 1]; o[2] = rgb[3 * i + 2]; }
    if (A.refl) A.refl_out[p] = A.refl[i];
}

static dim3 merge_blocks(int64_t rows) { return dim3((unsigned)((whole_waves(rows) + 255) / 256)); }

int launch_merge_find(pccm_ctx *ctx, const double *x64, int64_t n, uint32_t *words)
{
    ProfScope ps(ctx, PCCM_K_POINT);
    const MergeLayout L = merge_layout(n);
    PCCM_HIP(hipMemsetAsync(words + L.table, 0xff, (size_t)L.cap * sizeof(uint32_t), ctx->stream));     // kMergeEmpty
    MergeArgs A = {};
    A.x = x64;
    A.ws = words;
    A.err = ctx->host_err;
    A.n = n;
    PCCM_LAUNCH(ctx, k_merge_probe<false>, merge_blocks(n), dim3(256), 0, ctx->stream, A);
    PCCM_LAUNCH(ctx, k_merge_probe<true>, merge_blocks(n), dim3(256), 0, ctx->stream, A);
    PCCM_LAUNCH(ctx, k_merge_scan_waves, merge_blocks(L.nw), dim3(256), 0, ctx->stream, A);
    PCCM_LAUNCH(ctx, k_merge_scan_top, merge_blocks(64), dim3(256), 0, ctx->stream, A);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

int launch_occupancy(pccm_ctx *ctx, const double *x0, int64_t n1, const double *x1, int64_t n2, double voxel, uint32_t *words)
{
    ProfScope ps(ctx, PCCM_K_POINT);
    const OccupancyLayout L = occupancy_layout(n1, n2);
    PCCM_HIP(hipMemsetAsync(words + L.table, 0xff, (size_t)L.cap * sizeof(uint32_t), ctx->stream));     // kMergeEmpty
    PCCM_HIP(hipMemsetAsync(words + L.seen, 0, (L.words - L.seen) * sizeof(uint32_t), ctx->stream));    // seen, then the tallies
    MergeArgs A = {};
    A.x = x0;
    A.x2 = x1;
    A.n1 = n1;
    A.n = n1 + n2;
    A.voxel = voxel;
    A.ws = words + L.table;
    A.cap = L.cap;
    A.seen = words + L.seen;
    A.tally = (unsigned long long *)(words + L.tally);
    A.err = ctx->host_err;
    PCCM_LAUNCH(ctx, k_merge_probe<false>, merge_blocks(A.n), dim3(256), 0, ctx->stream, A);
    PCCM_LAUNCH(ctx, k_merge_probe<true>, merge_blocks(A.n), dim3(256), 0, ctx->stream, A);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

int launch_merge_gather(pccm_ctx *ctx, const double *x64, const double *nrm, const double *rgb, const double *refl, int64_t n, double *out,
                        double *refl_out, uint32_t *words, int32_t *map)
{
    ProfScope ps(ctx, PCCM_K_POINT);
    MergeArgs A = {};
    A.x = x64;
    A.nrm = nrm;
    A.rgb = rgb;
    A.out = out;
    A.refl = refl_out ? refl : nullptr;
    A.refl_out = refl_out;
    A.ws = words;
    A.map = map;
    A.n = n;
    PCCM_LAUNCH(ctx, k_merge_gather, merge_blocks(n), dim3(256), 0, ctx->stream, A);
    PCCM_HIP(hipGetLastError());
    return PCCM_OK;
}

}  // namespace pccm
