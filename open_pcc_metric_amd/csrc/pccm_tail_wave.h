// One wave settles one unsettled ring-1 query: rings 2..kMaxRing, lanes = x-runs of the cube [c-r, c+r]^3.  Written once for the
// two kernels that run it: k_grid_tail (pccm_grid.hip: a launch of its own over the direction's tail list) and the settling
// reduction (pccm_point.hip: a workgroup first settles the few entries filed under its own 4096 rows) -- the same arithmetic, the
// same (d2, row) tie rule, the same stop rule.
//
// Below it, the host side of the filed form: how the tail list of an eager step is binned by row block and what decides whether
// the graph captured behind that step may file its tails (no HIP call: tests/tailfile_host_main.cpp compiles this part alone).
#pragma once
#include <cstdint>
#include <vector>

namespace pccm {

// rows of one reduction workgroup: 32 leaves of 128 rows (unit_leaves, pccm_point.hip) -- a tail query is filed under row >> 12
constexpr int kTailBlockShift = 12;
// entries a block's list holds: ~7x the 4.3 a block expects at the shipped cell rule (1e-3 of the rows are tails)
constexpr int kTailBlockCap = 32;

// the largest number of tail rows any block of 4096 rows holds (rows relative to the shard's first row; nrows: rows of the shard);
// -1: a row outside [0, nrows) -- the list does not belong to this shard
inline int64_t tail_block_max(const int32_t *rows, int64_t n, int64_t nrows, std::vector<int64_t> *per_block = nullptr)
{
    const int64_t nblocks = (nrows + (1ll << kTailBlockShift) - 1) >> kTailBlockShift;
    std::vector<int64_t> own;
    std::vector<int64_t> &count = per_block ? *per_block : own;
    count.assign((size_t)(nblocks > 0 ? nblocks : 0), 0);
    int64_t worst = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (rows[i] < 0 || rows[i] >= nrows) return -1;
        const int64_t c = ++count[(size_t)(rows[i] >> kTailBlockShift)];
        worst = c > worst ? c : worst;
    }
    return worst;
}

// What the eager step in front of a capture showed of one searched direction
struct TailFacts {
    bool searched = false;       // the direction has a valid result of the brick search over all rows of its iterating cloud
    int64_t flagged = 0;         // queries three rings could not settle (the exact rescan's list)
    int64_t block_max = 0;       // tail_block_max of its tail list
};

// The capture rule: the filed form has no exact rescan and a fixed capacity per block, so a graph files its tails only when the
// eager step on the same resident clouds needed neither -- in every direction it searched.
inline bool tail_filing_allowed(const TailFacts *dirs, int ndirs, bool switched_on)
{
    if (!switched_on) return false;
    int searched = 0;
    for (int d = 0; d < ndirs; ++d) {
        if (!dirs[d].searched) continue;
        ++searched;
        if (dirs[d].flagged != 0) return false;
        if (dirs[d].block_max < 0 || dirs[d].block_max > kTailBlockCap) return false;
    }
    return searched > 0;
}

}  // namespace pccm

#ifdef __HIPCC__
#include "pccm_grid.h"

namespace pccm {

// the running minimum with the winner's coordinates kept (what the result record or the fused projection needs is then in
// registers when the search ends)
struct BestAt {
    double d, x, y, z;
    int idx;
};

template <typename REC, bool SELF, int kBatch>
__device__ __forceinline__ void scan_range_at(const REC *__restrict__ recs, uint32_t s, uint32_t e, double qx, double qy, double qz, int qrow,
                                              BestAt &b)
{
    for (uint32_t p = s; p < e; p += kBatch) {
        P3 a[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) a[j] = load_rec(recs, (p + j < e) ? p + j : e - 1);
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const double d = gdist64(qx, qy, qz, a[j].x, a[j].y, a[j].z);
            bool better = d < b.d || (d == b.d && a[j].row < b.idx);
            if (SELF) better = better && (a[j].row != qrow);
            b.d = better ? d : b.d;
            b.idx = better ? a[j].row : b.idx;
            b.x = better ? a[j].x : b.x;
            b.y = better ? a[j].y : b.y;
            b.z = better ? a[j].z : b.z;
        }
    }
}

// The query qa (wave-uniform) against the searched cloud's cell-sorted records: -> settled within kMaxRing rings?  b: the
// lexicographic (d2, row) minimum and its coordinates, the same in every lane.
// Every such query has been through a ring-1 kernel that could not settle it -- mostly because the stop rule failed, which a
// second look at ring 1 cannot change: start with the 5 x 5 x 5 cube (it contains ring 1, scanned here in exact fp64, so
// uncertified near ties are resolved too).  Rings already scanned are simply scanned again (the minimum is idempotent).
template <typename REC, bool SELF>
__device__ __forceinline__ bool wave_settle(const GridGeom &g, const uint32_t *__restrict__ cell_start, const REC *__restrict__ srecs,
                                            const P3 &qa, int lane, BestAt &b)
{
    const int dimx = g.dim[0], dimy = g.dim[1], dimz = g.dim[2];
    const double qx = qa.x, qy = qa.y, qz = qa.z;
    const int qrow = qa.row;
    const int cx = cell_coord(qx, g.org[0], g.inv_h[0], dimx);
    const int cy = cell_coord(qy, g.org[1], g.inv_h[1], dimy);
    const int cz = cell_coord(qz, g.org[2], g.inv_h[2], dimz);
    b.d = INFINITY;
    b.idx = 0x7fffffff;
    b.x = b.y = b.z = 0.0;
    bool done = false;
    for (int r = 2; r <= kMaxRing && !done; ++r) {
        const int side = 2 * r + 1;
        if (lane < side * side) {
            const int z = cz + lane / side - r, y = cy + lane % side - r;
            if (z >= 0 && z < dimz && y >= 0 && y < dimy) {
                const uint32_t row = ((uint32_t)z * dimy + y) * dimx;
                const int x0 = max(cx - r, 0), x1 = min(cx + r, dimx - 1);
                scan_range_at<REC, SELF, 8>(srecs, cell_start[row + x0], cell_start[row + x1 + 1], qx, qy, qz, qrow, b);
            }
        }
        double wm = b.d;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) wm = fmin(wm, __shfl_xor(wm, off));
        int wi = (b.d == wm) ? b.idx : 0x7fffffff;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) wi = min(wi, __shfl_xor(wi, off));
        // a lane that holds the winner hands its coordinates to everybody (rows are unique per record: one such lane)
        const unsigned long long holds = __ballot(b.d == wm && b.idx == wi);
        const int src = holds ? __ffsll((long long)holds) - 1 : 0;
        b.x = __shfl(b.x, src);
        b.y = __shfl(b.y, src);
        b.z = __shfl(b.z, src);
        b.d = wm;
        b.idx = wi;
        done = settled_by(face_bound(g, qx, qy, qz, cx, cy, cz, r), b.d);
    }
    return done;
}

// ---- filed tails ------------------------------------------------------------------------------------------------------------
// What a reduction workgroup needs to settle the queries filed under its rows: the grid, and per searched direction the searched
// cloud's cell starts and records, the block lists and the direction's result records (matched records, NNOut::layout 1, indexed by
// the iterating cloud's row: filing is for whole clouds).  A kernel argument of k_unit_lean.
struct TailSettleDir {
    const uint32_t *cs;
    const Rec32 *srecs;
    const float4 *list;         // [blocks][kTailBlockCap]
    const uint32_t *cnt;        // [blocks]
    float4 *out;
};
struct TailSettle {
    GridGeom g;
    TailSettleDir d[2];
    uint32_t *err;              // the context's device error word
    uint32_t on;                // 0: the launch settles nothing (the other fields are not read)
};

// ... and what the search keeps on the host until the lists are consumed: the settling kernel's argument, and everything the
// classic tail launch takes (filed_tails_resolve)
struct FiledTails {
    QueryJobs jobs;
    GridGeom g;
    int64_t nqmax = 0;
    int dirs[2] = {0, 0};
    TailSettle settle;
};

}  // namespace pccm
#endif
