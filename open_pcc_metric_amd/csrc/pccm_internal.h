// Internal declarations shared by the translation units of libpccm.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <string>
#include <variant>
#include <vector>

#include "pccm.h"
#include "pccm_slot.h"

// A/B switches that no test of the shipped library uses (brick length, register cap, build bins, cells per point, ...) exist in
// diagnostic builds only (make DIAG=1): the product reads the environment for the switches tests/test_gpu_ab_paths.py exercises
// and for nothing else.
#ifdef PCCM_DIAG
#define PCCM_DIAG_ENV(name) getenv(name)
#else
#define PCCM_DIAG_ENV(name) (static_cast<const char *>(nullptr))
#endif

namespace pccm {

// ---- geometry of the brute-force scan (K1) ------------------------------------------
constexpr int kScanThreads = 256;   // 4 waves of 64
constexpr int kScanTile = 1024;     // search points staged in LDS per buffer
constexpr int kTileVec = kScanTile / 4 * 3;   // float4 vectors per tile in the quad layout (12 KB)
constexpr int kGranule = 64;        // winner tracking granularity = one wave-wide fp64 rescan
constexpr float kBig32 = 3.0e38f;   // "no candidate" distance (finite: no inf arithmetic in the scan)
constexpr float kPadCoord = 1.0e18f;  // coordinates of padding points: d2 ~ 3e36, never wins
constexpr double kMaxAbsCoord = 1.0e15;

// (the reduction geometry -- kLeaf, kChunk -- is pccm_slot.h's)

struct Cloud {
    int64_t n = 0;
    int64_t n_pad = 0;          // multiple of kScanTile
    float4 *xyz32 = nullptr;    // [n_pad/4][3] quads: x0..3 | y0..3 | z0..3; padding rows = kPadCoord
    double *xyz64 = nullptr;    // [n][3]
    float4 *xyz32r = nullptr;   // [n] {x, y, z, 0}: the fp32 coordinates once more, one aligned 16-byte word per ROW (what the reductions
                                // of matched-record results read next to the record and the normal: three wide loads per row)
    size_t cap32r = 0;
    double *nrm64 = nullptr;    // [n_nrm][3]
    float4 *nrm32 = nullptr;    // [n_nrm] {nx, ny, nz, -}: the same normals in one aligned 16-byte word each, when nrm_exact32
    bool nrm_exact32 = false;   // every component survives fp64 -> fp32 -> fp64 (file normals usually do; estimated ones do not)
    int64_t n_nrm = 0;
    // pccm_set_normals_deferred: the normals are announced (n_nrm, buffers) but still lie in the caller's host array; they cross
    // PCIe when somebody needs them (normals_ready) or at pccm_flush_uploads -- behind the searches, which never read them when
    // results are matched records (NNOut::layout 1)
    const void *nrm_host = nullptr;
    int nrm_host_dtype = 0;
    bool nrm_deferred = false;
    double *rgb64 = nullptr;    // [n_rgb][3] colours as the caller gave them (RGB in [0, 1])
    int64_t n_rgb = 0;
    // colours that are k / 255.0 for bytes k -- what every file holds -- also live as one packed word per row (r | g << 8 |
    // b << 16): the colour kernels gather 4 bytes per row from a table the L2 holds instead of 24 from one it does not
    uint32_t *rgb8 = nullptr;
    bool rgb8_valid = false;
    size_t cap_rgb8 = 0;
    // allocations outlive their content (n / n_nrm / n_rgb say what is there): a context that serves one pair after
    // the other -- the engine pool of _native.py -- does not pay hipFree + hipMalloc per cloud
    // the same points in a spatially coherent order (fp32-exact clouds): Rec32 {x, y, z, original row} sorted along a Z-order
    // curve over the cloud's own bounding box, made once per cloud -- by the first pccm_drop_caches that follows a search, i.e. when
    // the caller shows that the resident clouds will be searched again (a one-shot pair never pays for it).  The per-step grid build reads it instead
    // of xyz32: rows that are neighbours in memory are neighbours in space, so the counting sort's scattered stores fall into a
    // few bins per tile and merge into whole lines (WRITE_SIZE 2x -> ~1x the records).  Results never depend on it.
    void *sp = nullptr;
    size_t cap_sp = 0;
    bool sp_valid = false;
    bool sp_tried = false;      // pccm_drop_caches has already made (or found no use for) the spatial order of this cloud
    size_t cap32 = 0, cap64 = 0, cap_nrm = 0, cap_nrm32 = 0, cap_rgb = 0;
    bool exact32 = true;        // every coordinate survives the fp64 -> fp32 -> fp64 round trip
    bool all_int = false;       // ... and is an integer (voxelised content: exact ties are the rule)
    double maxabs = 0.0;
    double bb_min[3] = {0, 0, 0}, bb_max[3] = {0, 0, 0};   // bounding box (fp64 coordinates)
    uint64_t version = 0;       // bumped by pccm_set_cloud (grid caches key on it)
    // PointSSIM features (pccm_ssim_features): [4][n] fp64 columns by attribute bit (geometry, normal, curvature, colour), valid for
    // the attributes in ssim_attrs at neighbourhood size ssim_k; a bit is cleared when what it was made from changes
    double *ssim64 = nullptr;
    size_t cap_ssim = 0;
    int ssim_attrs = 0, ssim_k = 0;
    // point spacings (pccm_resolution_build): [n] fp64, valid for res_k neighbours (0: not built); dropped with the points only
    double *res64 = nullptr;
    size_t cap_res = 0;
    int res_k = 0;
    // reflectance (pccm_set_reflectance*): [n_refl] fp64, one scalar per point with the values as given; n_refl is 0 or n
    double *refl64 = nullptr;
    size_t cap_refl = 0;
    int64_t n_refl = 0;
    double solo_scale = 1.0;    // cell-edge factor of a grid over this cloud alone (grid_ensure_solo), decided for ...
    uint64_t solo_scale_version = ~0ull;   // ... this version of the cloud
};

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

// Where the last search of a direction left its results: one value that holds only what the engines produce (a stride-4
// matched record, or a row that no record carries, cannot be written down); stride and layout are the kernels' view of it.
struct NNForm {
    enum Recs {
        kNone,            // no result records: the plain columns hold the results (brute-force engine, trivial self search,
                          // empty shard), or -- before a search -- nothing does
        kPairRows,        // layout 0, stride 4: {d2, projection, row, -}
        kPair,            // layout 0, stride 2: {d2, projection} (pccm_nn_want_idx off)
        kMatched,         // layout 1, stride 2: the matched record {rx, ry, rz, row}; the reductions form distance and projection
        kMatchedNoRows,   // ... whose row word is void (voxel-brick search): good for distances only
    } recs = kNone;
    enum Plain { kNoPlain, kPlainD2, kPlainAll } plain = kNoPlain;   // unpacked into d2 / idx: nothing, d2 alone, both
    int fused = -1;               // normal mode of the projection fused into the search, -1: none
    // the records of the queries ring 1 did not settle are not written yet: the queries lie filed by row block (pccm_tail_wave.h)
    // for the settling reduction; every other reader has the classic tail launch settle them first (filed_tails_resolve)
    bool tails_filed = false;

    static NNForm columns() { return {kNone, kPlainAll, -1}; }
    bool has_records() const { return recs != kNone; }
    int stride() const { return recs == kPairRows ? 4 : 2; }                       // doubles per record
    int layout() const { return recs == kMatched || recs == kMatchedNoRows ? 1 : 0; }
    bool has_rows() const { return recs == kPairRows || recs == kMatched; }        // the records carry the matched row ...
    bool rows_need_repeat() const { return has_records() && !has_rows(); }         // ... or who wants it repeats the search
    bool plain_ready(bool need_idx) const { return plain == kPlainAll || (!need_idx && plain == kPlainD2); }
    bool matched_in_place() const { return recs == kMatched && plain != kPlainAll; }   // the rows are read out of the records
    // the records hold the projection of normal mode m: fused into the search, or formed from matched records by the reduction
    bool holds_projection(int m) const
    {
        if (recs == kMatched) return m == PCCM_NORMAL_ROW || m == PCCM_NORMAL_NEIGHBOUR;
        return (recs == kPairRows || recs == kPair) && fused == m;
    }
};

struct NNResult {
    bool valid = false;
    int64_t begin = 0, end = 0; // shard rows of the iterating cloud
    int32_t *idx = nullptr;     // [end-begin]   plain columns: written by the brute-force engine, or unpacked from `rec`
    double *d2 = nullptr;       // [end-begin]   on demand (ensure_plain)
    int64_t cap = 0;
    DevBuf rec;                 // [end-begin] result records of up to 32 bytes (grid engine; NNOut in pccm_grid.h)
    NNForm form;                // what `rec`, idx and d2 hold of the last run's results
    int ties = PCCM_TIES_PICK;  // pccm_set_ties policy the search ran under (consumers read the virtual neighbours under MEAN)
    int64_t stats[3] = {0, 0, 0};
    uint32_t *nflag_dev = nullptr;  // device counters of the last run: [0] fallback queries, [1] grid tail length
    DevBuf flagged, flag_thr;       // queries handed to the exact rescan (k2b_fallback) and their thresholds
    DevBuf tail;                    // grid engine: unsettled ring-1 queries
};

// Uniform grid over one cloud (grid engine): cells in x-fastest order, points counting-sorted by cell.
struct GridRec {          // 32 B: fp64 position + original row
    double x, y, z;
    int32_t idx, pad;
};

struct PairSignature {           // what decide_scale looks at to tell "a pair like the last one"
    int64_t n[2] = {0, 0};
    int flags[2] = {0, 0};         // exact32 | all_int << 1
    double lo[2][3] = {{0, 0, 0}, {0, 0, 0}}, hi[2][3] = {{0, 0, 0}, {0, 0, 0}};
    bool resembles(const PairSignature &o) const
    {
        for (int k = 0; k < 2; ++k) {
            if (flags[k] != o.flags[k]) return false;
            const double dn = (double)(n[k] - o.n[k]);
            if (dn > 0.02 * (double)o.n[k] || -dn > 0.02 * (double)o.n[k]) return false;
            for (int a = 0; a < 3; ++a) {
                const double ext = o.hi[k][a] - o.lo[k][a], tol = 0.02 * ext;
                const double d0 = lo[k][a] - o.lo[k][a], d1 = hi[k][a] - o.hi[k][a];
                if (!(d0 <= tol && -d0 <= tol && d1 <= tol && -d1 <= tol)) return false;
            }
        }
        return true;
    }
};

struct Grid {                    // one geometry, both clouds (grid engine)
    uint64_t key = 0;              // derived from both Cloud::version values (0 = none)
    uint64_t scale_key = 0;        // clouds the cell-edge scale below was decided for
    double scale = 1.0;            // shrink factor of the volume-rule cell edge (occupancy-adaptive)
    bool boxed = false;            // the grid covers box_lo..box_hi (outliers trimmed) instead of the bounding box
    double box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0};
    bool hostile = false;          // even so the cells are too crowded: PCCM_ENGINE_AUTO uses the brute engine
    bool coop = true;              // cooperative ring-1 kernel (well-filled x-rows) or the per-thread search (surfaces, lattices)
    double sb = 0.0;               // size-biased points per cell the decision saw
    PairSignature sig;             // of the pair the decisions were last taken (or inherited) for
    uint64_t iso_key = 0;          // pair the isolation count below was taken for
    int64_t isolated[2] = {0, 0};  // points of cloud k with nothing of the other cloud within kMaxRing cells
    bool rec32 = false;            // records are Rec32 (both clouds fp32-exact) instead of GridRec
    int built = 0;                 // bit k: cloud k's records and cell starts are built (a rank that searches one direction
                                   // of a sharded pair builds only the cloud it searches)
    int dim[3] = {1, 1, 1};
    double org[3] = {0, 0, 0};
    double h[3] = {1, 1, 1}, inv_h[3] = {1, 1, 1};   // cell edge per axis
    int64_t ncells = 0, n[2] = {0, 0};
    DevBuf cell_start;             // uint32 [2][ncells + 1]: positions in recs
    bool lattice = false;          // voxelised pair on the per-thread path: pccm_lattice.hip searches it, with the bitmap below
    DevBuf occ;                    // uint32 [2][ncells / 32 + 2]: one bit per cell, set when the cell holds a record
    DevBuf recs;                   // GridRec or Rec32 [n[0] + n[1]]: cloud 0's records, then cloud 1's
    bool vox = false;              // voxel-brick flavour (pccm_vox.hip): cells of 8^3 voxels, searched through the bricks below;
                                   // built for distance-only requests on voxelised pairs, rebuilt with the usual cells otherwise
    DevBuf vbricks;                // uint32 [n[0] + n[1]][32]: occupancy + duplicate brick at the index of a cell's first record
    DevBuf vlist;                  // uint32 [n[0] + n[1]]: occupied cells of cloud 0, then (from n[0]) of cloud 1
    DevBuf vcount;                 // uint32 [2]
    bool vox_rows = false;         // ... and the bricks come with the rows' table below (searches that return the matched row)
    uint64_t vox_rows_pair = 0;    // pair key for which matched rows have been asked for (its later builds keep the table)
    DevBuf vminrow;                // int32 [n[0] + n[1]]: smallest row of every occupied voxel, at the cell's first record + the voxel's
                                   // rank among the set bits of the cell's brick
};

// What the last sort_by_cell job for one PCCM_BUILD_* structure left behind, noted on the host where the sort is called
// (pccm_build_plan / pccm_build_fetch: a diagnostic read-back; no device work)
struct BuildNote {
    bool valid = false;
    uint64_t gen = 0;              // pccm_ctx::scratch_gen of that call: shard structures (and the spatial order's cell starts)
                                   // live in scratch that later calls overwrite
    const void *recs = nullptr;    // the job's first record
    const uint32_t *cs = nullptr, *occ = nullptr;
    bool rec32 = false, morton = false, scan = false, read_sp = false;
    int dim[3] = {1, 1, 1};
    double org[3] = {0, 0, 0}, h[3] = {1, 1, 1};
    int64_t ncells = 0, n = 0, row0 = 0;
    int lg = 0, nbin = 0, njobs = 0, job = 0;
    int64_t tiles = 0, tile_rows = 0, scan_tiles = 0, job_row0[2] = {0, 0}, job_n[2] = {0, 0};
};

struct UnitCol {                // one column reduced from a job's array
    int off;                    // field of the 32-byte result record (0: squared distance, 1: projection); 0 for plain columns
    int square;                 // reduce value^2 (the D2 column from the records' signed projection; metric.py:179)
    double *out_units;          // pinned host memory [3][nunits] per-leaf sum/min/max, or null
    double *out_blocks;         // pinned host memory [3][nblocks] per-32-leaf tree sum/min/max
    double *out_tail;           // pinned host memory [tail_n]
    // a map applied to the value behind the pick and the square (k_unit_jobs alone: reduce_shape() gives a mapped job no lean
    // kernel): PCCM_MAP_CLAMP -- min(value, cap) -- then PCCM_MAP_ROOT -- the correctly rounded square root -- then
    // PCCM_MAP_DENSITY -- 1 - exp(-alpha value) / m, m the match count of the row's matched row (UnitJob::rows / cnt; never
    // with a clamp); 0: none.  PCCM_MAP_MOMENT | kind << 8 -- the alignment moment `kind` of the row (include/pccm.h), the value
    // being d2 and `cap` the inlier bound it is compared with (UnitJob::rows / mom_it / mom_se / pivot); alone
    int map = 0;
    double cap = 0.0;
    double alpha = 0.0;
};
struct UnitJob {                // one per-point array to reduce (k_unit_jobs): up to two columns per pass
    const double *val;          // plain column (stride 1) or the result records (stride 2 or 4 doubles)
    int stride;
    // records of layout 1 (the matched record {rx, ry, rz, row}, 16 bytes): field 0 = the squared distance to row row0 + i of the
    // iterating cloud (q32), field 1 = err . normal[row0 + i] (metric.py:146-153), both formed here -- the rows and the searched
    // cloud's row-indexed normals are read in row order, i.e. coalesced, where the search would have gathered the normal
    int defer;                  // 0: no; 1: normals as 16-byte fp32-exact words (nrm32); 2: as fp64 rows (nrm64); 3: no normals (field 0 only);
                                // 4 / 5: as 1 / 2 with the normal of the MATCHED row (the record's row: --normal-index neighbour)
    int64_t nrm_rows;           // rows of the searched cloud's normals (bounds the gather of 4 / 5)
    const double *nrm64;
    const float4 *nrm32;
    const float4 *q32;          // iterating cloud, one fp32 word per row (Cloud::xyz32r)
    int64_t row0;               // row of the cloud the shard's first record belongs to
    int ncols;
    UnitCol c[2];
    int64_t ns, nunits;
    int64_t tail_first, tail_n; // rows [tail_first, tail_first + tail_n) are copied out raw
    int64_t nblocks;            // ceil(nunits / 32)
    // PCCM_MAP_DENSITY: where the matched row of shard row i is read (matched_row below: the plain idx column, or null -- the
    // records `val` of stride 2 or 4) and the direction's match counts [cnt_rows] (pccm_ctx::match), gathered through it
    const int32_t *rows = nullptr;
    const uint32_t *cnt = nullptr;
    int64_t cnt_rows = 0;
    // PCCM_MAP_MOMENT: the matched rows as above (rows; cnt_rows: the searched cloud's rows), the fp64 coordinates of the iterating
    // cloud (row row0 + i) and of the searched one, and the pivot both are taken relative to
    const double *mom_it = nullptr, *mom_se = nullptr;
    double pivot[3] = {0.0, 0.0, 0.0};
    // k_unit_lean alone: 1 + the entry of TailSettle::d whose filed tails this job's workgroups settle before they reduce, 0: none
    int settle = 0;
};

// the shape SlotShape describes, as the kernels are told it: a job's rows, units and tail ...
inline void bind_shape(UnitJob &U, const SlotShape &s)
{
    U.ns = s.ns; U.nunits = s.nunits; U.nblocks = s.nblocks;
    U.tail_first = s.t0 - s.begin; U.tail_n = s.tail_n;
}
// ... and where in the slot's host buffer a column's results go (the per-leaf results only when somebody will read them)
inline void bind_outputs(UnitCol &c, const SlotView &v, bool want_units)
{
    c.out_units = want_units ? v.usum : nullptr;
    c.out_blocks = v.bsum;
    c.out_tail = v.tail;
}

struct ReduceWhat : SlotShape { // what a reduction slot holds: everything a captured graph's replay has to put back
    bool has_units = false;    // per-leaf results were written (needed by pccm_reduce's exchange vector)
    bool has_job = false;      // job below describes the column (pccm_select_*: a selection ranks what the reduction reduced)
    UnitJob job;               // the column as a one-column k_unit_jobs job, as bound when the reduction was enqueued
};

// the pinned host block a reduction or mapped-reduction slot owns (host_reserve, pccm_api.hip, grows it)
struct SlotHost {
    double *host = nullptr;
    size_t host_cap = 0;
};

struct ReduceSlot : SlotKey, ReduceWhat, SlotHost {   // one enqueued reduction (pccm_reduce_prefetch / pccm_reduce) and what the slot owns
    using What = ReduceWhat;
    DevBuf val;                // (host: SlotShape::host_doubles() doubles at least, SlotView names its regions)

    bool matches(int d, int m, int normal_mode, uint64_t gen_now, bool need_units = false) const
    {
        return SlotKey::matches(d, m, normal_mode, gen_now) && (has_units || !need_units);
    }
};

constexpr int kSlotSelect = 0, kSlotCount = 1;     // SelectWhat::kind
struct SelectWhat {
    int kind = kSlotSelect;
    int64_t k = 0;             // the rank; of a count: the bit pattern of its threshold
};
// one enqueued selection (pccm_select_*) or count (pccm_count_*); it owns nothing: slot s answers into pccm_ctx::sel_host[s]
struct SelectSlot : SlotKey, SelectWhat {
    using What = SelectWhat;

    bool matches(int d, int m, int normal_mode, uint64_t gen_now, int64_t rank, int what = kSlotSelect) const
    {
        return SlotKey::matches(d, m, normal_mode, gen_now) && kind == what && k == rank;
    }
};

// One enqueued mapped reduction (pccm_reduce_map_*): np.sum / min / max of f(column) for the column a reduction slot describes
// (ReduceWhat::job, as a selection ranks it).  It owns no device column -- only its pinned host region: block results and the
// raw tail, laid out by SlotView for `shape`, the column's SlotShape without per-leaf results (nunits 0).  A table of its own:
// a report's up to twenty mapped reductions never evict the plain columns they read.
struct MapWhat {
    SlotShape shape;
    int map = 0;
    uint64_t cap_bits = 0;     // map_cap_bits(map, cap) (PCCM_MAP_DENSITY: of alpha)
};
struct MapSlot : SlotKey, MapWhat, SlotHost {      // (host: shape.host_doubles() doubles at least)
    using What = MapWhat;

    bool matches(int d, int m, int normal_mode, uint64_t gen_now, int which_map, uint64_t bits) const
    {
        return SlotKey::matches(d, m, normal_mode, gen_now) && map == which_map && cap_bits == bits;
    }
};

struct ProfSpan {
    hipEvent_t a, b;
    int cls;
};

struct GraphOp {               // host-side effect of one captured call, replayed by pccm_graph_launch
    int kind = 0;              // 0 drop_caches, 1 nn(dir), 2 reduce_prefetch(slot), 3 select_prefetch / count_prefetch(slot),
                               // 4 reduce_map_prefetch / reduce_density_prefetch / reduce_moment_prefetch(slot), 5 match counts(dir)
    int dir = 0, slot = -1;
    NNForm form;               // kind 1: where the direction's results live once the graph has run
    // kinds 2, 3, 4 (2 + index()): the slot's key and description at capture time (pccm_slot.h)
    std::variant<SlotSnap<ReduceWhat>, SlotSnap<SelectWhat>, SlotSnap<MapWhat>> snap;
};

struct GraphRec {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    std::vector<GraphOp> ops;
    uint64_t epoch = 0;        // pccm_ctx::epoch it was captured under
    uint64_t batches = 0;      // reduction batches in it that publish on the completion counter (each replay adds as many)
    bool tails_filed = false;  // the searches' tails are settled by the reductions: no tail launch in it (pccm_set_tail_filing)
    bool valid = false;
};

struct FiledTails;               // pccm_tail_wave.h
struct TailSettle;

}  // namespace pccm

struct pccm_ctx {
    // one context = one caller at a time: every entry point holds this for its whole duration (recursive: entry points
    // call each other), so threads that share a context by mistake are serialised instead of corrupting it
    std::recursive_mutex mu;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t copy_stream = nullptr;     // deferred uploads (pccm_set_normals_deferred): they run beside the main stream's kernels
    pccm::DevBuf staging2;                 // ... through a staging buffer of their own
    // Large transfers between the CALLER's arrays and the device can go through pinned buffers of the context's own
    // (pccm_set_io_staged; off by default): the runtime otherwise pins the caller's pages itself and keep the mapping cached, and when the caller later
    // frees such an array the driver evicts and restores every queue of the process -- 13-27 ms during which a running kernel
    // stands still (measured: DESIGN.md section 4).  [0]: uploads on the main stream, [1]: on the copy stream, [2]: downloads.
    void *pin[3] = {nullptr, nullptr, nullptr};      // (at most 64 MB each: larger transfers reuse the buffer window by window)
    size_t pin_cap[3] = {0, 0, 0};
    hipEvent_t pin_ev[2] = {nullptr, nullptr};      // the last upload's copies out of pin[0] / pin[1] have been issued up to here
    bool pin_ev_set[2] = {false, false};
    bool io_staged = false;
    pccm::Cloud cloud[2];
    // query-axis shard per direction (pccm_set_shard / pccm_set_shard_dir): this context owns the rows shard_of(n, rank,
    // world) of the iterating cloud; world 0 = none of them (another group of ranks searches that direction)
    int shard_rank[3] = {0, 0, 0}, shard_world[3] = {1, 1, 1};
    bool sharded() const { return shard_world[0] != 1 || shard_world[1] != 1 || shard_world[2] != 1; }
    pccm::NNResult nn[3];
    // pccm_set_ties: PCCM_TIES_MEAN replaces the matched point of directions 0 and 1 by the mean of all equidistant nearest
    // points (tie_mean, pccm_grid.hip): per shard row the virtual neighbour's position, tie count and -- when asked for --
    // averaged normal and colour; valid for the search generation / colour upload / normals they were made from
    int ties = PCCM_TIES_PICK;
    struct TieCols {
        pccm::DevBuf pos, nrm, rgb, k, ang;
        uint64_t gen = 0, rgb_gen = 0, nrm_gen = 0, ang_gen = 0;   // 0: not made (ang: both clouds' normals, ctx->nrm_gen)
    } tie[2], tie_rows;                   // tie_rows: the whole iterating cloud, from caller-supplied rows (sharded colours)
    pccm::DevBuf tie_list;                // queries left to the exact scan (k_tie_mean_scan): [0] count, then shard rows
    uint64_t nrm_gen = 1;                 // bumped whenever any normals change
    // pccm_carry_normals: cloud `to` holds normals carried over from the other cloud (-1: neither does), made from the searches
    // whose run counts (nn_run) are run_f (the direction that iterates the source cloud) and run_g; whatever changes either cloud's
    // points or the source cloud's normals drops them (points_changed / normals_changed, pccm_stale.h)
    struct Carry {
        int to = -1;
        uint64_t run_f = 0, run_g = 0;
    } carry;
    uint64_t nn_run[3] = {0, 0, 0};       // searches of each direction so far (prepare_nn): which RESULT a direction holds -- nn_gen
                                          // also moves when normals or features change under a result that stays
    pccm::DevBuf carry_ws;                // pccm_carry_normals: header, counts, fills, segment starts, row lists, long-list queue
                                          // (pccm_merge_duplicates' colour averages run the same passes through it)
    // pccm_merge_duplicates: merge_map[k] holds, for each of the merge_n[k] rows cloud k had before its rows were merged, the merged
    // row of its group (merge_n 0: never merged, the map is the identity); new points for the cloud and pccm_ctx_reset clear it
    pccm::DevBuf merge_map[2];
    int64_t merge_n[2] = {0, 0};
    pccm::DevBuf merge_refl;              // ... and for a cloud with reflectance: the merged column [n], then (PCCM_DUP_AVERAGE) the averages by original row [n]
    pccm::DevBuf merge_ws;                // ... its workspace (merge_layout): averaged colours, merged rows, group table, scan words
    // scratch
    pccm::DevBuf part_b1, part_g, part_b2, val, stats, staging, counters;
    pccm::DevBuf rescan_part;             // k2b_fallback's split regime: partial minima per (query, workgroup)
    pccm::DevBuf ssim_scratch;            // pccm_ssim_features: neighbour rows [n][k] + curvatures [n]; pccm_p2d_build: neighbour rows [n][k]
    // point-to-distribution columns (pccm_p2d_build): M of every point of cloud d against the other cloud's k nearest points, valid
    // for neighbourhood size p2d_k (0: not built; new points in either cloud drop both)
    double *p2d64[2] = {nullptr, nullptr};
    size_t cap_p2d[2] = {0, 0};
    int p2d_k = 0;
    // ... and their colour [0] and joint [1] columns per direction (PCCM_P2D_COLOR), valid while p2d_color is set (then at p2d_k):
    // new colours in either cloud drop these and keep the geometry columns
    double *p2d_cj64[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    size_t cap_p2d_cj[2][2] = {{0, 0}, {0, 0}};
    bool p2d_color = false;
    pccm::DevBuf tail_sync;               // k_grid_tail: retired-entry counts + ticket, for the normal and the self pass
    bool tail_sync_clean = false;
    // filed tails (pccm_tail_wave.h): inside a capture the pair's brick search files its unsettled queries by row block and leaves
    // the tail launch out; the reduction of each direction settles them (k_unit_lean's settling head)
    struct TailFile {
        bool wish = false;                // the capture in progress may file (on from pccm_graph_begin; pccm_set_tail_filing)
        bool allowed = false;             // the capture rule held for the eager step in front of this capture (pccm_graph_begin) ...
        int fact_dirs = 0;                // ... bit d: direction d's lists were among those it read (a search of any other files nothing)
        bool left_out = false;            // the capture in progress has left a tail launch out ...
        bool resolved = false;            // ... and put it back for a reader other than the settling reduction
        pccm::DevBuf cnt, list;           // uint32 [blocks of dir 0 | of dir 1], float4 [the same][kTailBlockCap]
        uint64_t brick_key = 0;           // Grid::key / ncells of the last eager pair search when the brick kernel ran it on whole
        int64_t brick_ncells = 0;         // clouds (0: it did not): the lists the capture rule reads are that search's
        int eager_ok = 0, eager_bad = 0;  // bit d: since that search, a reduction batch read direction d's records and could have
                                          // settled its tails / could not (launch_unit_jobs).  A hint for speed alone: it keeps a
                                          // capture from filing what its reductions will not settle (the brick kernel would file
                                          // and the classic launch run all the same).  A wrong value costs time, never a result:
                                          // whoever reads a filed direction settles it or has it resolved first
        pccm::FiledTails *state = nullptr; // what the search left for whoever consumes the lists
    } tail_file;
    pccm::DevBuf color_cols, color_idx;   // colour pass: squares as three columns / caller-supplied neighbour rows
    pccm::DevBuf colsum_scratch;          // ... the column sums' chunk guesses and sub-chunk totals (pccm_color.hip)
    bool colsum_configured = false;       // k_colsum_chain's LDS opt-in was set on this context's device
    // pccm_color_reduce works on BOTH directions when it can (the same launches serve two column triples; the walk behind
    // NumPy's summation order is one wave's latency however many run side by side) and keeps the other direction's answer
    // here until that direction is asked for -- or a search, new colours or another scheme make it stale
    struct ColorMemo {
        bool valid = false, range_bad = false;
        int dir = 0, scheme = 0;
        double scale = 0.0, sum[3] = {0, 0, 0}, max[3] = {0, 0, 0};
        uint64_t gen = 0, rgb_gen = 0;
    } color_memo;
    uint64_t rgb_gen = 1;                 // bumped by every colour upload
    pccm::Grid grid;
    pccm::DevBuf g_cell_of, g_rank, g_hist, g_blocksum, g_qrecs;   // grid-engine scratch (g_qrecs: cell-sorted shard rows)
    pccm::DevBuf g_bins, g_tmp;            // grid build: per-tile bin histogram + scan state; bin-partitioned records
    hipEvent_t batch_ev = nullptr;   // recorded once behind every batch of reductions (SlotKey::wait_ev)
    // completion counter: k_publish, behind the last kernel of a reduction batch, adds 1 to *done (host-coherent pinned memory, a
    // cache line of its own) when the batch's results are on the host; batches_issued counts the publishing batches enqueued
    // so far, so a slot waits for *done to reach the count its batch was given (SlotKey::wait_seq) -- a spin on host
    // memory instead of the runtime's event completion path (pccm_set_wait)
    uint64_t *done = nullptr;
    uint64_t batches_issued = 0;
    uint64_t cap_batches = 0;        // ... publishing batches recorded by the capture in progress
    int wait_mode = PCCM_WAIT_SPIN;
    // device error word (pinned host memory the kernels can write): a kernel that meets a state it cannot be in -- a cell start
    // that contradicts the occupancy brick (pccm_vox.hip), a tail wait that ran out (k_grid_tail) -- sets a bit instead of
    // answering wrongly in silence; every call that hands results to the caller checks it behind its wait (check_device_errors)
    uint32_t *host_err = nullptr;
    bool bins_clean = false;   // the build's bin cursors (head of g_bins) are zero on the stream
    pccm::BuildNote builds[PCCM_BUILD_COUNT];   // what the builds left, per structure (pccm_build_plan)
    uint64_t scratch_gen = 0;  // bumped by whatever writes g_hist / g_qrecs: sort_by_cell, measure_occupancy, spatial_order
    int want_idx = 1;                      // pccm_nn_want_idx: searches store the matched row with every result
    int fuse_mode[3] = {-1, -1, -1};       // pccm_nn_fuse: normal mode of the D2 projection fused into the search, per direction
    pccm::ReduceSlot slots[24];           // (a report with every PointSSIM and point-to-distribution row holds up to 21 columns at once)
    // selections (pccm_select_*): slot s answers into sel_host[s] (host-coherent pinned memory); the histograms and pass states
    // are sized once per context
    static constexpr int kSelSlots = 32;
    pccm::SelectSlot sel_slots[kSelSlots];
    double *sel_host = nullptr;
    pccm::DevBuf sel_hist, sel_state;
    // mapped reductions (pccm_reduce_map_*): a report asks for up to twenty (two directions x D1 / D2 roots, and per threshold
    // the clamp and the clamped root of both directions)
    static constexpr int kMapSlots = 32;
    pccm::MapSlot map_slots[kMapSlots];
    // match counts (pccm_match_counts, the density-aware Chamfer terms): per direction 0 / 1 one uint32 per row of the SEARCHED
    // cloud -- how many shard rows matched it --, made once per search and valid while gen equals nn_gen[dir] (0: not made)
    struct MatchCounts {
        pccm::DevBuf buf;
        uint64_t gen = 0;
    } match[2];
    // the pivot (bit patterns) the pending alignment moments among the mapped-reduction slots were made with: a call with another
    // pivot gives them up (pccm_reduce_moment_*)
    uint64_t moment_pivot[3] = {0, 0, 0};
    // pccm_transform_cloud writes the moved rows here and swaps the buffer with the cloud's (grow() allocates both)
    double *xf_scratch = nullptr;
    size_t cap_xf = 0;
    uint64_t nn_gen[3] = {1, 1, 1};
    // hipGraph capture of a step (pccm_graph_*): epoch changes whenever inputs, shard or any device
    // buffer a captured kernel may reference changes, which invalidates every recorded graph
    uint64_t epoch = 1;
    bool capturing = false, capture_failed = false;
    std::vector<pccm::GraphOp> cap_ops;
    std::vector<pccm::GraphRec> graphs;
    // profiling
    bool prof_on = false;
    std::vector<pccm::ProfSpan> spans;
    std::vector<hipEvent_t> event_pool;
    double prof_ms[PCCM_K_COUNT] = {0};
    int64_t prof_n[PCCM_K_COUNT] = {0};
    // path log (pccm_nn_path): the kernels the last search of each direction ([0..2]) and the last reduction batch ([3]) enqueued,
    // as host kernel handles in launch order without repeats; noted by PCCM_LAUNCH into the logs of path_mask
    static constexpr int kPathMax = 64;
    const void *path[4][kPathMax] = {};
    int path_n[4] = {0, 0, 0, 0};
    bool path_over[4] = {false, false, false, false};   // a kernel did not fit: pccm_nn_path reports the list as incomplete
    unsigned path_mask = 0;
    // pccm_voxel_occupancy: its table, seen words and tallies (occupancy_layout), then the tallies of up to kOccupancyMax sizes
    // gathered for one copy back.  A buffer of its own: merge_ws holds the merged rows a cloud may still be read from
    pccm::DevBuf occupancy_ws;      // (last: every other member keeps its place)
};

namespace pccm {

// a captured batch is about to run (again): its slot waits for the context's batch event, or for the completion counter to reach
// the batch's ordinal in the captured sequence (snap_seq, 0: the event only) counted from the batches issued so far
inline void rearm(SlotKey &k, const pccm_ctx *ctx, uint64_t snap_seq)
{
    k.wait_ev = ctx->batch_ev;
    k.wait_seq = snap_seq ? ctx->batches_issued + snap_seq : 0;
}

// every slot of the three tables
template <class F>
inline void for_each_slot(pccm_ctx *ctx, F f)
{
    for (auto &s : ctx->slots) f(s);
    for (auto &s : ctx->sel_slots) f(s);
    for (auto &s : ctx->map_slots) f(s);
}

// ... and the table a captured op's snapshot belongs to
inline auto &table_of(pccm_ctx *ctx, const SlotSnap<ReduceWhat> &) { return ctx->slots; }
inline auto &table_of(pccm_ctx *ctx, const SlotSnap<SelectWhat> &) { return ctx->sel_slots; }
inline auto &table_of(pccm_ctx *ctx, const SlotSnap<MapWhat> &) { return ctx->map_slots; }

// error plumbing ---------------------------------------------------------------------
int fail(int code, const char *fmt, ...);
#define PCCM_HIP(expr)                                                                        \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return ::pccm::fail(_e == hipErrorOutOfMemory ? PCCM_E_OOM : PCCM_E_HIP, "%s: %s", \
                                #expr, hipGetErrorString(_e));                                \
    } while (0)

int ensure(pccm_ctx *ctx, DevBuf &b, size_t bytes);
int grow(void **p, size_t &cap, size_t bytes);      // (re)allocate *p to hold `bytes`; keeps a buffer that is large enough

// path log: note a kernel handle in every log of ctx->path_mask (host bookkeeping only: no GPU work, no synchronisation)
inline void note_kernel(pccm_ctx *ctx, const void *k)
{
    for (int l = 0; l < 4; ++l) {
        if (!(ctx->path_mask & (1u << l))) continue;
        int i = 0;
        while (i < ctx->path_n[l] && ctx->path[l][i] != k) ++i;
        if (i < ctx->path_n[l]) continue;
        if (i < pccm_ctx::kPathMax) ctx->path[l][ctx->path_n[l]++] = k;
        else ctx->path_over[l] = true;
    }
}

// hipLaunchKernelGGL that also notes the kernel in the path log
#define PCCM_LAUNCH(ctx, kernel, ...)                                                   \
    do {                                                                                \
        ::pccm::note_kernel((ctx), reinterpret_cast<const void *>(&(kernel)));          \
        hipLaunchKernelGGL(kernel, __VA_ARGS__);                                        \
    } while (0)
// ... through a pointer to the kernel's host stub (a table entry): the pointer's value is the handle, not its address
#define PCCM_LAUNCH_STUB(ctx, stub, ...)                                                \
    do {                                                                                \
        ::pccm::note_kernel((ctx), reinterpret_cast<const void *>(stub));               \
        hipLaunchKernelGGL(stub, __VA_ARGS__);                                          \
    } while (0)

// while alive, launches are noted in the logs of `mask` (bit d: search of direction d, bit 3: reduction batch), which start
// empty unless `keep` (work a search leaves for later -- tie means, tie exposure -- joins that search's log)
struct PathScope {
    pccm_ctx *ctx;
    unsigned saved;
    PathScope(pccm_ctx *c, unsigned mask, bool keep = false) : ctx(c), saved(c->path_mask)
    {
        for (int l = 0; l < 4; ++l)
            if ((mask & (1u << l)) && !keep) {
                ctx->path_n[l] = 0;
                ctx->path_over[l] = false;
            }
        ctx->path_mask = mask;
    }
    ~PathScope() { ctx->path_mask = saved; }
};

struct ProfScope {   // records a HIP-event pair around a launch group when profiling is on
    pccm_ctx *ctx;
    int cls;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(pccm_ctx *c, int k);
    ~ProfScope();
};

// kernel launchers (each returns PCCM_OK or an error) -----------------------------------
// The transforming mode of the two ingest kernels (pccm_transform_cloud): on != 0 -- every row read from `src` is mapped by the
// row-major 3 x 4 matrix m = [A | t] before it is ingested (normals: by A alone), one rounding per operation.  The source rows
// are the context's own fp64 rows, so the launcher is given a destination that is NOT the source (the kernels' pointers are
// __restrict__, and a normal's thread reads its whole row).
struct IngestMove {
    int on = 0;
    double m[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
};
int launch_ingest_points(pccm_ctx *ctx, const void *src, int dtype, int64_t n, int64_t n_pad, float4 *x32,
                         double *x64, float4 *x32r, unsigned long long *stats /*[3] device*/, const IngestMove *move = nullptr);
int launch_ingest_normals(pccm_ctx *ctx, const void *src, int dtype, int64_t n, double *out, float *out32,
                          unsigned long long *stats, const IngestMove *move = nullptr);

// brute-force engine: fills res.idx / res.d2 for rows [res.begin, res.end) of `it` searched in `se`
int nn_brute(pccm_ctx *ctx, const Cloud &it, const Cloud &se, bool self, NNResult &res);
// grid engine
int nn_grid(pccm_ctx *ctx, int ndirs, const int *dirs, int force_idx = 0);   // force_idx: records carry the matched row whatever pccm_nn_want_idx says
// filed tails: the classic tail launch over the lists nobody has consumed (every direction that says tails_filed), for a reader
// other than the settling reduction; no-op when there are none
int filed_tails_resolve(pccm_ctx *ctx);
// ... the kernel argument of the settling reduction and the entry of it that direction `dir` is (-1: not filed)
const TailSettle *filed_tails_settle(const pccm_ctx *ctx, int dir, int *entry);
int tail_facts(pccm_ctx *ctx, bool *allowed, int *dirs);      // the capture rule on the last eager step's lists (pccm_graph_begin)
void grid_release(pccm_ctx *ctx);
void grid_invalidate(pccm_ctx *ctx);
int grid_ensure(pccm_ctx *ctx, bool need64 = false, int need_mask = 3);
int build_plan(pccm_ctx *ctx, int which, int64_t *plan, double *geom);       // pccm_build_plan / pccm_build_fetch: what a build left
int build_fetch(pccm_ctx *ctx, int which, uint32_t *cell_start, int32_t *rows, double *xyz, uint32_t *occ);
int grid_ensure_solo(pccm_ctx *ctx, int which);    // GridRec grid over cloud `which` alone, cells sized for it (normal estimation)   // need64: GridRec records wanted (pccm_knn.hip reads them)
int spatial_order(pccm_ctx *ctx, Cloud &c);      // fills Cloud::sp (ingest; no-op for clouds that are not fp32-exact)
int grid_decide(pccm_ctx *ctx, bool *hostile);   // geometry decision for the current pair (cached per pair)
int grid_prefers_brute(pccm_ctx *ctx, bool *yes); // builds the grid if needed; isolation verdict (cached per pair)
int estimate_normals(pccm_ctx *ctx, int which, int k);
int ssim_features(pccm_ctx *ctx, int which, int k, int attrs, int *built);   // the checks are pccm_ssim_features'
int p2d_build(pccm_ctx *ctx, int k, int attrs, int *built);                  // the checks are pccm_p2d_build_attrs'
int resolution_build(pccm_ctx *ctx, int which, int K, int *built);           // the checks are pccm_resolution_build's
int p2d_neighbours(pccm_ctx *ctx, int dir, int k, const int32_t **nbr, const int32_t **cnt);   // device lists [n][k], [n]
int tie_exposure(pccm_ctx *ctx, int dir, const Cloud &it, const Cloud &se, const NNResult &res, int normal_mode, double out[8]);
// PCCM_TIES_MEAN producer: for the ns queries q_begin.. of direction dir (matched rows idx, squared distances d2 or null = formed
// from idx) the ascending-row mean of all equidistant nearest points -> pos[ns][3], k[ns]; nrm / rgb likewise when snrm / srgb;
// ang[ns] when ang: the mean over the tie set of PCCM_METRIC_ANGULAR (the iterating cloud's normals inrm against the searched
// cloud's anrm)
int tie_mean(pccm_ctx *ctx, int dir, const int32_t *idx, const double *d2, int64_t q_begin, int64_t ns, const double *snrm,
             const double *srgb, double *pos, int32_t *k, double *nrm, double *rgb, const double *inrm = nullptr,
             const double *anrm = nullptr, double *ang = nullptr);
int check_device_errors(pccm_ctx *ctx);
int normals_ready(pccm_ctx *ctx, Cloud &c);       // uploads normals announced by pccm_set_normals_deferred (no-op otherwise)           // PCCM_E_STATE when a kernel raised the context's device error word
// exact rescan of the flagged queries of njobs <= 2 results (k2b_fallback)
int launch_fallback(pccm_ctx *ctx, int njobs, const Cloud *const *its, const Cloud *const *ses, NNResult *const *ress, bool self);

constexpr int kSplitMax = 32;   // flagged queries up to which the rescan splits the cloud instead of the list
struct RescanJob {              // flagged queries of one result (k2b_fallback)
    const float *q32, *r32;     // fp32 quad layouts of the iterating / searched cloud
    const double *q64, *r64;
    int64_t q_begin, nr;
    const int32_t *flagged;     // rows relative to q_begin
    const float *flag_thr;      // fp32 filter threshold of each
    const uint32_t *nflag;      // list length (device)
    int32_t *idx_out;           // plain outputs (brute-force engine) ...
    double *d2_out;
    double *rec_out;            // ... or result records with the projection fused (grid engine), when non-null
    int rec_stride;             // doubles per record (NNForm::stride)
    int rec_layout;             // NNForm::layout
    const double *nrm;          // normals for the fused projection, or null
    int normal_mode;
    double *part_d;             // split regime: [kSplitMax][gridDim.x] partial minima
    int32_t *part_j;
    uint32_t *ticket;           // split regime: workgroups done (self-resetting)
};
struct RescanJobs {
    RescanJob j[2];
    int njobs;
};

// inclusive scan of v over the wave's 64 lanes (lane: the caller's lane)
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}

// The matched row of shard row i of a direction's result, read where the search left it: the plain idx column (the brute-force
// engine; results unpacked by ensure_plain), or -- idx null -- in place from the result records: the row word of a matched record
// (stride 2, NNForm::kMatched: rec.w, as matched_fields reads it) or the row field of a pair record (stride 4,
// NNForm::kPairRows: the low word of field 2, as k_unpack reads it).  The match-count pass and the density map both read through it.
__device__ __forceinline__ int32_t matched_row(const int32_t *idx, const double *rec, int stride, int64_t i)
{
    if (idx) return idx[i];
    if (stride == 4) return *reinterpret_cast<const int32_t *>(rec + 4 * i + 2);
    return __float_as_int(reinterpret_cast<const float4 *>(rec)[i].w);
}

// PCCM_METRIC_ANGULAR of one pair of normals (include/pccm.h): every operation separately rounded, as NumPy's element-wise ops
__device__ __forceinline__ double angular_similarity(const double *a, const double *b)
{
    const double dot = __dadd_rn(__dadd_rn(__dmul_rn(a[0], b[0]), __dmul_rn(a[1], b[1])), __dmul_rn(a[2], b[2]));
    const double na2 = __dadd_rn(__dadd_rn(__dmul_rn(a[0], a[0]), __dmul_rn(a[1], a[1])), __dmul_rn(a[2], a[2]));
    const double nb2 = __dadd_rn(__dadd_rn(__dmul_rn(b[0], b[0]), __dmul_rn(b[1], b[1])), __dmul_rn(b[2], b[2]));
    const double den = __dsqrt_rn(__dmul_rn(na2, nb2));
    if (den == 0.0) return 0.0;                                   // a zero-length normal: perpendicular
    const double q = __ddiv_rn(fabs(dot), den);
    const double c = q > 1.0 ? 1.0 : q;                           // np.minimum(q, 1.0) (a NaN stays NaN)
    return __dsub_rn(1.0, __ddiv_rn(__dmul_rn(2.0, acos(c)), M_PI));
}

// PCCM_METRIC_SSIM_*: a point's feature a against its matched point's b (include/pccm.h), every operation separately rounded
__device__ __forceinline__ double ssim_similarity(double a, double b)
{
    const double num = fabs(__dsub_rn(a, b));
    const double den = __dadd_rn(fmax(fabs(a), fabs(b)), 0x1.0p-52);
    return __dsub_rn(1.0, __ddiv_rn(num, den));
}

// (PCCM_METRIC_P2D, _P2D_COLOR and _P2D_JOINT are stored columns: pccm_api.hip binds them, no point kernel sees them)
__host__ __device__ __forceinline__ bool is_p2d_metric(int metric)
{
    return metric >= PCCM_METRIC_P2D && metric <= PCCM_METRIC_P2D_JOINT;
}

// every column kept in HBM and bound as it is (ColumnSource::kStored): the point-to-distribution columns of a direction, and the
// spacing column (PCCM_METRIC_RESOLUTION, pccm_resolution_build) of the cloud the direction iterates
__host__ __device__ __forceinline__ bool is_stored_metric(int metric)
{
    return is_p2d_metric(metric) || metric == PCCM_METRIC_RESOLUTION;
}

__host__ __device__ __forceinline__ bool is_ssim_metric(int metric)
{
    return metric >= PCCM_METRIC_SSIM_GEOMETRY && metric <= PCCM_METRIC_SSIM_COLOR;
}

// PCCM_METRIC_REFLECTANCE: a point's reflectance a against its matched point's b (include/pccm.h), each operation separately rounded
__device__ __forceinline__ double reflectance_error(double a, double b)
{
    const double d = __dsub_rn(a, b);
    return __dmul_rn(d, d);
}

// One per-point column formed from a search result (k_point_jobs, the only kernel that forms them): D2 / PROJ / ANGULAR / SSIM_* / REFLECTANCE as
// [ns] values, or -- PCCM_METRIC_D1 -- the error vectors as [ns][3] rows.  pccm_api.hip fills it in one place (point_job_fill), for
// the reduction batches and the one-job launches of pccm_point_metric / pccm_error_vectors alike.
struct PointJob {
    const double *q64, *r64, *nrm;
    const double *c64, *cn64;   // PCCM_TIES_MEAN: per shard row the virtual neighbour / its averaged normal (null: gather via idx)
    const double *inrm;         // PCCM_METRIC_ANGULAR: the iterating cloud's normals (nrm: the searched cloud's); PCCM_METRIC_SSIM_*:
                                // the iterating cloud's feature column (nrm: the searched cloud's); PCCM_METRIC_REFLECTANCE: the
                                // iterating cloud's reflectance column (nrm: the searched cloud's)
    const float4 *recs;         // PCCM_METRIC_ANGULAR / SSIM_* / REFLECTANCE: matched records {x, y, z, row} (NNForm::layout 1) instead of idx, or null
    const int32_t *idx;
    int64_t q_begin;
    int metric, normal_mode;
    double *val;                // [ns], or [ns][3] (PCCM_METRIC_D1)
};
constexpr uint32_t kErrMergeTable = 4u;            // device error word: a probe sequence of pccm_merge_duplicates ran through the whole table
// The workspace of pccm_merge_duplicates for a cloud of n rows.  Doubles first: the averaged colours [n][3] (by original row; only
// representatives are written), then the merged points, normals and colours [n][3] each.  Then uint32 words: head[4] ([0] = n'),
// the representative masks [2 * nw] (one 64-bit word per wave of 64 rows), rep[n], the waves' counts and then exclusive prefixes
// wpre[nw], the same per 64 waves spre[nsw], and the table [cap], cap = the power of two >= 2 n.
struct MergeLayout {
    int64_t nw, nsw;                // waves of 64 rows; groups of 64 waves
    uint64_t cap;
    size_t doubles;                 // 12 n
    size_t bits, rep, wpre, spre, table, words;      // offsets (and the total) in uint32 words behind the doubles
    size_t bytes() const { return doubles * sizeof(double) + words * sizeof(uint32_t); }
};
__host__ __device__ inline MergeLayout merge_layout(int64_t n)
{
    MergeLayout L;
    L.nw = (n + 63) / 64;
    L.nsw = (L.nw + 63) / 64;
    L.cap = 64;
    while (L.cap < 2 * (uint64_t)n) L.cap <<= 1;
    L.doubles = (size_t)12 * (size_t)n;
    L.bits = 4;
    L.rep = L.bits + 2 * (size_t)L.nw;
    L.wpre = L.rep + (size_t)n;
    L.spre = L.wpre + (size_t)L.nw;
    L.table = L.spre + (size_t)L.nsw;
    L.words = L.table + (size_t)L.cap;
    return L;
}
// The workspace of pccm_voxel_occupancy for clouds of n1 and n2 rows, in uint32 words: the table [cap] over the joint rows, cap =
// the power of two >= 2 (n1 + n2) and >= 64; seen [n1] (one word per row of cloud 0: a row of cloud 1 has met the voxel it
// represents); the three 64-bit tallies on an 8-byte boundary (the base is at least that aligned).  seen and the tallies are
// cleared by one memset.
constexpr int kOccupancyMax = 4;                   // voxel sizes per pccm_voxel_occupancy call
struct OccupancyLayout {
    uint64_t cap;
    size_t table, seen, tally, words;              // offsets (and the total) in uint32 words
    size_t bytes() const { return words * sizeof(uint32_t); }
};
__host__ __device__ inline OccupancyLayout occupancy_layout(int64_t n1, int64_t n2)
{
    OccupancyLayout L;
    const uint64_t n = (uint64_t)n1 + (uint64_t)n2;
    L.cap = 64;
    while (L.cap < 2 * n) L.cap <<= 1;
    L.table = 0;
    L.seen = (size_t)L.cap;
    L.tally = (L.seen + (size_t)n1 + 1) & ~(size_t)1;
    L.words = L.tally + 6;
    return L;
}
struct PointJobs {
    PointJob j[4];
    int njobs;
    int64_t off[5];             // prefix sums of the jobs' row counts
};
// Selection mode of k_unit_jobs (pccm_select_*): the k-th smallest value of a job's column 0, by a radix select over the order
// keys of the values unit_load / unit_pick form -- the values the reduction mode reduces.  kSelBits key bits per launch from the
// top down; launch p histograms the rows whose higher bits equal the prefix that launches 0..p-1 settled, and the launch boundary
// is the only synchronisation: every workgroup of launch p derives that prefix for itself from launch p-1's counts.
constexpr int kSelBits = 11, kSelBins = 1 << kSelBits;
constexpr int kSelPasses = 6;       // 6 x 11 >= 64 (the last pass holds the 9 lowest bits)
constexpr int kSelMax = 8;          // selections per launch sequence ...
constexpr int kSelPerCol = 4;       // ... of which at most this many rank one column (one 8 KB LDS histogram each)
constexpr size_t kSelLds = (size_t)kSelPerCol * kSelBins * sizeof(uint32_t) + 256;   // LDS of the selection mode
// Count mode of k_unit_jobs (pccm_count_*), the inverse query: how many rows of a job's column 0 are <= x, for up to kSelMax
// thresholds per launch sequence, kSelPerCol per column -- one streaming pass over the same values and one workgroup that stores.
constexpr int kSelCountPass = kSelPasses + 2, kSelStorePass = kSelPasses + 3;       // UnitSelect::pass of its two launches
struct SelState {
    unsigned long long prefix;  // the settled high bits of the key (zero below them)
    unsigned long long k;       // rank among the rows that share them (1-based)
};
struct UnitSelect {
    int pass = 0;               // 0: a reduction launch.  1..kSelPasses: histogram pass `pass - 1`; kSelPasses + 1: resolve and store;
                                // kSelCountPass: count rows <= x; kSelStorePass: store the counts
    int nsel = 0;
    int sfirst[9] = {};         // selections sfirst[j] .. sfirst[j + 1] - 1 rank column 0 of job j
    int boff[9] = {};           // prefix sums of the jobs' workgroups in a histogram pass
    unsigned long long k[kSelMax] = {};   // 1-based ranks (count mode: the bit patterns of the thresholds)
    double *out[kSelMax] = {};  // pinned host memory: one double per selection (count mode: one 64-bit count in its place)
    uint32_t *hist = nullptr;   // [kSelPasses][kSelMax][kSelBins], zeroed on the stream before pass 0 (count mode: the first
                                // kSelMax words are the counters, zeroed before the count launch)
    SelState *state = nullptr;  // [kSelPasses][kSelMax]: what pass p matched and ranked by (written by pass p, read by pass p + 1)
};
struct UnitJobs {
    UnitJob j[8];
    int njobs;
    int64_t uoff[9];            // prefix sums of 8 * nunits, each rounded up to a multiple of 256
    int64_t toff[9];            // prefix sums of tail_n
    UnitSelect sel;             // sel.pass != 0: a selection launch (uoff / toff are not read)
};
static_assert(sizeof(UnitJobs) <= 4096, "UnitJobs is passed by value: it must fit the 4 KB of kernel arguments");
// the rescan jobs of njobs <= 2 results (scratch allocated), for k2b_fallback or the rescan half of k_grid_tail
int rescan_jobs(pccm_ctx *ctx, int njobs, const Cloud *const *its, const Cloud *const *ses, NNResult *const *ress, bool self, RescanJobs *out);
constexpr unsigned kRescanCap = 512;   // most workgroups that ever share one job's list (sizes the split regime's partials)
int launch_point_jobs(pccm_ctx *ctx, const PointJobs &jobs);
// pccm_carry.hip: the passes of pccm_carry_normals on the stream (the caller has checked everything and sized ws: carry_ws_bytes).
// nn_f [n_from] / nn_g [n_to]: the matched rows of the two directions; nn_g null: rows of `out` that no row of nn_f names are left
// alone (pccm_merge_duplicates)
size_t carry_ws_bytes(int64_t n_from, int64_t n_to);
// nc: the doubles per row of n_from64 and out -- 3 (normals, colours) or 1 (a scalar column: the reflectance)
int launch_carry(pccm_ctx *ctx, const int32_t *nn_f, const int32_t *nn_g, const double *n_from64, int64_t n_from, int64_t n_to,
                 uint32_t *ws, double *out, int nc);
// the carry's count pass alone, for a direction's match counts: cnt [n_to] zeroed on the stream (a memset), then k_carry_count
// over the ns shard rows, whose matched rows are read through matched_row(idx, rec, stride, i)
int launch_match_counts(pccm_ctx *ctx, const int32_t *idx, const double *rec, int stride, int64_t ns, int64_t n_to, uint32_t *cnt);
inline size_t merge_ws_bytes(int64_t n) { return merge_layout(n).bytes(); }
// pccm_merge_duplicates on the stream, in two halves with the caller's read of n' (head[0] of the workspace's words) between them:
// table filled, insert | find | the two scans; then -- rows were merged away -- the gather into `out` (rgb: the colours to keep
// per representative row, the cloud's own or the averages).  `words`: the uint32 part of the workspace (MergeLayout)
int launch_merge_find(pccm_ctx *ctx, const double *x64, int64_t n, uint32_t *words);
// pccm_voxel_occupancy for one voxel size on the stream: the table filled, seen and the tallies cleared, then the insert and the
// find of the merge in their occupancy mode over the joint rows (x0's n1, then x1's n2).  `words`: an OccupancyLayout
int launch_occupancy(pccm_ctx *ctx, const double *x0, int64_t n1, const double *x1, int64_t n2, double voxel, uint32_t *words);
// refl / refl_out: the reflectance to keep per representative row [n] (the cloud's own column or the averages) and the merged
// column [n] (written), or both null
int launch_merge_gather(pccm_ctx *ctx, const double *x64, const double *nrm, const double *rgb, const double *refl, int64_t n, double *out,
                        double *refl_out, uint32_t *words, int32_t *map);
// pccm_point.hip: the reflectance ingest -- src [n] of PCCM_F32 or PCCM_F64 widened exactly into out [n] (the normals' widening
// copy over n values); stats[2] counts the waves that met a non-finite value
int launch_ingest_reflectance(pccm_ctx *ctx, const void *src, int dtype, int64_t n, double *out, unsigned long long *stats);
// result records -> plain columns (q32 / row0: the iterating cloud's rows, for records of layout 1)
int launch_unpack(pccm_ctx *ctx, const double *rec, int stride, int layout, const float4 *q32, int64_t row0, int64_t ns, int32_t *idx, double *d2);
// *seq: the value the context's completion counter reaches once the batch's host outputs are complete (k_publish), or 0 when
// nothing was launched
// (a direction whose tails lie filed is settled by the batch's own kernels where they can, by the classic tail launch in front of
// them otherwise: pccm_tail_wave.h)
int launch_unit_jobs(pccm_ctx *ctx, const UnitJobs &jobs, uint64_t *seq);
// the selection launches of jobs.sel (memset of the histograms, kSelPasses histogram passes, resolve); nothing is published
int launch_unit_select(pccm_ctx *ctx, UnitJobs &jobs);
// the count launches of jobs.sel (memset of the counters, the count pass, the store); nothing is published
int launch_unit_count(pccm_ctx *ctx, UnitJobs &jobs);
int launch_publish(pccm_ctx *ctx, uint64_t *seq);     // k_publish behind whatever the stream holds; *seq as for launch_unit_jobs

// minimal-OBB frame search (pccm_obb.hip)
int launch_obb_frames(pccm_ctx *ctx, const double *verts, int64_t nv, const double *tri, int64_t nt, double *ext_out, double *vol_out);
int launch_extreme_rows(pccm_ctx *ctx, const double *x64, int64_t n, const float *dirs, int ndirs, unsigned long long *best);
int launch_outside_planes(pccm_ctx *ctx, const double *x64, int64_t n, const double *planes, int nplanes, double margin,
                          int32_t *rows_out, unsigned int *count);

// colour columns (pccm_color.hip)
int launch_rgb8(pccm_ctx *ctx, Cloud &c, const unsigned char *bytes, unsigned int *flag);   // packs Cloud::rgb8 (from bytes, or from rgb64: *flag set when a value is no k / 255.0)
int launch_color_rows(pccm_ctx *ctx, const double *own, const double *other, const int32_t *rows, int64_t n,
                      int64_t n_other, int scheme, double scale, int what, double *out,
                      unsigned long long *maxkeys, unsigned int *bad, const uint32_t *own8 = nullptr, const uint32_t *other8 = nullptr,
                      const float4 *recs = nullptr,    // recs: matched records {x, y, z, row} instead of `rows`
                      const double *other_q = nullptr); // PCCM_TIES_MEAN: per row the averaged neighbour colour (no gather)
int launch_color_colsum(pccm_ctx *ctx, const double *cols, int64_t n, double *out3);
int launch_color_colsums(pccm_ctx *ctx, int njobs, const double *const cols[2], const int64_t n[2], double *const out3[2],
                         unsigned long long *const outmax[2]);   // outmax: [3] bit keys of the columns' maxima per job, or null
int launch_colors_from_u8(pccm_ctx *ctx, const unsigned char *src, int64_t n3, double *out);

}  // namespace pccm
