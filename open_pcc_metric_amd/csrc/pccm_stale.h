// What goes stale when a cloud's inputs change: every write that takes a product's validity away is here and nowhere else
// ("What goes stale when", is this file as a table).  Host-only bookkeeping: no HIP call, no allocation.
//
// The products: the searches' results (NNResult::valid, NNForm::fused), normals carried to a cloud (pccm_ctx::carry), the
// merge maps (merge_n), PointSSIM features (Cloud::ssim_attrs / ssim_k), point spacings (Cloud::res_k), the point-to-distribution
// columns (p2d_k, p2d_color), a cloud's reflectance (Cloud::n_refl), and everything keyed on a counter: pending reductions, selections and counts, tie columns, the colour memo,
// the directions' match counts (pccm_ctx::match),
// captured graphs, grid caches.  What ESTABLISHES a product stays with its builder (ssim_attrs = attrs, res_k = K, p2d_k = k,
// carry.to = to, merge_n = n, valid = true, form = ...).
//
// The counters.  Each is only ever compared for equality with a copy taken earlier; each counts one thing:
//   nn_gen[d]  whatever a reduction, selection or count of direction d reads has changed: the result itself, or normals, features and
//              stored columns under a result that stays.  Copies: SlotKey::gen (reductions, mapped reductions, selections, counts), TieCols::gen, ColorMemo::gen,
//              MatchCounts::gen (the counts read the matched rows alone: a bump for normals or features recounts them needlessly, never wrongly).
//   nn_run[d]  searches of direction d (prepare_nn alone bumps it): WHICH result the direction holds.  Copies: Carry::run_f / run_g.
//   nrm_gen    any cloud's normals changed.  Copies: TieCols::nrm_gen / ang_gen.
//   rgb_gen    any cloud's colours changed.  Copies: TieCols::rgb_gen, ColorMemo::rgb_gen.
//   version    (per cloud) its points changed.  Copies: Grid::key and its kin, Cloud::solo_scale_version.
//   epoch      something a captured graph has baked in changed: inputs, shards, policies, or the address of a device buffer.
//              Copy: GraphRec::epoch.  The bumps for buffers and policies stay where the buffer or policy is: ensure,
//              prepare_nn, host_reserve, pccm_drop_caches, pccm_set_ties, pccm_nn_want_idx, pccm_nn_fuse.
#pragma once
#include "pccm_internal.h"

namespace pccm {

constexpr int kDirsPair = 1 << PCCM_DIR_LEFT | 1 << PCCM_DIR_RIGHT, kDirsAll = kDirsPair | 1 << PCCM_DIR_SELF;

// The results of these directions' searches are gone (a new search begins: prepare_nn, which also counts the run).
inline void results_void(pccm_ctx *ctx, int dir_mask)
{
    for (int d = 0; d < 3; ++d) {
        if (!(dir_mask & (1 << d))) continue;
        ctx->nn[d].valid = false;
        ctx->nn_gen[d]++;
    }
}

// The records of direction `dir` were written again in another form under a result that stays valid (ensure_plain repeats a search
// that left the matched rows out): the values are the same, but the job a pending reduction was bound with (ReduceWhat::job -- what
// a later selection or count of the column would read) describes records that are gone.  Pending reductions, selections and
// counts of the direction are recomputed from the new records by whoever asks next.
inline void records_rewritten(pccm_ctx *ctx, int dir) { ctx->nn_gen[dir]++; }

// ... and what was enqueued on them is never to be consumed (a kernel raised the device error word, a capture failed)
inline void results_dropped(pccm_ctx *ctx)
{
    results_void(ctx, kDirsAll);
    for_each_slot(ctx, [](SlotKey &k) { k.pending = false; });
}

// The rows this context owns of these directions changed (pccm_set_shard, pccm_set_shard_dir): captured searches carry the old ones
inline void shard_changed(pccm_ctx *ctx, int dir_mask)
{
    ctx->epoch++;
    results_void(ctx, dir_mask);
}

// A column kept in HBM is about to be rebuilt: it claims nothing until its builder says otherwise, and pending reductions that
// may have bound it are stale.  A cloud's own columns are bound by whichever direction iterates or searches it (all three move,
// as ever); the point-to-distribution columns exist for the pair's two directions.
enum class Stored { kSsim, kSpacing, kP2d, kP2dColor };
inline void column_rebuild(pccm_ctx *ctx, Stored col, int which = 0)
{
    Cloud &c = ctx->cloud[which];
    switch (col) {
    case Stored::kSsim: c.ssim_attrs = 0; break;
    case Stored::kSpacing: c.res_k = 0; break;
    case Stored::kP2d: ctx->p2d_k = 0; [[fallthrough]];       // (the colour columns were made at the old k)
    case Stored::kP2dColor: ctx->p2d_color = false; break;
    }
    const int ndirs = col == Stored::kSsim || col == Stored::kSpacing ? 3 : 2;
    for (int d = 0; d < ndirs; ++d) ctx->nn_gen[d]++;
}

// ... and its buffer was reallocated on the way (the match counts' buffer likewise): captured graphs that read the old one are stale
inline void column_moved(pccm_ctx *ctx) { ctx->epoch++; }

// forget the content, keep the allocations
inline void drop_cloud(Cloud &c)
{
    c.n = c.n_pad = c.n_nrm = c.n_rgb = c.n_refl = 0;
    c.nrm_deferred = false;
    c.nrm_host = nullptr;
    c.sp_valid = c.sp_tried = false;
    c.rgb8_valid = false;
    c.ssim_attrs = c.ssim_k = 0;
    c.res_k = 0;
}

// a cloud loses its normals and what was made from them alone (the buffers stay)
inline void drop_normals(Cloud &c)
{
    c.n_nrm = 0;
    c.nrm_exact32 = false;
    c.nrm_deferred = false;
    c.nrm_host = nullptr;
    c.ssim_attrs &= ~PCCM_SSIM_NORMAL;
}

// Cloud `which` is getting new points (pccm_set_cloud; pccm_merge_duplicates through it).
inline void points_changed(pccm_ctx *ctx, int which)
{
    if (ctx->carry.to >= 0) {                          // both clouds' points enter a carry: the carried normals go, whoever holds them
        drop_normals(ctx->cloud[ctx->carry.to]);
        ctx->carry.to = -1;
    }
    drop_cloud(ctx->cloud[which]);                     // its normals, colours, features and spacings go with it
    ctx->merge_n[which] = 0;                           // (the merge map spoke of the old rows)
    ctx->p2d_k = 0;                                    // (both point-to-distribution columns depend on either cloud)
    ctx->p2d_color = false;
    // a new cloud 1 leaves the self search of cloud 0 -- cloud_pair.py:108-109 -- as valid as it was: one reference cloud
    // against several decoded ones, BASELINE configs[4], keeps it, see CloudPair.with_reconst
    results_void(ctx, which == 1 ? kDirsPair : kDirsAll);
    ctx->epoch++;
    ctx->cloud[which].version++;
}

// Cloud `which` is being moved in place (pccm_transform_cloud): the same rows at new coordinates, its own normals rotated with
// them.  What was made from the coordinates goes as in points_changed -- results of every direction that touches the cloud (the
// self search of cloud 0 survives a move of cloud 1), PointSSIM features, spacings, the point-to-distribution columns, the spatial
// order, normals carried to either cloud (the cloud's own, which stay, are rotated by the caller).  What is keyed on the ROWS
// stays: colours, packed colours, reflectance and the merge map.
inline void points_moved(pccm_ctx *ctx, int which)
{
    if (ctx->carry.to >= 0) {                          // both clouds' points enter a carry: the carried normals go, whoever holds them
        drop_normals(ctx->cloud[ctx->carry.to]);
        ctx->carry.to = -1;
    }
    Cloud &c = ctx->cloud[which];
    c.sp_valid = c.sp_tried = false;
    c.ssim_attrs = c.ssim_k = 0;
    c.res_k = 0;
    ctx->p2d_k = 0;
    ctx->p2d_color = false;
    results_void(ctx, which == 1 ? kDirsPair : kDirsAll);
    if (c.n_nrm > 0) ctx->nrm_gen++;                   // (averaged normals of PCCM_TIES_MEAN are stale)
    ctx->epoch++;
    c.version++;
}

// Cloud `which` is getting new normals: uploaded (pccm_set_normals), announced (pccm_set_normals_deferred -- everything moves
// now; the upload behind it, normals_ready, changes nothing anybody could have read in between, because whoever reads normals
// makes them ready first), estimated (estimate_normals) or carried (pccm_carry_normals, which records the new carry afterwards).
// The cloud is left without normals; the caller says what it has once they are there.
inline void normals_changed(pccm_ctx *ctx, int which)
{
    // normals carried FROM this cloud were made from the ones being replaced: the other cloud loses them.  Normals carried TO
    // it are being replaced: it is an ordinary cloud again, and the other cloud keeps its own.
    if (ctx->carry.to >= 0 && ctx->carry.to != which) drop_normals(ctx->cloud[ctx->carry.to]);
    ctx->carry.to = -1;
    drop_normals(ctx->cloud[which]);
    // a projection fused into a search took the searched cloud's normals as they were (pccm_nn_fuse: "results are bit-identical
    // either way"); matched records (NNForm::kMatched) are not concerned, the reduction projects with the current normals
    ctx->nn[which == 1 ? PCCM_DIR_LEFT : PCCM_DIR_RIGHT].form.fused = -1;
    if (which == 0) ctx->nn[PCCM_DIR_SELF].form.fused = -1;
    for (int d = 0; d < 3; ++d) ctx->nn_gen[d]++;      // pending D2, angular and PointSSIM reductions used the old normals
    ctx->epoch++;                                      // (captured reductions read nrm64 / nrm32, which may have moved)
    ctx->nrm_gen++;                                    // (averaged normals of PCCM_TIES_MEAN are stale)
}

// Cloud `which` is getting new colours.  The searches' results and the geometry columns stay, so neither epoch nor nn_gen moves
// -- a captured graph reads no colour -- unless colour or joint point-to-distribution columns exist: those are stored columns
// that pending reductions of both directions may have bound.
inline void colors_changed(pccm_ctx *ctx, int which)
{
    Cloud &c = ctx->cloud[which];
    c.n_rgb = 0;
    c.rgb8_valid = false;
    c.ssim_attrs &= ~PCCM_SSIM_COLOR;
    if (ctx->p2d_color) column_rebuild(ctx, Stored::kP2dColor);
    ctx->rgb_gen++;                                    // (the colour memo and the tie columns' averaged colours are stale)
}

// Cloud `which` is getting a new reflectance.  The column is read only by PCCM_METRIC_REFLECTANCE point jobs, so the searches'
// results, normals, colours, features, spacings and point-to-distribution columns stay; pending reductions of every direction may
// have bound the old column, and a captured graph's point job reads it (the buffer may move as well).  The cloud is left without
// reflectance; the setter says what it has once the values are there.
inline void reflectance_changed(pccm_ctx *ctx, int which)
{
    ctx->cloud[which].n_refl = 0;
    for (int d = 0; d < 3; ++d) ctx->nn_gen[d]++;
    ctx->epoch++;
}

// pccm_ctx_reset's bookkeeping: nothing of the last owner's inputs or results is left, the allocations stay
inline void context_cleared(pccm_ctx *ctx)
{
    ctx->carry.to = -1;
    for (int k = 0; k < 2; ++k) {
        ctx->merge_n[k] = 0;
        drop_cloud(ctx->cloud[k]);
        ctx->cloud[k].version++;
    }
    ctx->p2d_k = 0;
    ctx->p2d_color = false;
    for (int d = 0; d < 3; ++d) {
        ctx->shard_rank[d] = 0;
        ctx->shard_world[d] = 1;
    }
    results_dropped(ctx);
    ctx->epoch++;
}

}  // namespace pccm
