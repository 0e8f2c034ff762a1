// Host check of open_pcc_metric_amd/csrc/pccm_stale.h (tests/test_stale_host.py builds and runs it; no GPU, no HIP call: a
// pccm_ctx is plain host memory until something is allocated).  A context "with everything valid" is made by hand, one event is
// applied, and what every product may still claim afterwards is asserted product by product -- from what the product is made
// of ("What goes stale when"), not from what the header happens to write.
#include <stdio.h>

#include <initializer_list>
#include <memory>

#include "pccm_stale.h"

using namespace pccm;

static int g_failed = 0, g_checked = 0;
static const char *g_case = "";
#define EXPECT(cond)                                                              \
    do {                                                                          \
        ++g_checked;                                                              \
        if (!(cond)) {                                                            \
            ++g_failed;                                                           \
            printf("FAILED [%s] line %d: %s\n", g_case, __LINE__, #cond);        \
        }                                                                         \
    } while (0)

constexpr int kAllSsim = PCCM_SSIM_GEOMETRY | PCCM_SSIM_NORMAL | PCCM_SSIM_CURVATURE | PCCM_SSIM_COLOR;
static const int kHostNormals = 0;      // (something for nrm_host to point at)

// every product claims validity; normals were carried to cloud `carry_to` (-1: no carry); cloud `deferred` (-1: none) has
// announced normals that have not crossed yet
static std::unique_ptr<pccm_ctx> everything_valid(int carry_to, int deferred = -1)
{
    std::unique_ptr<pccm_ctx> ctx(new pccm_ctx());
    for (int k = 0; k < 2; ++k) {
        Cloud &c = ctx->cloud[k];
        c.n = c.n_nrm = c.n_rgb = 1500 + 200 * k;
        c.n_pad = 2048;
        c.nrm_exact32 = true;
        c.rgb8_valid = true;
        c.sp_valid = c.sp_tried = true;
        c.ssim_attrs = kAllSsim;
        c.ssim_k = 8;
        c.res_k = 4;
        c.version = 7 + k;
        ctx->merge_n[k] = 2000;
        ctx->shard_rank[k] = 1;
        ctx->shard_world[k] = 2;
    }
    if (deferred >= 0) {
        ctx->cloud[deferred].nrm_deferred = true;
        ctx->cloud[deferred].nrm_host = &kHostNormals;
    }
    for (int d = 0; d < 3; ++d) {
        ctx->nn[d].valid = true;
        ctx->nn[d].form = {NNForm::kPairRows, NNForm::kNoPlain, PCCM_NORMAL_ROW};
        ctx->nn_run[d] = 3;
    }
    ctx->carry.to = carry_to;
    ctx->carry.run_f = ctx->carry.run_g = 3;
    ctx->p2d_k = 6;
    ctx->p2d_color = true;
    ctx->slots[0].pending = ctx->sel_slots[0].pending = true;
    return ctx;
}

struct Counters {
    uint64_t nn_gen[3], nn_run[3], nrm_gen, rgb_gen, epoch, version[2];
    explicit Counters(const pccm_ctx &c)
        : nrm_gen(c.nrm_gen), rgb_gen(c.rgb_gen), epoch(c.epoch), version{c.cloud[0].version, c.cloud[1].version}
    {
        for (int d = 0; d < 3; ++d) {
            nn_gen[d] = c.nn_gen[d];
            nn_run[d] = c.nn_run[d];
        }
    }
};

// the searched cloud of a direction
static int searched(int dir) { return dir == PCCM_DIR_LEFT ? 1 : 0; }

static void test_points_changed(int w, int carry_to)
{
    auto ctx = everything_valid(carry_to);
    const Counters before(*ctx);
    points_changed(ctx.get(), w);
    const Cloud &c = ctx->cloud[w], &o = ctx->cloud[1 - w];
    // nothing made from cloud w's points claims validity: the cloud's own content ...
    EXPECT(c.n == 0 && c.n_nrm == 0 && c.n_rgb == 0 && !c.nrm_deferred && !c.nrm_host && !c.rgb8_valid && !c.sp_valid);
    EXPECT(c.ssim_attrs == 0 && c.res_k == 0);
    EXPECT(ctx->merge_n[w] == 0);
    // ... the searches it takes part in (both directional ones; the self search is cloud 0's alone) ...
    EXPECT(!ctx->nn[PCCM_DIR_LEFT].valid && !ctx->nn[PCCM_DIR_RIGHT].valid);
    EXPECT(ctx->nn[PCCM_DIR_SELF].valid == (w == 1));
    for (int d = 0; d < 3; ++d) EXPECT((ctx->nn_gen[d] != before.nn_gen[d]) == !ctx->nn[d].valid);
    // ... the columns of the pair, and a carry in either direction (it was made from both clouds' points)
    EXPECT(ctx->p2d_k == 0 && !ctx->p2d_color);
    EXPECT(ctx->carry.to == -1);
    if (carry_to >= 0) EXPECT(ctx->cloud[carry_to].n_nrm == 0 && !(ctx->cloud[carry_to].ssim_attrs & PCCM_SSIM_NORMAL));
    // grids and graphs see it
    EXPECT(c.version != before.version[w] && o.version == before.version[1 - w]);
    EXPECT(ctx->epoch != before.epoch);
    // the other cloud keeps what is its own: points, colours, spacings, merge map, features (and its normals and the features
    // made from them unless they were carried ones)
    EXPECT(o.n > 0 && o.n_rgb == o.n && o.rgb8_valid && o.res_k == 4 && o.ssim_k == 8 && ctx->merge_n[1 - w] == 2000);
    EXPECT((o.ssim_attrs | PCCM_SSIM_NORMAL) == kAllSsim);
    if (carry_to != 1 - w) EXPECT(o.n_nrm == o.n && o.nrm_exact32 && o.ssim_attrs == kAllSsim);
    for (int d = 0; d < 3; ++d) EXPECT(ctx->nn_run[d] == before.nn_run[d]);      // (no search ran)
    EXPECT(ctx->nrm_gen == before.nrm_gen && ctx->rgb_gen == before.rgb_gen);
}

static void test_normals_changed(int w, int carry_to, int deferred)
{
    auto ctx = everything_valid(carry_to, deferred);
    const Counters before(*ctx);
    normals_changed(ctx.get(), w);
    const Cloud &c = ctx->cloud[w], &o = ctx->cloud[1 - w];
    // the cloud is without normals until its caller says otherwise -- announced ones that never crossed among them
    EXPECT(c.n_nrm == 0 && !c.nrm_exact32 && !c.nrm_deferred && !c.nrm_host);
    EXPECT(ctx->nrm_gen != before.nrm_gen && ctx->epoch != before.epoch);
    for (int d = 0; d < 3; ++d) EXPECT(ctx->nn_gen[d] != before.nn_gen[d]);
    // the results stay, but a projection fused from the old normals does not: exactly the directions that search cloud w
    for (int d = 0; d < 3; ++d) {
        EXPECT(ctx->nn[d].valid && ctx->nn[d].form.recs == NNForm::kPairRows && ctx->nn_run[d] == before.nn_run[d]);
        EXPECT(ctx->nn[d].form.fused == (searched(d) == w ? -1 : PCCM_NORMAL_ROW));
        EXPECT(ctx->nn[d].form.holds_projection(PCCM_NORMAL_ROW) == (searched(d) != w));
    }
    // the PointSSIM normal bit of w is clear, its other bits, spacings, colours and points are kept
    EXPECT(c.ssim_attrs == (kAllSsim & ~PCCM_SSIM_NORMAL) && c.ssim_k == 8);
    EXPECT(c.res_k == 4 && o.res_k == 4 && ctx->p2d_k == 6 && ctx->p2d_color);
    EXPECT(c.n > 0 && c.n_rgb == c.n && c.rgb8_valid && o.n > 0 && o.n_rgb == o.n && o.rgb8_valid);
    EXPECT(ctx->merge_n[0] == 2000 && ctx->merge_n[1] == 2000);
    EXPECT(ctx->rgb_gen == before.rgb_gen && c.version == before.version[w] && o.version == before.version[1 - w]);
    // no carry survives: normals carried FROM w are gone with the PointSSIM features made from them; a carry TO w is closed and
    // the other cloud keeps its own normals
    EXPECT(ctx->carry.to == -1);
    if (carry_to == 1 - w) EXPECT(o.n_nrm == 0 && !o.nrm_exact32 && o.ssim_attrs == (kAllSsim & ~PCCM_SSIM_NORMAL));
    else EXPECT(o.n_nrm == o.n && o.nrm_exact32 && o.ssim_attrs == kAllSsim && o.nrm_deferred == (deferred == 1 - w));
}

static void test_colors_changed(int w, bool p2d_color)
{
    auto ctx = everything_valid(-1);
    ctx->p2d_color = p2d_color;
    const Counters before(*ctx);
    colors_changed(ctx.get(), w);
    const Cloud &c = ctx->cloud[w], &o = ctx->cloud[1 - w];
    EXPECT(c.n_rgb == 0 && !c.rgb8_valid);
    EXPECT(ctx->rgb_gen != before.rgb_gen);
    EXPECT(c.ssim_attrs == (kAllSsim & ~PCCM_SSIM_COLOR) && o.ssim_attrs == kAllSsim);
    // the colour and joint point-to-distribution columns go, the geometry columns stay
    EXPECT(!ctx->p2d_color && ctx->p2d_k == 6);
    // pending reductions of the pair's directions are stale only if they could have bound those columns
    EXPECT((ctx->nn_gen[PCCM_DIR_LEFT] != before.nn_gen[PCCM_DIR_LEFT]) == p2d_color);
    EXPECT((ctx->nn_gen[PCCM_DIR_RIGHT] != before.nn_gen[PCCM_DIR_RIGHT]) == p2d_color);
    EXPECT(ctx->nn_gen[PCCM_DIR_SELF] == before.nn_gen[PCCM_DIR_SELF]);
    // normals, spacings, search results, graphs and the other cloud's colours are kept
    for (int k = 0; k < 2; ++k) EXPECT(ctx->cloud[k].n_nrm == ctx->cloud[k].n && ctx->cloud[k].nrm_exact32 && ctx->cloud[k].res_k == 4);
    for (int d = 0; d < 3; ++d) EXPECT(ctx->nn[d].valid && ctx->nn[d].form.fused == PCCM_NORMAL_ROW);
    EXPECT(ctx->epoch == before.epoch && ctx->nrm_gen == before.nrm_gen);
    EXPECT(o.n_rgb == o.n && o.rgb8_valid && ctx->carry.to == -1 && ctx->merge_n[w] == 2000);
}

static void test_column_rebuild(Stored col, int w)
{
    auto ctx = everything_valid(-1);
    const Counters before(*ctx);
    column_rebuild(ctx.get(), col, w);
    const bool own = col == Stored::kSsim || col == Stored::kSpacing;       // a cloud's own column, or the pair's
    // the column claims nothing while it is rebuilt; its siblings and the other cloud's columns are untouched
    EXPECT(ctx->cloud[w].ssim_attrs == (col == Stored::kSsim ? 0 : kAllSsim) && ctx->cloud[1 - w].ssim_attrs == kAllSsim);
    EXPECT(ctx->cloud[w].res_k == (col == Stored::kSpacing ? 0 : 4) && ctx->cloud[1 - w].res_k == 4);
    EXPECT(ctx->p2d_k == (col == Stored::kP2d ? 0 : 6));
    EXPECT(ctx->p2d_color == own);
    EXPECT(ctx->nn_gen[PCCM_DIR_LEFT] != before.nn_gen[PCCM_DIR_LEFT] && ctx->nn_gen[PCCM_DIR_RIGHT] != before.nn_gen[PCCM_DIR_RIGHT]);
    EXPECT((ctx->nn_gen[PCCM_DIR_SELF] != before.nn_gen[PCCM_DIR_SELF]) == own);
    for (int d = 0; d < 3; ++d) EXPECT(ctx->nn[d].valid);
    EXPECT(ctx->epoch == before.epoch);                                      // (the buffer stayed where it was ...
    column_moved(ctx.get());
    EXPECT(ctx->epoch != before.epoch);                                      // ... or did not)
}

static void test_results(int mask)
{
    for (int kind = 0; kind < 3; ++kind) {      // results_void, shard_changed, results_dropped (all directions)
        auto ctx = everything_valid(0);
        const Counters before(*ctx);
        if (kind == 0) results_void(ctx.get(), mask);
        else if (kind == 1) shard_changed(ctx.get(), mask);
        else results_dropped(ctx.get()), mask = kDirsAll;
        for (int d = 0; d < 3; ++d) {
            const bool hit = (mask >> d) & 1;
            EXPECT(ctx->nn[d].valid == !hit && (ctx->nn_gen[d] != before.nn_gen[d]) == hit && ctx->nn_run[d] == before.nn_run[d]);
        }
        EXPECT((ctx->epoch != before.epoch) == (kind == 1));
        EXPECT(ctx->slots[0].pending == (kind != 2) && ctx->sel_slots[0].pending == (kind != 2));
        // inputs and what was built from them alone stay
        for (int k = 0; k < 2; ++k) EXPECT(ctx->cloud[k].n > 0 && ctx->cloud[k].ssim_attrs == kAllSsim && ctx->cloud[k].res_k == 4);
        EXPECT(ctx->p2d_k == 6 && ctx->p2d_color && ctx->carry.to == 0 && ctx->merge_n[0] == 2000);
    }
}

static void test_context_cleared()
{
    auto ctx = everything_valid(1, 0);
    const Counters before(*ctx);
    context_cleared(ctx.get());
    for (int k = 0; k < 2; ++k) {
        const Cloud &c = ctx->cloud[k];
        EXPECT(c.n == 0 && c.n_nrm == 0 && c.n_rgb == 0 && !c.nrm_deferred && !c.nrm_host && !c.rgb8_valid && !c.sp_valid && !c.sp_tried);
        EXPECT(c.ssim_attrs == 0 && c.res_k == 0 && ctx->merge_n[k] == 0 && c.version != before.version[k]);
    }
    for (int d = 0; d < 3; ++d) {
        EXPECT(!ctx->nn[d].valid && ctx->nn_gen[d] != before.nn_gen[d]);
        EXPECT(ctx->shard_rank[d] == 0 && ctx->shard_world[d] == 1);
    }
    EXPECT(!ctx->sharded() && ctx->carry.to == -1 && ctx->p2d_k == 0 && !ctx->p2d_color && ctx->epoch != before.epoch);
    EXPECT(!ctx->slots[0].pending && !ctx->sel_slots[0].pending);
}

int main()
{
    char name[96];
    g_case = name;
    for (int w = 0; w < 2; ++w)
        for (int carry_to = -1; carry_to < 2; ++carry_to) {
            snprintf(name, sizeof(name), "points_changed(%d), carry to %d", w, carry_to);
            test_points_changed(w, carry_to);
            for (int deferred = -1; deferred < 2; ++deferred) {
                if (deferred >= 0 && deferred == carry_to) continue;      // (carried normals are on the device)
                snprintf(name, sizeof(name), "normals_changed(%d), carry to %d, cloud %d announced", w, carry_to, deferred);
                test_normals_changed(w, carry_to, deferred);
            }
        }
    for (int w = 0; w < 2; ++w)
        for (int on = 0; on < 2; ++on) {
            snprintf(name, sizeof(name), "colors_changed(%d), p2d_color %d", w, on);
            test_colors_changed(w, on != 0);
        }
    for (Stored col : {Stored::kSsim, Stored::kSpacing, Stored::kP2d, Stored::kP2dColor})
        for (int w = 0; w < 2; ++w) {
            snprintf(name, sizeof(name), "column_rebuild(%d, %d)", (int)col, w);
            test_column_rebuild(col, w);
        }
    for (int mask = 0; mask < 8; ++mask) {
        snprintf(name, sizeof(name), "results of directions 0x%x", mask);
        test_results(mask);
    }
    g_case = "context_cleared";
    test_context_cleared();
    printf("%d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
