// Host check of the reflectance event of open_pcc_metric_amd/csrc/pccm_stale.h (tests/test_reflectance_host.py builds and runs it;
// no GPU, no HIP call: a pccm_ctx is plain host memory until something is allocated).  A context with every product valid --
// both clouds' reflectance among them -- is made by hand, reflectance_changed is applied, and what every product may still claim
// afterwards is asserted product by product ("What goes stale when"); then that new points and a context reset take
// the reflectance away.
#include <stdio.h>

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

static std::unique_ptr<pccm_ctx> everything_valid(int carry_to)
{
    std::unique_ptr<pccm_ctx> ctx(new pccm_ctx());
    for (int k = 0; k < 2; ++k) {
        Cloud &c = ctx->cloud[k];
        c.n = c.n_nrm = c.n_rgb = c.n_refl = 1500 + 200 * k;
        c.n_pad = 2048;
        c.nrm_exact32 = true;
        c.rgb8_valid = true;
        c.sp_valid = c.sp_tried = true;
        c.ssim_attrs = kAllSsim;
        c.ssim_k = 8;
        c.res_k = 4;
        c.version = 7 + k;
        ctx->merge_n[k] = 2000;
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

static void test_reflectance_changed(int w, int carry_to)
{
    auto ctx = everything_valid(carry_to);
    const Counters before(*ctx);
    reflectance_changed(ctx.get(), w);
    const Cloud &c = ctx->cloud[w], &o = ctx->cloud[1 - w];
    // what moved: the cloud is without reflectance until its setter says otherwise; pending reductions of all three directions
    // may have bound the column; a captured graph's point job reads it
    EXPECT(c.n_refl == 0);
    for (int d = 0; d < 3; ++d) EXPECT(ctx->nn_gen[d] != before.nn_gen[d]);
    EXPECT(ctx->epoch != before.epoch);
    // what stayed: the other cloud's reflectance ...
    EXPECT(o.n_refl == o.n);
    // ... the searches, which result each direction holds, and a projection fused into them
    for (int d = 0; d < 3; ++d) {
        EXPECT(ctx->nn[d].valid && ctx->nn_run[d] == before.nn_run[d]);
        EXPECT(ctx->nn[d].form.recs == NNForm::kPairRows && ctx->nn[d].form.fused == PCCM_NORMAL_ROW);
    }
    // ... points, normals (carried ones too), colours, features, spacings, merge maps of both clouds
    for (int k = 0; k < 2; ++k) {
        const Cloud &x = ctx->cloud[k];
        EXPECT(x.n == 1500 + 200 * k && x.n_pad == 2048 && x.n_nrm == x.n && x.nrm_exact32 && x.n_rgb == x.n && x.rgb8_valid);
        EXPECT(x.sp_valid && x.sp_tried && x.ssim_attrs == kAllSsim && x.ssim_k == 8 && x.res_k == 4);
        EXPECT(x.version == before.version[k] && ctx->merge_n[k] == 2000);
    }
    EXPECT(ctx->carry.to == carry_to && ctx->carry.run_f == 3 && ctx->carry.run_g == 3);
    // ... the point-to-distribution columns, and the counters of normals and colours
    EXPECT(ctx->p2d_k == 6 && ctx->p2d_color);
    EXPECT(ctx->nrm_gen == before.nrm_gen && ctx->rgb_gen == before.rgb_gen);
    // (slots are not cancelled: they are stale by their generation, like after any other column change)
    EXPECT(ctx->slots[0].pending && ctx->sel_slots[0].pending);
}

static void test_points_changed_drops_reflectance(int w)
{
    auto ctx = everything_valid(-1);
    points_changed(ctx.get(), w);
    EXPECT(ctx->cloud[w].n_refl == 0 && ctx->cloud[w].n == 0);
    EXPECT(ctx->cloud[1 - w].n_refl == ctx->cloud[1 - w].n && ctx->cloud[1 - w].n > 0);
}

static void test_context_cleared_drops_reflectance()
{
    auto ctx = everything_valid(1);
    context_cleared(ctx.get());
    for (int k = 0; k < 2; ++k) EXPECT(ctx->cloud[k].n_refl == 0 && ctx->cloud[k].n == 0);
}

static void test_other_events_keep_reflectance()
{
    for (int w = 0; w < 2; ++w) {
        auto ctx = everything_valid(-1);
        normals_changed(ctx.get(), w);
        colors_changed(ctx.get(), w);
        column_rebuild(ctx.get(), Stored::kSsim, w);
        column_rebuild(ctx.get(), Stored::kSpacing, w);
        column_rebuild(ctx.get(), Stored::kP2d);
        results_dropped(ctx.get());
        for (int k = 0; k < 2; ++k) EXPECT(ctx->cloud[k].n_refl == ctx->cloud[k].n && ctx->cloud[k].n > 0);
    }
}

int main()
{
    char name[96];
    g_case = name;
    for (int w = 0; w < 2; ++w) {
        for (int carry_to = -1; carry_to < 2; ++carry_to) {
            snprintf(name, sizeof(name), "reflectance_changed(%d), carry to %d", w, carry_to);
            test_reflectance_changed(w, carry_to);
        }
        snprintf(name, sizeof(name), "points_changed(%d)", w);
        test_points_changed_drops_reflectance(w);
    }
    g_case = "context_cleared";
    test_context_cleared_drops_reflectance();
    g_case = "other events";
    test_other_events_keep_reflectance();
    printf("%d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
