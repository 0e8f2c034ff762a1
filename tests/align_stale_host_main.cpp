// Host check of points_moved (open_pcc_metric_amd/csrc/pccm_stale.h; tests/test_align_host.py builds and runs it; no GPU, no HIP
// call: a pccm_ctx is plain host memory until something is allocated).  A context "with everything valid" is made by hand, cloud
// `which` is moved, and what every product may still claim afterwards is asserted product by product against DESIGN.md, "What
// goes stale when": what is made from coordinates goes, what is keyed on rows stays.
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
    ctx->slots[0].pending = ctx->map_slots[0].pending = true;
    ctx->match[0].gen = ctx->nn_gen[0];
    ctx->match[1].gen = ctx->nn_gen[1];
    return ctx;
}

static void test_points_moved(int w, int carry_to)
{
    auto ctx = everything_valid(carry_to);
    uint64_t gen[3], run[3];
    for (int d = 0; d < 3; ++d) { gen[d] = ctx->nn_gen[d]; run[d] = ctx->nn_run[d]; }
    const uint64_t epoch = ctx->epoch, rgb_gen = ctx->rgb_gen, nrm_gen = ctx->nrm_gen;
    const uint64_t version[2] = {ctx->cloud[0].version, ctx->cloud[1].version};
    points_moved(ctx.get(), w);
    const Cloud &c = ctx->cloud[w], &o = ctx->cloud[1 - w];
    // the rows are the same rows: the cloud keeps its size, and what is keyed on rows stays -- colours, packed colours,
    // reflectance, the merge map
    EXPECT(c.n == 1500 + 200 * w && c.n_pad == 2048);
    EXPECT(c.n_rgb == c.n && c.rgb8_valid && c.n_refl == c.n);
    EXPECT(ctx->merge_n[0] == 2000 && ctx->merge_n[1] == 2000);
    EXPECT(ctx->rgb_gen == rgb_gen);
    // the other cloud keeps everything of its own but normals carried to it
    EXPECT(o.n == 1500 + 200 * (1 - w) && o.n_rgb == o.n && o.rgb8_valid && o.n_refl == o.n);
    EXPECT(o.sp_valid && o.sp_tried && o.ssim_k == 8 && o.res_k == 4 && o.version == version[1 - w]);
    EXPECT((o.ssim_attrs | PCCM_SSIM_NORMAL) == kAllSsim);
    // what was made from the coordinates goes: features, spacings, the spatial order, both point-to-distribution columns
    EXPECT(c.ssim_attrs == 0 && c.ssim_k == 0 && c.res_k == 0 && !c.sp_valid && !c.sp_tried);
    EXPECT(ctx->p2d_k == 0 && !ctx->p2d_color);
    // the searches: every direction that touches the cloud; a move of cloud 1 leaves the self search of cloud 0 as it was
    EXPECT(!ctx->nn[PCCM_DIR_LEFT].valid && !ctx->nn[PCCM_DIR_RIGHT].valid);
    EXPECT(ctx->nn_gen[PCCM_DIR_LEFT] != gen[PCCM_DIR_LEFT] && ctx->nn_gen[PCCM_DIR_RIGHT] != gen[PCCM_DIR_RIGHT]);
    EXPECT(ctx->match[0].gen != ctx->nn_gen[0] && ctx->match[1].gen != ctx->nn_gen[1]);      // (the match counts with them)
    if (w == 1) {
        EXPECT(ctx->nn[PCCM_DIR_SELF].valid && ctx->nn_gen[PCCM_DIR_SELF] == gen[PCCM_DIR_SELF]);
    } else {
        EXPECT(!ctx->nn[PCCM_DIR_SELF].valid && ctx->nn_gen[PCCM_DIR_SELF] != gen[PCCM_DIR_SELF]);
    }
    for (int d = 0; d < 3; ++d) EXPECT(ctx->nn_run[d] == run[d]);       // (prepare_nn alone counts searches)
    // carried normals go in either direction, whoever holds them; normals of a cloud's own stay (the caller rotates them)
    EXPECT(ctx->carry.to == -1);
    if (carry_to >= 0) {
        const Cloud &held = ctx->cloud[carry_to], &source = ctx->cloud[1 - carry_to];
        EXPECT(held.n_nrm == 0 && !held.nrm_exact32 && !(held.ssim_attrs & PCCM_SSIM_NORMAL));
        EXPECT(source.n_nrm == source.n);
    } else {
        EXPECT(c.n_nrm == c.n && o.n_nrm == o.n);
        EXPECT(ctx->nrm_gen != nrm_gen);                   // (the moved cloud's normals turn with it: averaged normals are stale)
    }
    // counters: grids and captured graphs key on these
    EXPECT(ctx->epoch == epoch + 1);
    EXPECT(c.version == version[w] + 1);
}

int main()
{
    for (int w = 0; w < 2; ++w)
        for (int carry_to = -1; carry_to < 2; ++carry_to) {
            char name[64];
            snprintf(name, sizeof name, "points_moved which=%d carry.to=%d", w, carry_to);
            g_case = name;
            test_points_moved(w, carry_to);
        }
    printf("%d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
