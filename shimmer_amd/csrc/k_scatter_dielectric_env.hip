// k_scatter_dielectric_env.hip — k_scatter_dielectric.hip for scenes whose only image is an ImageInfinitelight (K_ENV_LIGHT, k_scatter.inl; k_vertex_env.hip says why).
// (options.force_diffuse renders of such a scene run the textured class's kernels: render.hip)
#define K_ENV_LIGHT true
#include "k_scatter.inl"

// (one body for both launchers, as in k_scatter_dielectric.hip)
#define WF_DIELECTRIC_LAUNCH(KERNEL, BLOCKS)                                                                          \
    do {                                                                                                              \
        if (geo == GEO_TRI) WF_SCATTER_LAUNCH_SUB(GEO_TRI, IMG_ENV, CLASS_DIELECTRIC, KERNEL, BLOCKS);                \
        else WF_SCATTER_LAUNCH_SUB(GEO_GEN, IMG_ENV, CLASS_DIELECTRIC, KERNEL, BLOCKS);                               \
    } while (0)
static int launch_dielectric(ShmScene* s, const ShadeArgs& a, int geo) {
    if (a.params.regularize != 0) {
        WF_DIELECTRIC_LAUNCH(k_scatter, a.blocks);
        return SHM_OK;
    }
    WF_DIELECTRIC_LAUNCH(k_scatter_specular, s->n_cu * 4);
    if (s->flat.has_rough_dielectric) WF_DIELECTRIC_LAUNCH(k_scatter_nonspecular, a.blocks);
    return SHM_OK;
}
#define WF_DIELECTRIC_STUB(GEO) \
    template <> int wf_shade<FAM_SCATTER_DIELECTRIC, GEO, IMG_ENV, K_ZSOBOL, K_DELTA_LIGHTS>(ShmScene* s, const ShadeArgs& a) { WF_ENV_UNIT_CHECK(IMG_ENV); return launch_dielectric(s, a, GEO); }
WF_DIELECTRIC_STUB(GEO_TRI)
WF_DIELECTRIC_STUB(GEO_GEN)
