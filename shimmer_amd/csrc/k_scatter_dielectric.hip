// k_scatter_dielectric.hip — the scattering half of a vertex (k_scatter.inl) for the CLASS_DIELECTRIC queue, in the three scene classes.
#include "k_scatter.inl"

// Without options.force_diffuse / regularize (which change the BxDF inside the scatter half) the class queue is worked through by TWO kernels: the specular
// entries — smooth DielectricBxDF, ThinDielectricBxDF: no NEE, no microfacet code — at four waves per SIMD, and the rough ones (launched only if the
// material table holds a dielectric that can be rough) by the general kernel; each skips the other's entries.
// (one body for the three launchers, which names the kernels in the order they are instantiated in — the order of the code object, on which the compiler's register
//  allocation depends: named scene class by scene class, the rough-dielectric kernels spilled other SGPR counts)
#define WF_DIELECTRIC_LAUNCH(KERNEL, BLOCKS)                                                                          \
    do {                                                                                                              \
        if (img == IMG_TEX) WF_SCATTER_LAUNCH_SUB(GEO_GEN, IMG_TEX, CLASS_DIELECTRIC, KERNEL, BLOCKS);                \
        else if (geo == GEO_TRI) WF_SCATTER_LAUNCH_SUB(GEO_TRI, IMG_NONE, CLASS_DIELECTRIC, KERNEL, BLOCKS);          \
        else WF_SCATTER_LAUNCH_SUB(GEO_GEN, IMG_NONE, CLASS_DIELECTRIC, KERNEL, BLOCKS);                              \
    } while (0)
static int launch_dielectric(ShmScene* s, const ShadeArgs& a, int geo, int img) {
    if (a.params.force_diffuse != 0 || a.params.regularize != 0) {
        WF_DIELECTRIC_LAUNCH(k_scatter, a.blocks);
        return SHM_OK;
    }
    WF_DIELECTRIC_LAUNCH(k_scatter_specular, s->n_cu * 4);
    if (s->flat.has_rough_dielectric) WF_DIELECTRIC_LAUNCH(k_scatter_nonspecular, a.blocks);
    return SHM_OK;
}
#define WF_DIELECTRIC_STUB(GEO, IMG) \
    template <> int wf_shade<FAM_SCATTER_DIELECTRIC, GEO, IMG, K_ZSOBOL, K_DELTA_LIGHTS>(ShmScene* s, const ShadeArgs& a) { WF_ENV_UNIT_CHECK(IMG); return launch_dielectric(s, a, GEO, IMG); }
WF_DIELECTRIC_STUB(GEO_GEN, IMG_TEX)
WF_DIELECTRIC_STUB(GEO_TRI, IMG_NONE)
WF_DIELECTRIC_STUB(GEO_GEN, IMG_NONE)
