// k_generate_spherical.hip — K1 for a scene whose camera is PBRT-v4's spherical one (SHM_CAMERA_SPHERICAL): k_generate.inl once more, with the spherical branch of
// camera_generate_ray_differential (shm/path.h, SHM_SPHERICAL_CAMERA) compiled in. One instantiation per cell render.hip has (HAS_TEX x LEAN x sampler x filter class);
// the render plan (host/render_plan.hpp, RenderPlan::spherical) names this set for such a scene and for no other, so that every other scene runs render.hip's kernels,
// which are those of a library without this camera. A unit of its own: it compiles beside render.hip.
#define K_SPHERICAL_CAMERA true
#include "wavefront.h"

namespace {
namespace spherical {
#include "k_generate.inl"
}  // namespace spherical
using spherical::k_generate;
using spherical::k_generate_filtered;

template <bool ZS>
constexpr SphericalGenerateCells spherical_cells = {
    // [HAS_TEX][LEAN]: the textured class has no lean build (shm_plan::HAS_LEAN_KERNELS)
    {{k_generate<false, false, ZS>, k_generate<false, true, ZS>}, {k_generate<true, false, ZS>, nullptr}},
    // [filter class: triangle, tabulated][HAS_TEX][LEAN]
    {{{k_generate_filtered<false, false, ZS, FILTER_CLASS_TRIANGLE>, k_generate_filtered<false, true, ZS, FILTER_CLASS_TRIANGLE>},
      {k_generate_filtered<true, false, ZS, FILTER_CLASS_TRIANGLE>, nullptr}},
     {{k_generate_filtered<false, false, ZS, FILTER_CLASS_TABULATED>, k_generate_filtered<false, true, ZS, FILTER_CLASS_TABULATED>},
      {k_generate_filtered<true, false, ZS, FILTER_CLASS_TABULATED>, nullptr}}},
};
}  // namespace

const SphericalGenerateCells& wf_generate_spherical(bool zs) { return zs ? spherical_cells<true> : spherical_cells<false>; }
