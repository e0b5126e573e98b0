// k_trace_alpha.hip — K2 / K3 of the scenes that hold a cutout (PBRT-v4's shape alpha: ShmTriangleMesh / ShmBilinearPatchMesh / ShmSphere::alpha, shm/alpha.h): k_trace.hip's
// body (k_trace.inl) a third time, with K_ALPHA — an alpha-tested triangle parks in the leaf phase, and the parked round runs the alpha test behind its sphere, patch and
// triangle tests — and with K_QUADRICS, since such a scene may hold a disk or a cylinder as well: one superset build keeps the count at six. The general rows only (a
// scene with a cutout plans no TRACE_TRI: flatten.h files an alpha-tested triangle under the non-triangle records): GEN and GEN_HEAVY, closest and any hit, and the STRICT
// any-hit pair, each under the waves, LDS levels and save area of its own row of host/render_plan.hpp's TRACE_SHAPES. wf_launch_trace (k_trace.hip) takes a kernel from
// here when the scene's plan says has_alpha; the kernels of every other scene are compiled without a trace of the feature.
#define K_QUADRICS true
#define K_ALPHA true
#include "k_trace.inl"

namespace {

template <bool ANY, bool HEAVY>
__global__ void __launch_bounds__(TRACE_BLOCK) k_trace5_alpha(K5_PARAMS);
TRACE_KERNEL(TRACE_GEN, RAY_CLOSEST, false, k_trace5_alpha<false, false>)
TRACE_KERNEL(TRACE_GEN, RAY_ANY, false, k_trace5_alpha<true, false>)
TRACE_KERNEL(TRACE_GEN_HEAVY, RAY_CLOSEST, false, k_trace5_alpha<false, true>)
TRACE_KERNEL(TRACE_GEN_HEAVY, RAY_ANY, false, k_trace5_alpha<true, true>)
template <bool HEAVY>
__global__ void __launch_bounds__(TRACE_BLOCK) k_trace5_alpha_any_strict(K5_PARAMS);
TRACE_KERNEL(trace_strict_variant(TRACE_GEN), RAY_ANY, true, k_trace5_alpha_any_strict<false>)
TRACE_KERNEL(trace_strict_variant(TRACE_GEN_HEAVY), RAY_ANY, true, k_trace5_alpha_any_strict<true>)
#undef TRACE_KERNEL
constexpr TraceKernel ALPHA_KERNELS[2][N_RAY] = {{k_trace5_alpha<false, false>, k_trace5_alpha<true, false>}, {k_trace5_alpha<false, true>, k_trace5_alpha<true, true>}};  // [variant - TRACE_GEN]
constexpr TraceKernel ALPHA_KERNELS_ANY_STRICT[2] = {k_trace5_alpha_any_strict<false>, k_trace5_alpha_any_strict<true>};  // [trace_strict_variant - TRACE_GEN]
static_assert(TRACE_GEN_HEAVY == TRACE_GEN + 1 && N_TRACE == TRACE_GEN + 2, "the general rows are the last two of TRACE_SHAPES");

// The alpha texture's evaluators are real calls that read the scene through a SceneView in memory (SceneView::call_copy, shm/texture.h). The shading kernels keep that copy
// in LDS; these kernels' rows have no LDS to spare (seven workgroups of eleven stack levels fill a CU's 160 KB but for 6 KB), so theirs lies in HBM — TraceSide::d_view,
// written here in stream order in front of every launch, since the view carries the render's options (quirks_off)
static_assert(sizeof(SceneView) % sizeof(uint32_t) == 0, "k_store_scene_view copies whole words");
__global__ void k_store_scene_view(SceneView sv, uint32_t* dst) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&sv);
    for (uint32_t i = threadIdx.x; i < sizeof(SceneView) / sizeof(uint32_t); i += blockDim.x) dst[i] = src[i];
}

}  // namespace

WF_INTERNAL void wf_trace_alpha_store_view(hipStream_t stream, const SceneView& view, SceneView* dst);
void wf_trace_alpha_store_view(hipStream_t stream, const SceneView& view, SceneView* dst) {
    hipLaunchKernelGGL(k_store_scene_view, dim3(1), dim3(64), 0, stream, view, reinterpret_cast<uint32_t*>(dst));
}

TraceKernel wf_trace_alpha_kernel(int variant, int ray, bool any_strict) {
    if (variant != TRACE_GEN && variant != TRACE_GEN_HEAVY) return nullptr;  // (a scene with a cutout never plans TRACE_TRI)
    return any_strict ? ALPHA_KERNELS_ANY_STRICT[trace_strict_variant(variant) - TRACE_GEN] : ALPHA_KERNELS[variant - TRACE_GEN][ray];
}
