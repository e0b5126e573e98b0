// k_trace_quadrics.hip — K2 / K3 of the scenes that hold a disk or a cylinder (ShmSphere::quadric; PBRT-v4's shapes, shm/shapes.h): k_trace.hip's body (k_trace.inl) a
// second time with K_QUADRICS, so that Sphere::intersect in the parked round dispatches on the record's kind. The general rows only — such a scene has a sphere record,
// so it is never TRACE_TRI —: GEN and GEN_HEAVY, closest and any hit, and the STRICT any-hit pair; six kernels, each under the waves, LDS levels and save area of its own
// row of host/render_plan.hpp's TRACE_SHAPES, which is what wf_trace_prepare sized the scene's grid, spill and save areas by. wf_launch_trace (k_trace.hip) takes a kernel
// from here when the scene's plan says has_quadric_kinds; k_trace.hip's own kernels are compiled without a trace of the shapes.
#define K_QUADRICS true
#include "k_trace.inl"

namespace {

template <bool ANY, bool HEAVY>
__global__ void __launch_bounds__(TRACE_BLOCK) k_trace5_quadrics(K5_PARAMS);
TRACE_KERNEL(TRACE_GEN, RAY_CLOSEST, false, k_trace5_quadrics<false, false>)
TRACE_KERNEL(TRACE_GEN, RAY_ANY, false, k_trace5_quadrics<true, false>)
TRACE_KERNEL(TRACE_GEN_HEAVY, RAY_CLOSEST, false, k_trace5_quadrics<false, true>)
TRACE_KERNEL(TRACE_GEN_HEAVY, RAY_ANY, false, k_trace5_quadrics<true, true>)
template <bool HEAVY>
__global__ void __launch_bounds__(TRACE_BLOCK) k_trace5_quadrics_any_strict(K5_PARAMS);
TRACE_KERNEL(trace_strict_variant(TRACE_GEN), RAY_ANY, true, k_trace5_quadrics_any_strict<false>)
TRACE_KERNEL(trace_strict_variant(TRACE_GEN_HEAVY), RAY_ANY, true, k_trace5_quadrics_any_strict<true>)
#undef TRACE_KERNEL
constexpr TraceKernel QUADRIC_KERNELS[2][N_RAY] = {{k_trace5_quadrics<false, false>, k_trace5_quadrics<true, false>}, {k_trace5_quadrics<false, true>, k_trace5_quadrics<true, true>}};  // [variant - TRACE_GEN]
constexpr TraceKernel QUADRIC_KERNELS_ANY_STRICT[2] = {k_trace5_quadrics_any_strict<false>, k_trace5_quadrics_any_strict<true>};  // [trace_strict_variant - TRACE_GEN]
static_assert(TRACE_GEN_HEAVY == TRACE_GEN + 1 && N_TRACE == TRACE_GEN + 2, "the general rows are the last two of TRACE_SHAPES");

}  // namespace

TraceKernel wf_trace_quadrics_kernel(int variant, int ray, bool any_strict) {
    if (variant != TRACE_GEN && variant != TRACE_GEN_HEAVY) return nullptr;  // (a scene with a sphere record never plans TRACE_TRI)
    return any_strict ? QUADRIC_KERNELS_ANY_STRICT[trace_strict_variant(variant) - TRACE_GEN] : QUADRIC_KERNELS[variant - TRACE_GEN][ray];
}
