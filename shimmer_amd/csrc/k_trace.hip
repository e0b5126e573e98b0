// k_trace.hip — K2 / K3: BVH traversal of the gfx950 wavefront path tracer (see wavefront.h).
//   aggregate.rs:71-139    BvhAggregate::intersect           -> k_trace5<false, GEN>
//   aggregate.rs:141-203   BvhAggregate::intersect_predicate -> k_trace5<true, GEN>
// One body (trace5_body), the reference's algorithm node for node, executed as UNIFORM steps; GEN = false for scenes made of top-level triangles only, GEN = true for
// scenes that also hold spheres, bilinear patches or instances. (Rounds 1-4 shipped a second body beside it, the one-node step k_trace3 — test the current node, push the
// far child untested — as the kernel of non-triangle scenes and the A/B partner of this one: retired in round 5, when the both-children step learned the other shapes
// and measured 112-171 ms where that kernel took 228-278 on the same frames, profiles/r05_cliff_before.json beside r05_bench_final.json. What it established stays in the
// comments below and in DESIGN.md section 4.)
// WHICH entry point a scene's rays take, and at what occupancy and LDS stack depth it is compiled, is one row of host/render_plan.hpp's TRACE_SHAPES: the kernels' attributes
// (below the body), the scene's grid and stack spill (wf_trace_prepare) and the launch (wf_launch_trace, through one table of kernel pointers) are all made from that row.
// The body itself is k_trace.inl: k_trace_quadrics.hip holds the general rows a second time, with PBRT-v4's disk and cylinder in the sphere test, under the same rows.
// Its loop is laid out for the COMMON iteration — no refill, a regular wave, a push to and a pop from LDS — to be straight-line code: the scalar unit is one per four
// SIMDs, and that iteration issued as many scalar and branch instructions as vector ones (profiles/trace_straight.md: what each piece of control flow compiles to).
#include "k_trace.inl"

namespace {

template <bool ANY, bool GEN = false, bool HEAVY = false>
__global__ void __launch_bounds__(TRACE_BLOCK) k_trace5(K5_PARAMS);
TRACE_KERNEL(TRACE_TRI, RAY_CLOSEST, false, k_trace5<false, false>)
TRACE_KERNEL(TRACE_TRI, RAY_ANY, false, k_trace5<true, false>)
TRACE_KERNEL(TRACE_GEN, RAY_CLOSEST, false, k_trace5<false, true>)
TRACE_KERNEL(TRACE_GEN, RAY_ANY, false, k_trace5<true, true>)
// HEAVY (round 6): scenes where the non-triangle tests are the RULE — a quad PLY file becomes one BilinearPatch per face in the reference (shape/mesh.rs:233-256), so a real
// scene's object is patches, not triangles. At seven waves (72 VGPRs) the parked round's arithmetic lives in spill code: 124 / 94 spilled VGPRs, 164 / 148 B of scratch per
// lane — harmless where a round runs every 270 iterations (one sphere among 4.3 M triangles), and 0.7 TB of scratch traffic per frame where one runs every 17 (S3 as 2.15 M
// patches: K2 263 ms, K3 171 ms against 92 / 59 for the same object as triangles). The SAME body at five waves per SIMD holds it in registers (96 VGPRs + 10 spilled / 93 + 0):
// K2 158, K3 87 ms, 2 261 -> 3 496 Mray/s; with the refill at 24 idle lanes and the patch's fourth corner in its own record (flatten.h) K2 147, K3 77 ms, 3 736 Mray/s
// (profiles/r06_patch_heavy_scenes.txt), with the save area around the test in LDS K2 138, K3 72 ms, 3 909 Mray/s; with few non-triangles the seven-wave build stays ahead by 3-10 % (occupancy for the node step): chosen per scene (ScenePlan::trace_variant).
TRACE_KERNEL(TRACE_GEN_HEAVY, RAY_CLOSEST, false, k_trace5<false, true, true>)
TRACE_KERNEL(TRACE_GEN_HEAVY, RAY_ANY, false, k_trace5<true, true, true>)
// the any-hit kernels of scenes with instances under ShmRenderParams::disable_reference_quirks (trace5_body, STRICT): seven waves, and the five-wave build for patch-heavy scenes
template <bool HEAVY>
__global__ void __launch_bounds__(TRACE_BLOCK) k_trace5_any_strict(K5_PARAMS);
TRACE_KERNEL(trace_strict_variant(TRACE_GEN), RAY_ANY, true, k_trace5_any_strict<false>)
TRACE_KERNEL(trace_strict_variant(TRACE_GEN_HEAVY), RAY_ANY, true, k_trace5_any_strict<true>)
#undef TRACE_KERNEL
constexpr TraceKernel TRACE_KERNELS[N_TRACE][N_RAY] = {
    {k_trace5<false, false>, k_trace5<true, false>}, {k_trace5<false, true>, k_trace5<true, true>}, {k_trace5<false, true, true>, k_trace5<true, true, true>}};
constexpr TraceKernel TRACE_KERNELS_ANY_STRICT[2] = {k_trace5_any_strict<false>, k_trace5_any_strict<true>};  // [trace_strict_variant - TRACE_GEN]

// (Round 5 built and measured k_trace6 here — TWO rays per lane, each phase run for whichever slot of a lane is ready: bit-exact, 23 % fewer wave iterations, 38.3 instead of 31.4
// lanes per VALU instruction, and 62 % more instructions per iteration for the selects that bring the chosen slot's state to each phase: K2 91 -> 133 ms, K3 58 -> 79 ms.
// Rejected with profiles/r05_rejected_two_rays_per_lane.txt; the code left the tree in round 6 (git history: round-5 commits of k_trace.hip).)

__global__ void k_reset_trace_heads(uint32_t* heads) { for (uint32_t i = threadIdx.x; i < TRACE_QUEUE_PARTS * TRACE_HEAD_STRIDE; i += blockDim.x) heads[i] = 0; }
}  // namespace

// k_trace_alpha.hip (scenes with shape alpha): the launch's SceneView to HBM (TraceSide::d_view), in stream order in front of the traversal kernel that reads the scene through it
WF_INTERNAL void wf_trace_alpha_store_view(hipStream_t stream, const SceneView& view, SceneView* dst);

void wf_trace_census() {
#ifdef K5_CENSUS
    unsigned long long c[32];
    if (hipMemcpyFromSymbol(c, HIP_SYMBOL(g_census), sizeof(c)) != hipSuccess || !c[0]) return;
    const double it = (double)c[0];
    fprintf(stderr, "[k5 census, %s] wave iterations %.3e | lanes per iteration: at a node %.1f, on a pending leaf %.1f, idle %.1f, pop pending %.1f | iterations with a node step %.3f\n"
                    "  leaf phases %.3e (one per %.2f iterations), primitive rounds %.3e at %.1f lanes | pop rounds %.3e at %.1f lanes | refills %.3e at %.1f rays\n",
            K5_CENSUS == 2 ? "any-hit" : "closest-hit", it, c[1] / it, c[2] / it, c[3] / it, c[4] / it, c[10] / it, (double)c[5], it / (double)c[5], (double)c[6], (double)c[7] / (double)c[6], (double)c[8], (double)c[9] / (double)c[8],
            (double)c[11], (double)c[12] / (double)c[11]);
    if (c[15]) fprintf(stderr, "  GEN: parked on a non-triangle test %.1f lanes per iteration | other phases %.3e (one per %.2f iterations) at %.1f lanes, %.1f %% of them because nothing else could run | instance entries %.3e | leave rounds %.3e at %.1f lanes\n",
                       c[21] / it, (double)c[15], it / (double)c[15], (double)c[16] / (double)c[15], 100.0 * (double)c[17] / (double)c[15], (double)c[18], (double)c[19], c[19] ? (double)c[20] / (double)c[19] : 0.0);
    fprintf(stderr, "  with 8 or fewer lanes on: %.1f %% of the node steps, %.1f %% of the leaf phases, %.1f %% of the pop rounds, %.1f %% of the %.3e retire rounds, %.1f %% of the other phases\n",
            100.0 * (double)c[22] / (double)(c[10] ? c[10] : 1), 100.0 * (double)c[23] / (double)(c[5] ? c[5] : 1), 100.0 * (double)c[24] / (double)(c[8] ? c[8] : 1), 100.0 * (double)c[25] / (double)(c[26] ? c[26] : 1), (double)c[26],
            100.0 * (double)c[27] / (double)(c[15] ? c[15] : 1));
    fprintf(stderr, "  s_memtime ticks: in refills %.3e of %.3e wave-loop ticks = %.1f %% (%.0f ticks per refill)\n", (double)c[13], (double)c[14], 100.0 * (double)c[13] / (double)c[14], (double)c[13] / (double)c[11]);
#endif
}

// The scene's side of its rows: the persistent grid (one workgroup per wave-per-SIMD and CU), the HBM stack spill and, for the GEN bodies, the ray-state save areas
int wf_trace_prepare(ShmScene* s) {
    if (s->flat.nodes.size() + s->flat.instances.size() + 2 > (size_t)1 << 27) { shm_err() = "more than 2^27 BVH nodes (the traversal kernels address the node array with 32-bit byte offsets)"; return SHM_ERR_UNSUPPORTED; }
    if (s->flat.instances.size() >= ((size_t)1 << 25)) { shm_err() = "more than 2^25 instances (the traversal kernels keep the instance index in 26 bits)"; return SHM_ERR_UNSUPPORTED; }
    const int variant = s->plan.trace_variant;
    for (int ray = 0; ray < N_RAY; ++ray) {
        TraceSide& side = s->trace[ray];
        side.blocks = s->n_cu * TRACE_SHAPES[variant][ray].waves;
        side.spill_levels = s->plan.trace_spill_levels[ray];
        const size_t lanes = (size_t)side.blocks * TRACE_BLOCK;
        void* d = nullptr;
        if (hipMalloc(&d, lanes * (size_t)side.spill_levels * 2u * sizeof(uint32_t)) != hipSuccess) { shm_err() = "hipMalloc of the traversal stack spill failed"; return SHM_ERR_OUT_OF_MEMORY; }  // (8-byte stack entries)
        s->allocs.push_back(d);
        side.d_spill = static_cast<uint32_t*>(d);
        if (variant != TRACE_TRI) {  // trace5_body<., GEN>: two 48-byte ray-state save areas per resident lane
            void* g = nullptr;
            if (hipMalloc(&g, lanes * 6 * sizeof(float4)) != hipSuccess) { shm_err() = "hipMalloc of the traversal save areas failed"; return SHM_ERR_OUT_OF_MEMORY; }
            s->allocs.push_back(g);
            side.d_gen_save = static_cast<float4*>(g);
        }
        if (s->plan.f.has_alpha) {  // k_trace_alpha.hip: the alpha texture's evaluators read the scene through a SceneView in memory
            void* v = nullptr;
            if (hipMalloc(&v, sizeof(SceneView)) != hipSuccess) { shm_err() = "hipMalloc of the traversal kernels' scene view failed"; return SHM_ERR_OUT_OF_MEMORY; }
            s->allocs.push_back(v);
            side.d_view = static_cast<SceneView*>(v);
        }
    }
    return SHM_OK;
}

// One launch through the kernel table, by the plan's coordinates: the scene's variant, the ray kind and — any hit only — the render's strictness; a scene with a disk or a
// cylinder takes k_trace_quadrics.hip's kernel of the same row (same grid, same spill, same save areas: wf_trace_prepare sized them by the row), a scene with a cutout
// (shape alpha) k_trace_alpha.hip's, which knows both
int wf_launch_trace(ShmScene* s, int ray, bool any_strict, const TraceArgs& t) {
    const TraceSide& side = s->trace[ray];
    const ScenePlan& p = s->plan;
    const bool any = ray == RAY_ANY;
    const TraceKernel kernel = p.f.has_alpha ? wf_trace_alpha_kernel(p.trace_variant, ray, any && any_strict)
                               : p.f.has_quadric_kinds ? wf_trace_quadrics_kernel(p.trace_variant, ray, any && any_strict)
                               : ((any && any_strict) ? TRACE_KERNELS_ANY_STRICT[trace_strict_variant(p.trace_variant) - TRACE_GEN] : TRACE_KERNELS[p.trace_variant][ray]);
    if (!kernel) { shm_err() = "internal: no traversal kernel with shape alpha or the disk and the cylinder for this scene's row"; return SHM_ERR_INTERNAL; }
    SceneView view = s->dsv;
    if (p.f.has_alpha) {
        if (!side.d_view) { shm_err() = "internal: a scene with shape alpha without its traversal scene view"; return SHM_ERR_INTERNAL; }
        view.call_copy = side.d_view;  // (the copy names itself: the evaluators hand it on to each other)
        wf_trace_alpha_store_view(t.stream, view, side.d_view);
    }
    hipLaunchKernelGGL(k_reset_trace_heads, dim3(1), dim3(64), 0, t.stream, side.d_heads);
    hipLaunchKernelGGL(kernel, dim3(side.blocks), dim3(TRACE_BLOCK), 0, t.stream, view, t.queue, t.n_ptr, t.n_direct, side.d_heads, t.rays, t.hits, t.occluded, t.L, t.contrib,
                       s->d_counters, side.d_spill, side.spill_levels, any ? p.refill_min_any : p.refill_min, any ? p.leaf_min_any : p.leaf_min, (int)TRACE_QUEUE_PARTS,
                       p.trace_rays_per_lane, t.hit16, s->d_big_leaf_n, side.d_gen_save, any ? p.other_min_any : p.other_min, t.hit2);
    LAUNCH_TRY(any ? "k_trace<any>" : "k_trace<closest>");
    return SHM_OK;
}
