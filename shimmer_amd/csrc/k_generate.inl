// k_generate.inl — K1, the camera rays of one batch: generate_paths, its kernels k_generate (box filter) / k_generate_filtered (the other pixel filters), and the unit's
// one launcher, wf_generate<K_SPHERICAL_CAMERA> (wavefront.h). Included behind wavefront.h by two units: render.hip (the reference's perspective and orthographic
// cameras: its kernels know nothing else) and k_generate_spherical.hip (K_SPHERICAL_CAMERA: the same kernels with PBRT-v4's spherical camera compiled into the leaf, for
// scenes whose camera is one). Which kernels a unit holds is not written here: the table at the end is computed from shm_plan::has_generate_build (host/render_plan.hpp).
#include <array>

namespace {
#if K_SPHERICAL_CAMERA
namespace spherical {  // (the spherical unit's kernels carry the camera in their names: a profile or a disassembly tells the two units' apart)
#endif
// ---------------------------------------------------------------------------------------------
// K1: camera rays for one batch, one path slot per lane (slot_of, wavefront.h, is the slots' order).
// ---------------------------------------------------------------------------------------------
// HAS_TEX: scenes that bind image textures carry the camera ray's auxiliary rays (a compile-time switch: with a run-time pointer the
// auxiliary-ray record lived in scratch memory, 52 B of stores per path, in every scene)
// FC: the pixel filter's class (shm/filter.h). filter_table: the tabulated class's table (the block's copy in LDS); filter_weight: where a filter whose weight differs
// from sample to sample (Mitchell, sinc) leaves it for k_film_weighted, null otherwise.
template <bool HAS_TEX, bool LEAN, bool ZS, int FC>
__device__ __forceinline__ void generate_paths(const SceneView& sv, const PathArrays& pa, const uint32_t* pixels, uint32_t n_pix, int sample_begin, int n_samples,
                                               const ShmRenderParams& params, uint32_t* q_active, QueueState* qs, uint32_t pix_group, const Float* filter_table,
                                               float* filter_weight) {
    uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t total = n_pix * (uint32_t)n_samples;
    if (slot >= total) return;
    uint32_t g = slot / (pix_group * (uint32_t)n_samples);
    uint32_t g0 = g * pix_group;
    uint32_t pg = min(pix_group, n_pix - g0);
    uint32_t rem = slot - g0 * (uint32_t)n_samples;
    uint32_t s_local = rem / pg;
    uint32_t p_local = g0 + (rem - s_local * pg);
    uint32_t pix = pixels[p_local];
    int px = (int)(pix & 0xffffu), py = (int)(pix >> 16);
    Rng rng = sampler_start_pixel_sample(px, py, sample_begin + (int)s_local, params.seed, sampler_word<ZS>(sv));
    Wavelengths lambda;
    Float weight;
    constexpr bool has_tex = HAS_TEX;
    AuxRays aux = aux_none();
    Ray r = generate_camera_ray<FC>(sv, px, py, rng, params.disable_wavelength_jitter != 0, params.disable_pixel_jitter != 0,
                                    lambda, weight, HAS_TEX ? &aux : nullptr, params.samples_per_pixel, filter_table);
    if (HAS_TEX) st_aux(pa, slot, aux);
    if (FC == FILTER_CLASS_TABULATED && filter_weight) filter_weight[slot] = weight;
    ShmRay ray;
    ray.o[0] = r.o.x; ray.o[1] = r.o.y; ray.o[2] = r.o.z;
    ray.d[0] = r.d.x; ray.d[1] = r.d.y; ray.d[2] = r.d.z;
    ray.t_max = infinity();
    ray.pad = 0.0f;
    pa.ray[slot] = ray;
    pa.L[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // LEAN (the fused kernel shades bounce 0 and knows it is bounce 0): the constants — beta = 1, p_b = eta_scale = 1, flags = 0, the identity queue — are not
    // written here nor read there (ShadeArgs::first_bounce): 32 of 124 bytes per path
    const float4 lambda4 = make_float4(lambda.lambda[0], lambda.lambda[1], lambda.lambda[2], lambda.lambda[3]);
    pa.lambda[slot] = lambda4;  // (the film's copy: k_film reads wavelengths and pdfs of every sample, and a 64-byte record for 16 of its bytes would triple that)
    pa.lambda_pdf[slot] = make_float4(lambda.pdf[0], lambda.pdf[1], lambda.pdf[2], lambda.pdf[3]);
    // (the CtxRec, the previous vertex's LightSampleContext, is first read at depth >= 1, after k_shade has written them)
    if (LEAN) {
        // no record: the fused kernel's bounce 0 reads these three arrays and writes the path's first record whole (one full 64-byte store instead of this kernel's
        // partial sectors: k_generate 10.5 -> 6 ms per headline frame)
        pa.rng0[slot] = sampler_store(rng);
        pa.pixel0[slot] = pix;
    } else {
        PathRec r;
        r.lambda = lambda4;
        r.rng = sampler_store(rng);
        r.pixel = pix;
        r.flags = has_tex ? (1u << 10) : 0u;  // camera rays always carry auxiliary rays (camera.rs:1070-1078)
        r.beta = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        r.pb_eta = make_float2(1.0f, 1.0f);
        r.pad[0] = 0u; r.pad[1] = 0u;
        pa.rec[slot] = r;
    }
    if (!LEAN) q_active[slot] = slot;  // first bounce: identity queue
    if (slot == 0) {
        qs->n_active[0] = total;
        qs->n_active[1] = 0;
        qs->n_shadow[0] = 0;
        qs->n_shadow[1] = 0;
        qs->n_scatter[0] = qs->n_scatter[1] = qs->n_scatter[2] = qs->n_scatter[3] = 0;
        qs->n_emit = 0;
        qs->n_lean = 0;
        qs->n_split = 0;
    }
}
// The box filter's kernel (the reference's filter; the headline path)
template <bool HAS_TEX, bool LEAN = false, bool ZS = false>  // ZS: the ZSobol sampler (wavefront.h, K_ZSOBOL)
__global__ void __launch_bounds__(SHADE_BLOCK) k_generate(SceneView sv, PathArrays pa, const uint32_t* pixels, uint32_t n_pix,
                                                        int sample_begin, int n_samples, ShmRenderParams params,
                                                        uint32_t* q_active, QueueState* qs, uint32_t pix_group) {
    generate_paths<HAS_TEX, LEAN, ZS, FILTER_CLASS_BOX>(sv, pa, pixels, n_pix, sample_begin, n_samples, params, q_active, qs, pix_group, nullptr, nullptr);
}
// The other pixel filters' kernels. The triangle filter is sampled in closed form. The tabulated class (gaussian, Mitchell, sinc) inverts two 1-D CDFs of up to 257 entries
// per path by binary search, every lane at an index of its own: the block copies the table (at most 6.2 KB, 3.1 KB at PBRT-v4's widest default radius) into LDS once and
// searches it there.
template <bool HAS_TEX, bool LEAN, bool ZS, int FC>
__global__ void __launch_bounds__(SHADE_BLOCK) k_generate_filtered(SceneView sv, PathArrays pa, const uint32_t* pixels, uint32_t n_pix,
                                                                 int sample_begin, int n_samples, ShmRenderParams params,
                                                                 uint32_t* q_active, QueueState* qs, uint32_t pix_group, float* filter_weight) {
    static_assert(FC == FILTER_CLASS_TRIANGLE || FC == FILTER_CLASS_TABULATED, "the box filter runs k_generate");
    if constexpr (FC == FILTER_CLASS_TABULATED) {
        __shared__ uint4 s_table[(FILTER_TABLE_MAX_FLOATS + 3) / 4];
        // (the table's length is in its head: flatten_scene bounds it by FILTER_TABLE_MAX_FLOATS and pads it to whole uint4s)
        const uint32_t nx = float_to_bits(sv.dist_data[1]), ny = float_to_bits(sv.dist_data[2]);
        const uint32_t n4 = min(((uint32_t)filter_table_floats((int)nx, (int)ny) + 3u) / 4u, (uint32_t)((FILTER_TABLE_MAX_FLOATS + 3) / 4));
        const uint4* g = reinterpret_cast<const uint4*>(sv.dist_data);
        for (uint32_t i = threadIdx.x; i < n4; i += blockDim.x) s_table[i] = g[i];
        __syncthreads();
        generate_paths<HAS_TEX, LEAN, ZS, FC>(sv, pa, pixels, n_pix, sample_begin, n_samples, params, q_active, qs, pix_group, reinterpret_cast<const Float*>(s_table),
                                              filter_weight);
    } else {
        generate_paths<HAS_TEX, LEAN, ZS, FC>(sv, pa, pixels, n_pix, sample_begin, n_samples, params, q_active, qs, pix_group, nullptr, nullptr);
    }
}
// The unit's kernels by the plan's coordinates, [ZS ? 0 : 1][filter class][HAS_TEX][LEAN]: a cell launches its kernel where shm_plan::has_generate_build says there is one and
// is null elsewhere. The box filter's kernel and the others' differ by the filter_weight argument.
using GenerateLaunch = void (*)(ShmScene*, const GenerateArgs&);
template <bool HAS_TEX, bool LEAN, bool ZS, int FC>
void launch_generate(ShmScene* s, const GenerateArgs& a) {
    const uint32_t total = a.n_pix * (uint32_t)a.n_samples;
    auto launch = [&](auto kernel, auto... more) {
        hipLaunchKernelGGL(kernel, dim3((total + SHADE_BLOCK - 1) / SHADE_BLOCK), dim3(SHADE_BLOCK), 0, a.stream, s->dsv, s->pa, a.pixels, a.n_pix, a.sample_begin, a.n_samples,
                           a.params, s->d_q_active[0], s->d_qs, s->pix_group, more...);
    };
    if constexpr (FC == FILTER_CLASS_BOX) launch(k_generate<HAS_TEX, LEAN, ZS>);
    else launch(k_generate_filtered<HAS_TEX, LEAN, ZS, FC>, s->d_filter_weight);
}
template <bool HAS_TEX, bool LEAN, bool ZS, int FC>
constexpr GenerateLaunch generate_cell() {
    if constexpr (shm_plan::has_generate_build(HAS_TEX, LEAN)) return launch_generate<HAS_TEX, LEAN, ZS, FC>;
    else return nullptr;
}
using GenerateClassCells = std::array<std::array<GenerateLaunch, 2>, 2>;  // [HAS_TEX][LEAN]
using GenerateSamplerCells = std::array<GenerateClassCells, 3>;           // [filter class]
template <bool ZS, int FC>
constexpr GenerateClassCells generate_class_cells = {{{generate_cell<false, false, ZS, FC>(), generate_cell<false, true, ZS, FC>()},
                                                      {generate_cell<true, false, ZS, FC>(), generate_cell<true, true, ZS, FC>()}}};
static_assert(FILTER_CLASS_BOX == 0 && FILTER_CLASS_TRIANGLE == 1 && FILTER_CLASS_TABULATED == 2, "the order of generate_sampler_cells' initializer");
template <bool ZS>
constexpr GenerateSamplerCells generate_sampler_cells = {generate_class_cells<ZS, FILTER_CLASS_BOX>, generate_class_cells<ZS, FILTER_CLASS_TRIANGLE>, generate_class_cells<ZS, FILTER_CLASS_TABULATED>};
// The order in which the cells are first named is the order of the kernels in the unit's code object, and that order is part of a ZSobol kernel's text: it calls
// shm::zsobol_bits, which heads the code object, by its distance. So the tables name ZSobol first, [ZS ? 0 : 1], and render.hip's unit, whose table once began with the box
// filter's row of both samplers, still names that row first (profiles/generate_launcher.md). A change that may alter the kernels' text can drop both.
#if !K_SPHERICAL_CAMERA
constexpr std::array<GenerateClassCells, 2> generate_box_cells_first = {generate_class_cells<true, FILTER_CLASS_BOX>, generate_class_cells<false, FILTER_CLASS_BOX>};
#endif
constexpr std::array<GenerateSamplerCells, 2> generate_table = {generate_sampler_cells<true>, generate_sampler_cells<false>};
// (an initializer with a cell left out would leave a null behind: the table is held to the rule here, not at the first render)
constexpr bool generate_table_is_the_rule() {
    for (int zs = 0; zs < 2; ++zs)
        for (int fc = 0; fc < 3; ++fc)
            for (int tex = 0; tex < 2; ++tex)
                for (int lean = 0; lean < 2; ++lean)
                    if ((generate_table[zs][fc][tex][lean] != nullptr) != shm_plan::has_generate_build(tex != 0, lean != 0)) return false;
    return true;
}
static_assert(generate_table_is_the_rule(), "k_generate.inl: the table lacks a build shm_plan::has_generate_build names, or holds one it does not name");
#if K_SPHERICAL_CAMERA
}  // namespace spherical
using namespace spherical;
#endif
}  // namespace

template <> int wf_generate<K_SPHERICAL_CAMERA>(ShmScene* s, const GenerateArgs& a) {
    const GenerateLaunch launch = generate_table[a.zs ? 0 : 1][shm_plan::generate_filter_class(a.flt)][a.tex ? 1 : 0][a.lean ? 1 : 0];
    if (!launch) { shm_err() = "internal: the render plan calls a k_generate build that does not exist"; return SHM_ERR_INTERNAL; }
    launch(s, a);
    LAUNCH_TRY("k_generate");
    return SHM_OK;
}
