// render.hip — the MI355X (gfx950, wave64) wavefront path tracer behind include/shimmer_hip.h.
//
// Replaces the tile-parallel loop of the reference (paths relative to /root/reference/src):
//   integrator.rs:226-322  ImageTileIntegrator::render      -> shm_render / shm_render_device / shm_render_wave (host loop below)
//   integrator.rs:326-396  evaluate_pixel_sample            -> K1 (wf_generate: the generate units)
//   aggregate.rs:71-139    BvhAggregate::intersect          -> K2 k_trace5<false, GEN> (persistent waves, LDS stack, both children per step)
//   aggregate.rs:141-203   BvhAggregate::intersect_predicate-> K3 k_trace5<true, GEN>
//   integrator.rs:772-892  PathIntegrator::li loop body     -> K4+K5 k_shade<HAS_LAYERED, TRI_ONLY> (one path vertex per launch)
//   integrator.rs:897-963  PathIntegrator::sample_ld        -> inside k_shade (shadow ray deferred to K3)
//   film.rs:548-574        RgbFilm::add_sample              -> K6 k_film (per-pixel ordered f64 sums)
// Leaf arithmetic is the single-source header library csrc/shm/*.h (compiled with -ffp-contract=off).
//
// Execution model: one (pixel, sample) per lane; paths live in SoA arrays in HBM; each bounce is
// trace_closest -> shade -> trace_any over index queues compacted with wave-aggregated atomics; queue
// sizes stay on the device (persistent / grid-stride kernels read them), so a whole render (all fused spp-waves)
// is enqueued on one HIP stream without host round trips. There is no CPU fallback anywhere in this file.
#include <chrono>
#include <functional>
#include "wavefront.h"
#include "host/integrator.hpp"

std::string& shm_err() {
    thread_local std::string e;
    return e;
}
#define g_err shm_err()

namespace {

// ---------------------------------------------------------------------------------------------
// K0: expand the tile list into a pixel list (reference loop order inside a tile: x outer, y inner;
// integrator.rs:257-258).  One thread per tile; tiny.
// ---------------------------------------------------------------------------------------------
__global__ void k_expand_tiles(const ShmTile* tiles, const uint32_t* tile_offset, uint32_t n_tiles, uint32_t* pixels) {
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    ShmTile tl = tiles[t];
    uint32_t k = tile_offset[t];
    for (int x = tl.x0; x < tl.x1; ++x)
        for (int y = tl.y0; y < tl.y1; ++y) pixels[k++] = (uint32_t)x | ((uint32_t)y << 16);
}

// Scene creation: the shading records of the flat triangles (shm/tri_shade.h), one thread per primitive slot. The record is what triangle_interaction + get_bsdf — the
// code the shading kernels would run at every hit on the slot — leave behind; the slot's PrimRec::pad[1] says that it is there.
// This unit is built without SHM_DIFFUSE_TRANSMISSION (wavefront.h), so get_bsdf here takes a diffuse transmission material down its last arm, the CoatedConductor's. Only
// the FRAME is kept, which no material kind enters (the displacement and the normal map are read before the kinds part), and flatten_scene (host/flatten.h, "A diffuse
// transmission material reads ...") clears every field of such a material that that arm reads and validation did not cover: the arm evaluates constants, and its result is dropped.
__global__ void __launch_bounds__(256) k_build_tri_shade(SceneView sv, PrimRec* prim_recs, TriShadeRec* recs, uint32_t n_prims, uint32_t* n_built, uint32_t plain_only) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_prims) return;
    const PrimRec pr = prim_recs[i];
    TriShadeRec r;
    if (!tri_shade_eligible(sv, pr, plain_only != 0u) || !tri_shade_record(sv, pr, r)) return;
    recs[i] = r;
    prim_recs[i].pad[1] = 1u;
    atomicAdd(n_built, 1u);
}
// Between bounces: recycle the counters (1 thread).
__global__ void k_next_bounce(QueueState* qs, int cur, int next_shadow_parity) {
    qs->n_active[cur] = 0;
    qs->n_scatter[0] = qs->n_scatter[1] = qs->n_scatter[2] = qs->n_scatter[3] = 0;
    qs->n_lean = 0;
    qs->n_split = 0;
    qs->n_emit = 0;
    qs->n_shadow[next_shadow_parity] = 0;  // the one the NEXT shade launch fills; this bounce's count stays for its K3
}
// ---------------------------------------------------------------------------------------------
// Scenes WITH textures (round 5): the split pass in front of the textured vertex kernel. Until then one textured material put every vertex of the scene through the textured
// class's kernels — ray differentials, the 48-byte differential arrays, 256 VGPRs at two waves per SIMD —: the headline scene with a textured material OUT OF SIGHT shaded in
// 207 ms per frame against 86. A vertex on a DiffuseMaterial that binds no texture (ShmMaterial::pad[0], flatten_scene) needs none of it, and a diffuse bounce ends the
// ray differentials (interaction.rs:430-514: only specular bounces carry them on): nothing a later texture look-up reads depends on which kernel shaded it. This pass — a
// few registers, full occupancy — sends such hits to q_lean (the lean fused kernel takes their whole vertex, as in the lean diversion of k_vertex.inl) and everything
// else, escaped rays included, to q_split, which the textured kernels work through. Paths are independent and every later queue is order-agnostic: films and counters
// do not change.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SHADE2_BLOCK) k_split_plain(SceneView sv, PathArrays pa, const uint32_t* __restrict__ q_cur, uint32_t* __restrict__ q_lean,
                                                             uint32_t* __restrict__ q_split, QueueState* qs, int cur) {
    const uint32_t n = qs->n_active[cur];
    __shared__ uint32_t s_q[2][SHADE_CHUNK];
    __shared__ uint32_t s_cnt[2], s_base[2];
    for (uint32_t chunk0 = blockIdx.x * SHADE_CHUNK; chunk0 < n; chunk0 += gridDim.x * SHADE_CHUNK) {
        if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t k = 0; k < SHADE_CHUNK / SHADE2_BLOCK; ++k) {
            const uint32_t i = chunk0 + k * SHADE2_BLOCK + threadIdx.x;
            bool plain = false, rest = false;
            uint32_t path = 0;
            if (i < n) {
                path = q_cur[i];
                const int prim = pa.hit16 ? hit_prim_of(__float_as_int(reinterpret_cast<const float*>(reinterpret_cast<const float4*>(pa.hit) + path)[0])) : __float_as_int(reinterpret_cast<const float*>(pa.hit + path)[0]);
                plain = prim >= 0 && (sv.materials[sv.prim_recs[prim].material].pad[0] & 1u) != 0u;
                rest = !plain;
            }
            const uint32_t a = queue_push_slot(&s_cnt[0], plain);
            if (plain) s_q[0][a] = path;
            const uint32_t b = queue_push_slot(&s_cnt[1], rest);
            if (rest) s_q[1][b] = path;
        }
        __syncthreads();
        if (threadIdx.x == 0) s_base[0] = s_cnt[0] ? atomicAdd(&qs->n_lean, s_cnt[0]) : 0u;
        if (threadIdx.x == 1) s_base[1] = s_cnt[1] ? atomicAdd(&qs->n_split, s_cnt[1]) : 0u;
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < s_cnt[0]; j += SHADE2_BLOCK) q_lean[s_base[0] + j] = s_q[0][j];
        for (uint32_t j = threadIdx.x; j < s_cnt[1]; j += SHADE2_BLOCK) q_split[s_base[1] + j] = s_q[1][j];
        __syncthreads();
    }
}
// ---------------------------------------------------------------------------------------------
// K6: RgbFilm::add_sample for every sample of the batch, per pixel in sample order (f64 sums are
// order dependent; the reference adds samples of a pixel in increasing sample_index).
// ---------------------------------------------------------------------------------------------
// W: where a sample's filter weight comes from (shm_plan::film_weight, host/render_plan.hpp). FILM_WEIGHT_ONE: it is 1 (box, triangle; every filter under
// options.disable_pixel_jitter); FILM_WEIGHT_CONSTANT: the one constant `weight_k` of the scene's table (gaussian: still accumulated as K, so that weight_sum is spp * K
// as in the oracle); FILM_WEIGHT_PER_SAMPLE: +-K as K1 left it per path slot (Mitchell, sinc).
using namespace shm_plan;
template <int W>
__device__ __forceinline__ void film_add_samples(const SceneView& sv, const PathArrays& pa, const uint32_t* pixels, uint32_t n_pix, int n_samples, ShmFilmPixel* film,
                                                 DeviceCounters* counters, uint32_t pix_group, const float* filter_weight, float weight_k) {
    uint32_t p_local = blockIdx.x * blockDim.x + threadIdx.x;
    if (p_local >= n_pix) return;
    uint32_t pix = pixels[p_local];
    int px = (int)(pix & 0xffffu), py = (int)(pix >> 16);
    int width = sv.pixel_bounds[2] - sv.pixel_bounds[0];
    ShmFilmPixel* fp = film + (size_t)(py - sv.pixel_bounds[1]) * (size_t)width + (size_t)(px - sv.pixel_bounds[0]);
    double r = fp->rgb_sum[0], g = fp->rgb_sum[1], b = fp->rgb_sum[2], w = fp->weight_sum;
    for (int s = 0; s < n_samples; ++s) {
        uint32_t slot = slot_of(p_local, (uint32_t)s, n_pix, (uint32_t)n_samples, pix_group);
        Spec L = ld_spec(pa.L[slot]);
        if (sv.quirks_off && !spec_is_finite(L)) L = spec_const(0.0f);  // integrator.rs:377-382's TODOs, done only with the quirks switched off
        Wavelengths lambda;
        float4 a = pa.lambda[slot], c = pa.lambda_pdf[slot];
        lambda.lambda[0] = a.x; lambda.lambda[1] = a.y; lambda.lambda[2] = a.z; lambda.lambda[3] = a.w;
        lambda.pdf[0] = c.x; lambda.pdf[1] = c.y; lambda.pdf[2] = c.z; lambda.pdf[3] = c.w;
        V3 rgb = film_sample_rgb(sv, L, lambda);
        const Float weight = W == FILM_WEIGHT_ONE ? 1.0f : (W == FILM_WEIGHT_CONSTANT ? weight_k : filter_weight[slot]);  // Filter::sample's weight (shm/filter.h)
        r += (double)(weight * rgb.x);
        g += (double)(weight * rgb.y);
        b += (double)(weight * rgb.z);
        w += (double)weight;
    }
    fp->rgb_sum[0] = r; fp->rgb_sum[1] = g; fp->rgb_sum[2] = b; fp->weight_sum = w;
    if (p_local == 0) atomicAdd(&counters->paths, (unsigned long long)n_pix * (unsigned long long)n_samples);
}
__global__ void __launch_bounds__(SHADE_BLOCK) k_film(SceneView sv, PathArrays pa, const uint32_t* pixels, uint32_t n_pix, int n_samples,
                                                    ShmFilmPixel* film, DeviceCounters* counters, uint32_t pix_group) {
    film_add_samples<FILM_WEIGHT_ONE>(sv, pa, pixels, n_pix, n_samples, film, counters, pix_group, nullptr, 1.0f);
}
template <int W>
__global__ void __launch_bounds__(SHADE_BLOCK) k_film_weighted(SceneView sv, PathArrays pa, const uint32_t* pixels, uint32_t n_pix, int n_samples,
                                                             ShmFilmPixel* film, DeviceCounters* counters, uint32_t pix_group, const float* filter_weight, float weight_k) {
    film_add_samples<W>(sv, pa, pixels, n_pix, n_samples, film, counters, pix_group, filter_weight, weight_k);
}

}  // namespace

// K1 for the reference's two cameras, perspective and orthographic: this unit is built without K_SPHERICAL_CAMERA, so the .inl defines wf_generate<false> here (wavefront.h).
// (Not yet a unit of its own like the spherical camera's: the ZSobol kernels call shm::zsobol_bits at the head of the code object by its distance, which is part of their
//  text, and only this unit's kernels in front of them keep that distance what it was — profiles/generate_launcher.md.)
#include "k_generate.inl"

namespace {

template <typename T>
int dev_upload(ShmScene* s, const std::vector<T>& v, const T** out) {
    size_t bytes = (std::max<size_t>(v.size(), 1) * sizeof(T) + 15u) & ~(size_t)15u;  // (whole 16-byte groups: the LDS staging of the small tables copies uint4s)
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, bytes));
    s->allocs.push_back(d);
    if (!v.empty()) HIP_TRY(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = reinterpret_cast<const T*>(d);
    return SHM_OK;
}
template <typename T>
int dev_alloc(ShmScene* s, size_t n, T** out) {
    return wf_scene_alloc(s, std::max<size_t>(n, 1) * sizeof(T), reinterpret_cast<void**>(out));
}

// Path workspace sized to the work: up to SHM_BATCH_PATHS (default 512 Mi paths: 148 GB of the 288 GB for a lean scene, bounded by 80 % of
// what is free) so that all 256 spp of the 1024^2 frame (268 M paths, 71 GB) and all 256 spp of the 1000x1400 crown-proxy frame (358 M paths:
// its 23 late bounces of < 1 M rays cost ~2.3 ms each whatever the batch holds, once instead of twice) are ONE batch. Small batches starve the persistent traversal kernels: with ~400 K resident lanes a
// 1 M-ray launch gives each lane ~3 rays and the launch time is set by the longest ray, not by throughput (profiles/r01_*).
static uint64_t max_batch_paths() {
    uint64_t max_cap = 1ull << 29;
    if (const char* e = getenv("SHM_BATCH_PATHS")) {
        long long v = atoll(e);
        if (v >= 4096) max_cap = std::min<uint64_t>((uint64_t)v, (1ull << 30) - 4096ull);  // (below 2^30: the layered scatter kernel's jobs carry two flag bits above the path index)
    }
    return max_cap;
}

// Which kernels a scene runs: one cell per geometry x image class x sampler x extended build (DL: the *_dl builds, wavefront.h K_DELTA_LIGHTS).
// WHICH cell a render takes, and which of its launchers run, is the RenderPlan's (host/render_plan.hpp); the staged pipeline replaced the fused general kernels of
// round 1 everywhere but in the lean class (round-2 A/B, same box: coated S3 1 208 -> 1 724 Mray/s, textured Cornell 768 -> 906, crown-proxy C4 1 758 -> 1 735).
// The table is computed: a cell's launcher of a family is the build shm_plan::serving_build names for it (host/render_plan.hpp — the rule, walked by
// tests/test_render_plan.py), null where it names none. (k_vertex draws nothing: its <., ZS = false, .> builds serve both samplers.)
template <int FAMILY, int GEO, int IMG, bool ZS, bool DL>
constexpr ShadeFn shade_fn() {
    constexpr ShadeBuild b = serving_build(FAMILY, GEO, IMG);
    if constexpr (has_build(b)) return wf_shade<FAMILY, b.geo, b.img, ZS && FAMILY != FAM_VERTEX, DL>;
    else return nullptr;
}
template <int GEO, int IMG, bool ZS, bool DL>
constexpr ShadeKernels shade_cell = {
    .lean = shade_fn<FAM_LEAN, GEO, IMG, ZS, DL>(), .lean_diverted = shade_fn<FAM_LEAN_DIVERTED, GEO, IMG, ZS, DL>(),
    .fused_all = shade_fn<FAM_FUSED_ALL, GEO, IMG, ZS, DL>(), .vertex = shade_fn<FAM_VERTEX, GEO, IMG, ZS, DL>(),
    .scatter = {shade_fn<FAM_SCATTER + CLASS_DIFFUSE, GEO, IMG, ZS, DL>(), shade_fn<FAM_SCATTER + CLASS_CONDUCTOR, GEO, IMG, ZS, DL>(),
                shade_fn<FAM_SCATTER + CLASS_DIELECTRIC, GEO, IMG, ZS, DL>(), shade_fn<FAM_SCATTER + CLASS_LAYERED, GEO, IMG, ZS, DL>()},
    .scatter_layered_onepass = shade_fn<FAM_SCATTER_LAYERED_ONEPASS, GEO, IMG, ZS, DL>(),
    .simple = shade_fn<FAM_SIMPLE, GEO, IMG, ZS, DL>(), .randomwalk = shade_fn<FAM_RANDOMWALK, GEO, IMG, ZS, DL>()};
static_assert(GEO_TRI == 0 && GEO_GEN == 1 && IMG_NONE == 0 && IMG_TEX == 1 && IMG_ENV == 2 && CLASS_LAYERED == CLS_LAYERED, "the order of shade_cells' initializer");
template <bool ZS, bool DL>
constexpr ShadeKernels shade_cells[N_GEO][N_IMG] = {
    {shade_cell<GEO_TRI, IMG_NONE, ZS, DL>, shade_cell<GEO_TRI, IMG_TEX, ZS, DL>, shade_cell<GEO_TRI, IMG_ENV, ZS, DL>},
    {shade_cell<GEO_GEN, IMG_NONE, ZS, DL>, shade_cell<GEO_GEN, IMG_TEX, ZS, DL>, shade_cell<GEO_GEN, IMG_ENV, ZS, DL>},
};
// A render's shading launchers: a lookup by the plan's coordinates (K1's launcher, wf_generate, and K6's, launch_film below, take the coordinates themselves)
static ShadeKernels select_kernels(const RenderPlan& p) {
    const ShadeKernels(&cells)[N_GEO][N_IMG] = p.dl ? (p.zs ? shade_cells<true, true> : shade_cells<false, true>) : (p.zs ? shade_cells<true, false> : shade_cells<false, false>);
    ShadeKernels k = cells[p.geo][p.img];
    k.lean = cells[p.geo][p.img_lean].lean;
    k.lean_diverted = cells[p.geo][p.img_lean].lean_diverted;
    if (p.layered_onepass) k.scatter[CLASS_LAYERED] = k.scatter_layered_onepass;
    return k;
}
// ... and the one validation behind it: every launcher the plan will call is there (the null cells follow from HAS_LEAN_KERNELS by construction — serving_build reads it)
static bool kernels_complete(const ShadeKernels& k, const ScenePlan& sp, const RenderPlan& p) {
    bool ok = true;
    if (p.route == ROUTE_LEAN) ok = ok && k.lean;
    if (p.route == ROUTE_SIMPLE) ok = ok && k.simple;
    if (p.route == ROUTE_RANDOM_WALK) ok = ok && k.randomwalk;
    if (p.route == ROUTE_STAGED && p.fused_from != NEVER) ok = ok && k.fused_all;
    if (p.staged_bounce(0)) {
        ok = ok && k.vertex && (!p.drain_lean || k.lean_diverted);
        for (int c = 0; c < N_BXDF_CLASSES; ++c) ok = ok && (!sp.f.has_class[c] || k.scatter[c]);
    }
    return ok;
}
// K6 of a batch: the film kernel that takes a sample's weight from where the render's filter class leaves it (shm_plan::film_weight)
static int launch_film(ShmScene* s, const RenderPlan& p, const uint32_t* pixels, uint32_t n_pix, int n_samples) {
    auto launch = [&](auto kernel, auto... more) {
        hipLaunchKernelGGL(kernel, dim3((n_pix + SHADE_BLOCK - 1) / SHADE_BLOCK), dim3(SHADE_BLOCK), 0, s->stream, s->dsv, s->pa, pixels, n_pix, n_samples, s->d_film, s->d_counters,
                           s->pix_group, more...);
    };
    switch (film_weight(p.flt)) {  // (the weighted kernels' two arguments: the per-path weights, and the constant K that heads the scene's filter table)
        case FILM_WEIGHT_CONSTANT: launch(k_film_weighted<FILM_WEIGHT_CONSTANT>, s->d_filter_weight, s->flat.dist_data[0]); break;
        case FILM_WEIGHT_PER_SAMPLE: launch(k_film_weighted<FILM_WEIGHT_PER_SAMPLE>, s->d_filter_weight, s->flat.dist_data[0]); break;
        default: launch(k_film); break;
    }
    LAUNCH_TRY("k_film");
    return SHM_OK;
}
// The batch limit on THIS device right now: SHM_BATCH_PATHS, bounded by 80 % of the memory that is free (plus what the
// current workspace already holds), so that a GPU shared with other allocations degrades to more batches, not to an error.
// (the staging arrays count whenever the upcoming render is staged — the budget must count them BEFORE the first staged allocation)
static uint64_t workspace_cap(const ShmScene* s, bool need_staged) {
    const uint64_t BYTES_PER_PATH = ws_bytes_per_path(s->plan, ws_staged_layout(s->plan, need_staged, s->ws_staged));
    uint64_t cap = max_batch_paths();
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        uint64_t avail = (uint64_t)free_b + (uint64_t)s->capacity * BYTES_PER_PATH;
        uint64_t by_mem = (uint64_t)((double)avail * 0.8) / BYTES_PER_PATH;
        if (by_mem < cap) cap = by_mem;
    }
    return std::max<uint64_t>(cap, 4096);
}

}  // namespace
int wf_scene_alloc(ShmScene* s, size_t bytes, void** out) {
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, bytes));
    s->allocs.push_back(d);
    *out = d;
    return SHM_OK;
}
void wf_scene_free(ShmScene* s, void* d) {
    hipFree(d);
    s->allocs.erase(std::find(s->allocs.begin(), s->allocs.end(), d));
}
int wf_read_pixels(ShmScene* s, const void* d_image, size_t bytes_per_pixel, void* out) {
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(out, d_image, s->n_film_pixels * bytes_per_pixel, hipMemcpyDeviceToHost));
    return SHM_OK;
}
// Which of the small scene tables a kernel with `budget` bytes of LDS to spare stages there (wavefront.h, stage_scene_tables): greedily, in the enum's order.
LdsTables wf_lds_tables(const ShmScene* s, uint32_t budget) {
    LdsTables t = {};
    const shm_host::FlatScene& f = s->flat;
    auto pad16 = [](size_t b) { return (size_t)((b + 15u) & ~(size_t)15u); };  // (dev_upload allocates whole 16-byte groups)
    const size_t want[N_LDS_TABLES] = {
        pad16(f.mesh_flags.size() * sizeof(uint32_t)), pad16(f.lights.size() * sizeof(ShmLight)), pad16(f.light_prim_recs.size() * sizeof(shm::PrimRec)), pad16(f.materials.size() * sizeof(ShmMaterial)), pad16(f.spectrum_data.size() * sizeof(float)),
        pad16(f.rgb2spec_scale.size() * sizeof(float)),
        pad16(f.image_textures.size() * sizeof(ShmImageTexture)), pad16(f.image_levels.size() * sizeof(ShmImageLevel)), pad16(f.float_textures.size() * sizeof(ShmFloatTexture)),
        pad16(f.ftex_ranges.size() * sizeof(shm::FloatTexRange)), pad16(f.ftex_ops.size() * sizeof(shm::FloatTexOp)), pad16(f.spectrum_textures.size() * sizeof(ShmSpectrumTexture)),
        pad16(f.stex_ranges.size() * sizeof(shm::FloatTexRange)), pad16(f.stex_ops.size() * sizeof(shm::FloatTexOp)), pad16(f.ewa_lut.size() * sizeof(float))};
    size_t left = budget;
    for (int k = 0; k < N_LDS_TABLES; ++k)
        if (want[k] && want[k] <= left) { t.bytes[k] = (uint32_t)want[k]; left -= want[k]; }
    return t;
}
namespace {
int ensure_workspace(ShmScene* s, uint64_t needed_paths, bool need_staged) {
    uint64_t max_cap = workspace_cap(s, need_staged);
    uint64_t want = std::min<uint64_t>(std::max<uint64_t>(needed_paths, 4096), max_cap);
    // a large request takes the whole budget at once: freeing and re-allocating ~140 GB because the next call needs a few percent more
    // paths costs seconds (measured: 3.7 s per regrow at 500 M paths)
    need_staged = ws_staged_layout(s->plan, need_staged, s->ws_staged);
    // (what decides is whether THIS render fits: the budget below moves by a few paths from call to call — the free-memory reading, the per-path estimate — and a
    //  workspace that already holds the render must not be freed and re-allocated for it: 7 s per frame at 150 GB)
    if (s->ws_staged || !need_staged) {
        if (s->capacity >= want) return SHM_OK;
        // a render that is batched anyway (it needs more than the budget): a workspace within 10 % of the budget is the budget
        if (needed_paths > max_cap && s->capacity * 10ull >= max_cap * 9ull) return SHM_OK;
    }
    if (want > max_cap / 8) want = max_cap;
    want = (want + 4095ull) & ~4095ull;
    if (want > 0xfffff000ull) want = 0xfffff000ull;
    want = std::max<uint64_t>(want, s->capacity);
    // the bound the staged LayeredBxDF kernel relies on (its jobs carry two flag bits above the path index): max_batch_paths() stays below 2^30, and so does every grant
    if (want >= (1ull << 30)) { g_err = "internal: path workspace of 2^30 paths or more"; return SHM_ERR_INTERNAL; }
    for (void* p : s->ws_allocs) hipFree(p);
    s->ws_allocs.clear();
    s->capacity = 0;
    s->ws_staged = false;
    const uint32_t cap = (uint32_t)want;
    auto ws_alloc = [&](size_t bytes, void** out) -> int {
        void* d = nullptr;
        if (hipMalloc(&d, bytes) != hipSuccess) { g_err = "hipMalloc of the path workspace failed"; return SHM_ERR_OUT_OF_MEMORY; }
        s->ws_allocs.push_back(d);
        *out = d;
        return SHM_OK;
    };
    // the walk over the one list of per-path arrays (host/render_plan.hpp, SHM_WS_ARRAYS): what the plan does not need stays null
    const ScenePlan& p = s->plan;
    const bool staged = need_staged;
    int rc;
#define WS_ALLOC(id, field, bytes, when)                                                        \
    static_assert(sizeof(*s->field) == bytes, "SHM_WS_ARRAYS: bytes per path of " #id);         \
    s->field = nullptr;                                                                         \
    if ((when) && (rc = ws_alloc((size_t)cap * bytes, (void**)&s->field)) != SHM_OK) return rc;
    SHM_WS_ARRAYS(WS_ALLOC)
#undef WS_ALLOC
    s->pa.has_layered = p.f.has_class[CLASS_LAYERED] ? 1u : 0u;
    s->ws_staged = staged;
    s->capacity = cap;
    DBG("workspace: %u paths", cap);
    return SHM_OK;
}
// The render's hit-record form and the per-bounce halves, set on the scene's one PathArrays (which every launcher reads) for the duration of a batch and taken back when it
// is through — so that whoever reads s->pa.hit outside a render (the public trace entry points, dist.hip) finds the allocation's base and 32-byte records. The one place.
struct BatchHitState {
    ShmScene* s;
    ShmHit* const base;
    BatchHitState(ShmScene* sc, const RenderPlan& p) : s(sc), base(sc->pa.hit) {
        s->pa.hit16 = p.hit16 ? 1u : 0u;
        s->pa.hit2 = p.hit_split ? reinterpret_cast<const float4*>(base) + s->capacity : nullptr;
    }
    // all-diffuse triangle scenes with 16-byte hit records: the records are double-buffered by bounce parity in the two halves of the ShmHit allocation, so that the
    // previous vertex's record — all the next vertex's emitter MIS weight needs (k_shade.inl, k_emit_jobs) — is still there and no vertex writes anything for it
    void keep_previous(int bounce) {
        float4* const h16 = reinterpret_cast<float4*>(base);
        s->pa.hit = reinterpret_cast<ShmHit*>(h16 + (size_t)(bounce & 1) * s->capacity);
        s->pa.hit_prev = h16 + (size_t)((bounce + 1) & 1) * s->capacity;
    }
    ~BatchHitState() { s->pa.hit = base; s->pa.hit_prev = nullptr; s->pa.hit16 = 0u; s->pa.hit2 = nullptr; }
};

// ---- scene creation, in parts ----
// the device copy of the scene: the BVH by sibling pairs (host/bvh_pairs.hpp) and every flat table; s->dsv points at them
int upload_scene(ShmScene* s) {
    const shm_host::FlatScene& f = s->flat;
    SceneView v = f.view();  // scalars + host pointers; pointers replaced below
    shm_host::BvhPairs bvh;
    int rc = shm_host::bvh_pairs(f, bvh, g_err);
    if (rc != SHM_OK) return rc;
#define UP(vec, field) if ((rc = dev_upload(s, vec, &v.field)) != SHM_OK) return rc
    UP(bvh.nodes, nodes);
    if (!bvh.big_leaf_n.empty()) { const uint32_t* d = nullptr; if ((rc = dev_upload(s, bvh.big_leaf_n, &d)) != SHM_OK) return rc; s->d_big_leaf_n = const_cast<uint32_t*>(d); }
    UP(f.prim_recs, prim_recs); UP(f.primitives, primitives); UP(f.mesh_flags, mesh_flags); UP(f.vi, vi); UP(f.vn, vn); UP(f.vs, vs); UP(f.vuv, vuv);
    UP(f.spheres, spheres); UP(f.patches, patches); UP(f.patch_vi, patch_vi); UP(f.patch_vn, patch_vn); UP(f.patch_vuv, patch_vuv);
    UP(f.materials, materials); UP(f.lights, lights);
    v.light_prim_recs = nullptr;
    // (uploaded whenever the scene has a light: a spot light's record lives ONLY here — light_side_rec, shm/scene.h, has no fallback to prim_recs)
    if (!f.light_prim_recs.empty()) UP(f.light_prim_recs, light_prim_recs);
    UP(f.infinite_lights, infinite_lights); UP(f.spectrum_data, spectrum_data); UP(f.sensor_r, sensor_r_bar); UP(f.sensor_g, sensor_g_bar); UP(f.sensor_b, sensor_b_bar);
    UP(f.image_textures, image_textures); UP(f.image_levels, image_levels); UP(f.texel_data, texel_data); UP(f.rgb2spec_scale, rgb2spec_scale);
    UP(f.rgb2spec_data, rgb2spec_data); UP(f.cs_illuminant, cs_illuminant); UP(f.ewa_lut, ewa_lut);
    UP(bvh.instances, instances); UP(bvh.inst_roots, inst_roots);
    UP(f.float_textures, float_textures); UP(f.ftex_ranges, ftex_ranges); UP(f.ftex_ops, ftex_ops);
    UP(f.spectrum_textures, spectrum_textures); UP(f.stex_ranges, stex_ranges); UP(f.stex_ops, stex_ops);
    UP(f.image_lights, image_lights); UP(f.dist_data, dist_data);
#undef UP
    v.tri_shade = nullptr;  // (build_tri_shade, once the scene's plan is known)
    s->dsv = v;
    size_t w = (size_t)(f.film.pixel_bounds[2] - f.film.pixel_bounds[0]);
    size_t h = (size_t)(f.film.pixel_bounds[3] - f.film.pixel_bounds[1]);
    s->n_film_pixels = w * h;
    if ((rc = dev_alloc<ShmFilmPixel>(s, s->n_film_pixels, &s->d_film)) != SHM_OK) return rc;
    if (hipMemset(s->d_film, 0, s->n_film_pixels * sizeof(ShmFilmPixel)) != hipSuccess) { g_err = "hipMemset film"; return SHM_ERR_DEVICE; }
    if ((rc = dev_alloc<QueueState>(s, 1, &s->d_qs)) != SHM_OK) return rc;
    if ((rc = dev_alloc<DeviceCounters>(s, 1, &s->d_counters)) != SHM_OK) return rc;
    uint32_t* heads = nullptr;
    if ((rc = dev_alloc<uint32_t>(s, N_RAY * TRACE_QUEUE_PARTS * TRACE_HEAD_STRIDE, &heads)) != SHM_OK) return rc;
    for (int ray = 0; ray < N_RAY; ++ray) s->trace[ray].d_heads = heads + ray * TRACE_QUEUE_PARTS * TRACE_HEAD_STRIDE;
    hipMemset(s->d_qs, 0, sizeof(QueueState));
    hipMemset(s->d_counters, 0, sizeof(DeviceCounters));
    return SHM_OK;
}
// the flat triangles' shading records (shm/tri_shade.h), 48 bytes per primitive slot, where the plan has a kernel that reads them (ScenePlan::tri_shade)
int build_tri_shade(ShmScene* s) {
    const shm_host::FlatScene& f = s->flat;
    TriShadeRec* recs = nullptr;
    uint32_t* d_n = nullptr;
    int rc;
    if ((rc = dev_alloc<TriShadeRec>(s, f.prim_recs.size(), &recs)) != SHM_OK) return rc;
    if ((rc = dev_alloc<uint32_t>(s, 1, &d_n)) != SHM_OK) return rc;
    const uint32_t n_prims = (uint32_t)f.prim_recs.size();
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t n_built = 0;
    hipError_t err = hipMemset(d_n, 0, sizeof(uint32_t));
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_build_tri_shade, dim3((n_prims + 255u) / 256u), dim3(256), 0, 0, s->dsv, const_cast<PrimRec*>(s->dsv.prim_recs), recs, n_prims, d_n,
                           s->plan.tri_shade_plain_only ? 1u : 0u);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipDeviceSynchronize();
    if (err == hipSuccess) err = hipMemcpy(&n_built, d_n, sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (err != hipSuccess) { g_err = std::string("k_build_tri_shade: ") + hipGetErrorString(err); return SHM_ERR_DEVICE; }
    s->n_tri_shade_records = n_built;
    s->tri_shade_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    DBG("scene: %u shading records of %u primitives built in %.3f ms (%.1f MB)", n_built, n_prims, s->tri_shade_build_ms, (double)n_prims * sizeof(TriShadeRec) / 1e6);
    s->dsv.tri_shade = recs;
    return SHM_OK;
}
}  // namespace

extern "C" {

const char* shm_last_error(void) { return g_err.c_str(); }
// for the host mirror (host_mirror.cpp), which shares this thread-local message; not exported
__attribute__((visibility("hidden"))) void shm_set_last_error(const char* msg) { g_err = msg ? msg : ""; }

int shm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void shm_scene_destroy(ShmScene* s) {
    if (!s) return;
    hipSetDevice(s->device);
    wf_trace_census();  // (prints in -DK5_CENSUS development builds only)
    wf_layered_census();  // (-DLJ_CENSUS)
    wf_dist_release(s);
    for (void* p : s->allocs) hipFree(p);
    for (void* p : s->ws_allocs) hipFree(p);
    if (s->d_rw) hipFree(s->d_rw);
    if (s->d_tiles) hipFree(s->d_tiles);
    if (s->d_tile_offset) hipFree(s->d_tile_offset);
    if (s->d_pixels) hipFree(s->d_pixels);
    for (hipEvent_t e : s->events) hipEventDestroy(e);
    if (s->stream2) hipStreamDestroy(s->stream2);
    for (hipStream_t st : s->stream_cls) if (st) hipStreamDestroy(st);
    if (s->stream) hipStreamDestroy(s->stream);
    delete s;
}

int shm_scene_create(const ShmSceneDesc* desc, int device, ShmScene** out) {
    if (!out) { g_err = "out is null"; return SHM_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    ShmScene* s = new ShmScene();
    int rc = shm_host::flatten_scene(desc, s->flat, g_err);
    if (rc != SHM_OK) { delete s; return rc; }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
        g_err = "no HIP device visible (libshimmer_hip has no CPU fallback)";
        delete s;
        return SHM_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n_dev) { g_err = "device ordinal out of range"; delete s; return SHM_ERR_INVALID_ARGUMENT; }
    s->device = device;
    auto fail = [&](int code) { shm_scene_destroy(s); return code; };
    if (hipSetDevice(device) != hipSuccess) { g_err = "hipSetDevice failed"; return fail(SHM_ERR_DEVICE); }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) s->n_cu = prop.multiProcessorCount;
    if (hipStreamCreate(&s->stream) != hipSuccess) { g_err = "hipStreamCreate failed"; return fail(SHM_ERR_DEVICE); }
    if (hipStreamCreate(&s->stream2) != hipSuccess) { g_err = "hipStreamCreate failed"; return fail(SHM_ERR_DEVICE); }
    for (hipStream_t& st : s->stream_cls) if (hipStreamCreate(&st) != hipSuccess) { g_err = "hipStreamCreate failed"; return fail(SHM_ERR_DEVICE); }
    if ((rc = upload_scene(s)) != SHM_OK) return fail(rc);
    s->plan = scene_plan(scene_facts(s->flat), read_knobs());
    if (!s->flat.cs_illuminant.empty()) s->ao_illum_scale = host_illuminant_scale(s->flat.cs_illuminant.data());
    s->lds_tables = wf_lds_tables(s, LDS_TABLE_BUDGET);
    s->lds_tables_small = wf_lds_tables(s, LDS_TABLE_BUDGET_SMALL);
    if (s->plan.tri_shade && (rc = build_tri_shade(s)) != SHM_OK) return fail(rc);
    if ((rc = wf_trace_prepare(s)) != SHM_OK) return fail(rc);
    DBG("scene: %u nodes, depth %u, trace blocks %d / %d, spill levels %d / %d", (unsigned)s->flat.nodes.size(), s->flat.max_leaf_depth, s->trace[RAY_CLOSEST].blocks, s->trace[RAY_ANY].blocks,
        s->trace[RAY_CLOSEST].spill_levels, s->trace[RAY_ANY].spill_levels);
    *out = s;
    return SHM_OK;
}

int shm_scene_shading_records(ShmScene* s, uint64_t* n_records_out, double* build_ms_out) {
    if (!s || !n_records_out) return SHM_ERR_INVALID_ARGUMENT;
    *n_records_out = s->n_tri_shade_records;
    if (build_ms_out) *build_ms_out = s->tri_shade_build_ms;
    return SHM_OK;
}

// The camera lives in the scene's two views (the host's flat scene, the by-value kernel argument): both are set, nothing is uploaded. The plan is kept, so the kind stays.
int shm_scene_set_camera(ShmScene* s, const ShmCamera* camera) {
    if (!s || !camera) { g_err = "set_camera: no scene or no camera"; return SHM_ERR_INVALID_ARGUMENT; }
    if (s->dist) { g_err = "set_camera: the scene holds multi-GPU state (shm_dist_init / shm_render_sharded); shm_dist_finalize first"; return SHM_ERR_UNSUPPORTED; }
    if (camera->kind != s->flat.camera.kind) {
        g_err = "set_camera: the camera's kind (" + std::to_string(camera->kind) + ") is not the scene's (" + std::to_string(s->flat.camera.kind) + "): the scene's plan chose its generate kernel by kind";
        return SHM_ERR_INVALID_ARGUMENT;
    }
    if (camera->kind == SHM_CAMERA_SPHERICAL && camera->mapping > SHM_SPHERICAL_EQUIRECTANGULAR) { g_err = "spherical camera: unknown mapping (equal-area, equirectangular)"; return SHM_ERR_INVALID_ARGUMENT; }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));  // (every entry point blocks; this only says so)
    s->flat.camera = *camera;
    s->dsv.camera = *camera;
    return SHM_OK;
}

int shm_film_clear(ShmScene* s) {
    if (!s) return SHM_ERR_INVALID_ARGUMENT;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemsetAsync(s->d_film, 0, s->n_film_pixels * sizeof(ShmFilmPixel), s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SHM_OK;
}

int shm_film_read(ShmScene* s, ShmFilmPixel* film_out) {
    if (!s || !film_out) return SHM_ERR_INVALID_ARGUMENT;
    return wf_read_pixels(s, s->d_film, sizeof(ShmFilmPixel), film_out);
}

int shm_film_device_ptr(ShmScene* s, void** ptr_out, uint64_t* bytes_out) {
    if (!s || !ptr_out || !bytes_out) return SHM_ERR_INVALID_ARGUMENT;
    *ptr_out = s->d_film;
    *bytes_out = (uint64_t)(s->n_film_pixels * sizeof(ShmFilmPixel));
    return SHM_OK;
}

// ---- a wave call (shm_render_wave, shm_gbuffer_render_wave), in parts ----
// the tiles of a call: inside the film, disjoint; expanded into the pixel list on the device (s->d_pixels)
static int build_pixel_list(ShmScene* s, const ShmTile* tiles, uint32_t n_tiles, uint64_t* n_pixels_out) {
    const int32_t* pb = s->flat.film.pixel_bounds;
    std::vector<uint32_t> tile_offset(n_tiles);
    uint64_t n_pixels = 0;
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const ShmTile& tl = tiles[t];
        if (tl.x0 < pb[0] || tl.y0 < pb[1] || tl.x1 > pb[2] || tl.y1 > pb[3] || tl.x1 <= tl.x0 || tl.y1 <= tl.y0 || tl.x1 > 65535 || tl.y1 > 65535 ||
            tl.x0 < 0 || tl.y0 < 0) {
            g_err = "tile outside pixel bounds";
            return SHM_ERR_INVALID_ARGUMENT;
        }
        tile_offset[t] = (uint32_t)n_pixels;
        n_pixels += (uint64_t)(tl.x1 - tl.x0) * (uint64_t)(tl.y1 - tl.y0);
    }
    if (n_pixels > 0xffffffffull) { g_err = "too many pixels"; return SHM_ERR_INVALID_ARGUMENT; }
    // Tiles must be disjoint: the film update is one unsynchronised read-modify-write per pixel, as in the reference
    // (integrator.rs:277-295 relies on Tile::tile's exclusive ownership). One bit per film pixel, one masked word per tile row.
    const uint32_t fw = (uint32_t)(pb[2] - pb[0]);
    const size_t words_per_row = (fw + 63u) / 64u;
    s->tile_bitmap.assign(words_per_row * (size_t)(pb[3] - pb[1]), 0ull);
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const ShmTile& tl = tiles[t];
        const uint32_t x0 = (uint32_t)(tl.x0 - pb[0]), x1 = (uint32_t)(tl.x1 - pb[0]);
        for (int y = tl.y0; y < tl.y1; ++y) {
            uint64_t* row = s->tile_bitmap.data() + (size_t)(y - pb[1]) * words_per_row;
            for (uint32_t w0 = x0 / 64u; w0 * 64u < x1; ++w0) {
                const uint32_t lo = std::max(x0, w0 * 64u) - w0 * 64u, hi = std::min(x1, w0 * 64u + 64u) - w0 * 64u;  // bits [lo, hi)
                const uint64_t mask = (hi - lo == 64u ? ~0ull : ((1ull << (hi - lo)) - 1ull)) << lo;
                if (row[w0] & mask) { g_err = "tiles overlap (each pixel must belong to at most one tile of a call)"; return SHM_ERR_INVALID_ARGUMENT; }
                row[w0] |= mask;
            }
        }
    }
    // the tile / pixel lists are regrown on demand; the superseded buffers are released (the stream is idle between calls)
    if (s->tiles_capacity < n_tiles) {
        if (s->d_tiles) hipFree(s->d_tiles);
        if (s->d_tile_offset) hipFree(s->d_tile_offset);
        s->d_tiles = nullptr; s->d_tile_offset = nullptr; s->tiles_capacity = 0;
        if (hipMalloc((void**)&s->d_tiles, (size_t)n_tiles * sizeof(ShmTile)) != hipSuccess ||
            hipMalloc((void**)&s->d_tile_offset, (size_t)n_tiles * sizeof(uint32_t)) != hipSuccess) { g_err = "hipMalloc of the tile list failed"; return SHM_ERR_OUT_OF_MEMORY; }
        s->tiles_capacity = n_tiles;
    }
    if (s->pixels_capacity < n_pixels) {
        if (s->d_pixels) hipFree(s->d_pixels);
        s->d_pixels = nullptr; s->pixels_capacity = 0;
        if (hipMalloc((void**)&s->d_pixels, (size_t)n_pixels * sizeof(uint32_t)) != hipSuccess) { g_err = "hipMalloc of the pixel list failed"; return SHM_ERR_OUT_OF_MEMORY; }
        s->pixels_capacity = n_pixels;
    }
    HIP_TRY(hipMemcpyAsync(s->d_tiles, tiles, n_tiles * sizeof(ShmTile), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->d_tile_offset, tile_offset.data(), n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemsetAsync(s->d_counters, 0, sizeof(DeviceCounters), s->stream));
    hipLaunchKernelGGL(k_expand_tiles, dim3((n_tiles + 255) / 256), dim3(256), 0, s->stream, s->d_tiles, s->d_tile_offset, n_tiles, s->d_pixels);
    *n_pixels_out = n_pixels;
    return SHM_OK;
}
// the random walk keeps 32 B per depth per path beside the path state (up to 8 KB per path at max_depth 254): shrink the batch until the records fit in 80 % of what is free
static int ensure_randomwalk_records(ShmScene* s, int max_depth, uint32_t* cap_eff) {
    const size_t per_path = (size_t)2 * (size_t)(max_depth + 1) * sizeof(float4);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const size_t avail = (size_t)((double)(free_b + s->rw_floats4 * sizeof(float4)) * 0.8);
        while (*cap_eff > 4096u && (size_t)*cap_eff * per_path > avail) *cap_eff = (*cap_eff / 2u + 63u) & ~63u;
    }
    size_t need = (size_t)2 * (size_t)(max_depth + 1) * (size_t)*cap_eff;
    if (s->rw_floats4 < need) {
        if (s->d_rw) hipFree(s->d_rw);
        s->d_rw = nullptr;
        s->rw_floats4 = 0;
        if (hipMalloc((void**)&s->d_rw, need * sizeof(float4)) != hipSuccess) { g_err = "hipMalloc of the random-walk records failed"; return SHM_ERR_OUT_OF_MEMORY; }
        s->rw_floats4 = need;
    }
    return SHM_OK;
}
// One wave call — shm_render_wave's or shm_gbuffer_render_wave's: what its batches share. wave_begin fills it, wave_run walks the batches, add_wave_stats reads it out.
struct Render {
    ShmScene* s;
    const ShmRenderParams* params;
    RenderPlan plan;      // of the parameters the entry point plans with (the G-buffer pass: gbuffer_plan_params)
    ShadeKernels k = {};  // the film render's shading launchers (select_kernels)
    int sample_begin = 0, n_samples = 0;
    uint64_t n_pixels = 0;
    uint32_t cap_eff = 0;  // paths per batch
    EventPool ev;
    hipEvent_t e_begin = nullptr, e_end = nullptr;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_closest, ev_any, ev_shade;
    bool used_overlap = false;
    Render(ShmScene* sc, const ShmRenderParams* prm) : s(sc), params(prm), ev{sc} {}
};
// (apart from wave_begin: an entry point's own argument checks stand between the two, and the order in which a call's errors are reported is part of the interface)
static bool wave_args_ok(const ShmScene* s, const ShmRenderParams* params, const ShmTile* tiles, uint32_t n_tiles, int32_t sample_begin, int32_t sample_end) {
    if (s && params && tiles && n_tiles != 0 && sample_end > sample_begin) return true;
    g_err = "invalid render arguments";
    return false;
}
// The head of a wave call, behind the entry point's own argument checks: the sampler's checks, the pixel list, the per-render state on the scene, the plan of
// `plan_params` and the workspace it asks for, of at most `max_batch` paths per batch
static int wave_begin(Render& r, const ShmRenderParams& plan_params, const ShmTile* tiles, uint32_t n_tiles, int32_t sample_begin, int32_t sample_end, uint64_t max_batch) {
    ShmScene* s = r.s;
    const ShmRenderParams* params = r.params;
    if (params->sampler > SHM_SAMPLER_ZSOBOL || params->sampler_randomization > SHM_SAMPLER_RANDOMIZE_NONE) { g_err = "unknown sampler or sampler randomization"; return SHM_ERR_INVALID_ARGUMENT; }
    // ZSobol: the per-render constants of the stream (shm/sampling.h); its sample indices are the low log2spp bits of the Morton index
    const uint32_t zsobol = zsobol_config(params->samples_per_pixel, s->flat.film.full_resolution[0], s->flat.film.full_resolution[1],
                                          params->sampler_randomization == SHM_SAMPLER_RANDOMIZE_NONE);
    if (params->sampler == SHM_SAMPLER_ZSOBOL && (sample_begin < 0 || (int64_t)sample_end > (int64_t)1 << zsobol_log2spp(zsobol))) {
        g_err = "zsobol: sample index outside [0, 2^ceil(log2(samples_per_pixel)))";
        return SHM_ERR_INVALID_ARGUMENT;
    }
    HIP_TRY(hipSetDevice(s->device));
    int rc;
    if ((rc = build_pixel_list(s, tiles, n_tiles, &r.n_pixels)) != SHM_OK) return rc;
    s->dsv.quirks_off = params->disable_reference_quirks ? 1u : 0u;  // SHM_REFERENCE_QUIRKS: every kernel of this wave takes s->dsv by value
    s->dsv.zsobol = zsobol;  // (read only by the ZSobol kernels: sampler_word)
    r.plan = render_plan(s->plan, plan_params);
    r.sample_begin = sample_begin;
    r.n_samples = sample_end - sample_begin;
    const uint64_t n_paths = r.n_pixels * (uint64_t)r.n_samples;
    if ((rc = ensure_workspace(s, std::min(n_paths, max_batch), r.plan.route == ROUTE_STAGED)) != SHM_OK) return rc;
    r.cap_eff = (uint32_t)std::min<uint64_t>(s->capacity, max_batch);
    return SHM_OK;
}
// The batches of a wave call, `batch(pixels, n_pix)` each, between the call's two events; blocks until the stream is through
static int wave_run(Render& r, const std::function<int(const uint32_t*, uint32_t)>& batch) {
    ShmScene* s = r.s;
    uint32_t pix_per_batch = r.cap_eff / (uint32_t)r.n_samples;
    if (pix_per_batch == 0) { g_err = "spp-wave larger than the path workspace"; return SHM_ERR_INVALID_ARGUMENT; }
    if (pix_per_batch > 64) pix_per_batch &= ~63u;  // whole 8x8 tiles per wavefront
    r.e_begin = r.ev.get();
    r.e_end = r.ev.get();
    HIP_TRY(hipEventRecord(r.e_begin, s->stream));
    int rc;
    for (uint64_t p0 = 0; p0 < r.n_pixels; p0 += pix_per_batch) {
        if ((rc = batch(s->d_pixels + p0, (uint32_t)std::min<uint64_t>(pix_per_batch, r.n_pixels - p0))) != SHM_OK) return rc;
        if (r.ev.failed) { g_err = "hipEventCreate failed"; return SHM_ERR_DEVICE; }
    }
    HIP_TRY(hipEventRecord(r.e_end, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipGetLastError());
    return SHM_OK;
}
// One path vertex for every entry of q_active[cur]: the route's kernel, or — a staged bounce — the hit half, then one scattering kernel per BxDF class the scene holds,
// each over its own material-sorted queue
static int shade_vertex(Render& r, const ShadeArgs& sa, int bounce, bool overlap) {
    ShmScene* s = r.s;
    const RenderPlan& p = r.plan;
    const ShadeKernels& k = r.k;
    if (p.route == ROUTE_RANDOM_WALK) return k.randomwalk(s, sa);
    if (p.route == ROUTE_AO) return wf_launch_shade_ao(s, sa, p.zs);  // (outside the table: one build for every scene class, k_ao.hip)
    if (p.route == ROUTE_SIMPLE) return k.simple(s, sa);
    if (p.route == ROUTE_LEAN) return k.lean(s, sa);
    if (!p.staged_bounce(bounce)) return k.fused_all(s, sa);
    ShadeArgs va = sa;  // (k_vertex's arguments: its queue is q_split behind the split pass)
    if (p.split) {  // plain-diffuse hits -> q_lean (their whole vertex in the lean fused kernel, below), the rest -> q_split for k_vertex
        hipLaunchKernelGGL(k_split_plain, dim3(s->n_cu * 8), dim3(SHADE2_BLOCK), 0, s->stream, s->dsv, s->pa, s->d_q_active[sa.cur], s->d_q_lean, s->d_q_split, s->d_qs, sa.cur);
        LAUNCH_TRY("k_split_plain");
        va.q_in = s->d_q_split;
        va.n_in = &s->d_qs->n_split;
    }
    if (p.divert_vertex) va.q_divert = s->d_q_lean;  // (the textured k_vertex diverts nothing: in a textured scene the split pass fills q_lean)
    int rc = k.vertex(s, va);
    // The classes' scatter kernels — the diverted hits' lean kernel is the first member of the group — are independent of each other (own queue each, disjoint paths,
    // wave-aggregated atomics on the shared next / shadow queues): the first runs on the render stream, the others beside it on their own streams, and the render
    // stream waits for them — for small batches only (the same threshold as the K3 / K2 overlap), where the launches are
    // tail-dominated: textured Cornell 512^2 x 64 1 376 -> 1 486 Mray/s. With large queues each kernel fills the device by itself and
    // sharing it costs (coated S3 at 256 spp 1 944 -> 1 864), and C4's late bounces did not gain (2 044 either way).
    // ... and at any batch size where the diverted fused kernel (latency-bound, three waves per SIMD) has the LayeredBxDF class's scatter kernel
    // (issue-bound, two) to run beside: complementary bounds (RenderPlan::group_big; coated S3 at 256 spp: see DESIGN.md section 6)
    int n_cls = p.drain_lean ? 1 : 0;
    for (int c = 0; c < N_BXDF_CLASSES; ++c) n_cls += s->plan.f.has_class[c] ? 1 : 0;
    hipEvent_t vertex_done = nullptr;
    if ((overlap || p.group_big) && n_cls > 1) { vertex_done = r.ev.get(); hipEventRecord(vertex_done, s->stream); }  // (before the first class's launch)
    std::vector<hipEvent_t> side_done;
    int k_cls = 0;
    auto scatter_on = [&](bool runs, ShadeFn launch) {
        if (rc != SHM_OK || !runs) return;
        ShadeArgs sc = sa;
        const bool side = k_cls > 0 && vertex_done != nullptr;
        if (side) {
            sc.stream = s->stream_cls[k_cls - 1];
            hipStreamWaitEvent(sc.stream, vertex_done, 0);
        }
        rc = launch(s, sc);
        if (side && rc == SHM_OK) {
            hipEvent_t done = r.ev.get();
            hipEventRecord(done, sc.stream);
            side_done.push_back(done);
        }
        ++k_cls;
    };
    scatter_on(p.drain_lean, k.lean_diverted);
    for (int c = 0; c < N_BXDF_CLASSES; ++c) scatter_on(s->plan.f.has_class[c], k.scatter[c]);
    for (hipEvent_t e : side_done) hipStreamWaitEvent(s->stream, e, 0);
    return rc;
}
// One batch of paths — n_pix pixels x n_samples — from camera rays to the film: the bounce loop
static int render_batch(Render& r, const uint32_t* pixels, uint32_t n_pix) {
    ShmScene* s = r.s;
    const RenderPlan& p = r.plan;
    const ShmRenderParams* params = r.params;
    EventPool& ev = r.ev;
    int rc;
    const uint32_t total = n_pix * (uint32_t)r.n_samples;
    BatchHitState hits{s, p};
    const GenerateArgs ga{s->stream, pixels, n_pix, r.sample_begin, r.n_samples, *params, p.img_generate == IMG_TEX, p.lean_first, p.zs, p.flt};
    if ((rc = (p.spherical ? wf_generate<true> : wf_generate<false>)(s, ga)) != SHM_OK) return rc;
    int cur = 0;
    // K3 of bounce b on a second stream beside K2 of bounce b+1 — they are independent: K3 reads the shadow buffers and adds into L, K2 reads the extension rays and
    // writes hit records — and the next shade launch waits for both: where the plan's overlap policy says so (small batches; late bounces)
    bool overlap = p.overlap_batch(total);
    hipStream_t any_stream = overlap ? s->stream2 : s->stream;
    r.used_overlap = r.used_overlap || overlap;
    hipEvent_t k3_done = nullptr;
    const int shade_blocks = s->n_cu * 4;  // (the fused / vertex / scatter launchers scale this by their own waves per SIMD)
    // The ambient occlusion integrator is this loop run once, whatever max_depth says: its shade kernel queues the occlusion rays and the any-hit launch behind it adds
    // the unoccluded contributions into L — at bounce 0, where a path render of max_depth 0 traces no shadow ray
    const bool ao = p.route == ROUTE_AO;
    const int last_bounce = ao ? 0 : params->max_depth;
    for (int bounce = 0; bounce <= last_bounce; ++bounce) {
        if (p.hit_kept) hits.keep_previous(bounce);
        const int sh = bounce & 1;
        if (!overlap && bounce >= p.late_overlap_bounce) {
            // (the switch is safe at a bounce boundary: everything so far was ordered on the render stream)
            overlap = true;
            any_stream = s->stream2;
            r.used_overlap = true;
        }
        hipEvent_t a = ev.get(), b = ev.get();
        hipEventRecord(a, s->stream);
        const bool first_lean = p.lean_first && bounce == 0;  // (the identity queue was not written: K2 takes slot = queue index, k_shade knows the constants)
        TraceArgs closest{.stream = s->stream, .rays = s->pa.ray, .hits = s->pa.hit, .hit16 = (int)s->pa.hit16, .hit2 = const_cast<float4*>(s->pa.hit2)};
        if (first_lean) closest.n_direct = total;
        else { closest.queue = s->d_q_active[cur]; closest.n_ptr = &s->d_qs->n_active[cur]; }
        if ((rc = wf_launch_trace(s, RAY_CLOSEST, false, closest)) != SHM_OK) return rc;
        hipEventRecord(b, s->stream);
        r.ev_closest.push_back({a, b});
        if (overlap && k3_done) hipStreamWaitEvent(s->stream, k3_done, 0);  // shade(b) touches L and refills the shadow buffers
        {
            hipEvent_t s0 = ev.get(), s1 = ev.get();
            hipEventRecord(s0, s->stream);
            const ShadeArgs sa{s->stream, cur, *params, sh, shade_blocks, first_lean ? 1 : 0, p.hit_kept ? 1 : 0, r.cap_eff};
            if ((rc = shade_vertex(r, sa, bounce, overlap)) != SHM_OK) return rc;
            hipEventRecord(s1, s->stream);
            r.ev_shade.push_back({s0, s1});
        }
        if ((bounce < params->max_depth || ao) && p.route != ROUTE_RANDOM_WALK) {
            hipEvent_t c = ev.get(), d = ev.get();
            if (overlap) {
                hipEvent_t shaded = ev.get();
                hipEventRecord(shaded, s->stream);
                hipStreamWaitEvent(any_stream, shaded, 0);
            }
            hipEventRecord(c, any_stream);
            const TraceArgs shadow{.stream = any_stream, .queue = s->d_q_shadow, .n_ptr = &s->d_qs->n_shadow[sh], .rays = s->pa.shadow_ray, .L = s->pa.L,
                                   .contrib = s->pa.shadow_contrib};
            if ((rc = wf_launch_trace(s, RAY_ANY, p.trace_any_strict, shadow)) != SHM_OK) return rc;
            hipEventRecord(d, any_stream);
            r.ev_any.push_back({c, d});
            k3_done = d;
        }
        if (dbg_on()) {  // queue sizes per bounce (costs a sync: debug only)
            QueueState q;
            hipStreamSynchronize(s->stream);
            hipStreamSynchronize(any_stream);
            hipMemcpy(&q, s->d_qs, sizeof(q), hipMemcpyDeviceToHost);
            DBG("bounce %d: traced %u, next %u, shadow %u, emitter hits deferred %u, diverted %u", bounce, q.n_active[cur], q.n_active[cur ^ 1], q.n_shadow[sh], q.n_emit, q.n_lean);
        }
        hipLaunchKernelGGL(k_next_bounce, dim3(1), dim3(1), 0, s->stream, s->d_qs, cur, sh ^ 1);
        cur ^= 1;
    }
    if (overlap && k3_done) hipStreamWaitEvent(s->stream, k3_done, 0);  // the film reads L
    if (p.route == ROUTE_RANDOM_WALK)
        if ((rc = wf_launch_fold_randomwalk(s, s->stream, r.cap_eff, total)) != SHM_OK) return rc;
    return launch_film(s, p, pixels, n_pix, r.n_samples);  // (EventPool::failed: wave_run looks after every batch)
}
// A finished wave call's counters and times, added to `stats`. The two kinds of wave differ in two places, both here:
//   paths     the film render's K6 counts them on the device (DeviceCounters::paths); the G-buffer pass runs no K6, so its wave counts them on the host (`film` = false);
//   ms_shade  everything that is not traversal. Only a film render overlaps K3 with K2 (Render::used_overlap) and then sums its shade launches; the G-buffer pass never
//             does, and takes the rest of the wall time: K1 and its own two kernels.
static int add_wave_stats(Render& r, bool film, ShmStats* stats) {
    DeviceCounters c;
    HIP_TRY(hipMemcpy(&c, r.s->d_counters, sizeof(c), hipMemcpyDeviceToHost));
    stats->paths += film ? c.paths : r.n_pixels * (uint64_t)r.n_samples;
    stats->rays_closest += c.rays_closest;
    stats->rays_any += c.rays_any;
    stats->nodes_closest += c.nodes_closest;
    stats->tris_closest += c.tris_closest;
    stats->nodes_any += c.nodes_any;
    stats->tris_any += c.tris_any;
    float ms = 0.0f, tot = 0.0f;
    hipEventElapsedTime(&tot, r.e_begin, r.e_end);
    stats->ms_total += tot;
    double mc = 0.0, ma = 0.0, msh = 0.0;
    for (auto& p : r.ev_closest) { hipEventElapsedTime(&ms, p.first, p.second); mc += ms; DBG("closest launch %.3f ms", ms); }
    for (auto& p : r.ev_any) { hipEventElapsedTime(&ms, p.first, p.second); ma += ms; DBG("any launch %.3f ms", ms); }
    for (auto& p : r.ev_shade) { hipEventElapsedTime(&ms, p.first, p.second); msh += ms; DBG("shade launch %.3f ms", ms); }
    stats->ms_trace_closest += mc;
    stats->ms_trace_any += ma;
    // Without overlap the rest is the wall time less the traversal; with K3 running beside K2 the kernels' own durations add up to more than the wall time, so the
    // shade launches are summed instead.
    stats->ms_shade += r.used_overlap ? msh : (double)tot - mc - ma;
    stats->launches_closest += (uint32_t)r.ev_closest.size();
    stats->launches_any += (uint32_t)r.ev_any.size();
    return SHM_OK;
}
// How many samples per pixel one wave call over `tiles` may take: as many as fit the path workspace in one batch, at least 64
static int fuse_width(const ShmScene* s, const ShmRenderParams& plan_params, const ShmTile* tiles, uint32_t n_tiles) {
    uint64_t n_pixels = 0;
    for (uint32_t t = 0; tiles && t < n_tiles; ++t)
        n_pixels += (uint64_t)std::max(0, tiles[t].x1 - tiles[t].x0) * (uint64_t)std::max(0, tiles[t].y1 - tiles[t].y0);
    const bool staged = render_plan(s->plan, plan_params).route == ROUTE_STAGED;
    return (int)std::min<uint64_t>(std::max<uint64_t>(64, n_pixels ? workspace_cap(s, staged) / n_pixels : 64), 1u << 20);
}
// The G-buffer pass's camera rays are the path integrator's, whatever integrator the parameters name: its plan gives K1's coordinates, the filter weight's source and
// the workspace a render of this scene would ask for — so that a render before or after the pass finds the workspace it left
static ShmRenderParams gbuffer_plan_params(const ShmRenderParams& params) {
    ShmRenderParams as_path = params;
    as_path.integrator = SHM_INTEGRATOR_PATH;
    as_path.force_diffuse = 0;
    return as_path;
}

int shm_render_wave(ShmScene* s, const ShmRenderParams* params, const ShmTile* tiles, uint32_t n_tiles, int32_t sample_begin,
                    int32_t sample_end, ShmStats* stats) {
    if (!wave_args_ok(s, params, tiles, n_tiles, sample_begin, sample_end)) return SHM_ERR_INVALID_ARGUMENT;
    if (params->max_depth < 0 || params->max_depth > 254) { g_err = "max_depth out of range"; return SHM_ERR_INVALID_ARGUMENT; }
    if (params->integrator > SHM_INTEGRATOR_AMBIENT_OCCLUSION) { g_err = "unknown integrator"; return SHM_ERR_UNSUPPORTED; }
    if (params->integrator == SHM_INTEGRATOR_AMBIENT_OCCLUSION) {  // (its two parameters are read by no other integrator, and checked for no other)
        if (const char* e = shm_host::ao_params_error(*params, s->flat)) { g_err = e; return SHM_ERR_INVALID_ARGUMENT; }
    }
    // (the random walk's batches are capped at 16 Mi paths: 32 B per depth per path beside the path state)
    const bool random_walk = params->integrator == SHM_INTEGRATOR_RANDOM_WALK;
    Render r(s, params);
    int rc;
    if ((rc = wave_begin(r, *params, tiles, n_tiles, sample_begin, sample_end, random_walk ? 1ull << 24 : ~0ull)) != SHM_OK) return rc;
    if (random_walk && (rc = ensure_randomwalk_records(s, params->max_depth, &r.cap_eff)) != SHM_OK) return rc;
    r.k = select_kernels(r.plan);
    if (const char* e = render_plan_error(s->plan, r.plan)) { g_err = e; return SHM_ERR_INTERNAL; }
    if (!kernels_complete(r.k, s->plan, r.plan)) { g_err = "internal: the render plan calls a kernel its table cell does not hold"; return SHM_ERR_INTERNAL; }
    rc = wave_run(r, [&](const uint32_t* pixels, uint32_t n_pix) { return render_batch(r, pixels, n_pix); });
    return rc == SHM_OK && stats ? add_wave_stats(r, true, stats) : rc;
}

int shm_render_device(ShmScene* s, const ShmRenderParams* params, const ShmTile* tiles, uint32_t n_tiles, ShmStats* stats) {
    if (!s || !params) { g_err = "invalid render arguments"; return SHM_ERR_INVALID_ARGUMENT; }
    // ImageTileIntegrator::render's wave schedule (integrator.rs:231-233, 306-308: 1,1,2,4,...,64,64,...). The waves only
    // exist there to show progress / write intermediate images (TODO at :311); a pixel's samples are added to the film in
    // increasing sample_index whatever the grouping, so consecutive waves are fused into launches of at least 64 spp (the
    // reference's own maximum wave size) and as many more as fit the path workspace in one batch (a rank that owns 1/8 of
    // the tiles takes all 256 spp at once), without changing a single film sum (shm_render_wave is the one-launch-per-wave entry: tests/test_gpu_parity.py holds the two against each other).
    int spp = params->samples_per_pixel;
    HIP_TRY(hipSetDevice(s->device));
    const int max_fuse = fuse_width(s, *params, tiles, n_tiles);
    int wave_start = 0, wave_end = 1, next_wave_size = 1;
    int pend_begin = 0, pend_end = 0;
    while (wave_start < spp) {
        if (pend_end == pend_begin) pend_begin = wave_start;
        pend_end = wave_end;
        int nws = wave_end;  // advance the reference's schedule
        wave_start = wave_end;
        wave_end = std::min(spp, nws + next_wave_size);
        next_wave_size = std::min(2 * next_wave_size, 64);
        if (wave_start >= spp || (wave_end - pend_begin) > max_fuse) {
            int rc = shm_render_wave(s, params, tiles, n_tiles, pend_begin, pend_end, stats);
            if (rc != SHM_OK) return rc;
            pend_begin = pend_end;
        }
    }
    return SHM_OK;
}

int shm_render(ShmScene* s, const ShmRenderParams* params, const ShmTile* tiles, uint32_t n_tiles, ShmFilmPixel* film, ShmStats* stats) {
    if (!s || !params || !film) { g_err = "invalid render arguments"; return SHM_ERR_INVALID_ARGUMENT; }
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc = shm_film_clear(s);
    if (rc != SHM_OK) return rc;
    rc = shm_render_device(s, params, tiles, n_tiles, stats);
    if (rc != SHM_OK) return rc;
    std::vector<ShmFilmPixel> tmp(s->n_film_pixels);
    rc = shm_film_read(s, tmp.data());
    if (rc != SHM_OK) return rc;
    for (size_t i = 0; i < tmp.size(); ++i) {
        film[i].rgb_sum[0] += tmp[i].rgb_sum[0];
        film[i].rgb_sum[1] += tmp[i].rgb_sum[1];
        film[i].rgb_sum[2] += tmp[i].rgb_sum[2];
        film[i].weight_sum += tmp[i].weight_sum;
    }
    return SHM_OK;
}

// ---- the G-buffer pass: a wave call (wave_begin / wave_run, above) whose batch is K1 as a render's, the scene's own closest-hit launch, then
//      k_gbuffer.hip's two kernels ----
// the device G-buffer, pixel_bounds-sized and zeroed: made by the first call that needs it (shm_scene_destroy frees it with the scene's other allocations)
static int ensure_gbuffer(ShmScene* s) {
    if (s->d_gbuffer) return SHM_OK;
    int rc;
    if ((rc = dev_alloc<ShmGBufferPixel>(s, s->n_film_pixels, &s->d_gbuffer)) != SHM_OK) return rc;
    if (hipMemset(s->d_gbuffer, 0, s->n_film_pixels * sizeof(ShmGBufferPixel)) != hipSuccess) { s->d_gbuffer = nullptr; g_err = "hipMemset of the G-buffer"; return SHM_ERR_DEVICE; }
    return SHM_OK;
}

int shm_gbuffer_clear(ShmScene* s) {
    if (!s) return SHM_ERR_INVALID_ARGUMENT;
    HIP_TRY(hipSetDevice(s->device));
    int rc;
    if ((rc = ensure_gbuffer(s)) != SHM_OK) return rc;
    HIP_TRY(hipMemsetAsync(s->d_gbuffer, 0, s->n_film_pixels * sizeof(ShmGBufferPixel), s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->gbuffer_filled = false;
    return SHM_OK;
}

int shm_gbuffer_read(ShmScene* s, ShmGBufferPixel* out) {
    if (!s || !out) return SHM_ERR_INVALID_ARGUMENT;
    HIP_TRY(hipSetDevice(s->device));
    int rc;
    if ((rc = ensure_gbuffer(s)) != SHM_OK) return rc;
    return wf_read_pixels(s, s->d_gbuffer, sizeof(ShmGBufferPixel), out);
}

int shm_gbuffer_render_wave(ShmScene* s, const ShmRenderParams* params, uint32_t space, const ShmTile* tiles, uint32_t n_tiles, int32_t sample_begin, int32_t sample_end,
                            ShmStats* stats) {
    if (!wave_args_ok(s, params, tiles, n_tiles, sample_begin, sample_end)) return SHM_ERR_INVALID_ARGUMENT;
    if (space > SHM_GBUFFER_SPACE_CAMERA) { g_err = "unknown G-buffer space"; return SHM_ERR_INVALID_ARGUMENT; }
    Render r(s, params);
    int rc;
    if ((rc = wave_begin(r, gbuffer_plan_params(*params), tiles, n_tiles, sample_begin, sample_end, ~0ull)) != SHM_OK) return rc;
    if ((rc = ensure_gbuffer(s)) != SHM_OK) return rc;
    const RenderPlan& p = r.plan;
    const bool tex = p.img_generate == IMG_TEX;
    rc = wave_run(r, [&](const uint32_t* pixels, uint32_t n_pix) {
        int rc;
        const GenerateArgs ga{s->stream, pixels, n_pix, r.sample_begin, r.n_samples, *params, tex, false, p.zs, p.flt};
        if ((rc = (p.spherical ? wf_generate<true> : wf_generate<false>)(s, ga)) != SHM_OK) return rc;
        hipEvent_t a = r.ev.get(), b = r.ev.get();
        hipEventRecord(a, s->stream);
        // (K1 left the identity queue: the batch's slots in order, 32-byte hit records)
        const TraceArgs closest{.stream = s->stream, .n_direct = n_pix * (uint32_t)r.n_samples, .rays = s->pa.ray, .hits = s->pa.hit};
        if ((rc = wf_launch_trace(s, RAY_CLOSEST, false, closest)) != SHM_OK) return rc;
        hipEventRecord(b, s->stream);
        r.ev_closest.push_back({a, b});
        const GBufferArgs gb{s->stream, pixels, n_pix, r.n_samples, *params, tex, space, film_weight(p.flt)};
        return wf_launch_gbuffer(s, gb);
    });
    if (rc != SHM_OK) return rc;
    s->gbuffer_filled = true;
    s->gbuffer_space = space;
    return stats ? add_wave_stats(r, false, stats) : SHM_OK;
}

int shm_render_gbuffer(ShmScene* s, const ShmRenderParams* params, uint32_t space, const ShmTile* tiles, uint32_t n_tiles, ShmGBufferPixel* out, ShmStats* stats) {
    if (!s || !params || !out || params->samples_per_pixel < 1) { g_err = "invalid render arguments"; return SHM_ERR_INVALID_ARGUMENT; }
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc = shm_gbuffer_clear(s);
    if (rc != SHM_OK) return rc;
    // every sample of a pixel in one launch where the workspace holds them, in waves of 64 otherwise: the sums do not depend on the split
    const int spp = params->samples_per_pixel;
    const int wave = fuse_width(s, gbuffer_plan_params(*params), tiles, n_tiles);
    for (int begin = 0; begin < spp; begin += wave)
        if ((rc = shm_gbuffer_render_wave(s, params, space, tiles, n_tiles, begin, std::min(spp, begin + wave), stats)) != SHM_OK) return rc;
    return shm_gbuffer_read(s, out);
}

static int trace_device_impl(ShmScene* s, bool any, const void* rays_dev, uint32_t n, void* out_dev, int repeat, ShmStats* stats) {
    if (!s || !rays_dev || !out_dev || n == 0 || repeat < 1) { g_err = "invalid trace arguments"; return SHM_ERR_INVALID_ARGUMENT; }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemsetAsync(s->d_counters, 0, sizeof(DeviceCounters), s->stream));
    EventPool ev{s};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> evs;
    for (int r = 0; r < repeat; ++r) {
        hipEvent_t a = ev.get(), b = ev.get();
        hipEventRecord(a, s->stream);
        // (not strict: the reference-exact any-hit kernels, whatever the scene's last render used; 32-byte hit records)
        TraceArgs t{.stream = s->stream, .n_direct = n, .rays = (const ShmRay*)rays_dev};
        if (any) t.occluded = (uint8_t*)out_dev;
        else t.hits = (ShmHit*)out_dev;
        const int rc = wf_launch_trace(s, any ? RAY_ANY : RAY_CLOSEST, false, t);
        if (rc != SHM_OK) return rc;
        hipEventRecord(b, s->stream);
        evs.push_back({a, b});
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipGetLastError());
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        DeviceCounters c;
        HIP_TRY(hipMemcpy(&c, s->d_counters, sizeof(c), hipMemcpyDeviceToHost));
        stats->rays_closest = c.rays_closest; stats->rays_any = c.rays_any;
        stats->nodes_closest = c.nodes_closest; stats->tris_closest = c.tris_closest;
        stats->nodes_any = c.nodes_any; stats->tris_any = c.tris_any;
        double tot = 0.0;
        for (auto& p : evs) { float ms = 0.0f; hipEventElapsedTime(&ms, p.first, p.second); tot += ms; }
        if (any) { stats->ms_trace_any = tot; stats->launches_any = (uint32_t)repeat; }
        else { stats->ms_trace_closest = tot; stats->launches_closest = (uint32_t)repeat; }
        stats->ms_total = tot;
    }
    return SHM_OK;
}

int shm_integrator_render(const char* name, const ShmSceneDesc* scene, int device, int32_t max_depth, int regularize,
                          int sample_lights, int sample_bsdf, int32_t samples_per_pixel, int32_t seed, int disable_pixel_jitter,
                          int disable_wavelength_jitter, ShmFilmPixel* film_out, ShmStats* stats_out, int32_t* n_waves_out) {
    if (!name || !scene || !film_out) { g_err = "invalid integrator arguments"; return SHM_ERR_INVALID_ARGUMENT; }
    try {
        shimmer::PathIntegratorParameters p;
        p.max_depth = max_depth;
        p.regularize = regularize != 0;
        p.sample_lights = sample_lights != 0;
        p.sample_bsdf = sample_bsdf != 0;
        p.samples_per_pixel = samples_per_pixel;
        std::unique_ptr<shimmer::Integrator> integrator = shimmer::create_integrator(name, p, *scene, device);
        shimmer::Options options;
        options.seed = seed;
        options.disable_pixel_jitter = disable_pixel_jitter != 0;
        options.disable_wavelength_jitter = disable_wavelength_jitter != 0;
        integrator->render(options);
        auto* w = static_cast<shimmer::WavefrontPathIntegrator*>(integrator.get());
        std::copy(w->film().begin(), w->film().end(), film_out);
        if (stats_out) *stats_out = w->stats();
        if (n_waves_out) *n_waves_out = w->waves();
        return SHM_OK;
    } catch (const shimmer::IntegratorError& e) {
        g_err = e.what();
        return SHM_ERR_UNSUPPORTED;
    } catch (const std::exception& e) {  // nothing unwinds across the ABI
        g_err = e.what();
        return SHM_ERR_INTERNAL;
    }
}

int shm_trace_closest_device(ShmScene* s, const void* rays_dev, uint32_t n, void* hits_dev, int repeat, ShmStats* stats) {
    return trace_device_impl(s, false, rays_dev, n, hits_dev, repeat, stats);
}
int shm_trace_any_device(ShmScene* s, const void* rays_dev, uint32_t n, void* occluded_dev, int repeat, ShmStats* stats) {
    return trace_device_impl(s, true, rays_dev, n, occluded_dev, repeat, stats);
}

static int trace_host_impl(ShmScene* s, bool any, const ShmRay* rays, uint32_t n, void* out, ShmStats* stats) {
    if (!s || !rays || !out || n == 0) { g_err = "invalid trace arguments"; return SHM_ERR_INVALID_ARGUMENT; }
    HIP_TRY(hipSetDevice(s->device));
    void *d_rays = nullptr, *d_out = nullptr;
    size_t out_bytes = any ? (size_t)n : (size_t)n * sizeof(ShmHit);
    HIP_TRY(hipMalloc(&d_rays, (size_t)n * sizeof(ShmRay)));
    if (hipMalloc(&d_out, out_bytes) != hipSuccess) { hipFree(d_rays); g_err = "hipMalloc"; return SHM_ERR_OUT_OF_MEMORY; }
    int rc = SHM_OK;
    if (hipMemcpy(d_rays, rays, (size_t)n * sizeof(ShmRay), hipMemcpyHostToDevice) != hipSuccess) { g_err = "hipMemcpy rays"; rc = SHM_ERR_DEVICE; }
    if (rc == SHM_OK) rc = trace_device_impl(s, any, d_rays, n, d_out, 1, stats);
    if (rc == SHM_OK && hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess) { g_err = "hipMemcpy out"; rc = SHM_ERR_DEVICE; }
    hipFree(d_rays);
    hipFree(d_out);
    return rc;
}
int shm_trace_closest(ShmScene* s, const ShmRay* rays, uint32_t n, ShmHit* hits_out, ShmStats* stats) { return trace_host_impl(s, false, rays, n, hits_out, stats); }
int shm_trace_any(ShmScene* s, const ShmRay* rays, uint32_t n, uint8_t* occluded_out, ShmStats* stats) { return trace_host_impl(s, true, rays, n, occluded_out, stats); }

}  // extern "C"