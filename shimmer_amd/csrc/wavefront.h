// wavefront.h — shared declarations of the gfx950 wavefront path tracer behind include/shimmer_hip.h: path state (SoA in HBM), queue
// bookkeeping, the scene object, and the launchers each kernel translation unit exports. WHICH of them a scene and a render run is decided in
// host/render_plan.hpp (ScenePlan at scene creation, RenderPlan per render: pure C++, tested on the CPU); render.hip looks the launchers up and calls them. The kernels are split over several .hip files
// (k_trace.hip, k_generate_spherical.hip, k_shade_*.hip, render.hip) so that they compile in parallel; nothing here is exported from the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

// K_QUADRICS (a translation unit's switch; it follows K_DELTA_LIGHTS, below, unless the unit sets it): PBRT-v4's disk and cylinder (shm/shapes.h, SHM_QUADRICS:
// ShmSphere::quadric) are compiled into a unit's sphere code only where it is true — the *_dl builds, which RenderPlan::dl names for a scene that holds one
// (FlatScene::has_quadric_kinds), and k_trace_quadrics.hip: k_trace.hip's general traversal kernels a second time (k_trace.inl), which wf_launch_trace takes for such a
// scene. Every other unit's sphere code is that of a build without the shapes. (Up here: host/flatten.h brings shm/shapes.h in.)
#ifndef K_DELTA_LIGHTS
#define K_DELTA_LIGHTS false
#endif
#ifndef K_QUADRICS
#define K_QUADRICS K_DELTA_LIGHTS
#endif
#define SHM_QUADRICS K_QUADRICS
// K_ALPHA (a translation unit's switch; only k_trace_alpha.hip sets it): PBRT-v4's shape alpha (shm/alpha.h) in the traversal body (k_trace.inl) — an alpha-tested triangle
// parks, and the parked round runs the alpha test behind its three shape tests. Without it both fold away: the traversal kernels of every scene without a cutout
// (FlatScene::has_alpha) are those of a build without the feature.
#ifndef K_ALPHA
#define K_ALPHA false
#endif
#include "host/flatten.h"
#include "shm/bvh_link.h"
#include "host/bvh_pairs.hpp"
#include "host/render_plan.hpp"
#include "host/illuminant_scale.hpp"
// K_DELTA_LIGHTS (a translation unit's switch, like K_ZSOBOL below): PBRT-v4's distant and spot lights are compiled into a unit's light sampling only where it is true
// (shm/path.h, SHM_DELTA_LIGHTS). The Makefile compiles every unit that samples lights once more with it into *_dl (and *_zs_dl) objects, whose kernels carry a _dl
// suffix and whose launchers are the <., DL = true> specializations of wf_shade (below); the render's plan (host/render_plan.hpp, RenderPlan::dl) names that set for a scene that holds such a light
// (FlatScene::has_directed_lights). Without the switch the two branches fold away: the kernels of every other scene are those of a build without the lights.
#ifndef K_DELTA_LIGHTS
#define K_DELTA_LIGHTS false
#endif
#define SHM_DELTA_LIGHTS K_DELTA_LIGHTS
// The same switch is "the extended kernels": PBRT-v4's diffuse transmission material (shm/bxdf.h, SHM_DIFFUSE_TRANSMISSION) is compiled only into the *_dl / *_zs_dl builds —
// which k_vertex_*.hip gets for it too (get_bsdf and the class of kind 8; it draws nothing, so no *_zs_dl) — and RenderPlan::dl names that set for a scene that holds the
// material (FlatScene::has_diffuse_transmission), as it does for one that holds a distant or spot light.
#define SHM_DIFFUSE_TRANSMISSION K_DELTA_LIGHTS
// K_SPHERICAL_CAMERA (a translation unit's switch): PBRT-v4's spherical camera is compiled into camera_generate_ray_differential (shm/path.h, SHM_SPHERICAL_CAMERA) only
// where it is true, and only k_generate_spherical.hip — k_generate.inl beside render.hip's — sets it: its launcher is wf_generate<true> (below), which
// RenderPlan::spherical names for a scene whose camera is one.
#ifndef K_SPHERICAL_CAMERA
#define K_SPHERICAL_CAMERA false
#endif
#define SHM_SPHERICAL_CAMERA K_SPHERICAL_CAMERA
#include "shm/path.h"
#include "shm/tri_shade.h"
// (the kernels' names: the *_dl builds' carry the suffix after the sampler's, k_*.inl)
#define WF_CAT_(a, b) a##b
#define WF_CAT(a, b) WF_CAT_(a, b)
#if K_DELTA_LIGHTS
#define WF_DL_NAME(name) WF_CAT(name, _dl)
#else
#define WF_DL_NAME(name) name
#endif

using namespace shm;

// thread-local message behind shm_last_error() (defined in render.hip)
__attribute__((visibility("hidden"))) std::string& shm_err();

namespace wf {

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            shm_err() = std::string(#expr) + ": " + hipGetErrorString(_e);                           \
            (void)hipGetLastError(); /* reported here: must not resurface at the next launch's LAUNCH_TRY */ \
            return SHM_ERR_DEVICE;                                                               \
        }                                                                                        \
    } while (0)

// every kernel launch is followed by LAUNCH_TRY: a failed launch (bad configuration, missing code object) is reported by the call that
// made it, not by the stream synchronisation at the end
#define LAUNCH_TRY(what)                                                                         \
    do {                                                                                         \
        hipError_t _e = hipGetLastError();                                                       \
        if (_e != hipSuccess) {                                                                  \
            shm_err() = std::string("launch of ") + (what) + ": " + hipGetErrorString(_e);           \
            return SHM_ERR_DEVICE;                                                               \
        }                                                                                        \
    } while (0)

static inline bool dbg_on() { static int v = -1; if (v < 0) v = getenv("SHM_DEBUG") ? 1 : 0; return v == 1; }
#define DBG(...) do { if (dbg_on()) { fprintf(stderr, "[shm] " __VA_ARGS__); fprintf(stderr, "\n"); fflush(stderr); } } while (0)

constexpr int WAVE = 64;
constexpr int TRACE_BLOCK = 256;  // 4 waves per workgroup
constexpr int SHADE_BLOCK = 128;
// The traversal queue's partitions — one per XCD, with stealing — and the dwords between their head words: one 128-B line each (k_trace.hip)
constexpr uint32_t TRACE_QUEUE_PARTS = 8, TRACE_HEAD_STRIDE = 32;

// The DEVICE copy of a BVH node (host/bvh_pairs.hpp lays the tree out by sibling pairs and rewrites `offset` into a link word; the ABI's array and the
// oracle's keep the reference's fields): everything a traversal step needs to go on from a node without reading it again —
//   interior  axis << 29 | index of the first child (the second is + 1; pairs start at even indices, so (index << 5) ^ 32 is the sibling's byte offset)
//   leaf      1 << 31 | min(n_prims, 7) << 27 | offset of its first primitive record (a count of 7 means: read ShmScene::d_big_leaf_n[offset], the primitives left from that slot on);
//             bit 30 is 0 in the array and set by a traversing lane (k_trace5<., GEN>): "the record at this slot is no triangle, its test is pending"
// `n_prims` and `axis` stay where they were (no kernel reads them since the one-node-step kernels were retired: the link word holds everything).
constexpr uint32_t HIT_HAS_SECOND = 0x40000000u;  // the compact hit records' primitive word, split form (scenes with spheres / patches, no instances): this hit has a second record
// (LINK_LEAF, LINK_OTHER, LINK_INDEX_MASK, LINK_COUNT_SHIFT, LINK_COUNT_MAX, LINK_AXIS_SHIFT: shm/bvh_link.h)

struct DeviceCounters {
    unsigned long long rays_closest, rays_any, nodes_closest, tris_closest, nodes_any, tris_any, paths;
};

// Queue bookkeeping that lives in HBM so that no launch needs a host round trip.
struct QueueState {
    uint32_t n_active[2];   // entries in q_active[0/1]
    uint32_t n_shadow[2];   // entries in q_shadow, double-buffered by bounce parity: K3 of bounce b may still be reading its count
                            // while the counters of bounce b+1 are recycled (K3(b) overlaps K2(b+1) on a second stream)
    uint32_t n_scatter[4];  // staged shading: entries in q_scatter[class], filled by k_vertex, drained by k_scatter<class>
    uint32_t n_lean;        // staged shading with the lean diversion: hits on plain DiffuseMaterial, which k_vertex hands to the fused kernel whole
    uint32_t n_emit;        // the fused kernel's deferred emitter hits (q_emit), worked off by k_emit_jobs after it
    uint32_t n_split;       // scenes with textures: the hits the split pass left to the textured kernels (q_split; the plain-diffuse ones went to q_lean)
};

// The part of a path's state that EVERY vertex reads (and rewrites), as one 64-byte record. As six separate arrays (rounds 1-4) a vertex touched six cache lines for
// these 56 bytes — harmless while every path of a line is alive, but paths die (Russian roulette, escapes) and the survivors stay where they are: at bounce 4 of the
// headline frame one path in ten is left, a 128-byte line serves one of them, and the fused kernel fetched 666 bytes per vertex against 108 at bounce 0
// (rocprofv3 FETCH_SIZE per dispatch). One record: one half line per vertex whatever the survival.
struct alignas(64) PathRec {
    // first 32-byte sector: what k_generate writes (all of it, so that a new path costs one full sector, not two partial ones) and bounce 0 reads
    float4 lambda;     // (the film reads its own copy, PathArrays::lambda)
    uint2 rng;         // sampler state (sampler_load / sampler_store below: the rest is re-derived from pixel + seed)
    uint32_t pixel;    // x | y << 16 (absolute pixel coordinates, < 65536)
    uint32_t flags;    // depth | specular_bounce << 8 | any_non_specular << 9 | ray has auxiliary rays << 10
    // second sector: written by the first vertex (a new path's constants — beta = 1, p_b = eta_scale = 1 — are not stored where the consumer knows them: k_generate<LEAN>)
    float4 beta;
    float2 pb_eta;     // p_b, eta_scale
    uint32_t pad[2];
};
static_assert(sizeof(PathRec) == 64, "PathRec is one half cache line");
// K_ZSOBOL (a translation unit's switch, like K_ENV_LIGHT): the Makefile compiles every unit whose kernels draw twice, the second time with K_ZSOBOL
// true into *_zs objects whose kernels carry a _zs suffix (k_shade.inl, k_scatter.inl, k_scatter_layered.inl, k_shade_other.hip) and whose launchers are the
// <., ZS = true, .> specializations of wf_shade (below). select_kernels (render.hip) picks the set from ShmRenderParams::sampler, so the sampler is a compile-time constant of every kernel: with the independent
// sampler the ZSobol code folds away and the kernels are those of a build without it (tools/kernel_resources.py).
#ifndef K_ZSOBOL
#define K_ZSOBOL false
#endif
// The sampler state a path carries between kernels (PathRec::rng / PathArrays::rng0: the PCG32 state, or ZSobol's sample index and dimension; shm/sampling.h):
// the one load and the one store of every kernel that draws.
template <bool ZS = K_ZSOBOL>
__device__ __forceinline__ uint32_t sampler_word(const SceneView& sv) {
    return ZS ? sv.zsobol : 0u;
}
__device__ __forceinline__ Rng sampler_load(uint2 rs, uint32_t pix, const SceneView& sv, const ShmRenderParams& params) {
    return sampler_resume((uint64_t)rs.x | ((uint64_t)rs.y << 32), pix & 0xffffu, pix >> 16, params.seed, sampler_word(sv));
}
__device__ __forceinline__ uint2 sampler_store(const Rng& r) {
    const uint64_t w = sampler_save(r);
    return make_uint2((uint32_t)w, (uint32_t)(w >> 32));
}
// Staged shading's parameter block — what get_bsdf left at a vertex, written by k_vertex and read by the scatter kernel of the vertex's BxDF class (the layered one
// reads it in each of its stages) — as one 128-byte record, ordered so that a class reads whole 32-byte sectors: {bx0, bx2 | fr, bx1} for diffuse / conductor /
// dielectric, + {bx3, bx4} for the coated ones, + {siwo} in scenes with quadrics, patches or instances. Six separate arrays before (PathRec, above, for the why).
struct alignas(128) BxRec {
    float4 bx0;   // r[4]: reflectance (Diffuse, CoatedDiffuse) / conductor eta (Conductor, CoatedConductor)
    float4 bx2;   // eta, alpha_x, alpha_y, kind | max_depth << 8 | n_samples << 20 (as bits)
    float4 fr;    // shading frame x = normalize(dpdus) (y = z cross x is recomputed; z = ns lives in CtxRec::c2)
    float4 bx1;   // k[4]: conductor absorption
    float4 bx3;   // albedo[4]                         (coated materials)
    float4 bx4;   // alpha_x2, alpha_y2, thickness, g  (coated materials)
    float4 siwo;  // intr.wo (scenes with non-triangle shapes or instances only: elsewhere it is -ray.d bit for bit)
    float4 pad;
};
static_assert(sizeof(BxRec) == 128, "BxRec is one cache line");
// A vertex's LightSampleContext (light.rs:1001-1009): the scatter half's geometry and the next vertex's prev_intr_ctx, one record
struct alignas(64) CtxRec { float4 c0, c1, c2, pad; };
// Path state (DESIGN.md §"Data layout in HBM"). All arrays have `capacity` entries.
struct PathArrays {
    ShmRay* ray;            // 32 B: o, d, t_max — input of K2
    ShmHit* hit;            // 32 B: output of K2 — or, with hit16, 16 B per path in the same allocation: {primitive, b0, b1, b2} as one float4
    const float4* hit_prev; // hit16 renders of an all-diffuse triangle scene: the 16-byte records are double-buffered by bounce parity in the two halves of `hit`; this is the previous bounce's
    uint32_t hit16;         // set per render: a triangle scene without textures under the path integrator (every consumer is a TRI_ONLY kernel, none reads a triangle hit's t)
    ShmRay* shadow_ray;     // 32 B: input of K3
    float4* shadow_contrib; // beta * Ld, added to L by K3 when unoccluded
    float4* L;
    PathRec* rec;           // 64 B: beta, lambda, p_b / eta_scale, sampler state, pixel, flags — what every vertex reads of its path, in ONE half line (below)
    float4* lambda;         // the film's copy of the wavelengths (written once by k_generate; the shading kernels read PathRec::lambda)
    uint2* rng0;            // all-diffuse triangle scenes (bounce 0 on known constants): what k_generate<LEAN> leaves INSTEAD of a record — the sampler state ...
    uint32_t* pixel0;       // ... and the pixel; the fused kernel's bounce 0 reads them (and `lambda`) and writes the path's first record whole
    float4* lambda_pdf;
    CtxRec* ctx;            // 64 B: prev_intr_ctx — c0 = pi.low.xyz, pi.high.x; c1 = pi.high.yz, n.xy; c2 = n.z, ns.xyz (one record: three arrays before)
    // scenes with image textures only (null otherwise): the ray's AuxiliaryRays (ray.rs:104-135)
    float4* aux0;           // rx_origin.xyz, rx_direction.x
    float4* aux1;           // rx_direction.yz, ry_origin.xy
    float4* aux2;           // ry_origin.z, ry_direction.xyz
    // staged shading (k_vertex -> k_scatter<class>; null when the scene runs the fused kernel): the BxDF parameter block get_bsdf
    // left at this vertex and the x axis of its shading frame. The rest of the vertex geometry (pi, n, ns) is the CtxRec, which
    // k_vertex overwrites with THIS vertex's LightSampleContext once the previous one has served the emitter MIS weight.
    BxRec* bx;              // 128 B: the parameter block as ONE record per path (above)
    uint32_t has_layered;   // the scene holds coated materials: k_vertex writes the record's third sector (bx3, bx4)
    // scenes with image textures only: what Igehy's specular differentials need beside the auxiliary rays (interaction.rs:430-514)
    const float4* hit2;     // hit16 in a scene with spheres / patches: the second records (t, phi) of the hits that have one (HIT_HAS_SECOND), behind the first ones in the hit allocation
    float4* dd0;            // dpdx.xyz, dpdy.x
    float4* dd1;            // dpdy.yz, dndx.xy
    float4* dd2;            // dndx.z, dndy.xyz
    // scenes whose vertices (or some of them: the lean diversion) run the fused kernel: what emission at the hit needs of the state that kernel overwrites,
    // written for the rare vertex that hit an emitter and read back by k_emit_jobs (k_shade.inl)
    float4* e_ray;          // ray.d.xyz, p_b
    float4* e_beta;
    float4* e_ctx0;         // prev_intr_ctx as ctx0..2 (only written when the MIS weight needs it)
    float4* e_ctx1;
    float4* e_ctx2;
    uint32_t* e_flags;      // the path's flags word at the hit (depth, specular_bounce)
};
enum : int { CLASS_DIFFUSE = 0, CLASS_CONDUCTOR = 1, CLASS_DIELECTRIC = 2, CLASS_LAYERED = 3, N_BXDF_CLASSES = 4 };
// (device only: its body depends on the unit's SHM_DIFFUSE_TRANSMISSION, and host code of a unit built without the switch — render.hip — would file kind 8 under
//  CLASS_LAYERED. The same holds for every shm:: function that reads SHM_DELTA_LIGHTS or SHM_DIFFUSE_TRANSMISSION (get_bsdf, base_f_v, base_sample_f_v, base_pdf_v,
//  base_flags, the light sampling): the kernel units differ in them, so no HOST code of a kernel unit may call one: the linker would keep one unit's body for all of them.)
__device__ inline int bxdf_class_of(uint32_t kind) {
    if (SHM_DIFFUSE_TRANSMISSION && kind == SHM_MATERIAL_DIFFUSE_TRANSMISSION) return CLASS_DIFFUSE;  // non-specular, takes NEE, no microfacet code
    return kind == SHM_MATERIAL_DIFFUSE ? CLASS_DIFFUSE : (kind == SHM_MATERIAL_CONDUCTOR ? CLASS_CONDUCTOR : (kind <= SHM_MATERIAL_THIN_DIELECTRIC ? CLASS_DIELECTRIC : CLASS_LAYERED));
}

__device__ __forceinline__ AuxRays ld_aux(const PathArrays& pa, uint32_t path) {
    float4 a = pa.aux0[path], b = pa.aux1[path], c = pa.aux2[path];
    AuxRays x;
    x.has = true;
    x.rx_o = v3(a.x, a.y, a.z); x.rx_d = v3(a.w, b.x, b.y);
    x.ry_o = v3(b.z, b.w, c.x); x.ry_d = v3(c.y, c.z, c.w);
    return x;
}
__device__ __forceinline__ void st_aux(const PathArrays& pa, uint32_t path, const AuxRays& x) {
    pa.aux0[path] = make_float4(x.rx_o.x, x.rx_o.y, x.rx_o.z, x.rx_d.x);
    pa.aux1[path] = make_float4(x.rx_d.y, x.rx_d.z, x.ry_o.x, x.ry_o.y);
    pa.aux2[path] = make_float4(x.ry_o.z, x.ry_d.x, x.ry_d.y, x.ry_d.z);
}

// ---- small scene tables staged in LDS --------------------------------------------------------------------------------------------------
// The material table, the light table and the spectrum pool are tens of bytes to a few KB, and every vertex reaches them at the END of a chain of dependent
// gathers (hit -> primitive -> material -> spectrum samples; light -> spectrum samples): from L2 each link costs a vector-memory round trip. A workgroup copies them
// into LDS once and the kernel goes on with a SceneView whose pointers name the copies — generic pointers into the LDS aperture: the shared leaf code (shm/*.h,
// compiled for the oracle too) reads them through the same flat loads as before, at LDS latency. Same bytes: results cannot change. `LdsTables` says what fits
// (host side: wf_lds_tables); a scene whose tables exceed the budget runs with the global pointers (bytes = 0).
constexpr uint32_t LDS_TABLE_BUDGET = 12 * 1024, LDS_TABLE_BUDGET_SMALL = 1536;
// the tables a kernel may stage, hottest and smallest first (the host fills a kernel's budget greedily in this order: wf_lds_tables, render.hip)
enum : int { LT_MESH_FLAGS, LT_LIGHTS, LT_LIGHT_PRIMS, LT_MATERIALS, LT_SPECTRUM, LT_RGB2SPEC_SCALE, LT_IMAGE_TEXTURES, LT_IMAGE_LEVELS, LT_FLOAT_TEXTURES, LT_FTEX_RANGES, LT_FTEX_OPS, LT_SPECTRUM_TEXTURES,
              LT_STEX_RANGES, LT_STEX_OPS, LT_EWA_LUT, N_LDS_TABLES };  // (rgb2spec's scale table: 64 floats, walked by a binary search of six DEPENDENT loads per lookup)
struct LdsTables {
    uint32_t bytes[N_LDS_TABLES];  // each a multiple of 16 (dev_upload allocates whole 16-byte groups); 0: that table stays in global memory
};
__device__ __forceinline__ SceneView stage_scene_tables(const SceneView& sv, const LdsTables& t, uint4* lds) {
    SceneView out = sv;
    uint32_t total = 0;
#pragma unroll
    for (int k = 0; k < N_LDS_TABLES; ++k) total += t.bytes[k];
    if (total == 0u) return out;
    uint32_t at = 0;  // in uint4s
#define SHM_STAGE_TABLE(K, FIELD, TYPE)                                                                \
    if (t.bytes[K]) {                                                                                  \
        const uint32_t n = t.bytes[K] / 16u;                                                           \
        const uint4* g = reinterpret_cast<const uint4*>(sv.FIELD);                                     \
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) lds[at + i] = g[i];                     \
        out.FIELD = reinterpret_cast<const TYPE*>(lds + at);                                           \
        at += n;                                                                                       \
    }
    SHM_STAGE_TABLE(LT_MESH_FLAGS, mesh_flags, uint32_t)
    SHM_STAGE_TABLE(LT_LIGHTS, lights, ShmLight)
    SHM_STAGE_TABLE(LT_LIGHT_PRIMS, light_prim_recs, PrimRec)
    SHM_STAGE_TABLE(LT_MATERIALS, materials, ShmMaterial)
    SHM_STAGE_TABLE(LT_SPECTRUM, spectrum_data, Float)
    SHM_STAGE_TABLE(LT_RGB2SPEC_SCALE, rgb2spec_scale, Float)
    SHM_STAGE_TABLE(LT_IMAGE_TEXTURES, image_textures, ShmImageTexture)
    SHM_STAGE_TABLE(LT_IMAGE_LEVELS, image_levels, ShmImageLevel)
    SHM_STAGE_TABLE(LT_FLOAT_TEXTURES, float_textures, ShmFloatTexture)
    SHM_STAGE_TABLE(LT_FTEX_RANGES, ftex_ranges, FloatTexRange)
    SHM_STAGE_TABLE(LT_FTEX_OPS, ftex_ops, FloatTexOp)
    SHM_STAGE_TABLE(LT_SPECTRUM_TEXTURES, spectrum_textures, ShmSpectrumTexture)
    SHM_STAGE_TABLE(LT_STEX_RANGES, stex_ranges, FloatTexRange)
    SHM_STAGE_TABLE(LT_STEX_OPS, stex_ops, FloatTexOp)
    SHM_STAGE_TABLE(LT_EWA_LUT, ewa_lut, Float)
#undef SHM_STAGE_TABLE
    __syncthreads();
    return out;
}

// ... and for the kernels that evaluate textures: the staged view itself copied to LDS once per workgroup, for the evaluators that are real calls (shm/texture.h)
constexpr uint32_t SCENE_VIEW_UINT4S = (sizeof(SceneView) + 15) / 16;
__device__ __forceinline__ void attach_call_copy(SceneView& sv, uint4* slot) {
    SceneView* call_copy = reinterpret_cast<SceneView*>(slot);
    sv.call_copy = call_copy;
    if (threadIdx.x == 0) *call_copy = sv;
    __syncthreads();
}
// (HAS_TEX = false: the plain staging; `slot` is a one-element dummy then)
template <bool HAS_TEX>
__device__ __forceinline__ SceneView stage_scene_tables_tex(const SceneView& sv, const LdsTables& t, uint4* lds, uint4* slot) {
    SceneView out = stage_scene_tables(sv, t, lds);
    if (HAS_TEX) attach_call_copy(out, slot);
    return out;
}

// the primitive of a compact hit record's first word (a miss stays negative)
__device__ __forceinline__ int hit_prim_of(int w) { return w < 0 ? w : (int)((uint32_t)w & ~HIT_HAS_SECOND); }
// a path's hit record as the TRI_ONLY shading kernels read it: the 32-byte ShmHit, or the compact form the render's own traversal launches write (PathArrays::hit16)
// (the compact form from a record already in registers: k_shade<lean> fetches a vertex's record while it shades the one before, k_shade.inl)
__device__ __forceinline__ Hit hit_from_record16(const PathArrays& pa, const float4& h, uint32_t path) {
    Hit hit;
    const int w = __float_as_int(h.x);
    hit.prim = hit_prim_of(w); hit.t = 0.0f; hit.b0 = h.y; hit.b1 = h.z; hit.b2 = h.w; hit.phi = 0.0f; hit.inst = -1;
    if (w >= 0 && ((uint32_t)w & HIT_HAS_SECOND)) {  // (the split form: a sphere / patch hit's t and phi — p_obj / (u, v) ride in b0..b2)
        const float4 h2 = pa.hit2[path];
        hit.t = h2.x; hit.phi = h2.y;
    }
    return hit;
}
__device__ __forceinline__ Hit load_hit_tri(const PathArrays& pa, uint32_t path) {
    Hit hit;
    if (pa.hit16) {
        hit = hit_from_record16(pa, reinterpret_cast<const float4*>(pa.hit)[path], path);
    } else {
        const float4* hp = reinterpret_cast<const float4*>(pa.hit + path);
        const float4 h0 = hp[0], h1 = hp[1];
        hit.prim = __float_as_int(h0.x); hit.t = h0.y; hit.b0 = h0.z; hit.b1 = h0.w; hit.b2 = h1.x; hit.phi = h1.y; hit.inst = __float_as_int(h1.z) - 1;
    }
    return hit;
}

__device__ __forceinline__ uint32_t wave_lane() { return __lane_id(); }

// Wave-aggregated append: one atomic per wave, lanes get consecutive slots.
__device__ __forceinline__ uint32_t queue_push_slot(uint32_t* counter, bool pred) {
    unsigned long long mask = __ballot(pred);
    if (mask == 0ull) return 0u;
    uint32_t lane = wave_lane();
    int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if ((int)lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = __shfl(base, leader);
    uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    return base + rank;
}
// A path's slot in a batch, shared by K1 (k_generate.inl), which fills the slots, and K6 (k_film, render.hip), which reads them back per pixel in sample order: slots are
// ordered [pixel group][sample][pixel in group] with groups of `pix_group` consecutive pixels of the tile-ordered pixel list (pix_group >= n_pix is the plain sample-major
// order slot = s_local * n_pix + p_local; pix_group = 64 keeps all samples of one 8x8 tile adjacent in the queues, so that a wave's private queue range, and an XCD's
// queue partition, is a compact image region).
__device__ __forceinline__ uint32_t slot_of(uint32_t p_local, uint32_t s_local, uint32_t n_pix, uint32_t n_samples, uint32_t pix_group) {
    uint32_t g = p_local / pix_group;
    uint32_t g0 = g * pix_group;
    uint32_t pg = min(pix_group, n_pix - g0);
    return g0 * n_samples + s_local * pg + (p_local - g0);
}
__device__ __forceinline__ Spec ld_spec(const float4& f) { Spec s; s.v[0] = f.x; s.v[1] = f.y; s.v[2] = f.z; s.v[3] = f.w; return s; }
__device__ __forceinline__ float4 st_spec(const Spec& s) { return make_float4(s.v[0], s.v[1], s.v[2], s.v[3]); }
constexpr int SHADE2_BLOCK = 256;
constexpr int SHADE_CHUNK = 2048;  // queue entries per workgroup chunk: ONE global atomic per queue per chunk (a single
                                   // counter word saturates near 88 atomics/us: MI355X_MICROARCH.md "dequeue")
// Two waves per SIMD for every instantiation: the lean one needs 236 VGPRs anyway; the ones with the quadric / patch or the
// LayeredBxDF code want 264 / 460 and are better off spilling a little than running one wave per SIMD (measured: patch scene
// shade 16.6 -> 10.9 ms, coated S3 187 -> 177 ms; 3 or 4 waves lose to spills).
#ifndef K_SHADE_WAVES
#define K_SHADE_WAVES 2
#endif
#define K_SHADE_ATTR __attribute__((amdgpu_waves_per_eu(K_SHADE_WAVES, K_SHADE_WAVES)))
}  // namespace wf
using namespace wf;

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------
// One side of the traversal kernels' state, closest hit [RAY_CLOSEST] / any hit [RAY_ANY] — the any-hit kernel may run beside the closest-hit one (second stream):
// sized by wf_trace_prepare from the scene's row of shm_plan::TRACE_SHAPES
struct TraceSide {
    int blocks = 0;                // the persistent grid
    int spill_levels = 1;          // stack levels beyond the kernel's LDS levels (ScenePlan::trace_spill_levels) ...
    uint32_t* d_spill = nullptr;   // ... per resident lane, in HBM
    float4* d_gen_save = nullptr;  // trace5_body<., GEN> (scenes with spheres / patches / instances): per resident lane two 48-byte areas for the ray state
    uint32_t* d_heads = nullptr;   // the queue's head words: [TRACE_QUEUE_PARTS][TRACE_HEAD_STRIDE]
    SceneView* d_view = nullptr;   // scenes with shape alpha (k_trace_alpha.hip): the SceneView of the launch in HBM, which the texture evaluators that are real calls read the
                                   // scene through (SceneView::call_copy; the shading kernels keep theirs in LDS, which these kernels' rows have none to spare of)
};
struct ShmScene {
    int device = 0;
    hipStream_t stream = nullptr;
    shm_host::FlatScene flat;
    SceneView dsv;                 // device pointers
    shm_plan::ScenePlan plan;      // which pipeline the scene runs, its thresholds and knobs: fixed at creation (host/render_plan.hpp)
    std::vector<void*> allocs;
    std::vector<void*> ws_allocs;  // path workspace (regrown on demand)
    ShmFilmPixel* d_film = nullptr;
    size_t n_film_pixels = 0;
    // path workspace
    uint32_t capacity = 0;
    PathArrays pa;
    uint32_t* d_q_active[2] = {nullptr, nullptr};
    uint32_t* d_q_shadow = nullptr;
    float* d_filter_weight = nullptr;  // per path slot: the pixel filter's weight (scenes whose filter has negative lobes only; render.hip, ensure_workspace)
    uint32_t* d_q_scatter[4] = {nullptr, nullptr, nullptr, nullptr};  // staged shading: one queue per BxDF class present in the scene
    uint32_t* d_q_split = nullptr; // scenes with textures and plain diffuse materials: what the split pass leaves to the textured kernels
    uint32_t* d_q_lean = nullptr;  // the lean diversion's queue (triangle-only scenes without textures that hold plain diffuse materials beside others)
    bool ws_staged = false;        // the workspace holds the staging arrays
    QueueState* d_qs = nullptr;
    DeviceCounters* d_counters = nullptr;
    uint32_t* d_pixels = nullptr;
    size_t pixels_capacity = 0;
    ShmTile* d_tiles = nullptr;
    uint32_t* d_tile_offset = nullptr;
    size_t tiles_capacity = 0;
    std::vector<uint64_t> tile_bitmap;  // host scratch of the tiles' disjointness check: a wave call's (render.hip, build_pixel_list) and shm_moments_update's
    int n_cu = 256;
    TraceSide trace[shm_plan::N_RAY];
    uint32_t* d_big_leaf_n = nullptr;  // n_prims by first primitive slot, only in scenes with a leaf of >= 7 primitives (LINK_COUNT_MAX: the link word holds smaller counts)
    LdsTables lds_tables = {};        // the small tables the shading kernels stage in LDS within the full budget (render.hip: wf_lds_tables)
    LdsTables lds_tables_small = {};  // ... within the 1.5 KB the material-sorted triangle vertex kernel has to spare
    uint32_t* d_q_emit = nullptr;      // paths of the current fused-kernel launch that hit an emitter (k_emit_jobs)
    float4* d_rw = nullptr;          // RandomWalk: (le, f cos) per depth per path, 2 * (max_depth + 1) * capacity float4
    size_t rw_floats4 = 0;
    hipStream_t stream2 = nullptr;
    hipStream_t stream_cls[4] = {nullptr, nullptr, nullptr, nullptr};  // staged shading: the scatter kernels of the 2nd .. 4th BxDF class of a bounce run beside the first one's
    uint32_t pix_group = 1024;      // path-slot order [tile][sample][pixel in tile] (>= n_pix would be sample-major; swept in round 1: profiles/r01_*)
    std::vector<hipEvent_t> events;
    struct DistState* dist = nullptr;  // multi-GPU state (dist.hip): communicator, this rank's tile shard, the gather plan
    uint32_t n_tri_shade_records = 0;   // the flat triangles' shading records built at scene creation (shm/tri_shade.h; shm_scene_shading_records) ...
    double tri_shade_build_ms = 0.0;    // ... and the wall-clock time that took
    ShmGBufferPixel* d_gbuffer = nullptr;  // the G-buffer pass's sums, pixel_bounds-sized: allocated by the first shm_gbuffer_* call (render.hip), null in a scene that never asks
    bool gbuffer_filled = false;           // a G-buffer wave has run since the scene was made or the G-buffer last cleared: what the denoiser asks for its guides
    float4* d_denoise = nullptr;           // the denoiser's planes (k_denoise.hip: five float4 per pixel) and, behind them, its result — made by the first shm_denoise_device
    ShmFilmPixel* d_denoised = nullptr;
    bool denoised = false;                 // d_denoised holds a result
    ShmMomentsPixel* d_moments = nullptr;  // the moments pass's records (k_moments.hip), pixel_bounds-sized: made by the first shm_moments_clear, null in a scene that never asks
    ShmTile* d_moments_tiles = nullptr;    // that pass's own tile list and its per-tile result, one allocation in `allocs`, regrown on demand
    ShmTileError* d_tile_error = nullptr;
    uint32_t moments_tiles_capacity = 0;
    uint32_t gbuffer_space = 0;            // SHM_GBUFFER_SPACE_* of the last G-buffer wave: the temporal pass reprojects render-space positions only
    float4* d_temporal[2] = {nullptr, nullptr};  // the temporal pass's two record arrays (k_temporal.hip: four float4 per pixel) and, behind them, its result: one allocation, made by the first shm_temporal_clear / _accumulate_device
    ShmFilmPixel* d_temporal_out = nullptr;
    int temporal_cur = 0;                  // which array holds the records just written
    bool temporal_has_camera = false;      // an accumulate has run since the last clear: temporal_camera is the camera it saw, d_temporal[temporal_cur] its records
    bool temporal_filled = false;          // d_temporal_out holds a result
    ShmCamera temporal_camera = {};
    uint32_t* d_display = nullptr;         // the display pass's RGBA8 image (k_display.hip), pixel_bounds-sized, and, behind it, the histogram's per-workgroup slabs and the 256 counts + state: one allocation, made by the first shm_display_clear / _device
    uint32_t* d_display_slabs = nullptr;
    uint32_t* d_display_state = nullptr;   // 256 counts, then a ShmDisplayState
    bool display_filled = false;           // d_display holds an image
    float ao_illum_scale = 0.0f;           // the ambient occlusion integrator's illum_scale: 1 / CIE Y of the colour space's illuminant, in double at scene creation, rounded once
                                           // (0: the scene came without an illuminant, and a render under that integrator is refused)
};
// dist.hip: releases s->dist (RCCL communicator included); called by shm_scene_destroy
__attribute__((visibility("hidden"))) void wf_dist_release(ShmScene* s);

struct EventPool {
    ShmScene* s;
    size_t used = 0;
    bool failed = false;  // hipEventCreate failed: checked once per render (events are only used for timing / stream ordering)
    hipEvent_t get() {
        if (used == s->events.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) { failed = true; return nullptr; }
            s->events.push_back(e);
        }
        return s->events[used++];
    }
};

// ---- launchers exported by the kernel translation units (hidden visibility: library-internal) ----
#define WF_INTERNAL __attribute__((visibility("hidden")))
WF_INTERNAL LdsTables wf_lds_tables(const ShmScene* s, uint32_t budget);  // render.hip: which small tables fit `budget` bytes of LDS
// render.hip: a device allocation the scene owns (ShmScene::allocs: shm_scene_destroy frees it), and one given back before that
WF_INTERNAL int wf_scene_alloc(ShmScene* s, size_t bytes, void** out);
WF_INTERNAL void wf_scene_free(ShmScene* s, void* d);
// render.hip: a pixel_bounds-sized device image (the film, the G-buffer, the moments, the denoiser's result) read back once the render stream is through
WF_INTERNAL int wf_read_pixels(ShmScene* s, const void* d_image, size_t bytes_per_pixel, void* out);
WF_INTERNAL void wf_trace_census();  // k_trace.hip: prints the per-phase lane census of a -DK5_CENSUS development build (a no-op otherwise)
WF_INTERNAL void wf_layered_census();  // k_scatter_layered_staged_tri.hip: the same for a -DLJ_CENSUS build of the staged LayeredBxDF kernel
WF_INTERNAL int wf_trace_prepare(ShmScene* s);  // ShmScene::trace: grid sizes, stack spill and save areas of the scene's two traversal kernels (at scene creation)
// k_trace.hip: BvhAggregate::intersect (RAY_CLOSEST) / intersect_predicate (RAY_ANY) over a queue of path slots, or over slots 0 .. n_direct - 1 without one
struct TraceArgs {
    hipStream_t stream;
    const uint32_t* queue = nullptr;  // the path slots to trace, and their count (on the device)
    const uint32_t* n_ptr = nullptr;
    uint32_t n_direct = 0;            // (queue == nullptr: this many rays)
    const ShmRay* rays = nullptr;
    ShmHit* hits = nullptr;           // closest hit: the hit records
    uint8_t* occluded = nullptr;      // any hit: one flag per ray, or
    float4* L = nullptr;              // ... `contrib` added to L where the ray is unoccluded
    const float4* contrib = nullptr;
    int hit16 = 0;                    // the render's compact hit records (PathArrays::hit16) ...
    float4* hit2 = nullptr;           // ... and, in their split form, the second records (PathArrays::hit2)
};
// (any_strict: RenderPlan::trace_any_strict — the any-hit kernels with PBRT-v4's way into an instance; the public trace entry points keep the reference-exact ones)
WF_INTERNAL int wf_launch_trace(ShmScene* s, int ray, bool any_strict, const TraceArgs& t);
// shading of one path vertex of PathIntegrator::li for every entry of q_active[cur]
struct ShadeArgs {
    hipStream_t stream;
    int cur;
    ShmRenderParams params;
    int shadow_parity;
    int blocks;
    int first_bounce = 0;  // 1: bounce 0 of a render whose k_generate left the constants out (beta = 1, p_b = eta_scale = 1, flags = 0, the identity queue): the fused kernel knows them
    int hit_kept = 0;      // 1: the hit records are double-buffered by bounce parity (PathArrays::hit_prev is the previous bounce's): the fused kernel leaves nothing for the next vertex
    uint32_t cap_eff = 0;  // RandomWalk: paths per batch (the stride of ShmScene::d_rw)
    const uint32_t* q_in = nullptr;  // k_vertex: the queue to work through instead of q_active[cur], and its count (the split pass's q_split)
    const uint32_t* n_in = nullptr;
    uint32_t* q_divert = nullptr;    // k_vertex: where it diverts the hits on plain diffuse materials (RenderPlan::divert_vertex: q_lean), null: nowhere
};
// Every shading launcher launches ONE build of its family's kernel for ONE scene class: geometry (GEO_TRI: top-level triangles only, GEO_GEN: spheres / patches /
// instances too) x image class (IMG_NONE, IMG_TEX: image textures — ray differentials, MIP filtering —, IMG_ENV: an ImageInfinitelight alone, the K_ENV_LIGHT units).
// They are the explicit specializations of ONE template, addressed by coordinates: the family (shm_plan::FAM_*, host/render_plan.hpp), the build's scene class, the
// sampler and the extended build. Each kernel unit defines <., K_ZSOBOL, K_DELTA_LIGHTS> of the builds it holds — the Makefile compiles the units that draw and sample
// lights four times (K_ZSOBOL x K_DELTA_LIGHTS) and k_vertex_*.hip, which draws nothing, twice: it defines <., false, K_DELTA_LIGHTS> for both samplers. Which build
// serves which cell is shm_plan::serving_build, from which render.hip computes its table (ShadeKernels by geometry, image class, sampler, extended build); a render's
// RenderPlan holds the coordinates and select_kernels looks them up. The template has no definition: a build the rule names and no unit defines is a link error
// (an undefined hidden symbol) whose name spells the coordinates.
//   FAM_LEAN, FAM_LEAN_DIVERTED  k_shade<lean> (k_shade_lean*.hip): all-diffuse scenes without textures — every hit of the queue — / the hits k_vertex or the split pass diverted
//   FAM_FUSED_ALL                the material-sorted fused all-materials kernel (k_shade_tail_sorted*.hip, k_shade_fused_*.hip): scenes without coated materials
//   FAM_VERTEX                   staged shading (k_vertex_*.hip): the hit half of a vertex (interaction, emission + MIS, get_bsdf with its texture evaluation -> BxDF parameter
//                                block, pushed to the queue of its BxDF class); its K_DELTA_LIGHTS build knows the diffuse transmission material
//   FAM_SCATTER + class          ... then per class the scattering half (k_scatter_*.hip: NEE, sample_f, RR); the LayeredBxDF class as dense per-wave stages
//                                (k_scatter_layered.inl): every render but options.force_diffuse ...
//   FAM_SCATTER_LAYERED_ONEPASS  ... and in one pass per vertex (k_scatter.inl), which has force_diffuse's code
//   FAM_SIMPLE, FAM_RANDOMWALK   the other integrators (k_shade_other.hip): one kernel each for every scene class
using ShadeFn = int (*)(ShmScene*, const ShadeArgs&);
template <int FAMILY, int GEO, int IMG, bool ZS, bool DL> WF_INTERNAL int wf_shade(ShmScene* s, const ShadeArgs& a);
// k_shade_lean_prefetch.hip: the (GEO_TRI, IMG_NONE) lean launchers' other kernel, k_shade<lean>'s PREFETCH instantiation (k_shade.inl: K_SHADE_PREFETCH), the whole queue or
// the diverted hits — called by those launchers for the renders that take it, and like them defined once per (sampler, extended build)
template <bool ZS, bool DL> WF_INTERNAL int wf_shade_lean_prefetch(ShmScene* s, const ShadeArgs& a, bool diverted);
// A build's coordinates as its kernels' template parameters: the stubs of the kernel units (WF_*_STUB, k_*.inl) take (GEO, IMG) and derive these, so that a launcher's
// place in the table and the kernel it launches cannot disagree. (The one textured build of the staged families is (GEO_GEN, IMG_TEX): TRI_ONLY = false.)
constexpr bool build_tri_only(int geo) { return geo == shm_plan::GEO_TRI; }
constexpr bool build_has_tex(int img) { return img == shm_plan::IMG_TEX; }
constexpr bool build_env_light(int img) { return img == shm_plan::IMG_ENV; }
// (the units that compile the environment light in by their switch, not by a template parameter: an env build belongs in a K_ENV_LIGHT unit, and no other does)
#define WF_ENV_UNIT_CHECK(IMG) static_assert(build_env_light(IMG) == (K_ENV_LIGHT), "an IMG_ENV build is a K_ENV_LIGHT unit's, and such a unit holds no other")
WF_INTERNAL int wf_launch_fold_randomwalk(ShmScene* s, hipStream_t stream, uint32_t cap_eff, uint32_t total);  // k_shade_other.hip: RandomWalk's sum over depths, after the last bounce
// K1, the camera rays of one batch (k_generate.inl): ONE launcher per unit that holds the kernels — <false>: render.hip, the reference's perspective and orthographic
// cameras; <true>: k_generate_spherical.hip — addressed by the plan's coordinates: image textures (the camera rays' auxiliary rays: RenderPlan::img_generate == IMG_TEX),
// bounce 0 on known constants (lean_first), the sampler and the pixel filter's class (FLT_*). Which (tex, lean) builds exist, and the class a FLT_* runs, is
// shm_plan::has_generate_build / generate_filter_class (host/render_plan.hpp); like wf_shade the template has no definition.
struct GenerateArgs {
    hipStream_t stream;
    const uint32_t* pixels;
    uint32_t n_pix;
    int sample_begin, n_samples;
    ShmRenderParams params;
    bool tex, lean, zs;
    int flt;
};
template <bool SPHERICAL> WF_INTERNAL int wf_generate(ShmScene* s, const GenerateArgs& a);
// k_gbuffer.hip: the G-buffer pass behind K1 and the closest-hit launch of a batch — k_gbuffer<tex> per path slot (shm/gbuffer.h; the slot's record goes where the
// path's CtxRec lives, which no kernel of this pass reads), then k_gbuffer_accumulate per pixel into ShmScene::d_gbuffer, in sample order. `film_weight`: where a
// sample's filter weight comes from (shm_plan::FILM_WEIGHT_*), as for K6.
struct GBufferArgs {
    hipStream_t stream;
    const uint32_t* pixels;
    uint32_t n_pix;
    int n_samples;
    ShmRenderParams params;
    bool tex;
    uint32_t space;
    int film_weight;
};
WF_INTERNAL int wf_launch_gbuffer(ShmScene* s, const GBufferArgs& a);
// k_ao.hip: the ambient occlusion integrator's shade kernel, k_shade_ao (shm/ao.h), over q_active[cur] — one build for every scene class, one instantiation per sampler;
// it fills the shadow buffers and the shadow queue as a path vertex's light sample does (ShmScene::ao_illum_scale rides along as an argument)
WF_INTERNAL int wf_launch_shade_ao(ShmScene* s, const ShadeArgs& a, bool zs);
// k_denoise.hip: shm_denoise_device's body over `film` — the scene's, or the temporal pass's result (shm_denoise_temporal_device, k_temporal.hip) — into ShmScene::d_denoised;
// `temporal_records` not null: behind the variance pass, k_temporal.hip's kernel puts the records' temporal variance over plane A's at the pixels whose history is long enough
WF_INTERNAL int wf_denoise_run(ShmScene* s, const ShmDenoiseParams* params, const ShmFilmPixel* film, const float4* temporal_records, double* ms_out);
// k_temporal.hip: that kernel, on `stream`; A, C: the denoiser's planes (e.rgb | var, p.xyz | valid)
WF_INTERNAL int wf_launch_temporal_variance(hipStream_t stream, float4* A, const float4* C, const float4* temporal_records, uint32_t n);
// The shading launchers of one scene class: a cell of render.hip's table by geometry x image class x sampler x extended build (nullptr: no such
// build, shm_plan::serving_build), of which select_kernels makes a render's set by the RenderPlan's coordinates. The plan says which of them run; the bounce loop calls them.
struct ShadeKernels {
    ShadeFn lean, lean_diverted;      // k_shade<lean>: the whole queue of an all-diffuse scene / the hits k_vertex or the split pass diverted
    ShadeFn fused_all;                // the material-sorted fused all-materials kernel
    ShadeFn vertex;                   // staged shading: the hit half ...
    ShadeFn scatter[N_BXDF_CLASSES];  // ... and the scattering half of each BxDF class
    ShadeFn scatter_layered_onepass;  // (the LayeredBxDF class in one pass per vertex: select_kernels puts it in scatter[CLASS_LAYERED] where it runs)
    ShadeFn simple, randomwalk;       // the other integrators
};
