// host/render_plan.hpp — WHICH pipeline a scene and a render run, and what path workspace that needs, decided once and kept as data (plain C++17, no HIP:
// oracle/oracle.cpp exports the two functions to tests/test_render_plan.py, which walks their whole domain).
//   ScenePlan   at scene creation, from the class facts of the FlatScene and the environment knobs (read_knobs: the only getenv of the decisions); with it the
//               traversal kernels' variant table (TRACE_SHAPES)
//   RenderPlan  once per shm_render_wave, from the ScenePlan and the render's options
// render.hip's select_kernels is a lookup by the RenderPlan's coordinates, K1's launcher (wf_generate, k_generate.inl) and K6's (launch_film) go by the same coordinates
// and the rule below serving_build, and the bounce loop asks the plan and nothing else; WS_ARRAYS below is the one list of
// per-path arrays behind both the workspace budget and its allocation.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "flatten.h"

namespace shm_plan {

enum : int { CLS_DIFFUSE = 0, CLS_CONDUCTOR = 1, CLS_DIELECTRIC = 2, CLS_LAYERED = 3, N_CLS = 4 };  // (wavefront.h: CLASS_*)
// The coordinates of render.hip's launcher table
enum : int { GEO_TRI, GEO_GEN, N_GEO };            // top-level triangles only / spheres, bilinear patches or instances too
enum : int { IMG_NONE, IMG_TEX, IMG_ENV, N_IMG };  // no image / image textures (ray differentials, MIP filtering) / an ImageInfinitelight alone (the K_ENV_LIGHT units)
// the pixel filter's class: box (and every filter under options.disable_pixel_jitter: k_generate, k_film) / triangle / tabulated with a constant weight (gaussian) /
// tabulated with a signed one (Mitchell, sinc)
enum : int { FLT_BOX, FLT_TRIANGLE, FLT_TABULATED, FLT_TABULATED_SIGNED, N_FLT };
enum : int { ROUTE_LEAN, ROUTE_STAGED, ROUTE_SIMPLE, ROUTE_RANDOM_WALK,
              ROUTE_AO };  // PBRT-v4's ambient occlusion integrator: k_shade_ao (k_ao.hip) in a vertex's place, and the bounce loop runs once whatever max_depth says
constexpr int NEVER = 1 << 30;  // a bounce no render reaches (max_depth <= 254)
// The table's null cells, by image class: the textured classes have no lean kernel (direct or diverted) and no k_generate<., LEAN>. serving_build and has_generate_build
// (below) go by it.
constexpr bool HAS_LEAN_KERNELS[N_IMG] = {true, false, true};
// The shading launchers by family (wavefront.h: wf_shade<FAMILY, GEO, IMG, ZS, DL>), and the ONE rule for which build of a family serves a cell of the table. A build
// goes by the coordinates of the cell it was written for; a family with fewer builds than cells has some of them serve several:
//   LEAN, LEAN_DIVERTED      k_shade<lean>, over the whole queue / over q_lean: a build per cell that has lean kernels, none for the textured class
//   FUSED_ALL                the material-sorted fused all-materials kernel: a build per cell
//   VERTEX, SCATTER + class  staged shading (SCATTER_LAYERED: the dense per-wave stages): a build per geometry without textures and under an environment map; ONE textured
//                            build, <TRI_ONLY = false, HAS_TEX = true>, for both geometries: (GEN, TEX)
//   SCATTER_LAYERED_ONEPASS  the LayeredBxDF class in one pass per vertex: as above, but no K_ENV_LIGHT build — it runs under options.force_diffuse, where the image
//                            class is never env (render_plan, below): the env cells get the build without the light
//   SIMPLE, RANDOMWALK       the other integrators: one build of every material and shape kind for every cell, filed under (GEN, TEX)
// 44 builds in all (tests/test_render_plan.py counts them); render.hip computes its table from this function and a build that is missing fails the link.
enum : int { FAM_LEAN, FAM_LEAN_DIVERTED, FAM_FUSED_ALL, FAM_VERTEX, FAM_SCATTER, FAM_SCATTER_DIFFUSE = FAM_SCATTER + CLS_DIFFUSE, FAM_SCATTER_CONDUCTOR = FAM_SCATTER + CLS_CONDUCTOR,
              FAM_SCATTER_DIELECTRIC = FAM_SCATTER + CLS_DIELECTRIC, FAM_SCATTER_LAYERED = FAM_SCATTER + CLS_LAYERED, FAM_SCATTER_LAYERED_ONEPASS, FAM_SIMPLE, FAM_RANDOMWALK, N_FAM };
constexpr int scatter_class(int family) { return family == FAM_SCATTER_LAYERED_ONEPASS ? CLS_LAYERED : family - FAM_SCATTER; }  // the queue a SCATTER family works through
struct ShadeBuild { int geo, img; };
constexpr ShadeBuild NO_BUILD = {-1, -1};
constexpr bool has_build(const ShadeBuild& b) { return b.geo >= 0; }
constexpr ShadeBuild serving_build(int family, int geo, int img) {
    if (family == FAM_LEAN || family == FAM_LEAN_DIVERTED) return HAS_LEAN_KERNELS[img] ? ShadeBuild{geo, img} : NO_BUILD;
    if (family == FAM_FUSED_ALL) return {geo, img};
    if (family == FAM_SIMPLE || family == FAM_RANDOMWALK) return {GEO_GEN, IMG_TEX};
    if (img == IMG_TEX) return {GEO_GEN, IMG_TEX};
    return {geo, family == FAM_SCATTER_LAYERED_ONEPASS ? IMG_NONE : img};
}
// K1 and K6 by the plan's coordinates: the one rule behind k_generate.inl's table (wf_generate) and render.hip's launch_film.
//   the filter class K1 is compiled for (shm/filter.h): both tabulated classes of the plan run the one tabulated kernel — the sign rides in the weight it leaves
constexpr int generate_filter_class(int flt) { return flt == FLT_BOX ? shm::FILTER_CLASS_BOX : (flt == FLT_TRIANGLE ? shm::FILTER_CLASS_TRIANGLE : shm::FILTER_CLASS_TABULATED); }
//   where K6 takes a sample's weight from: it is 1 (box, triangle) / the one constant K that heads the scene's table (gaussian) / +-K per path slot, as K1 left it (Mitchell, sinc)
enum : int { FILM_WEIGHT_ONE, FILM_WEIGHT_CONSTANT, FILM_WEIGHT_PER_SAMPLE };
constexpr int film_weight(int flt) { return flt == FLT_TABULATED ? FILM_WEIGHT_CONSTANT : (flt == FLT_TABULATED_SIGNED ? FILM_WEIGHT_PER_SAMPLE : FILM_WEIGHT_ONE); }
//   which K1 builds exist, per camera, sampler and filter class: <HAS_TEX, LEAN> unless LEAN in a class without lean kernels — 3 x 3 filter classes = 9, 36 in all
constexpr bool has_generate_build(bool tex, bool lean) { return !lean || HAS_LEAN_KERNELS[tex ? IMG_TEX : IMG_NONE]; }

// What flatten_scene found, as far as a decision reads it
struct SceneFacts {
    bool has_class[N_CLS] = {false, false, false, false};
    bool diffuse_only = true, has_material_textures = false, has_image_light = false, has_spheres = false, has_instances = false;
    bool extended = false;         // a distant or spot light, a diffuse transmission material or a disk / cylinder: the *_dl builds (wavefront.h, K_DELTA_LIGHTS) and no others
    bool has_quadric_kinds = false;  // a disk or a cylinder (ShmSphere::quadric): the traversal kernels of k_trace_quadrics.hip (and `extended`: the shading kernels that know the shapes)
    bool has_alpha = false;          // a shape with an alpha texture (shm/alpha.h): the traversal kernels of k_trace_alpha.hip (its alpha-tested triangles count as non-triangle records
                                     // in has_spheres and patch_heavy: flatten.h)
    bool has_plain_diffuse = false, plain_quarter = false;  // primitives on a plain DiffuseMaterial: any / a quarter or more by count or by surface area
    bool patch_heavy = false, has_quadric_patch = false;    // spheres / bilinear patches: a twelfth of the primitive records or more / any
    bool small_tree = false, has_prims = false;             // fewer than 4096 BVH nodes / any primitive record
    uint32_t filter = SHM_FILTER_BOX;
    bool spherical_camera = false;  // PBRT-v4's spherical camera: K1 is k_generate_spherical.hip's; nothing else depends on it
    int max_leaf_depth = 0;         // the deepest leaf of the BVH (root = 0; below 64, flatten.h): bounds the traversal stack
};
inline SceneFacts scene_facts(const shm_host::FlatScene& f) {
    SceneFacts s;
    for (int c = 0; c < N_CLS; ++c) s.has_class[c] = f.has_class[c];
    s.diffuse_only = f.diffuse_only; s.has_material_textures = f.has_material_textures; s.has_image_light = f.has_image_light;
    s.has_spheres = f.has_spheres; s.has_instances = f.has_instances;
    s.has_quadric_kinds = f.has_quadric_kinds;
    s.has_alpha = f.has_alpha;
    s.extended = f.has_directed_lights || f.has_diffuse_transmission || f.has_quadric_kinds;
    s.has_plain_diffuse = f.n_plain_diffuse_prims > 0;
    // (round 6: ... or a quarter of the SURFACE AREA — hits fall by area, not by count: a textured 4.3 M-triangle object in a plain room of 14 triangles sent every wall and
    //  floor hit through the textured class: 2 796 -> 3 127 Mray/s with the pass, profiles/r06_textured_object.txt)
    s.plain_quarter = f.n_plain_diffuse_prims * 4ull >= (uint64_t)f.prim_recs.size() || (f.n_plain_diffuse_prims > 0 && f.area_plain_diffuse * 4.0 >= f.area_total);
    s.patch_heavy = f.n_quadric_patch_prims * 12ull >= (uint64_t)f.prim_recs.size();
    s.has_quadric_patch = f.n_quadric_patch_prims != 0;
    s.small_tree = f.nodes.size() < 4096;
    s.has_prims = !f.prim_recs.empty();
    s.filter = f.film.filter;
    s.spherical_camera = f.camera.kind == SHM_CAMERA_SPHERICAL;
    s.max_leaf_depth = (int)f.max_leaf_depth;
    return s;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------------------
// The traversal kernels (k_trace.hip): ONE row per scene variant and ray kind — what the kernel is compiled with (waves per SIMD, the stack levels its LDS holds, the
// five-wave builds' LDS save area) and, from the same row, what the scene allocates for it (the persistent grid, the HBM stack spill). A sweep edits a row;
// tests/test_render_plan.py holds every row to the CU's LDS and every scene's stack to its tree.
//   TRI        top-level triangles only. Closest hit at eight waves; any hit at seven (r04 sweep: 8 waves x 9 levels 65.5 ms of any-hit launches per headline frame,
//              7 waves x 11 levels 62.8). S3: 98.5 % of the pushes land below level 9, 99.95 % below 12 (tools/sim/run_pair_sim.py); the rest goes to the HBM spill.
//   GEN        spheres, bilinear patches or instances too: the direction, the instance slot and the parked round's live values take the closest-hit kernel past the 64
//              registers of eight waves; seven waves (<= 72 VGPRs) cost the triangle kernel under 1 % (r04 sweep: 98.0 -> 98.7 ms).
//   GEN_HEAVY  the same body at five waves, for scenes where the non-triangle tests are the RULE (ScenePlan::gen_heavy; the measurements: k_trace.hip, at the kernels):
//              the five-wave share of 15 levels less the six levels' worth (12 KiB) of the save area around a quadric / patch test (trace5_body<SAVE_LDS>).
// A workgroup is four waves, one per SIMD: `waves` per SIMD is also workgroups per CU.
// ---------------------------------------------------------------------------------------------------------------------------------------------------------------
enum : int { TRACE_TRI, TRACE_GEN, TRACE_GEN_HEAVY, N_TRACE };
enum : int { RAY_CLOSEST, RAY_ANY, N_RAY };
struct TraceShape { int waves, lds_levels, lds_save_bytes; };
constexpr TraceShape TRACE_SHAPES[N_TRACE][N_RAY] = {
    {{8, 9, 0}, {7, 11, 0}},
    {{7, 11, 0}, {7, 11, 0}},
    {{5, 15 - 6, 12 << 10}, {5, 15 - 6, 12 << 10}},
};
constexpr int TRACE_LDS_LEVEL_BYTES = 256 * 8;  // one stack level of a workgroup: 256 lanes x an 8-byte entry
constexpr int trace_lds_bytes(const TraceShape& k) { return k.lds_levels * TRACE_LDS_LEVEL_BYTES + k.lds_save_bytes; }  // per workgroup
// ShmRenderParams::disable_reference_quirks in a scene with instances: the any-hit kernels' STRICT pair (k_trace5_any_strict) — the general any-hit row, five waves for
// a GEN_HEAVY scene and seven for every other. It runs on the grid and the spill of the scene's own any-hit row: the two must agree (the plan test holds them to it).
constexpr int trace_strict_variant(int variant) { return variant == TRACE_GEN_HEAVY ? TRACE_GEN_HEAVY : TRACE_GEN; }

// Tuning knobs (development): defaults are the measured optimum on S3. -1 / 0: not set.
struct Knobs {
    int split_pass = -1, gen_heavy = -1, tri_shade = -1;  // SHM_SPLIT_PASS, SHM_GEN_HEAVY, SHM_TRI_SHADE: 0 / 1
    int shade_prefetch = -1;                              // SHM_SHADE_PREFETCH: 0 / 1
    int tail_fused_bounce = 0;                            // SHM_TAIL_FUSED_BOUNCE (negative = never)
    int trace_rays_per_lane = -1;                         // SHM_TRACE_RAYS_PER_LANE, 0 .. 4096
    int refill_min = 0, refill_min_any = 0, leaf_min = 0, leaf_min_any = 0, other_min = 0, other_min_any = 0;  // SHM_REFILL_MIN .. SHM_OTHER_MIN_ANY, 1 .. 64
    uint64_t overlap_paths = 96ull << 20;                 // SHM_OVERLAP_PATHS (0 = never)
};
inline Knobs read_knobs() {
    Knobs k;
    auto flag = [](const char* name, int& out) { if (const char* e = getenv(name)) out = atoi(e) != 0 ? 1 : 0; };
    auto lanes = [](const char* name, int& out) { if (const char* e = getenv(name)) { const int v = atoi(e); if (v >= 1 && v <= 64) out = v; } };
    flag("SHM_SPLIT_PASS", k.split_pass); flag("SHM_GEN_HEAVY", k.gen_heavy); flag("SHM_TRI_SHADE", k.tri_shade);
    flag("SHM_SHADE_PREFETCH", k.shade_prefetch);
    if (const char* e = getenv("SHM_TAIL_FUSED_BOUNCE")) { const int v = atoi(e); k.tail_fused_bounce = v >= 0 ? v : NEVER; }
    if (const char* e = getenv("SHM_TRACE_RAYS_PER_LANE")) { const int v = atoi(e); if (v >= 0 && v <= 4096) k.trace_rays_per_lane = v; }
    lanes("SHM_REFILL_MIN", k.refill_min); lanes("SHM_REFILL_MIN_ANY", k.refill_min_any); lanes("SHM_LEAF_MIN", k.leaf_min); lanes("SHM_LEAF_MIN_ANY", k.leaf_min_any);
    lanes("SHM_OTHER_MIN", k.other_min); lanes("SHM_OTHER_MIN_ANY", k.other_min_any);
    if (const char* e = getenv("SHM_OVERLAP_PATHS")) { const long long v = atoll(e); if (v >= 0) k.overlap_paths = (uint64_t)v; }
    return k;
}

struct ScenePlan {
    SceneFacts f;
    // the scene's classes
    bool env_plain = false;  // the scene's only image is an environment map: no path-integrator render of it reaches a HAS_TEX kernel unless options.force_diffuse asks for
                             // that code — and even there the differentials are dead values (no material binds a texture), so it never holds auxiliary-ray arrays
    bool lean = false;       // all-diffuse without material textures: k_shade<lean> shades every vertex (measured through the staged pipeline: shade + generate + film
                             // 130 -> 165 ms per headline frame)
    bool tex_ws = false;     // material textures: the auxiliary-ray arrays and k_generate<true>
    int n_classes = 0;
    // the pipeline
    bool split_pass = false;   // scenes with material textures: k_split_plain in front of the textured k_vertex where a quarter of the primitives, or of the surface, carry a
                               // plain DiffuseMaterial (the textured Cornell box, whose only plain material is its emitter's, would pay a pass per bounce for a handful of hits).
                               // (without textures k_vertex diverts such hits itself — its triangle instantiation runs three waves per SIMD; the pass as a kernel of its own in
                               //  front of it, forced with SHM_SPLIT_PASS=1, changes nothing there: coated S3 3 258-3 284 Mray/s either way)
    bool lean_divert = false;  // hits on plain diffuse materials BESIDE other classes go to q_lean and the lean fused kernel: diverted by k_vertex, or by the split pass
    int tail_fused_bounce = 0; // scenes without a coated material: ONE fused all-materials launch per bounce from this bounce on, its chunks sorted by material
    bool fused_from_0 = false; // ... from the camera ray on, whatever the render (k_shade_tail*.hip, k_shade_fused_*.hip)
    bool first_bounce = false; // a render's bounce 0 may run on known constants (k_generate<., LEAN>, ShadeArgs::first_bounce): the workspace holds rng0 / pixel0
    bool lean_kernel = false;  // k_shade<lean> runs, direct or diverted: the workspace holds the deferred emitter hits (PathArrays::e_*, q_emit)
    bool tri_shade = false, tri_shade_plain_only = false;  // build the flat triangles' shading records (shm/tri_shade.h) / of plain DiffuseMaterials only
    bool shade_prefetch = true;  // k_shade<lean> fetches the next vertex's queue entry and hit record while it shades this one (k_shade.inl, K_SHADE_PREFETCH); SHM_SHADE_PREFETCH=0:
                                 // the same kernel loads them where it needs them (the A/B instrument: films and counters cannot differ)
    // the traversal kernels (k_trace.hip)
    int trace_variant = TRACE_TRI;         // the row of TRACE_SHAPES (and of k_trace.hip's kernel table) this scene's rays take
    int trace_spill_levels[N_RAY] = {1, 1};  // stack levels in the per-lane HBM spill: what the tree's depth needs beyond the row's LDS levels, and one more
    bool gen_heavy = false;    // the five-wave instantiations for scenes where spheres / patches are a twelfth of the primitive records or more (TRACE_GEN_HEAVY; S3 with
                               // 100 / 50 / 25 / 10 % of the object's cells as patches, five against seven waves: +73 / +38 / +13 / 0 %, with ONE patch in 4.3 M triangles -7 %)
    // idle lanes before a traversal wave refills: the kernels set a ray up with the root test and six IEEE divisions (200 VALU instructions), so that fewer, fuller refills
    // win although a quarter of the lanes idle (r04 sweep on the headline frame, closest / any ms: 24: 97.4 / 62.3, 40: 96.5 / 60.9, 48: 102.1 / 63.5, 56: 119.1 / 78.1)
    int refill_min = 40, refill_min_any = 40;
    int leaf_min = 16, leaf_min_any = 8;    // lanes with a pending leaf before the triangle phase runs (closest / any hit)
    int other_min = 16, other_min_any = 16; // the parked non-triangle tests a wave collects before it runs them
    int trace_rays_per_lane = 4;  // a traversal launch uses as much of its persistent grid as gives each resident lane about this many rays (0 = always the whole grid).
                                  // profiles/r03_trace_rays_per_lane_sweep.txt: C2 16.8 / 16.1 / 15.8 / 15.8 / 16.5 ms at 0 / 4 / 8 / 16 / 32, C4's K2 276.7 / 276.8 / 282 / 307 / 362
    uint64_t overlap_paths = 96ull << 20;  // batches below this many paths run K3(b) beside K2(b+1) (0 = never)
};
inline ScenePlan scene_plan(const SceneFacts& f, const Knobs& k) {
    ScenePlan p;
    p.f = f;
    const bool has_textures = f.has_material_textures || f.has_image_light;
    p.env_plain = f.has_image_light && !f.has_material_textures;
    p.lean = f.diffuse_only && !f.has_material_textures;
    p.tex_ws = f.has_material_textures;
    for (int c = 0; c < N_CLS; ++c) p.n_classes += f.has_class[c] ? 1 : 0;
    p.split_pass = k.split_pass >= 0 ? (k.split_pass != 0 && !p.lean && f.has_plain_diffuse) : (f.has_material_textures && !p.lean && f.plain_quarter);
    p.lean_divert = ((!has_textures || p.env_plain) && f.has_class[CLS_DIFFUSE] && !p.lean) || p.split_pass;
    p.tail_fused_bounce = k.tail_fused_bounce;
    p.fused_from_0 = !f.has_class[CLS_LAYERED] && p.tail_fused_bounce == 0;
    p.first_bounce = p.lean || (!f.has_material_textures && p.fused_from_0);
    p.lean_kernel = p.lean || p.lean_divert;
    // the shading records, for the triangle scenes in which a kernel that reads them shades vertices:
    //   k_shade<lean> without an environment map — all-diffuse scenes, the lean diversion of scenes with coated materials (or of any mixed scene whose early bounces are
    //   staged, SHM_TAIL_FUSED_BOUNCE), and, in scenes with material textures, behind the split pass: there only hits on plain DiffuseMaterials reach the kernel, and only
    //   those primitives get a record;
    //   the staged k_vertex of scenes without textures.
    // SHM_TRI_SHADE=0 builds none: every hit takes the fallback of the same kernels (the A/B instrument of the record path)
    const bool lean_reads = !f.has_image_light && (p.lean || (p.lean_divert && (p.split_pass || !p.fused_from_0)));
    const bool vertex_reads = !f.has_material_textures && !p.lean && !p.fused_from_0;
    p.tri_shade = !f.has_spheres && f.has_prims && (lean_reads || vertex_reads) && k.tri_shade != 0;
    p.tri_shade_plain_only = f.has_material_textures;
    p.shade_prefetch = k.shade_prefetch != 0;
    // a shallow tree means short rays, and short rays want fewer, fuller waves (C2's 63-node box: 15.5 -> 15.1 ms per frame at 8 rays per lane); a deep
    // tree means long dependent chains per ray, which want every wave the device has (C4: 8 costs 2 %)
    p.trace_rays_per_lane = k.trace_rays_per_lane >= 0 ? k.trace_rays_per_lane : (f.small_tree ? 8 : 4);
    p.gen_heavy = f.has_spheres && (k.gen_heavy >= 0 ? k.gen_heavy != 0 : f.patch_heavy);
    p.trace_variant = !f.has_spheres ? TRACE_TRI : (p.gen_heavy ? TRACE_GEN_HEAVY : TRACE_GEN);
    for (int r = 0; r < N_RAY; ++r) {
        const int beyond_lds = f.max_leaf_depth + 1 - TRACE_SHAPES[p.trace_variant][r].lds_levels;
        p.trace_spill_levels[r] = (beyond_lds > 0 ? beyond_lds : 0) + 1;
    }
    // at five waves a refill is cheaper to make early (24 idle lanes: S3 as patches 3 506 -> 3 685 Mray/s; profiles/r06_patch_heavy_scenes.txt)
    p.refill_min = k.refill_min ? k.refill_min : (p.gen_heavy ? 24 : 40);
    p.refill_min_any = k.refill_min_any ? k.refill_min_any : p.refill_min;
    if (k.leaf_min) p.leaf_min = k.leaf_min;
    if (k.leaf_min_any) p.leaf_min_any = k.leaf_min_any;
    // parked rounds of a scene whose only non-triangles are instances are ray set-ups in another space (~450 instructions): worth waiting for 32 lanes (S3 instanced
    // 4 263 -> 4 354, its object as 4 x 4 x 4 instances 2 703 -> 2 839 Mray/s; with spheres / patches 16 stays ahead: profiles/r06_instance_grid.txt)
    p.other_min = k.other_min ? k.other_min : ((f.has_instances && !f.has_quadric_patch) ? 32 : 16);
    p.other_min_any = k.other_min_any ? k.other_min_any : p.other_min;
    p.overlap_paths = k.overlap_paths;
    return p;
}

struct RenderPlan {
    int route = ROUTE_LEAN;  // what shades a vertex: k_shade<lean> alone / the staged pipeline (k_vertex -> k_scatter<class>, or the fused all-materials kernel) / the other integrators
                             // (ROUTE_AO, like them: 32-byte hit records, K1's full record, no known-constants bounce 0; of the coordinates below it reads zs, flt and spherical)
    bool lean_first = false; // bounce 0 on known constants: k_generate<., LEAN> wrote no record and no identity queue
    // the render's hit records: 16 bytes {primitive, b0, b1, b2} where every kernel that reads them takes that form (triangle and textured scenes; with spheres / patches the
    // split form, a second record with t and phi — not with instances: a hit inside one names it in the 32-byte record); kept: double-buffered by bounce parity
    bool hit16 = false, hit_split = false, hit_kept = false;
    bool trace_any_strict = false;  // the shadow rays take the any-hit kernels' STRICT pair: PBRT-v4's way into an instance (k_trace.hip)
    int fused_from = NEVER;        // the first bounce the fused all-materials kernel shades (staged route)
    bool split = false;            // k_split_plain runs in front of k_vertex: plain-diffuse hits -> q_lean, the rest -> q_split
    bool divert_vertex = false;    // k_vertex itself diverts plain-diffuse hits to q_lean (ShadeArgs::q_divert)
    bool drain_lean = false;       // the diverted lean kernel works q_lean off: exactly where one of the two above fills it
    bool layered_onepass = false;  // the LayeredBxDF class in one pass per vertex (options.force_diffuse replaces the BxDF inside that kernel's code)
    // table coordinates
    int geo = GEO_TRI, img = IMG_NONE, img_lean = IMG_NONE, img_generate = IMG_NONE, flt = FLT_BOX;
    bool zs = false, dl = false;
    bool spherical = false;        // K1's launcher is k_generate_spherical.hip's, wf_generate<true>: the same cells (HAS_TEX x LEAN x sampler x filter class)
    bool film_per_sample = false;  // k_film_weighted reads the per-path weights k_generate_filtered left
    // overlap policy
    uint64_t overlap_paths = 0;       // a batch below this many paths runs K3(b) beside K2(b+1) and the class scatter kernels beside each other ...
    bool mixed_lean_layered = false;  // ... and every batch of a render shaded by the diverted lean kernel AND the LayeredBxDF scatter kernel
    int late_overlap_bounce = NEVER;  // ... and, whatever the batch, every bounce from this one on
    bool group_big = false;           // the scatter group goes to the side streams at any batch size (the diverted lean kernel beside the LayeredBxDF one)
    bool staged_bounce(int bounce) const { return route == ROUTE_STAGED && bounce < fused_from; }
    bool overlap_batch(uint64_t total) const { return overlap_paths > 0 && (total < overlap_paths || mixed_lean_layered); }
};
inline RenderPlan render_plan(const ScenePlan& s, const ShmRenderParams& o) {
    const SceneFacts& f = s.f;
    RenderPlan p;
    const bool path = o.integrator == SHM_INTEGRATOR_PATH, fd = o.force_diffuse != 0, layered = f.has_class[CLS_LAYERED];
    // staged shading: everything but the lean class, which keeps the fused kernel (one BxDF class: nothing to sort, and the parameter block would be pure traffic);
    // options.force_diffuse always takes the staged path
    p.route = !path ? (o.integrator == SHM_INTEGRATOR_RANDOM_WALK ? ROUTE_RANDOM_WALK : (o.integrator == SHM_INTEGRATOR_AMBIENT_OCCLUSION ? ROUTE_AO : ROUTE_SIMPLE))
                    : ((!s.lean || fd) ? ROUTE_STAGED : ROUTE_LEAN);
    const bool staged = p.route == ROUTE_STAGED;
    p.lean_first = path && !fd && s.first_bounce;
    p.hit16 = path && (!f.has_spheres || !f.has_instances);
    p.hit_split = p.hit16 && f.has_spheres;
    p.hit_kept = p.route == ROUTE_LEAN && p.hit16 && !f.has_spheres;  // (the split form keeps its second records in the other half)
    p.trace_any_strict = f.has_instances && o.disable_reference_quirks != 0;
    // a scene with several BxDF classes but without coated materials: ONE fused all-materials launch per bounce instead of the staged four or five, from bounce
    // `tail_fused_bounce` on. Rounds 3-4, chunks unsorted: only the late bounces paid (C4 frame 522-528 ms staged throughout, 510-512 from bounce 6, 511-513 from 8).
    // Round 5, chunks counting-sorted by material (k_shade_tail_sorted.hip): the earlier the better — C4 403.2 ms from bounce 8, 399 from 4, 388 from 2, 378 from 1,
    // 365 from 0: the default.
    // (with material textures: where there is more than one BxDF class to sort — one class: the fused textured kernel's 128 spilled VGPRs cost more than the staged pair's
    //  parameter block — and no split pass takes most hits away from the textured kernels; an environment map alone is no texture)
    const bool fused_tex_ok = !s.split_pass && s.n_classes > 1;
    if (staged && !layered && !fd && (!f.has_material_textures || fused_tex_ok)) p.fused_from = s.tail_fused_bounce;
    p.split = staged && s.split_pass && !fd;
    p.drain_lean = staged && s.lean_divert && !fd;
    p.divert_vertex = p.drain_lean && !p.split;
    p.layered_onepass = fd;
    p.geo = f.has_spheres ? GEO_GEN : GEO_TRI;
    // The staged and the all-materials fused kernels: env where the only image is an environment map and options.force_diffuse is off, tex where the scene has
    // textures, none otherwise — under force_diffuse an env-only scene runs the textured units (the differentials are dead values there: no material binds a texture).
    p.img = (s.env_plain && !fd) ? IMG_ENV : ((f.has_material_textures || f.has_image_light) ? IMG_TEX : IMG_NONE);
    // The lean kernels, direct or diverted: env exactly where the scene has an image light — also in a textured scene behind the split pass, whose k_vertex runs the
    // textured class (the lean kernel takes the hits on plain DiffuseMaterials, and nothing filters a texture there).
    p.img_lean = f.has_image_light ? IMG_ENV : IMG_NONE;
    // (k_generate writes the camera rays' auxiliary rays where the workspace holds them — under force_diffuse an env-only scene has none)
    p.img_generate = s.tex_ws ? IMG_TEX : IMG_NONE;
    p.zs = o.sampler == SHM_SAMPLER_ZSOBOL;
    // (the *_dl builds for a scene with a distant or spot light, a diffuse transmission material or a disk / cylinder, in every class: a kernel built without them would
    //  sample the lights as area lights, shade the material as a CoatedConductor and the shapes as spheres. This is the only place the set is chosen.)
    p.dl = f.extended;
    // (the generate kernels that know PBRT-v4's spherical camera, for a scene whose camera is one and for no other: every other kernel would read it as a perspective camera)
    p.spherical = f.spherical_camera;
    // the pixel filter: box — and every filter under options.disable_pixel_jitter, where the film point is the pixel centre and the weight 1 whatever was drawn — runs
    // k_generate and k_film; the others their own K1 / K6 pair
    if (f.filter != SHM_FILTER_BOX && o.disable_pixel_jitter == 0)
        p.flt = f.filter == SHM_FILTER_TRIANGLE ? FLT_TRIANGLE : (shm::filter_weight_is_signed(f.filter) ? FLT_TABULATED_SIGNED : FLT_TABULATED);
    p.film_per_sample = film_weight(p.flt) == FILM_WEIGHT_PER_SAMPLE;
    // Small batches are tail-dominated (the last rays of a persistent traversal launch take ~0.5 ms whatever its size): there K3 of bounce b runs on a second stream
    // beside K2 of bounce b+1 and the next shade launch waits for both. Large batches (the 1-GPU headline frame) keep everything on one stream.
    // (a scene shaded by the diverted fused kernel AND the LayeredBxDF scatter kernel runs in this mode at any batch size: its any-hit share is large and its
    //  two shading kernels are bound differently — coated S3 at 256 spp 447 -> 437.5 ms; the headline frame is indifferent, C4 loses 1 %)
    p.group_big = p.drain_lean && layered;
    if (o.max_depth > 0) { p.overlap_paths = s.overlap_paths; p.mixed_lean_layered = p.group_big; }
    // ... and, whatever the batch size, the LATE bounces of a deep render: from bounce 6 on the queues hold a few percent of the paths (C4: 7 % at bounce 6, 1 % at 12)
    // and every launch is a tail (profiles/r03_c4_per_bounce.txt). C4 frame 541 -> 522 ms at 6 (524-528 at 10, 528-534 at 16, 530 at 4)
    if (s.overlap_paths > 0) p.late_overlap_bounce = 6;
    return p;
}
// What must hold of a plan before its first launch: the extended set for exactly the scenes that need it, and no coordinate on a null cell of the table.
inline const char* render_plan_error(const ScenePlan& s, const RenderPlan& p) {
    if (p.dl != s.f.extended) return "internal: the kernel set does not match the scene's delta lights / materials";
    if (p.spherical != s.f.spherical_camera) return "internal: the generate kernels do not match the scene's camera";
    if ((p.route == ROUTE_LEAN || p.drain_lean) && !HAS_LEAN_KERNELS[p.img_lean]) return "internal: the plan calls a lean kernel of a textured class";
    if (p.lean_first && !has_generate_build(p.img_generate == IMG_TEX, true)) return "internal: the plan calls k_generate<HAS_TEX, LEAN>";
    return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------------------
// The path workspace: ONE list of the per-path arrays — X(id, where the pointer lives in ShmScene, bytes per path, needed when) — in allocation order. The budget
// (ws_bytes_per_path) is the sum over it and the allocation (render.hip, ensure_workspace) is the walk. `p` is the ScenePlan; `staged`: the workspace holds the staging
// arrays — every scene class but the lean one, and the lean one too once a render under options.force_diffuse has asked for them.
// ---------------------------------------------------------------------------------------------------------------------------------------------------------------
#define SHM_WS_ARRAYS(X)                                                                             \
    X(RAY, pa.ray, 32, true) X(HIT, pa.hit, 32, true) X(SHADOW_RAY, pa.shadow_ray, 32, true)         \
    X(SHADOW_CONTRIB, pa.shadow_contrib, 16, true) X(L, pa.L, 16, true) X(REC, pa.rec, 64, true)     \
    X(LAMBDA, pa.lambda, 16, true) X(LAMBDA_PDF, pa.lambda_pdf, 16, true) X(CTX, pa.ctx, 64, true)   \
    X(RNG0, pa.rng0, 8, p.first_bounce) X(PIXEL0, pa.pixel0, 4, p.first_bounce)                      \
    X(E_RAY, pa.e_ray, 16, p.lean_kernel) X(E_BETA, pa.e_beta, 16, p.lean_kernel)                    \
    X(E_CTX0, pa.e_ctx0, 16, p.lean_kernel) X(E_CTX1, pa.e_ctx1, 16, p.lean_kernel)                  \
    X(E_CTX2, pa.e_ctx2, 16, p.lean_kernel) X(E_FLAGS, pa.e_flags, 4, p.lean_kernel)                 \
    X(Q_EMIT, d_q_emit, 4, p.lean_kernel)                                                            \
    /* a pixel filter with negative lobes: the sample's weight, from k_generate_filtered to k_film_weighted (outside PathArrays: no other kernel sees it) */ \
    X(FILTER_WEIGHT, d_filter_weight, 4, shm::filter_weight_is_signed(p.f.filter))                   \
    X(AUX0, pa.aux0, 16, p.tex_ws) X(AUX1, pa.aux1, 16, p.tex_ws) X(AUX2, pa.aux2, 16, p.tex_ws)    \
    /* the staging arrays: the parameter block, one BxRec per path; the differentials; the class queues; the lean diversion's and the split pass's queues */ \
    X(BX, pa.bx, 128, staged)                                                                        \
    X(DD0, pa.dd0, 16, staged && (p.f.has_material_textures || p.f.has_image_light))                 \
    X(DD1, pa.dd1, 16, staged && (p.f.has_material_textures || p.f.has_image_light))                 \
    X(DD2, pa.dd2, 16, staged && (p.f.has_material_textures || p.f.has_image_light))                 \
    X(Q_SCATTER0, d_q_scatter[0], 4, staged && p.f.has_class[0]) X(Q_SCATTER1, d_q_scatter[1], 4, staged && p.f.has_class[1]) \
    X(Q_SCATTER2, d_q_scatter[2], 4, staged && p.f.has_class[2]) X(Q_SCATTER3, d_q_scatter[3], 4, staged && p.f.has_class[3]) \
    X(Q_LEAN, d_q_lean, 4, staged && p.lean_divert) X(Q_SPLIT, d_q_split, 4, staged && p.split_pass) \
    X(Q_ACTIVE0, d_q_active[0], 4, true) X(Q_ACTIVE1, d_q_active[1], 4, true) X(Q_SHADOW, d_q_shadow, 4, true)
enum WsArray : int {
#define SHM_WS_ID(id, field, bytes, when) WS_##id,
    SHM_WS_ARRAYS(SHM_WS_ID)
#undef SHM_WS_ID
    N_WS_ARRAYS
};
inline uint64_t ws_bytes_per_path(const ScenePlan& p, bool staged) {
    uint64_t b = 0;
#define SHM_WS_SUM(id, field, bytes, when) if (when) b += bytes;
    SHM_WS_ARRAYS(SHM_WS_SUM)
#undef SHM_WS_SUM
    return b;
}
// (for the tests: the walk itself — bytes per path of every array, 0 where it is not allocated; names[] gets the identifiers)
inline void ws_layout(const ScenePlan& p, bool staged, uint32_t bytes_out[N_WS_ARRAYS], const char* names_out[N_WS_ARRAYS]) {
#define SHM_WS_ROW(id, field, bytes, when) bytes_out[WS_##id] = (when) ? bytes : 0u; if (names_out) names_out[WS_##id] = #id;
    SHM_WS_ARRAYS(SHM_WS_ROW)
#undef SHM_WS_ROW
}
// Every non-lean scene keeps the staging arrays whether or not the upcoming render uses them; the lean class gets them with its first staged render and keeps them.
inline bool ws_staged_layout(const ScenePlan& p, bool render_staged, bool ws_has_staged) { return render_staged || ws_has_staged || !p.lean; }

}  // namespace shm_plan
