// shm/tri_shade.h — the per-primitive shading record of a flat triangle (device only: SceneView::tri_shade; the oracle never sees one).
//
// For a top-level triangle whose mesh has neither per-vertex normals nor tangents, on a material that is no MixMaterial and binds neither a displacement texture nor a
// normal map, everything triangle_interaction (shapes.h) + get_bsdf<false> (path.h) leave in si.n, si.shading.n and bsdf.shading_frame is a function of the three vertices,
// the mesh's flags, the vertex uv and the material's constant displacement: dpdu / dpdv with their 1 / determinant, the degenerate-uv fallback, the normal, the
// reference's constant-displacement bump map, set_shading_geometry's rescale loop and bsdf_new's frame — 3 square roots and 11 IEEE divisions per vertex, none of which
// depends on the barycentrics, wo, the wavelengths or the path. A scene is immutable after shm_scene_create, so the record is built there once (render.hip,
// k_build_tri_shade) by running that very pair and storing its output: no formula is restated here. What stays per vertex is p_hit / p_error and the material's BxDF parameters.
#pragma once
#include "path.h"

namespace shm {

struct alignas(16) TriShadeRec {  // 48 bytes: n | frame x | frame y | frame z (z is the final shading normal)
    float4 a, b, c;
};
static_assert(sizeof(TriShadeRec) == 48, "TriShadeRec is three 16-byte loads");

// PrimRec::pad[1] of the DEVICE copy: non-zero where SceneView::tri_shade holds the slot's record (set by the kernel that builds it)
SHM_HD bool tri_shade_valid(const PrimRec& pr) { return pr.pad[1] != 0u; }

// Which primitives get a record. plain_only (scenes with material textures, where the record path only ever sees what the split pass sends to the lean kernel): only those on a
// DiffuseMaterial that binds no texture at all (ShmMaterial::pad[0] bit 0 of the device copy, flatten_scene)
SHM_HD bool tri_shade_eligible(const SceneView& sv, const PrimRec& pr, bool plain_only) {
    if (pr.kind_index & ~PRIM_INDEX_MASK) return false;  // sphere, patch, instance, or a degenerate triangle (never hit)
    if (sv.mesh_flags[pr.mesh] & (MESH_HAS_N | MESH_HAS_S)) return false;
    const ShmMaterial& m = sv.materials[pr.material];
    if (m.kind == SHM_MATERIAL_MIX) return false;  // (its choice hashes wo and p)
    if (plain_only && !(m.pad[0] & 1u)) return false;
    return m.float_tex[SHM_FLOATSLOT_DISPLACEMENT] == 0u && m.normal_map == 0u;
}

// The record of one eligible primitive: the existing pair's output for any barycentrics, any wo and any wavelengths. False — no record, the slot keeps the full
// interaction — for a triangle whose dpdu / dpdv are infinite (non-finite or overflowing vertices): set_shading_geometry's rescale loop does not end on those, and here
// it would run at scene creation, for a triangle no ray may ever hit.
SHM_HD bool tri_shade_record(const SceneView& sv, const PrimRec& pr, TriShadeRec& r) {
    TriangleIntersection ti;
    ti.b0 = 0.25f; ti.b1 = 0.25f; ti.b2 = 0.5f; ti.t = 1.0f;
    SurfaceInteraction si = triangle_interaction(load_triangle_rec(sv, pr), ti, v3(0.0f, 0.0f, 1.0f));
    for (int k = 0; k < 3; ++k)
        if (is_inf(si.shading.dpdu[k]) || is_inf(si.shading.dpdv[k])) return false;
    Wavelengths lambda = sample_visible(0.5f);
    const BSDF bsdf = get_bsdf<false>(sv, si, sv.materials[pr.material], lambda);
    const Frame& f = bsdf.shading_frame;
    r.a = make_float4(si.n.x, si.n.y, si.n.z, f.x.x);
    r.b = make_float4(f.x.y, f.x.z, f.y.x, f.y.y);
    r.c = make_float4(f.y.z, f.z.x, f.z.y, f.z.z);
    return true;
}

// The interaction of a hit on a primitive with a record: pi from p_hit / p_error as triangle_interaction computes them, n and shading.n from the record. The no-texture
// kernels read nothing else of it (uv and the derivatives only feed textures and ray differentials: zeros here).
SHM_HD SurfaceInteraction tri_shade_interaction(const PrimRec& pr, const TriShadeRec& r, const Hit& h, V3 wo) {
    const V3 p0 = ld3(pr.p0), p1 = ld3(pr.p1), p2 = ld3(pr.p2);
    V3 p_hit = h.b0 * p0 + h.b1 * p1 + h.b2 * p2;
    V3 p_abs_sum = abs3(h.b0 * p0) + abs3(h.b1 * p1) + abs3(h.b2 * p2);
    V3 p_error = gamma(7) * p_abs_sum;
    SurfaceInteraction si;
    si.pi = p3i_from_value_and_error(p_hit, p_error);
    si.wo = wo;
    si.n = v3(r.a.x, r.a.y, r.a.z);
    si.uv = v2(0.0f, 0.0f);
    si.dpdu = si.dpdv = si.dndu = si.dndv = v3s(0.0f);
    si.shading.n = v3(r.c.y, r.c.z, r.c.w);
    si.shading.dpdu = si.shading.dpdv = si.shading.dndu = si.shading.dndv = v3s(0.0f);
    return si;
}

SHM_HD Frame tri_shade_frame(const TriShadeRec& r) {
    Frame f;
    f.x = v3(r.a.w, r.b.x, r.b.y);
    f.y = v3(r.b.z, r.b.w, r.c.x);
    f.z = v3(r.c.y, r.c.z, r.c.w);
    return f;
}

// The BSDF of a vertex whose shading frame is known — the record's, or, for a hit without one, the frame get_bsdf built on the full interaction —: the BxDF parameters are
// get_bsdf's material half, run as it stands on an interaction that carries the vertex's wo and pi (what MixMaterial's choice hashes) and no geometry; nobody reads that
// interaction afterwards, so what get_bsdf does to its shading geometry is dead arithmetic.
// INVARIANT: this and tri_shade_fallback_frame below each keep HALF of an inlined get_bsdf and rely on the compiler deleting the other half (pure arithmetic and loads whose
// results nobody reads). It does: the division / square-root counts of the kernels that call them equal the parent's (profiles/tri_shade_records.md has the counts and the
// command). Check them again after any change to get_bsdf's inlining: kept alive, the dead halves would cost every vertex a second bump map.
SHM_HD BSDF tri_shade_bsdf(const SceneView& sv, const SurfaceInteraction& si, const Frame& frame, const ShmMaterial& m, Wavelengths& lambda) {
    SurfaceInteraction carrier;
    carrier.pi = si.pi;
    carrier.wo = si.wo;
    carrier.n = carrier.dpdu = carrier.dpdv = carrier.dndu = carrier.dndv = v3s(0.0f);
    carrier.uv = v2(0.0f, 0.0f);
    carrier.shading.n = carrier.shading.dpdu = carrier.shading.dpdv = carrier.shading.dndu = carrier.shading.dndv = v3s(0.0f);
    BSDF bsdf = get_bsdf<false>(sv, carrier, m, lambda);
    bsdf.shading_frame = frame;
    return bsdf;
}
// ... and the frame of a hit without a record: the full get_bsdf on the full interaction (which it updates, as ever); its material half is dead arithmetic here
SHM_HD Frame tri_shade_fallback_frame(const SceneView& sv, SurfaceInteraction& si, const ShmMaterial& m, const Wavelengths& lambda) {
    Wavelengths lw = lambda;
    return get_bsdf<false>(sv, si, m, lw).shading_frame;
}

}  // namespace shm
