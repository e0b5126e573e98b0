// shm/alpha.h — PBRT-v4's shape alpha (GeometricPrimitive::Intersect / IntersectP): a primitive may carry a float texture that cuts holes in it. One text for the
// device (the parked round of k_trace_alpha.hip's kernels, k_trace.inl) and the host (prim_intersect below: the oracle's two traversals accept a leaf primitive
// through it and nothing else).
//   After the shape test has accepted a candidate (t < t_max, as ever):  a = FloatTexture::evaluate(alpha, ctx);  a >= 1: accept;  a <= 0: reject;  otherwise
//   u = HashFloat(ray.o, ray.d), reject if u > a. A rejected candidate is a miss: t_max and the hit stay as they were. The any-hit predicate runs the same test
//   (PBRT-v4: IntersectP of an alpha primitive is Intersect(...).has_value()).
//   ctx: the candidate's p, uv and n from the interaction builders themselves (triangle_interaction, blp_interaction, sphere_interaction: the statements a material
//   texture on the same surface is evaluated with, so a cutout lines up with it bit for bit), every differential zero — PBRT-v4 evaluates alpha before a ray has any.
//   n is the GEOMETRIC normal: the builders run without the mesh's shading normals (which only a FloatDirectionMixTexture could see), so that the traversal kernel
//   gathers nothing but the uv of a mesh that has them. Everything else the builders compute is dead code here.
//   Where alpha lives (flatten.h): a triangle's in the low 28 bits of PrimRec::kind_index — the word the traversal's leaf phase reads anyway —, a bilinear patch's in
//   PatchExtra::alpha, a sphere / disk / cylinder's in its ShmSphere; 0 = none, else 1 + the index into SceneView::float_textures.
#pragma once
#include "bxdf.h"
#include "scene.h"
#include "texture.h"

namespace shm {

// HashFloat(ray.o, ray.d): ours to define (the LayeredBxDF seeds' hash, shm/bxdf.h); 24 bits convert exactly, so host and device agree. The six floats are the ray's AS
// THE TRAVERSAL HOLDS IT at the test: inside an instance, the instance-space ray
SHM_HD Float alpha_hash_float(V3 o, V3 d) {
    const uint64_t h = hash_v3(hash_v3(0ULL, o), d);
    return (Float)(uint32_t)(h >> 40) * 0x1p-24f;
}

// the alpha texture of a record: 0 = none, else 1 + its index
SHM_HD uint32_t prim_alpha(const SceneView& sv, const PrimRec& pr) {
    const uint32_t k = pr.kind_index;
    if (k & PRIM_SPHERE_BIT) return sv.spheres[k & PRIM_INDEX_MASK].alpha;
    if (k & PRIM_PATCH_BIT) return sv.patches[k & PRIM_INDEX_MASK].alpha;
    if (k & PRIM_INSTANCE_BIT) return 0u;
    return k & PRIM_INDEX_MASK;
}

// TextureEvalContext of a candidate hit `h` (prim_intersect's record: barycentrics | (u, v) | p_obj + phi) on the record `pr`
SHM_HD TextureEvalContext alpha_context(const SceneView& sv, const PrimRec& pr, const Hit& h) {
    const V3 wo = v3s(0.0f);  // (no statement that p, uv or n depend on reads it)
    SurfaceInteraction si;
    if (pr.kind_index & PRIM_SPHERE_BIT) {
        QuadricIntersection qi;
        qi.t_hit = h.t; qi.p_obj = v3(h.b0, h.b1, h.b2); qi.phi = h.phi;
        si = sphere_interaction(sv.spheres[pr.kind_index & PRIM_INDEX_MASK], qi, wo, sv.quirks_off != 0);
    } else if (pr.kind_index & PRIM_PATCH_BIT) {
        PatchData pd = load_patch_rec(sv, pr);
        pd.has_n = false;
        si = blp_interaction(pd, h.b0, h.b1, wo);
    } else {
        TriangleData tr = load_triangle_rec(sv, pr);
        tr.has_n = tr.has_s = false;
        TriangleIntersection ti;
        ti.b0 = h.b0; ti.b1 = h.b1; ti.b2 = h.b2; ti.t = h.t;
        si = triangle_interaction(tr, ti, wo);
    }
    TextureEvalContext c;
    c.p = si.p(); c.n = si.n; c.uv = si.uv;
    c.dpdx = c.dpdy = v3s(0.0f);
    c.dudx = c.dudy = c.dvdx = c.dvdy = 0.0f;
    return c;
}

// the test itself: true = the candidate stands. `alpha` != 0; (ro, rd): the ray the shape test ran with
SHM_HD bool alpha_accept(const SceneView& sv, const PrimRec& pr, uint32_t alpha, const Hit& h, V3 ro, V3 rd) {
    const Float a = float_texture_evaluate(sv, alpha - 1u, alpha_context(sv, pr, h));
    if (a >= 1.0f) return true;
    if (a <= 0.0f) return false;
    return !(alpha_hash_float(ro, rd) > a);
}

// Primitive::intersect for one leaf-order slot (primitive.rs:95-103 -> shape/shape.rs:164-170), with PBRT-v4's alpha test behind the shape's.
// Updates hit/t_max on acceptance exactly as aggregate.rs:101-110 does.
SHM_HD bool prim_intersect(const SceneView& sv, uint32_t slot, V3 ro, V3 rd, Float t_max, Hit& h) {
    const PrimRec& pr = sv.prim_recs[slot];
    Hit c;
    c.prim = (int32_t)slot;
    if (pr.kind_index & PRIM_SPHERE_BIT) {
        QuadricIntersection qi;
        if (!sphere_basic_intersect(sv.spheres[pr.kind_index & PRIM_INDEX_MASK], ro, rd, t_max, qi)) return false;
        c.t = qi.t_hit; c.b0 = qi.p_obj.x; c.b1 = qi.p_obj.y; c.b2 = qi.p_obj.z; c.phi = qi.phi;
    } else if (pr.kind_index & PRIM_PATCH_BIT) {
        BilinearIntersection bi;
        if (!blp_intersect(ro, rd, t_max, ld3(pr.p0), ld3(pr.p1), ld3(pr.p2), ld3(sv.patches[pr.kind_index & PRIM_INDEX_MASK].p11), bi)) return false;
        c.t = bi.t; c.b0 = bi.u; c.b1 = bi.v; c.b2 = 0.0f; c.phi = 0.0f;
    } else {
        TriangleIntersection ti;
        if (!intersect_triangle(ro, rd, t_max, ld3(pr.p0), ld3(pr.p1), ld3(pr.p2), ti)) return false;
        c.t = ti.t; c.b0 = ti.b0; c.b1 = ti.b1; c.b2 = ti.b2; c.phi = 0.0f;
    }
    const uint32_t alpha = prim_alpha(sv, pr);
    if (alpha != 0u && !alpha_accept(sv, pr, alpha, c, ro, rd)) return false;
    h.prim = c.prim; h.t = c.t; h.b0 = c.b0; h.b1 = c.b1; h.b2 = c.b2; h.phi = c.phi;
    return true;
}

}  // namespace shm
