/* shimmer_hip.h — C ABI of libshimmer_hip.so: the MI355X (gfx950) wavefront path tracer that drops in
 * behind Shimmer's `Integrator::render()`.
 *
 * The reference has no FFI/plugin interface; its only seam is
 *     pub trait Integrator { fn render(&mut self, options: &Options); }      (src/integrator.rs:52-54)
 * constructed by create_integrator(name, params, camera, sampler, aggregate, lights, color_space)
 * (src/integrator.rs:16-42) and invoked once from render_cpu (src/render.rs:51-54).  A GPU backend is a
 * new `impl Integrator` whose render() marshals the already-built scene objects (flattened BVH of
 * src/aggregate.rs:471-481, triangle meshes of src/shape/mesh.rs:9-20, materials, lights, camera, film
 * sensor) into the flat POD arrays below and calls shm_scene_create + shm_render_wave per spp-wave
 * (src/integrator.rs:241-320), then reads the film sums back.  INTEGRATION.md shows that Rust shim.
 *
 * Conventions: every function returns 0 (SHM_OK) or a negative ShmError; nothing throws, aborts or
 * unwinds across this boundary (the reference panics; a Rust caller maps codes to Result).  All pointers
 * are borrowed for the duration of the call only; the library copies what it keeps.  Everything is
 * little-endian f32/u32/i32 unless stated.  One in-flight render per ShmScene; distinct scenes may be
 * used from distinct host threads.  No callbacks into the host.
 */
#ifndef SHIMMER_HIP_H
#define SHIMMER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Enum values added WITHOUT a version step are additive: no struct changes size or layout and a caller built against the earlier header never passes them.
 * Under version 10 these are SHM_TEXMAP_POINT3D, SHM_FLOATTEX_CHECKERBOARD .. SHM_FLOATTEX_BILERP, the mapping-only ShmImageTexture record (n_levels == 0) and
 * SHM_MATERIAL_DIFFUSE_TRANSMISSION, and SHM_QUADRIC_DISK / SHM_QUADRIC_CYLINDER in ShmSphere::quadric (a byte of its padding). */
#define SHM_ABI_VERSION 10

/* The library is built with -fvisibility=hidden; only these entry points are exported. */
#if defined(__GNUC__)
#define SHM_API __attribute__((visibility("default")))
#else
#define SHM_API
#endif

typedef enum ShmError {
    SHM_OK = 0,
    SHM_ERR_INVALID_ARGUMENT = -1,
    SHM_ERR_UNSUPPORTED = -2,   /* valid input the backend does not take (nested instances, trees over the node limits, BVH deeper than 64, ...) */
    SHM_ERR_DEVICE = -3,        /* HIP runtime error; see shm_last_error() */
    SHM_ERR_NO_DEVICE = -4,     /* no gfx950 device visible: there is NO CPU fallback */
    SHM_ERR_OUT_OF_MEMORY = -5,
    SHM_ERR_INTERNAL = -6
} ShmError;

/* ---- geometry -------------------------------------------------------------------------------- */

/* LinearBvhNode (src/aggregate.rs:471-481; 64 B in the reference) narrowed to 32 B.
 * DFS order: first child of interior node i is i+1; `offset` is second_child_offset (interior) or
 * primitive_offset into the leaf-ordered primitive list (leaf); n_prims > 0 marks a leaf. */
typedef struct ShmBvhNode {
    float bmin[3];
    float bmax[3];
    uint32_t offset;
    uint16_t n_prims;
    uint8_t axis;
    uint8_t pad;
} ShmBvhNode;

/* TriangleMesh (src/shape/mesh.rs:9-20), vertices already in render space (mesh.rs:43-46). */
typedef struct ShmTriangleMesh {
    uint32_t n_triangles;
    uint32_t n_vertices;
    const uint32_t* vertex_indices; /* 3*n_triangles (the reference's Vec<usize>, narrowed) */
    const float* p;                 /* 3*n_vertices */
    const float* n;                 /* 3*n_vertices or NULL */
    const float* s;                 /* 3*n_vertices or NULL */
    const float* uv;                /* 2*n_vertices or NULL */
    uint8_t reverse_orientation;
    uint8_t transform_swaps_handedness;
    uint8_t pad[2];
    uint32_t alpha;                 /* PBRT-v4's shape alpha (see below ShmSphere): 0 = none, else 1 + index into ShmSceneDesc::float_textures */
} ShmTriangleMesh;

/* BilinearPatchMesh (src/shape/mesh.rs:289-376) for BilinearPatch (src/shape/bilinear_patch.rs), vertices in render space.
 * (Image-valued emission on a patch light is not carried: `uv` only drives the (s, t) parameterisation of the interaction.) */
typedef struct ShmBilinearPatchMesh {
    uint32_t n_patches;
    uint32_t n_vertices;
    const uint32_t* vertex_indices; /* 4*n_patches: p00, p10, p01, p11 (bilinear_patch.rs:87-98) */
    const float* p;                 /* 3*n_vertices */
    const float* n;                 /* 3*n_vertices or NULL */
    const float* uv;                /* 2*n_vertices or NULL */
    uint8_t reverse_orientation;
    uint8_t transform_swaps_handedness;
    uint8_t pad[2];
    uint32_t alpha;                 /* shape alpha: 0 = none, else 1 + index into ShmSceneDesc::float_textures */
} ShmBilinearPatchMesh;

/* Sphere (src/shape/sphere.rs:27-38); matrices row-major m[r][c] as SquareMatrix<4>.
 * The record also carries PBRT-v4's two other quadrics with the sphere's hit record {t_hit, p_obj, phi} (the reference has neither): `quadric` says which. They stay
 * SHM_SHAPE_SPHERE primitives, and a zeroed byte (the former pad: every scene written before it had a name) is a sphere.
 *   SHM_QUADRIC_DISK      radius; z_min == z_max = the height; theta_z_min = the inner radius, 0 <= inner < radius; theta_z_max = 0; phi_max in radians, in (0, 2 pi]
 *   SHM_QUADRIC_CYLINDER  radius; z_min < z_max; theta_z_min = theta_z_max = 0; phi_max in radians, in (0, 2 pi]
 * shm_scene_create answers any other kind with SHM_ERR_UNSUPPORTED and a field outside these ranges with SHM_ERR_INVALID_ARGUMENT. */
enum { SHM_QUADRIC_SPHERE = 0, SHM_QUADRIC_DISK = 1, SHM_QUADRIC_CYLINDER = 2 };
typedef struct ShmSphere {
    float radius, z_min, z_max, theta_z_min, theta_z_max, phi_max;
    float render_from_object[16];
    float object_from_render[16];
    uint8_t reverse_orientation;
    uint8_t transform_swaps_handedness;
    uint8_t quadric;   /* SHM_QUADRIC_* */
    uint8_t pad[1];
    uint32_t alpha;    /* shape alpha: 0 = none, else 1 + index into ShmSceneDesc::float_textures */
} ShmSphere;
/* Shape alpha (PBRT-v4's "float alpha" / "texture alpha" shape parameter; the reference has none): ShmTriangleMesh::alpha, ShmBilinearPatchMesh::alpha and
 * ShmSphere::alpha name a float texture that cuts holes in every primitive of the shape. Where the shape's own test has accepted a candidate hit, the texture is
 * evaluated at the candidate's p, uv and geometric normal (all differentials zero): a >= 1 accepts, a <= 0 rejects, anything between rejects where
 * HashFloat(ray.o, ray.d) > a — a stochastic cutout that is the same for the same ray —; a rejected candidate is a miss. Closest-hit and any-hit (shadow) rays
 * run the same test. The fields are carved out of the structs' former padding: a zeroed one is "no alpha", and no size or offset changed.
 * shm_scene_create answers an index beyond the table with SHM_ERR_INVALID_ARGUMENT and alpha on a primitive that is also an area light with SHM_ERR_UNSUPPORTED
 * (PBRT-v4 masks the emitted radiance and the light's sampling by the alpha as well: not carried). */

enum { SHM_SHAPE_TRIANGLE = 0, SHM_SHAPE_SPHERE = 1, SHM_SHAPE_BILINEAR_PATCH = 2,
       SHM_SHAPE_INSTANCE = 3 /* ABI v6: a TransformedPrimitive (primitive.rs:136-176): shape_index = index into ShmSceneDesc::instances;
                                 its material / area_light fields are ignored (the instanced primitives carry their own) */ };
/* TransformedPrimitive {primitive, render_from_primitive}: the instanced primitive is a BvhAggregate of the object's shapes
 * (loading/scene.rs:817-829) stored as ANOTHER tree in ShmSceneDesc::nodes starting at root_node (DFS order and absolute
 * offsets as for the top-level tree at node 0; its leaves index ShmSceneDesc::primitives like every other leaf). An object with a
 * single shape is a one-leaf tree. Constraints: the instance primitive is alone in its top-level leaf (the reference's builder puts
 * one primitive per leaf unless centroids coincide); instanced primitives are not instances and carry no area light.
 * Reference behaviour kept as written: intersect() maps the ray with apply_ray_inverse, intersect_predicate() with the FORWARD
 * apply_ray (primitive.rs:158-175), and Transform::apply(SurfaceInteraction) maps every vector with the inverse (quirk 6). */
typedef struct ShmInstance {
    float render_from_primitive[16];  /* matrix m, row-major */
    float primitive_from_render[16];  /* m_inv */
    uint32_t root_node;
    uint32_t pad[3];
} ShmInstance;

/* GeometricPrimitive / SimplePrimitive (src/primitive.rs:66-130): shape + material (+ area light).
 * Listed in the order of BvhAggregate::primitives AFTER the build's reordering (aggregate.rs:270),
 * i.e. leaf node `offset` indexes this array directly. */
typedef struct ShmPrimitive {
    uint32_t shape_kind;   /* SHM_SHAPE_* */
    uint32_t shape_index;  /* triangle: global triangle index (mesh base + tri_index); sphere: index;
                              bilinear patch: global patch index (patch-mesh base + blp_index) */
    uint32_t material;     /* index into materials. 0xffffffff (the reference's `material: None`, a medium interface that li() skips with
                              skip_intersection, interaction.rs:410-427) is rejected with SHM_ERR_UNSUPPORTED: media are todo!() there */
    int32_t area_light;    /* index into lights, or -1 */
} ShmPrimitive;

/* ---- spectra, materials, lights -------------------------------------------------------------- */

enum {
    SHM_SPECTRUM_CONSTANT = 0,         /* ConstantSpectrum          (spectra/spectrum.rs:143-166) */
    SHM_SPECTRUM_DENSE = 1,            /* DenselySampledSpectrum, lambda_min..=lambda_max, 1 nm (:168-291) */
    SHM_SPECTRUM_PIECEWISE_LINEAR = 2, /* PiecewiseLinearSpectrum   (:293-428): n lambdas then n values */
    /* RGB-derived spectra: the host looks the sigmoid coefficients up (RgbColorSpace::to_rgb_coeffs, colorspace.rs:95) and
     * hands them over; the device evaluates RgbSigmoidPolynomial::get = s(c0 l^2 + c1 l + c2) (color.rs:333-383). */
    SHM_SPECTRUM_RGB_ALBEDO = 3,       /* RgbAlbedoSpectrum     (:498-528) */
    SHM_SPECTRUM_RGB_UNBOUNDED = 4,    /* RgbUnboundedSpectrum  (:531-565): c = scale (2 max(r,g,b)) */
    SHM_SPECTRUM_RGB_ILLUMINANT = 5,   /* RgbIlluminantSpectrum (:568-607): c = scale; offset / n / lambda_min: the colour space's
                                          illuminant as a densely sampled table */
    /* ABI v6. A SpectrumImageTexture (texture.rs:689-808) bound to a material's SpectrumTexture slot (ShmMaterial a, b, c):
     * `offset` = index into ShmSceneDesc::image_textures. Not valid for eta (a Spectrum, not a texture, in the reference) nor
     * for lights. The device filters the MIP pyramid, looks the sigmoid coefficients up in ShmSceneDesc::color_space and
     * evaluates the resulting Rgb{Albedo,Unbounded,Illuminant}Spectrum at the path's wavelengths. */
    SHM_SPECTRUM_IMAGE_TEXTURE = 6,
    /* ABI v6. A composite SpectrumTexture (scale / mix / directionmix, texture.rs:536-687, 810-828) bound to a material's
     * SpectrumTexture slot: `offset` = index into ShmSceneDesc::spectrum_textures (the root of its tree). */
    SHM_SPECTRUM_TEXTURE_NODE = 7
};
typedef struct ShmSpectrum {
    uint32_t kind;
    float c;              /* CONSTANT */
    uint32_t offset;      /* DENSE / PIECEWISE: first float in ShmSceneDesc::spectrum_data */
    uint32_t n;           /* DENSE: number of samples; PIECEWISE: number of knots */
    int32_t lambda_min;   /* DENSE */
    float rgb_c[3];       /* RGB_*: c0, c1, c2 of the sigmoid polynomial */
} ShmSpectrum;

enum {
    SHM_MATERIAL_DIFFUSE = 0,         /* material.rs:247-332 */
    SHM_MATERIAL_CONDUCTOR = 1,       /* material.rs:334-516 */
    SHM_MATERIAL_DIELECTRIC = 2,      /* material.rs:518-650 */
    SHM_MATERIAL_THIN_DIELECTRIC = 3, /* material.rs:652-768 */
    SHM_MATERIAL_COATED_DIFFUSE = 4,  /* material.rs:772-1005: LayeredBxDF<Dielectric, Diffuse, two-sided> (bxdf.rs:269-290, 883-1620) */
    SHM_MATERIAL_COATED_CONDUCTOR = 5,/* material.rs:1007-1286: LayeredBxDF<Dielectric, Conductor, two-sided> (bxdf.rs:460-480) */
    SHM_MATERIAL_MIX = 6,             /* material.rs:1288-1330: MixMaterial, resolved per hit in get_bsdf (interaction.rs:205-220).
                                         The reference draws the choice from the tile's entropy-seeded SmallRng (integrator.rs:255);
                                         here it is a hash of (wo, p), the way PBRT-v4 defines it: reproducible, parity unpinned. */
    /* 7 is reserved: shm_scene_create answers it with SHM_ERR_UNSUPPORTED, as it answers every kind above 8 */
    SHM_MATERIAL_DIFFUSE_TRANSMISSION = 8 /* PBRT-v4's DiffuseTransmissionMaterial / DiffuseTransmissionBxDF (the reference has none): `a` = reflectance, `b` = transmittance,
                                         both SpectrumTexture slots, each clamped to [0, 1]; f = a / pi on wo's side, b / pi on the other. No other field is read but
                                         has_displacement / displacement / float_tex[SHM_FLOATSLOT_DISPLACEMENT] and normal_map (a displacement applies only when given).
                                         PBRT-v4's `scale` parameter is no field: a front end wraps both slots in a SHM_SPECTEX_SCALED node. May be a Mix child. */
};
/* FloatTexture (texture.rs:88-305, 309-403), ABI v6: a node table; children are indices into ShmSceneDesc::float_textures and must
 * precede their parent (no cycles); a tree (counting a shared child once per use) may hold at most 32 nodes. Materials refer to a node through ShmMaterial::float_tex. */
enum {
    SHM_FLOATTEX_CONSTANT = 0,      /* FloatConstantTexture: value */
    SHM_FLOATTEX_SCALED = 1,        /* FloatScaledTexture:  tex = a, scale = b */
    SHM_FLOATTEX_MIX = 2,           /* FloatMixTexture:     tex1 = a, tex2 = b, amount = c */
    SHM_FLOATTEX_DIRECTION_MIX = 3, /* FloatDirectionMixTexture: tex1 = a, tex2 = b, dir */
    SHM_FLOATTEX_IMAGE = 4,         /* FloatImageTexture: image = index into ShmSceneDesc::image_textures (its spectrum_type and
                                       has_color_space are ignored) */
    /* PBRT-v4's procedural float textures (the reference has none). `image` names the texture MAPPING: the index of a mapping-only ShmImageTexture
     * (n_levels == 0; only mapping, su sv du dv, vs vt and texture_from_render are read). CHECKERBOARD and DOTS compute a weight w and
     * t1 = (w != 1) ? a : 0, t2 = (w != 0) ? b : 0, value = (1 - w) * t1 + w * t2, with a, b child nodes; a == b == 0xffffffff is the WEIGHT FORM:
     * the node yields w itself (tex1 = 0, tex2 = 1 folded), a tree of one node. A spectrum checkerboard / dots texture is SHM_SPECTEX_MIX(tex1, tex2,
     * f = the weight form): the same arithmetic as PBRT-v4's SpectrumCheckerboardTexture / SpectrumDotsTexture. */
    SHM_FLOATTEX_CHECKERBOARD = 5,  /* tex1 = a, tex2 = b; image: a 2-D mapping (PBRT's dimension 2) or SHM_TEXMAP_POINT3D (dimension 3); w = the box-filtered checkerboard weight */
    SHM_FLOATTEX_DOTS = 6,          /* inside = a, outside = b; image: a 2-D mapping; w = 0 inside a dot, 1 outside */
    SHM_FLOATTEX_FBM = 7,           /* value = roughness (omega), pad[0] = octaves (<= 32); image: a SHM_TEXMAP_POINT3D mapping; FBm(p, dpdx, dpdy, omega, octaves) */
    SHM_FLOATTEX_WRINKLED = 8,      /* as FBM; Turbulence(p, dpdx, dpdy, omega, octaves) */
    SHM_FLOATTEX_WINDY = 9,         /* image: a SHM_TEXMAP_POINT3D mapping; |FBm(0.1 p, 0.1 dpdx, 0.1 dpdy, 0.5, 3)| * FBm(p, dpdx, dpdy, 0.5, 6) */
    SHM_FLOATTEX_BILERP = 10        /* value, dir[0], dir[1], dir[2] = v00, v01, v10, v11; image: a 2-D mapping; (1-s)(1-t) v00 + s(1-t) v10 + (1-s) t v01 + s t v11 */
};
typedef struct ShmFloatTexture {
    uint32_t kind;
    float value;
    uint32_t a, b, c;
    float dir[3];
    uint32_t image;
    uint32_t pad[3];          /* pad[0]: FBM / WRINKLED: octaves */
} ShmFloatTexture;
/* SpectrumTexture node table (texture.rs:411-503): a LEAF is a spectrum or an image texture (SpectrumConstantTexture /
 * SpectrumImageTexture); composites name their children by index (children precede parents; a tree holds at most 8 nodes) and
 * their FloatTexture parameter by index into ShmSceneDesc::float_textures. */
enum {
    SHM_SPECTEX_LEAF = 0,          /* leaf: any ShmSpectrum kind except TEXTURE_NODE */
    SHM_SPECTEX_SCALED = 1,        /* SpectrumScaledTexture: tex = a, scale = float texture f */
    SHM_SPECTEX_MIX = 2,           /* SpectrumMixTexture: tex1 = a, tex2 = b, amount = float texture f */
    SHM_SPECTEX_DIRECTION_MIX = 3  /* SpectrumDirectionMixTexture: tex1 = a, tex2 = b, dir */
};
typedef struct ShmSpectrumTexture {
    uint32_t kind;
    uint32_t a, b;
    uint32_t f;
    float dir[3];
    uint32_t pad;
    ShmSpectrum leaf;
} ShmSpectrumTexture;
/* indices into ShmMaterial::float_tex */
enum {
    SHM_FLOATSLOT_DISPLACEMENT = 0, SHM_FLOATSLOT_U_ROUGHNESS = 1, SHM_FLOATSLOT_V_ROUGHNESS = 2, SHM_FLOATSLOT_U2_ROUGHNESS = 3,
    SHM_FLOATSLOT_V2_ROUGHNESS = 4, SHM_FLOATSLOT_THICKNESS = 5, SHM_FLOATSLOT_G = 6, SHM_FLOATSLOT_MIX_AMOUNT = 7
};
/* Every float parameter is a constant unless float_tex[slot] != 0; spectrum slots a, b, c may bind image textures. */
typedef struct ShmMaterial {
    uint32_t kind;
    uint32_t has_displacement; /* Diffuse: always 1 with a constant-0 texture (material.rs:280, quirk 8) */
    float displacement;        /* the constant displacement value */
    uint32_t remap_roughness;
    float u_roughness, v_roughness; /* Conductor / Dielectric; Coated*: the dielectric interface */
    float u2_roughness, v2_roughness; /* CoatedConductor: the conductor (material.rs:1237-1244 derives it from the interface
                                         roughness when remap_roughness is set: reference behaviour, done in get_bsdf) */
    float thickness, g;               /* Coated*: layer thickness, HG asymmetry of the medium between the interfaces */
    int32_t max_depth, n_samples;     /* Coated*: random-walk depth and walks per evaluation (defaults 10, 1) */
    uint32_t conductor_from_reflectance; /* CoatedConductor: `a` is a reflectance (material.rs:1224-1231), not eta */
    uint32_t mix_material[2];         /* Mix: indices into the material table (may themselves be Mix; no cycles) */
    float mix_amount;                 /* Mix: constant `amount` texture (default 0.5): <= 0 -> [0], >= 1 -> [1], else [amount < u ? 0 : 1] */
    ShmSpectrum a;  /* Diffuse / CoatedDiffuse / DiffuseTransmission: reflectance; Conductor / CoatedConductor: eta (or reflectance); Dielectric/Thin: eta */
    ShmSpectrum b;  /* Conductor / CoatedConductor: k; DiffuseTransmission: transmittance */
    ShmSpectrum c;  /* Coated*: albedo of the medium */
    ShmSpectrum d;  /* Coated*: eta of the dielectric interface */
    uint32_t float_tex[8];  /* ABI v6: SHM_FLOATSLOT_*: 0 = the constant field above, else 1 + index into ShmSceneDesc::float_textures */
    uint32_t normal_map;    /* 0 = none, else 1 + index into ShmSceneDesc::image_textures of the normal map (3 channels; only its finest
                               level, repeat wrap and bilinear lookup are used: material::normal_map, material.rs:1453-1475). Ignored
                               when has_displacement is set (interaction.rs:223-236), so never reached on a DiffuseMaterial (quirk 8) */
    uint32_t pad[3];
} ShmMaterial;

enum {
    SHM_LIGHT_POINT = 0,            /* light.rs:392-497 */
    SHM_LIGHT_DIFFUSE_AREA = 1,     /* light.rs:499-690; one per emissive shape (loading/scene.rs:609-624) */
    SHM_LIGHT_UNIFORM_INFINITE = 2, /* light.rs:692-816 */
    SHM_LIGHT_IMAGE_INFINITE = 3,   /* ImageInfinitelight, light.rs:805-981 (ABI v6): `primitive` = index into ShmSceneDesc::image_lights;
                                       `scale` as for the others; `spectrum` unused (the radiance is the image's RGB as an
                                       RgbIlluminantSpectrum of ShmSceneDesc::color_space, which must carry table and illuminant) */
    SHM_LIGHT_DISTANT = 4,          /* PBRT-v4's DistantLight (ABI v10; the reference has none): `position` = the unit vector TOWARDS the light in render space,
                                       normalize(render_from_light(from - to)); scale * spectrum = the emitted radiance L (numerically the irradiance on a
                                       surface that faces the light). A delta light; NOT an infinite light for escaped rays */
    SHM_LIGHT_SPOT = 5              /* PBRT-v4's SpotLight (ABI v10): `position` = the apex render_from_light(0,0,0); `primitive` = index into
                                       ShmSceneDesc::spot_lights; scale * spectrum = the intensity I on the axis. A delta light */
};
typedef struct ShmLight {
    uint32_t kind;
    uint32_t primitive;    /* DIFFUSE_AREA: index into primitives (leaf order) of its shape; IMAGE_INFINITE: into image_lights; SPOT: into spot_lights */
    float scale;           /* final scale (after /spectrum_to_photometric, power...) */
    uint32_t two_sided;
    float position[3];     /* POINT, SPOT: render_from_light(0,0,0); DISTANT: the unit direction towards the light */
    float area;            /* DIFFUSE_AREA: shape.area() (light.rs:543) */
    ShmSpectrum spectrum;  /* DenselySampledSpectrum of I / Lemit (must be DENSE) */
} ShmLight;

/* What a SHM_LIGHT_SPOT needs beside its ShmLight (ABI v10; PBRT-v4 SpotLight). Light space: the apex at the origin, the axis along +z. */
typedef struct ShmSpotLight {
    float render_from_light[16];  /* SpotLight::renderFromLight, row-major 4x4: render_from_object * translate(from) * inverse(frame with z = normalize(to - from)) */
    float light_from_render[16];  /* its inverse: a direction w is taken to light space by the 3x3 linear part of THIS matrix (renderFromLight.ApplyInverse) */
    float cos_falloff_start;      /* SpotLight::cosFalloffStart = cos(radians(coneangle - conedelta)): full intensity inside */
    float cos_falloff_end;        /* SpotLight::cosFalloffEnd = cos(radians(coneangle)): zero outside; -1 <= cos_falloff_end <= cos_falloff_start <= 1 */
    uint32_t pad[2];
} ShmSpotLight;

/* ---- camera, film ---------------------------------------------------------------------------- */

enum {
    SHM_CAMERA_PERSPECTIVE = 0,  /* camera.rs:866-1079 */
    SHM_CAMERA_ORTHOGRAPHIC = 1, /* camera.rs:658-840: rays start at camera_from_raster(p_film) and run along +z; the reference
                                    has no depth of field for it yet ("TODO Adjust for depth-of-field here", :762) */
    SHM_CAMERA_SPHERICAL = 2     /* PBRT-v4's SphericalCamera (the reference has none): every direction around the camera's origin, laid out by ShmCamera::mapping.
                                    No lens. shm_camera_spherical builds it; shm_camera_create / ShmCameraParams know the two projective kinds only */
};
/* ShmCamera::mapping of a spherical camera (PBRT-v4's SphericalCamera::Mapping; `"string mapping"` in a scene file) */
enum {
    SHM_SPHERICAL_EQUAL_AREA = 0,      /* "equalarea", PBRT-v4's default: the equal-area octahedral square, the layout of an ImageInfinitelight's map */
    SHM_SPHERICAL_EQUIRECTANGULAR = 1  /* "equirectangular": theta = pi v down the film, phi = 2 pi u across it */
};
/* ---- image textures (ABI v6) ------------------------------------------------------------------ */

/* One level of a MIPMap pyramid (Image::generate_pyramid, image.rs:699-800): `width * height * n_channels` floats at
 * ShmSceneDesc::texel_data + texel_offset, row-major from the TOP row, channels interleaved, each value what
 * Image::get_channel returns for that texel (image.rs:452-476: u8 through the colour encoding, f16 widened, f32 as is). */
typedef struct ShmImageLevel {
    int32_t width, height;
    uint32_t texel_offset;
    uint32_t pad;
} ShmImageLevel;
enum { SHM_TEXMAP_UV = 0, SHM_TEXMAP_SPHERICAL = 1, SHM_TEXMAP_CYLINDRICAL = 2, SHM_TEXMAP_PLANAR = 3, /* texture.rs:838-843 */
       SHM_TEXMAP_POINT3D = 4 /* PBRT-v4's PointTransformMapping: p = texture_from_render(ctx.p) as a point, dpdx and dpdy as vectors through the same matrix. Only on a
                                 mapping-only record (n_levels == 0), for the procedural float textures that take a 3-D point */ };
enum { SHM_TEXFILTER_POINT = 0, SHM_TEXFILTER_BILINEAR = 1, SHM_TEXFILTER_TRILINEAR = 2, SHM_TEXFILTER_EWA = 3 }; /* mipmap.rs:334-341 */
enum { SHM_WRAP_BLACK = 0, SHM_WRAP_CLAMP = 1, SHM_WRAP_REPEAT = 2, SHM_WRAP_OCTAHEDRAL_SPHERE = 3 };  /* image.rs:73-78 */
enum { SHM_SPECTRUM_TYPE_ALBEDO = 0, SHM_SPECTRUM_TYPE_UNBOUNDED = 1, SHM_SPECTRUM_TYPE_ILLUMINANT = 2 };
/* SpectrumImageTexture = ImageTextureBase {mapping, scale, invert, mipmap} + spectrum_type (texture.rs:19-26, 689-693);
 * MIPMap {pyramid, color_space, wrap_mode, options} (mipmap.rs:8-14). */
typedef struct ShmImageTexture {
    uint32_t mapping;            /* SHM_TEXMAP_* */
    float su, sv, du, dv;        /* UVMapping (texture.rs:896-905); PlanarMapping: du, dv are its ds, dt */
    float vs[3], vt[3];          /* PlanarMapping (texture.rs:1012-1019) */
    float texture_from_render[16]; /* Spherical / Cylindrical / Planar: the matrix m of texture_from_render, row-major */
    uint32_t filter;             /* SHM_TEXFILTER_* ("filter", default bilinear, texture.rs:738) */
    float max_anisotropy;        /* "maxanisotropy", default 8 */
    uint32_t wrap;               /* SHM_WRAP_* ("wrap", default repeat) */
    float scale;                 /* "scale", default 1 */
    uint8_t invert;
    uint8_t spectrum_type;       /* SHM_SPECTRUM_TYPE_* */
    uint8_t n_channels;          /* 1 or 3 (an RGBA image hands over its RGB: texel_rgb / bilerp read channels 0..2, mipmap.rs:204-231) */
    uint8_t has_color_space;     /* MIPMap::get_color_space().is_some(); 0: one-channel texture -> constant spectrum (texture.rs:801-805) */
    uint32_t first_level;        /* index into ShmSceneDesc::image_levels, finest level first */
    uint32_t n_levels;           /* 0: a MAPPING-ONLY record, which only the procedural SHM_FLOATTEX_* kinds may name (filter .. first_level are not read) */
} ShmImageTexture;
/* What RgbColorSpace::to_rgb_coeffs reads (colorspace.rs:95-98 -> rgb_to_spectra.rs:16-25): the rgb2spec coefficient table of
 * the colour space's gamut (the `.spec` file the reference loads: res, scale[res], data[3][res][res][res][3]) and its
 * illuminant (for SHM_SPECTRUM_TYPE_ILLUMINANT). One colour space per scene. */
typedef struct ShmColorSpace {
    uint32_t rgb2spec_res;       /* 0: no table (then no texture may have has_color_space) */
    uint32_t pad;
    const float* rgb2spec_scale; /* res floats */
    const float* rgb2spec_data;  /* 3 * res^3 * 3 floats */
    const float* illuminant;     /* DenselySampledSpectrum 360..=830, 471 floats (may be NULL without ILLUMINANT textures) */
} ShmColorSpace;

/* ImageInfinitelight (light.rs:805-816, 915-981): the environment map and the light's transform. The library derives both sampling
 * distributions from the image exactly as ImageInfinitelight::new does (Image::get_default_sampling_distribution = the channel
 * average per pixel, image.rs:1379-1405; PiecewiseConstant2D::new, sampling.rs:124-153; the compensated one with the average
 * subtracted, light.rs:948-955). */
typedef struct ShmImageInfiniteLight {
    float render_from_light[16];  /* matrix m, row-major */
    float light_from_render[16];  /* its inverse m_inv */
    uint32_t image_level;         /* index into ShmSceneDesc::image_levels: a square image, 3 channels, equal-area octahedral layout */
    uint32_t pad;
} ShmImageInfiniteLight;

/* PerspectiveCamera / OrthographicCamera after construction (ProjectiveCameraBase, camera.rs:594-642), or PBRT-v4's SphericalCamera. Matrices row-major.
 * SHM_CAMERA_SPHERICAL: camera_from_raster is diag(1 / W, 1 / H, 1, 1) of the film's full resolution, so that it takes a film point to (u, v, 0). (PBRT-v4 divides
 * by the resolution; this multiplies by the rounded reciprocal: the same for power-of-two resolutions, within one ulp of uv otherwise.) dx_camera, dy_camera,
 * lens_radius and focal_distance are zero and not read. */
typedef struct ShmCamera {
    float camera_from_raster[16];
    float render_from_camera[16];
    float dx_camera[3];
    float dy_camera[3];
    float lens_radius;
    float focal_distance;
    float shutter_open, shutter_close;
    uint32_t kind;                /* SHM_CAMERA_* (ABI v4) */
    uint32_t mapping;             /* SHM_SPHERICAL_*: read only for SHM_CAMERA_SPHERICAL (the former pad word: 0 in every projective camera) */
    /* ABI v6, read only by scenes with image textures (the ray-differential fallback Camera::approximate_dp_dxy, camera.rs:307-354):
     * the inverse matrix of render_from_camera and the four vectors CameraBase::find_minimum_differentials leaves (camera.rs:356-440).
     * shm_camera_perspective / shm_camera_orthographic / shm_camera_spherical fill them. */
    float camera_from_render[16];
    float min_pos_differential_x[3], min_pos_differential_y[3];
    float min_dir_differential_x[3], min_dir_differential_y[3];
} ShmCamera;

/* The pixel reconstruction filter (ABI v9): the reference's BoxFilter (filter.rs:61-105) and PBRT-v4's gaussian, Mitchell, windowed sinc and triangle filters.
 * A sample is added to its own pixel with the weight of the importance-sampled filter (PBRT-v4's FilterSampler); nothing is splatted. 0 = box. */
enum { SHM_FILTER_BOX = 0, SHM_FILTER_GAUSSIAN = 1, SHM_FILTER_MITCHELL = 2, SHM_FILTER_SINC = 3, SHM_FILTER_TRIANGLE = 4 };

/* RgbFilm + PixelSensor (film.rs:470-574, 754-914) + the pixel filter. */
typedef struct ShmFilm {
    int32_t pixel_bounds[4];      /* min.x, min.y, max.x, max.y (max exclusive) */
    int32_t full_resolution[2];
    float filter_radius[2];       /* "xradius", "yradius" > 0 (PBRT-v4's defaults: box 0.5, gaussian 1.5, mitchell 2, sinc 4, triangle 2); gaussian / mitchell / sinc: 1/32 <= radius <= 8 */
    float imaging_ratio;
    float max_component_value;
    uint32_t filter;              /* SHM_FILTER_* (ABI v9); zeroed = box */
    float filter_params[2];       /* gaussian: {sigma > 0 (0.5), -}; mitchell: {B, C} (1/3, 1/3); sinc: {tau > 0 (3), -}; box, triangle: unused */
    uint32_t pad;
    const float* sensor_r_bar;    /* DenselySampledSpectrum 360..=830, 471 floats */
    const float* sensor_g_bar;
    const float* sensor_b_bar;
} ShmFilm;

typedef struct ShmSceneDesc {
    uint32_t abi_version;         /* SHM_ABI_VERSION */
    uint32_t n_nodes;
    const ShmBvhNode* nodes;
    uint32_t n_primitives;
    const ShmPrimitive* primitives;
    uint32_t n_meshes;
    const ShmTriangleMesh* meshes;
    uint32_t n_spheres;
    const ShmSphere* spheres;
    uint32_t n_materials;
    const ShmMaterial* materials;
    uint32_t n_lights;
    const ShmLight* lights;       /* the integrator's `lights` vector, in order (light_sampler.rs:83-103) */
    uint32_t n_spectrum_floats;
    const float* spectrum_data;
    ShmCamera camera;
    ShmFilm film;
    uint32_t n_patch_meshes;      /* ABI v3 */
    uint32_t pad;
    const ShmBilinearPatchMesh* patch_meshes;
    /* ABI v6: image textures */
    uint32_t n_image_textures;
    uint32_t n_image_levels;
    const ShmImageTexture* image_textures;
    const ShmImageLevel* image_levels;
    uint64_t n_texel_floats;
    const float* texel_data;
    ShmColorSpace color_space;
    const float* ewa_filter_lut;  /* MIP_FILTER_LUT (mipmap.rs:390-521), 128 floats; required when a texture uses SHM_TEXFILTER_EWA */
    uint32_t n_image_lights;
    uint32_t n_float_textures;
    const ShmImageInfiniteLight* image_lights;
    const ShmFloatTexture* float_textures;
    uint32_t n_spectrum_textures;
    uint32_t n_instances;
    const ShmSpectrumTexture* spectrum_textures;
    const ShmInstance* instances;
    /* ABI v10: the side records of the SHM_LIGHT_SPOT lights (ShmLight::primitive indexes them) */
    uint32_t n_spot_lights;
    uint32_t pad2;
    const ShmSpotLight* spot_lights;
} ShmSceneDesc;

/* ---- render parameters ----------------------------------------------------------------------- */

/* options.rs:15-61 (the five flags the path reads) + PathIntegrator params (integrator.rs:188-192)
 * + sampler params (sampler.rs:95-99). */
typedef struct ShmRenderParams {
    uint64_t seed;
    int32_t samples_per_pixel;    /* total spp (ray-differential scale, integrator.rs:356-359) */
    int32_t max_depth;            /* "maxdepth", default 5 */
    uint8_t regularize;
    uint8_t disable_pixel_jitter;
    uint8_t disable_wavelength_jitter;
    uint8_t force_diffuse;        /* options.force_diffuse: every BSDF becomes DiffuseBxDF(rho_hd estimate), interaction.rs:256-275 */
    uint8_t integrator;           /* SHM_INTEGRATOR_* (ABI v5); 0 = "path" */
    uint8_t sample_lights;        /* SimplePath "samplelights" (default true in the reference, integrator.rs:135-137) */
    uint8_t sample_bsdf;          /* SimplePath "samplebsdf"   (default true) */
    uint8_t disable_texture_filtering; /* options.disable_texture_filtering: compute_differentials leaves zeros (interaction.rs:287-295) */
    /* ABI v8 — SHM_REFERENCE_QUIRKS. 0 (the default) = reference-exact: every deviation of the reference from PBRT-v4 that SURVEY 7
     * lists is reproduced, and every parity test runs this way. 1 = the PBRT-v4 behaviour at the sites where the reference's produces invalid or
     * biased values: LayeredBxDF::pdf tests the reflected sample (`rs.f != 0 && rs.pdf > 0`, bxdf.rs:1491-1506 omits it: 0/0 -> NaN film
     * pixels in coated scenes); a radiance sample with a NaN or an infinite component is dropped before RgbFilm::add_sample (the two TODOs of
     * integrator.rs:377-382); safe_acos is acos (math.rs:272-274 calls asin): Sphere (u, v) and SphericalMapping (which then also uses phi
     * for t, texture.rs:972); uniform_hemisphere_pdf = 1/(2 pi) (sampling.rs:306-308 returns 1/(4 pi)); Sphere::pdf_with_context uses
     * 2 pi and multiplies by the squared distance inside the sphere (sphere.rs:438-440, 456); triangle emitters are sampled as PBRT-v4 samples them
     * (round 6): sample_spherical_triangle's barycentrics divided by s1 . e1 (sampling.rs:477: e1 . e1) and renormalised as in PBRT-v4 (:493-497),
     * Triangle::sample_with_context drawing from the warped u whose density it reports (triangle.rs:639-641 shadows it), Triangle::sample negating
     * the normal of a mesh without normals only with reverse_orientation ^ transform_swaps_handedness (triangle.rs:558-560: always); a non-rectangular
     * bilinear patch is area-sampled with PBRT-v4's edge points in sample() and pdf() (bilinear_patch.rs:549-553, 627-628); a shadow ray enters an instance
     * through apply_ray_inverse with its t_max (primitive.rs:173-176 maps it forward) and an instanced hit's interaction is mapped back by PBRT-v4's
     * Transform::operator() (transform.rs:573-608 uses the inverse for everything but the point): instances render as their baked copies. Reference-exact,
     * BASELINE's C1 scene is 19 % darker than an estimator that samples no lights; with 1 it agrees with it (tests/test_quirks_switch.py). */
    uint8_t disable_reference_quirks;
    /* The sampler (DESIGN.md "Sampler"). SHM_SAMPLER_INDEPENDENT (0, the default and the reference's only sampler): one PCG32 stream per pixel.
     * SHM_SAMPLER_ZSOBOL (1): PBRT-v4's ZSobolSampler — a Morton-ordered, per-digit shuffled Sobol' (0, 2)-sequence with log2spp = ceil(log2(spp))
     * (PBRT-v4 takes the floor); sample indices must stay below 2^log2spp. sampler_randomization applies to ZSobol only: SHM_SAMPLER_FASTOWEN (0,
     * the default) or SHM_SAMPLER_RANDOMIZE_NONE (1, the bare sequence). Callers that zero `pad` keep the independent sampler. */
    uint8_t sampler;
    uint8_t sampler_randomization;
    /* The ambient occlusion integrator's two parameters (SHM_INTEGRATOR_AMBIENT_OCCLUSION), carved out of the five bytes that were `pad`: no size
     * or offset changed, `pad` still names the five bytes, and a caller that zeroes them gets PBRT-v4's defaults. Every other integrator ignores them.
     *   ao_uniform_sample  0 (the default, PBRT-v4's "cossample" true): cosine-weighted hemisphere sampling; anything else: uniform hemisphere sampling, pdf 1 / (2 pi)
     *   ao_max_distance    0 (the default, PBRT-v4's "maxdistance" infinity): the occlusion ray is unbounded; a finite positive value is its t_max. Negative or NaN:
     *                      SHM_ERR_INVALID_ARGUMENT */
    union {
        uint8_t pad[5];
        struct __attribute__((packed)) {
            uint8_t ao_uniform_sample;
            float ao_max_distance;   /* at offset 28 of the struct: aligned */
        };
    };
} ShmRenderParams;
enum {
    SHM_SAMPLER_INDEPENDENT = 0,
    SHM_SAMPLER_ZSOBOL = 1
};
enum {
    SHM_SAMPLER_FASTOWEN = 0,
    SHM_SAMPLER_RANDOMIZE_NONE = 1
};
enum {
    SHM_INTEGRATOR_PATH = 0,        /* PathIntegrator,       integrator.rs:748-963 */
    SHM_INTEGRATOR_SIMPLE_PATH = 1, /* SimplePathIntegrator, integrator.rs:573-733 */
    SHM_INTEGRATOR_RANDOM_WALK = 2, /* RandomWalkIntegrator, integrator.rs:445-563: le + f cos Li / (1/4pi), folded innermost-first */
    /* PBRT-v4's AOIntegrator (`Integrator "ambientocclusion"`; the reference has none): one camera ray and one occlusion ray per sample, no material, texture or light.
     * At a hit, with n the geometric normal facing the camera ray and u the 2-D draw behind the camera sample: wi = Frame::from_z(n).from_local(w(u)), w cosine- or
     * uniform-hemisphere distributed (ShmRenderParams::ao_uniform_sample), and if the interaction's spawn_ray(wi) is unoccluded within ao_max_distance
     * L = illum_scale * illuminant(lambda) * dot(wi, n) / (pi * pdf), else 0. An escaped camera ray is black. illuminant: ShmSceneDesc::color_space.illuminant, which
     * must be there (SHM_ERR_INVALID_ARGUMENT otherwise); illum_scale = 1 / its CIE Y, computed in double at scene creation and rounded to float once. max_depth is not
     * looked at. The film is the ordinary film: every pass behind it takes it unchanged. */
    SHM_INTEGRATOR_AMBIENT_OCCLUSION = 3
};

/* Tile (tile.rs:5-7): Bounds2i, max exclusive. */
typedef struct ShmTile {
    int32_t x0, y0, x1, y1;
} ShmTile;

/* RgbFilmPixel without the unused splat (film.rs:470-479). */
typedef struct ShmFilmPixel {
    double rgb_sum[3];
    double weight_sum;
} ShmFilmPixel;

typedef struct ShmStats {
    uint64_t paths;
    uint64_t rays_closest;     /* camera + extension rays traced by BvhAggregate::intersect */
    uint64_t rays_any;         /* shadow rays traced by intersect_predicate */
    uint64_t nodes_closest;    /* BVH nodes visited (bounds tests) */
    uint64_t tris_closest;     /* primitive tests */
    uint64_t nodes_any;
    uint64_t tris_any;
    double ms_total;           /* HIP-event time of the whole call on the render stream */
    double ms_trace_closest;   /* summed HIP-event time of K2 launches */
    double ms_trace_any;       /* summed HIP-event time of K3 launches */
    double ms_shade;           /* K1 + K5 + K6 */
    uint32_t launches_closest;
    uint32_t launches_any;
    /* ABI v7 (multi-GPU entry points): */
    double ms_gather;          /* HIP-event time of the film gather on this rank's render stream (RCCL send / recv group or xGMI peer copies) */
    uint64_t gather_bytes;     /* film bytes this rank sent (peers) or received (root) */
} ShmStats;

typedef struct ShmRay {
    float o[3];
    float d[3];
    float t_max;
    float pad;
} ShmRay;

/* ShapeIntersection reduced to what identifies it: primitive (leaf-order index), t_hit and the
 * shape-local hit parameters (triangle: b0,b1,b2; sphere: p_obj.xyz in b0..b2 and phi). */
typedef struct ShmHit {
    int32_t prim;   /* -1: miss */
    float t;
    float b0, b1, b2;
    float phi;
    uint32_t instance;  /* 0: a top-level primitive; else 1 + the leaf-order slot of the SHM_SHAPE_INSTANCE primitive it was found
                           through (prim, t and b* are then in that instance's space) */
    uint32_t pad;
} ShmHit;

typedef struct ShmScene ShmScene;

/* Scene lifetime.  `device` is the HIP device ordinal (one process per GPU: pass LOCAL_RANK). */
SHM_API int shm_scene_create(const ShmSceneDesc* desc, int device, ShmScene** out);
SHM_API void shm_scene_destroy(ShmScene* scene);
/* Replace the scene's camera: the next wave renders from `camera`. The scene view is a by-value kernel argument, so nothing is uploaded again; the geometry stays
 * in the render space it was baked in, which is the space `camera` must be expressed in (shm_camera_create_in, below, builds such a camera). The film, the
 * G-buffer, the moments and the temporal history are left as they are: the caller clears what it wants cleared. SHM_ERR_INVALID_ARGUMENT, with the cause in
 * shm_last_error(): a camera whose `kind` is not the scene's (the scene's plan chose its generate kernel by kind) or whose spherical mapping is unknown.
 * SHM_ERR_UNSUPPORTED on a scene that holds multi-GPU state (from shm_dist_init, or shm_render_sharded, until shm_dist_finalize). */
SHM_API int shm_scene_set_camera(ShmScene* scene, const ShmCamera* camera);

/* How many primitives got a per-primitive shading record at scene creation (flat triangles of the scene classes whose kernels read one; 0 under SHM_TRI_SHADE=0 and
 * in every other class), and, where build_ms_out is not NULL, the wall-clock milliseconds scene creation spent building them. */
SHM_API int shm_scene_shading_records(ShmScene* scene, uint64_t* n_records_out, double* build_ms_out);

/* Film accumulation buffer resident in HBM, pixel_bounds-sized, zero-initialised. */
SHM_API int shm_film_clear(ShmScene* scene);
/* Render one spp-wave [sample_begin, sample_end) (integrator.rs:257-260) of the given tiles into the
 * device film (+=).  Blocking.  stats may be NULL.  The tiles of one call must be pairwise disjoint and inside pixel_bounds
 * (Tile::tile's exclusive ownership, which the reference's unsynchronised film writes rely on, integrator.rs:277-295):
 * overlapping tiles return SHM_ERR_INVALID_ARGUMENT. */
SHM_API int shm_render_wave(ShmScene* scene, const ShmRenderParams* params, const ShmTile* tiles, uint32_t n_tiles,
                    int32_t sample_begin, int32_t sample_end, ShmStats* stats);
/* Copy the device film to a caller-allocated pixel_bounds-sized row-major array. */
SHM_API int shm_film_read(ShmScene* scene, ShmFilmPixel* film_out);
/* Device pointer + byte size of the film (for device-side gathers, e.g. RCCL through torch). */
SHM_API int shm_film_device_ptr(ShmScene* scene, void** ptr_out, uint64_t* bytes_out);

/* Whole ImageTileIntegrator::render (integrator.rs:226-322) into the DEVICE film (+=, no clear, no read-back): all
 * spp-waves over the given tiles. Consecutive waves of the reference's schedule are fused into launches of up to 64 spp
 * (identical film sums: a pixel's samples are always added in increasing sample_index). */
SHM_API int shm_render_device(ShmScene* scene, const ShmRenderParams* params, const ShmTile* tiles, uint32_t n_tiles,
                              ShmStats* stats);
/* The same with clear + read-back: whole ImageTileIntegrator::render (integrator.rs:226-322): all waves 1,1,2,4,...,64,64,... over the
 * given tiles; `film` += on the host. */
SHM_API int shm_render(ShmScene* scene, const ShmRenderParams* params, const ShmTile* tiles, uint32_t n_tiles,
               ShmFilmPixel* film, ShmStats* stats);

/* Bring-up / microbenchmark entries for K2/K3 alone (BvhAggregate::intersect / intersect_predicate,
 * aggregate.rs:71-203).  Host arrays in, host arrays out. */
SHM_API int shm_trace_closest(ShmScene* scene, const ShmRay* rays, uint32_t n, ShmHit* hits_out, ShmStats* stats);
SHM_API int shm_trace_any(ShmScene* scene, const ShmRay* rays, uint32_t n, uint8_t* occluded_out, ShmStats* stats);
/* Same, rays already resident in HBM (device pointers); used by bench.py's traversal roofline leg.
 * `repeat` launches back-to-back; stats->ms_trace_* is the HIP-event total over all of them. */
SHM_API int shm_trace_closest_device(ShmScene* scene, const void* rays_dev, uint32_t n, void* hits_dev, int repeat,
                             ShmStats* stats);
SHM_API int shm_trace_any_device(ShmScene* scene, const void* rays_dev, uint32_t n, void* occluded_dev, int repeat,
                         ShmStats* stats);

/* ---- the G-buffer pass: first-hit guide images for a denoiser ------------------------------------------
 * A pass of its own beside the render, after PBRT-v4's GBufferFilm / VisibleSurface: for sample i of a pixel it traces exactly the camera ray the
 * render's sample i traces (same sampler, seed, jitter options, pixel filter, camera and ray-differential scale; no further sampler dimension is drawn)
 * and adds what the first hit shows to the pixel's sums with the sample's filter weight w, negative lobes included:
 *   an escaped ray   w to weight_sum only;
 *   a hit            w to weight_sum and weight_hit, and w * value to p (the hit point), n (the geometric normal, facing the camera ray's origin side:
 *                    negated where dot(n, -d) < 0), ns (the shading normal the BSDF is built on, after bump and normal maps, flipped the same way), uv, and
 *                    albedo: BSDF::rho_hd(-d) over 16 fixed sample points at the camera sample's wavelengths, weighted by the sensor's three response
 *                    curves WITHOUT the film's imaging ratio and clamp (exposure does not scale an albedo); force_diffuse and regularize are ignored.
 * A pixel's samples are added in increasing sample index, in double precision: the sums are deterministic, and a split into waves or into disjoint tile
 * sets gives the same bits as one call. The pass touches neither the film nor anything a later render reads. */
typedef struct ShmGBufferPixel {
    double p[3], n[3], ns[3], uv[2], albedo[3];
    double weight_hit, weight_sum;
} ShmGBufferPixel;   /* 128 bytes */
enum {
    SHM_GBUFFER_SPACE_RENDER = 0,  /* p, n, ns in render space */
    SHM_GBUFFER_SPACE_CAMERA = 1   /* p through camera_from_render as a point, n and ns as normals (not renormalised) */
};
/* The device G-buffer: pixel_bounds-sized, allocated by the first of these calls and freed by shm_scene_destroy. */
SHM_API int shm_gbuffer_clear(ShmScene* scene);
/* Samples [sample_begin, sample_end) of the given tiles into the device G-buffer (+=). Blocking; stats may be NULL. The tiles are validated as
 * shm_render_wave validates them; an unknown `space` returns SHM_ERR_INVALID_ARGUMENT. */
SHM_API int shm_gbuffer_render_wave(ShmScene* scene, const ShmRenderParams* params, uint32_t space, const ShmTile* tiles, uint32_t n_tiles,
                                    int32_t sample_begin, int32_t sample_end, ShmStats* stats);
/* Copy the device G-buffer to a caller-allocated pixel_bounds-sized row-major array. */
SHM_API int shm_gbuffer_read(ShmScene* scene, ShmGBufferPixel* out);
/* clear + all params->samples_per_pixel samples + read. */
SHM_API int shm_render_gbuffer(ShmScene* scene, const ShmRenderParams* params, uint32_t space, const ShmTile* tiles, uint32_t n_tiles,
                               ShmGBufferPixel* out, ShmStats* stats);
/* The pass's CPU twin (no GPU needed): the same shared arithmetic on the host, one sample at a time, for tests and for hosts that trace themselves.
 * pixels_xy: n (x, y) pairs; sample_index: n indices.
 *   shm_gbuffer_camera_rays   the rays the pass traces for those samples.
 *   shm_gbuffer_samples_host  given the closest hits of those rays (ShmHit records, as shm_trace_closest returns them), 16 doubles per sample in
 *                             ShmGBufferPixel's order: what the sample adds to its pixel's sums.
 *   shm_gbuffer_rho_host      12 floats per sample: the spectral rho_hd[4] behind the albedo and the wavelengths[4] and pdfs[4] it is weighted with
 *                             (zeros for an escaped ray). */
SHM_API int shm_gbuffer_camera_rays(const ShmSceneDesc* desc, const ShmRenderParams* params, const int32_t* pixels_xy, const int32_t* sample_index,
                                    uint32_t n, ShmRay* out);
SHM_API int shm_gbuffer_samples_host(const ShmSceneDesc* desc, const ShmRenderParams* params, uint32_t space, const int32_t* pixels_xy,
                                     const int32_t* sample_index, const ShmHit* hits, uint32_t n, double* out);
SHM_API int shm_gbuffer_rho_host(const ShmSceneDesc* desc, const ShmRenderParams* params, const int32_t* pixels_xy, const int32_t* sample_index,
                                 const ShmHit* hits, uint32_t n, float* out);
/* The ambient occlusion integrator's CPU twin (SHM_INTEGRATOR_AMBIENT_OCCLUSION; no GPU needed): the same shared arithmetic (shm/ao.h) on the host, one sample at a time.
 * Given the closest hits of the samples' camera rays (shm_gbuffer_camera_rays gives the rays: they are the path integrator's), per sample i:
 *   rays_out[i]          the occlusion ray with its t_max (zeros where none is queued)
 *   queued_out[i]        1: the ray is queued; 0: none — the camera ray escaped, or the direction's density is 0 — and the sample is black
 *   sample_out[5 i ..]   r, g, b: what film_sample_rgb makes of the sample's radiance IF the occlusion ray is unoccluded (zeros where none is queued); the filter weight w;
 *                        the density the direction was drawn with (0 where none is queued)
 * A film pixel from these, as the film kernel makes it: over the pixel's samples in increasing sample index, in double, rgb_sum[c] += (double)(w * (unoccluded ? rgb[c] : 0.0f))
 * and weight_sum += (double)w, where `unoccluded` is: queued, and an any-hit traversal of rays_out[i] finds nothing. Parameters and scene are checked as shm_render_wave
 * checks them (a negative or NaN ao_max_distance, a scene without an illuminant: SHM_ERR_INVALID_ARGUMENT). */
SHM_API int shm_ao_samples_host(const ShmSceneDesc* desc, const ShmRenderParams* params, const int32_t* pixels_xy, const int32_t* sample_index, const ShmHit* hits,
                                uint32_t n, ShmRay* rays_out, uint8_t* queued_out, float* sample_out);
/* W_c: the sum of the 471-entry table of sensor channel c (1 nm steps), in double — a surface of rho = 1 has an expected albedo sum / W_c of 1. */
SHM_API int shm_gbuffer_white(const ShmSceneDesc* desc, double white[3]);
/* The sums as images, 15 floats per pixel: p[3], n[3], ns[3], uv[2] — each sum / weight_hit —, albedo[3] = (M a) / (M W) per channel with a the albedo sums
 * / weight_hit, W = `white` and M = output_rgb_from_sensor_rgb (row-major 3x3; NULL: the identity), and coverage = weight_hit / weight_sum. A pixel whose
 * weight_hit is 0 gets zeros. */
SHM_API int shm_gbuffer_resolve(const ShmGBufferPixel* pixels, uint64_t n, const double white[3], const float* output_rgb_from_sensor_rgb, float* out15);

/* ---- the denoiser: an edge-avoiding a-trous filter over the film, guided by the G-buffer ------------------
 * A single-frame wavelet filter after Dammertz et al. 2010 with SVGF's weights and its spatial variance estimate: the film's sensor RGB c = rgb_sum / weight_sum is divided
 * by an effective albedo a_eff (the G-buffer's albedo over shm_gbuffer_white, blended towards 1 by the coverage weight_hit / weight_sum; a channel below albedo_floor is left as it is: a_eff = 1),
 * filtered `iterations` times with a 5x5 B3 spline whose taps stand 2^i pixels apart in iteration i — each tap weighted by the normals' agreement (sigma_normal), the
 * tap's angle off the pixel's tangent plane (sigma_plane) and the luminance difference against the locally estimated standard deviation (sigma_luminance; +inf: not at
 * all) — and multiplied by a_eff again. A pixel without a usable guide (weight_sum <= 0, weight_hit <= 0, a zero shading normal, anything non-finite: escaped rays, a
 * pixel whose negative filter lobes outweigh the rest) passes through — its result is c, bit for bit — and no other pixel reads it. Taps outside the film are skipped.
 * The result is a ShmFilmPixel array: rgb_sum the denoised sensor RGB, weight_sum 1 (0 where the film's was 0), so shm_film_get_image takes it as it takes a film.
 * Device and CPU twin run the same header (shm/denoise.h) and give the same bits. */
typedef struct ShmDenoiseParams {
    uint32_t iterations;      /* 0..8; 0: the result is c for every pixel */
    uint32_t demodulate;      /* 0: a_eff = 1 */
    float sigma_luminance;    /* > 0, +inf allowed */
    float sigma_normal;       /* > 0 */
    float sigma_plane;        /* > 0 */
    float albedo_floor;       /* in (0, 1]: the least effective albedo a channel is divided by */
    uint32_t variance_source; /* SHM_DENOISE_VARIANCE_*: where the filter's initial variance of l comes from */
    uint32_t reserved[1];
} ShmDenoiseParams;
#define SHM_DENOISE_VARIANCE_SPATIAL 0u  /* the default: the 7x7 spatial estimate */
#define SHM_DENOISE_VARIANCE_MEASURED 1u /* the moments pass's variance of the pixel's mean (adaptive sampling, below) at every valid pixel whose record holds two batches
                                            or more — var = (mean_c(sqrt(v_c) / a_eff_c))^2 — and the spatial estimate elsewhere. SHM_ERR_INVALID_ARGUMENT on a scene
                                            without moments */
/* 5 iterations, demodulate 1, sigma_luminance 1.5, sigma_normal 128, sigma_plane 0.1, albedo_floor 0.01 */
SHM_API int shm_denoise_default_params(ShmDenoiseParams* out);
/* The device film and the device G-buffer into a device result; neither input is written. Blocking; ms_out (may be NULL) receives the HIP-event time of the kernels.
 * The first call allocates the filter's planes (80 bytes per pixel) and the result, which shm_scene_destroy frees. SHM_ERR_INVALID_ARGUMENT, with the cause in
 * shm_last_error(): no G-buffer wave has run on the scene since its creation or since the last shm_gbuffer_clear; iterations > 8; a sigma that is NaN or <= 0;
 * albedo_floor outside (0, 1]. */
SHM_API int shm_denoise_device(ShmScene* scene, const ShmDenoiseParams* params, double* ms_out);
/* Copy the last result to a caller-allocated pixel_bounds-sized row-major array (SHM_ERR_INVALID_ARGUMENT before the first shm_denoise_device). */
SHM_API int shm_denoise_read(ShmScene* scene, ShmFilmPixel* out);
/* shm_denoise_device + shm_denoise_read */
SHM_API int shm_denoise(ShmScene* scene, const ShmDenoiseParams* params, ShmFilmPixel* out, double* ms_out);
/* The CPU twin (no GPU needed): the same arithmetic on the host, from read-back buffers (shm_film_read, shm_gbuffer_read) and shm_gbuffer_white's W. `out` must not
 * overlap the inputs. */
SHM_API int shm_denoise_host(const ShmFilmPixel* film, const ShmGBufferPixel* gbuffer, int32_t width, int32_t height, const double white[3],
                             const ShmDenoiseParams* params, ShmFilmPixel* out);

/* ---- adaptive sampling: per-pixel moments of the film, a tile error, and a render loop that stops by it ----
 * The moments pass only reads the device film: a batch's contribution to a pixel is the film after the batch's wave minus the film as the pass last saw it
 * (`prev`), its mean x = d rgb_sum / d weight_sum and its weight dw = d weight_sum. Over the batches of a pixel the pass keeps West's weighted Welford
 * recurrence per channel (mean, m2 = sum dw (x - mean)^2), the weight W and the batch count B. A batch with dw <= 0 or a non-finite mean is not counted. From a
 * record: the per-sample variance s2 = m2 / (B - 1), the variance of the pixel's mean v = s2 / W (both 0 while B < 2), and the squared relative error
 * e2 = mean_c(v_c) / max(mean_c(mean_c), floor)^2. A pixel is converged iff B >= min_spp / batch_spp and e2 < threshold^2 (strictly: a threshold of 0
 * converges nothing, +inf everything with a finite e2; a NaN never converges). mean, m2, s2 and v are in SENSOR RGB: an output matrix
 * (output_rgb_from_sensor_rgb) cannot be applied to variances without the covariances between channels, which the pass does not keep.
 * Device and CPU twin run the same header (shm/moments.h) and give the same bits. */
typedef struct ShmMomentsPixel {
    double prev[4];   /* the film pixel (rgb_sum, weight_sum) as the pass last saw it */
    double mean[3];   /* weighted mean of the batch means */
    double m2[3];     /* sum over batches of dw (x - mean)^2 */
    double weight;    /* W: the sum of the counted batches' dw */
    double batches;   /* B: the counted batches */
} ShmMomentsPixel;
typedef struct ShmTileError {
    uint32_t unconverged;  /* pixels of the tile that are not converged */
    float max_e2;          /* the largest e2 among the tile's pixels, as a float; a NaN counts as +inf */
} ShmTileError;
typedef struct ShmAdaptiveParams {
    int32_t min_spp;     /* samples every tile receives before it may stop: a multiple of batch_spp, at least 2 * batch_spp */
    int32_t batch_spp;   /* samples per batch, >= 1 */
    float threshold;     /* relative standard error below which a pixel is converged: >= 0, +inf allowed */
    float floor;         /* > 0, finite: the least mean (film units: a lit white surface is near 1) the error is taken relative to */
    uint32_t reserved[4];
} ShmAdaptiveParams;
/* min_spp 16, batch_spp 4, threshold 0.05, floor 0.01 */
SHM_API int shm_adaptive_default_params(ShmAdaptiveParams* out);
/* Zero every record and set its prev to the device film AS IT STANDS: after shm_film_clear or in the middle of a render, the pass counts from here. The first
 * call allocates the records (96 bytes per pixel), which shm_scene_destroy frees. Blocking. */
SHM_API int shm_moments_clear(ShmScene* scene);
/* One batch: update the records of the tiles' pixels from the device film and write one ShmTileError per tile, in the tiles' order, to `out` (host memory,
 * n_tiles entries). The tiles are held to what shm_render_wave asks (inside pixel_bounds, disjoint). Blocking. SHM_ERR_INVALID_ARGUMENT, with the cause in
 * shm_last_error(): invalid tiles or parameters; no shm_moments_clear on the scene yet. */
SHM_API int shm_moments_update(ShmScene* scene, const ShmTile* tiles, uint32_t n_tiles, const ShmAdaptiveParams* params, ShmTileError* out);
/* Copy the records to a caller-allocated pixel_bounds-sized row-major array. */
SHM_API int shm_moments_read(ShmScene* scene, ShmMomentsPixel* out);
/* Host side (no GPU needed): 8 floats per record — v[3], s2[3], B, e2 (with `floor` as ShmAdaptiveParams::floor) — in sensor RGB (see above). */
SHM_API int shm_moments_resolve(const ShmMomentsPixel* moments, uint64_t n, float floor, float* out8);
/* The pass's CPU twin (no GPU needed): shm_moments_update on a read-back film (width x height, row-major, pixel_bounds (0, 0, width, height)) and records
 * updated in place. */
SHM_API int shm_moments_update_host(const ShmFilmPixel* film, ShmMomentsPixel* moments_in_out, int32_t width, int32_t height, const ShmTile* tiles, uint32_t n_tiles,
                                    const ShmAdaptiveParams* params, ShmTileError* tile_error_out);
/* A whole render that spends its samples by the measured error. params->samples_per_pixel is the CAP and the value every wave is launched with (so the
 * ray-differential scale and ZSobol's index width are the full render's). shm_film_clear and shm_moments_clear; min_spp / batch_spp base batches over all
 * tiles, each followed by shm_moments_update; then rounds: the tiles with unconverged > 0 and fewer samples than the cap get [spp, min(spp + batch_spp, cap))
 * and an update, until none is left. A tile that stops never returns, and every pixel receives its samples in increasing index: a tile that stopped at s holds
 * the bits of a plain render of [0, s). The film stays on the device (shm_film_read, the G-buffer pass and the denoiser take it as it is; pixels differ in
 * weight_sum). tile_spp_out (may be NULL): the samples tile i received. stats (may be NULL): the waves' sums. The cap must not be below min_spp.
 * One host synchronisation and one 8-byte-per-tile read-back per round. */
SHM_API int shm_render_adaptive(ShmScene* scene, const ShmRenderParams* params, const ShmTile* tiles, uint32_t n_tiles, const ShmAdaptiveParams* adaptive,
                                uint32_t* tile_spp_out, ShmStats* stats);
/* The denoiser's CPU twin with the records beside the film: shm_denoise_host for either variance_source (shm_denoise_host itself, which has no records, refuses
 * SHM_DENOISE_VARIANCE_MEASURED). `moments`: width x height records, as shm_moments_read gives them. */
SHM_API int shm_denoise_host_moments(const ShmFilmPixel* film, const ShmGBufferPixel* gbuffer, const ShmMomentsPixel* moments, int32_t width, int32_t height,
                                     const double white[3], const ShmDenoiseParams* params, ShmFilmPixel* out);

/* ---- temporal accumulation: the frame blended into a history reprojected through the G-buffer -----------
 * A pass over the frame just rendered, for a static scene under a moving camera (shm_scene_set_camera). Per pixel it takes c, the guide's validity, a_eff, the
 * render-space position P and the unit shading normal N exactly as the denoiser does; finds where P lay on the PREVIOUS frame's film — the motion vector
 * m = raster_prev(P) - raster_cur(P), so that a still camera gives m = 0 exactly and a history that is not blurred —; takes the four bilinear taps of the previous
 * frame's records around (x + 0.5 + m.x, y + 0.5 + m.y), of which one counts iff it is inside the film, its bilinear weight is above 0, its record has a history, dot(N, N_tap) >= normal_cos_min and
 * |dot(N, P_tap - P)| <= plane_tolerance * scale (scale: P's depth along the previous camera's axis for a perspective camera, 1 for an orthographic one); and blends:
 *   no tap counts   length = 1, rgb = c' (c, or c / a_eff when demodulating), m1 = l, m2 = l l with l the mean of c''s three channels
 *   otherwise       h = the taps' weighted mean; length = min(h.length + 1, max_history); a = max(1 / length, alpha_min); rgb = h.rgb + a (c' - h.rgb); m1 and m2 alike
 *                   with alpha_min_moments
 * The result is rgb a_eff. A pixel without a usable guide passes through (its result is c, bit for bit) and gets a record of length 0, which no later frame reads; a P
 * at or behind a perspective previous camera, or one whose motion is not finite, has no history. Gather only: no pixel writes another's record.
 * Device and CPU twin run the same header (shm/temporal.h) and give the same bits. */
typedef struct ShmTemporalParams {
    float alpha_min;          /* in [0, 1]: least weight of the new frame in the colour; 0 = a plain running mean up to max_history */
    float alpha_min_moments;  /* the same for the two luminance moments */
    float max_history;        /* >= 1: cap of the history length */
    float normal_cos_min;     /* in [-1, 1]: a tap is rejected when dot(N, N_tap) is below it */
    float plane_tolerance;    /* > 0, +inf allowed: a tap is rejected when |dot(N, P_tap - P)| > plane_tolerance * scale */
    float albedo_floor;       /* as ShmDenoiseParams::albedo_floor */
    uint32_t demodulate;      /* as ShmDenoiseParams::demodulate: accumulate c / a_eff and multiply the current a_eff back */
    uint32_t reserved[1];
} ShmTemporalParams;
typedef struct ShmTemporalPixel {   /* 64 bytes; one per pixel, twice per scene (ping-pong) */
    float rgb[3];     /* accumulated (demodulated) colour */
    float m1, m2;     /* accumulated luminance and luminance squared of the per-frame colour */
    float length;     /* history length; 0 = no history here (no guide this frame) */
    float p[3];       /* this frame's P, render space */
    float ns[3];      /* this frame's N, unit */
    uint32_t pad[4];
} ShmTemporalPixel;
/* alpha_min 0.2, alpha_min_moments 0.2, max_history 32, normal_cos_min 0.9, plane_tolerance 0.02, albedo_floor 0.01, demodulate 0 (at a few samples per pixel a pixel's a_eff
 * moves from frame to frame — most of all on an emitter's edge — and a history divided by one frame's a_eff and multiplied by another's is worse than the frame:
 * profiles/temporal.md) */
SHM_API int shm_temporal_default_params(ShmTemporalParams* out);
/* Forget the history: every record's length becomes 0 and the stored camera is dropped, so the next accumulate starts a history at every pixel. The first call
 * allocates the two record arrays and the result (160 bytes per pixel), which shm_scene_destroy frees. Blocking. */
SHM_API int shm_temporal_clear(ShmScene* scene);
/* One frame: the device film and the device G-buffer of the frame just rendered, and the records of the previous call, into the other record array and a device result;
 * then the scene's current camera is stored as the next call's previous camera. Neither the film nor the G-buffer is written. The first call on a scene, and the first
 * after shm_temporal_clear, has no previous camera and starts every history. Blocking; ms_out (may be NULL) receives the HIP-event time of the kernel.
 * SHM_ERR_INVALID_ARGUMENT, with the cause in shm_last_error(): no G-buffer wave since the scene's creation or the last shm_gbuffer_clear; the last G-buffer wave was
 * not SHM_GBUFFER_SPACE_RENDER; a parameter outside its range. SHM_ERR_UNSUPPORTED: a SHM_CAMERA_SPHERICAL scene. */
SHM_API int shm_temporal_accumulate_device(ShmScene* scene, const ShmTemporalParams* params, double* ms_out);
/* Copy the last result — rgb_sum the accumulated sensor RGB, weight_sum 1 (0 where the film's was 0) — or the records just written to a caller-allocated
 * pixel_bounds-sized row-major array (SHM_ERR_INVALID_ARGUMENT before the first shm_temporal_accumulate_device). */
SHM_API int shm_temporal_read(ShmScene* scene, ShmFilmPixel* out);
SHM_API int shm_temporal_read_history(ShmScene* scene, ShmTemporalPixel* out);
/* The CPU twin (no GPU needed): one frame from read-back buffers. history_in: the previous frame's records, or NULL for none (previous_camera is then not read and may
 * be NULL). Film coordinates are pixel_bounds' own: (0, 0, width, height). The outputs must not overlap the inputs. */
SHM_API int shm_temporal_accumulate_host(const ShmFilmPixel* film, const ShmGBufferPixel* gbuffer, const ShmTemporalPixel* history_in,
                                         const ShmCamera* camera, const ShmCamera* previous_camera, int32_t width, int32_t height, const double white[3],
                                         const ShmTemporalParams* params, ShmTemporalPixel* history_out, ShmFilmPixel* out);
/* The a-trous filter of shm_denoise_device over the temporal result in place of the film (it is a ShmFilmPixel array of weight 1, so the kernels take it as they take a
 * film); the result is read with shm_denoise_read. params->variance_source must be SHM_DENOISE_VARIANCE_SPATIAL. temporal_variance = 1 replaces the filter's initial
 * variance by max(0, m2 - m1^2) / length at every valid pixel whose record has length >= 4 (SVGF's rule) and keeps the 7x7 spatial estimate elsewhere; 0 is the plain
 * spatial filter of the accumulated image. SHM_ERR_INVALID_ARGUMENT before the first shm_temporal_accumulate_device, and as shm_denoise_device. */
SHM_API int shm_denoise_temporal_device(ShmScene* scene, const ShmDenoiseParams* params, uint32_t temporal_variance, double* ms_out);
/* Its CPU twin: `temporal` as shm_temporal_read gives it, `history` as shm_temporal_read_history does. */
SHM_API int shm_denoise_temporal_host(const ShmFilmPixel* temporal, const ShmGBufferPixel* gbuffer, const ShmTemporalPixel* history, int32_t width, int32_t height,
                                      const double white[3], const ShmDenoiseParams* params, uint32_t temporal_variance, ShmFilmPixel* out);

/* ---- the display pass: auto-exposure, tone mapping and 8-bit output on the device ------------------------
 * From a float film to a picture, while the film is still in HBM: 32 bytes per pixel in, 4 out. Per pixel, in this order:
 *   linear     rgb = rgb_sum / weight_sum (where the weight is not 0) times output_rgb_from_sensor_rgb: shm_film_get_image's arithmetic with write_fp16 = 0
 *   luminance  Y = 0.2126 R + 0.7152 G + 0.0722 B
 *   histogram  256 bins of log2(Y): bin 0 below log2_min, bin 255 at and above log2_max, bins 1 .. 254 of equal width between. A pixel counts iff its weight_sum is
 *              not 0 and Y is finite and above 0.
 *   exposure   the mean of the bins' centres (bins 0 and 255: log2_min and log2_max) over the counted mass between percentile_low N and percentile_high N, a bin that
 *              straddles an end counted in part; log2_target = log2(key) - mean, 0 where nothing counts
 *   adapt      log2_exposure = previous + (log2_target - previous) (1 - exp(-adaptation_rate dt)); log2_target itself when the scene has no valid state yet, dt <= 0 or
 *              adaptation_rate <= 0. scale = exposure 2^log2_exposure
 *   sanitise   c = c scale > 0 ? min(c scale, 65504) : 0 per channel: NaN and negative values become 0, +inf the reference's f16 cap
 *   tone       SHM_TONEMAP_NONE; SHM_TONEMAP_REINHARD: Yd = Y (1 + Y / white^2) / (1 + Y) on the luminance, every channel times Yd / Y; SHM_TONEMAP_ACES: Narkowicz's
 *              fit x (2.51 x + 0.03) / (x (2.43 x + 0.59) + 0.14) per channel. Then a clamp to [0, 1].
 *   transfer   SHM_TRANSFER_LINEAR, or SHM_TRANSFER_SRGB: v <= 0.0031308 ? 12.92 v : 1.055 v^(1 / 2.4) - 0.055
 *   quantise   floor(255 v + 0.5); with dither, floor(255 v + (b + 0.5) / 64), b the 8x8 recursive Bayer matrix at (x & 7, y & 7) of the pixel's film coordinates.
 *              The pixel is the four bytes R, G, B, 255 in memory order.
 * With auto_exposure = 0 the histogram, the exposure and the adaptation are skipped: scale = exposure, and neither the counts nor the state change.
 * Device and CPU twin run the same header (shm/display.h), with its own log2, log and exp, and give the same bits. */
#define SHM_DISPLAY_SOURCE_FILM 0u      /* the scene's film */
#define SHM_DISPLAY_SOURCE_DENOISED 1u  /* the denoiser's last result (shm_denoise_device / shm_denoise_temporal_device) */
#define SHM_DISPLAY_SOURCE_TEMPORAL 2u  /* the temporal pass's last result (shm_temporal_accumulate_device) */
#define SHM_TONEMAP_NONE 0u
#define SHM_TONEMAP_REINHARD 1u
#define SHM_TONEMAP_ACES 2u
#define SHM_TRANSFER_LINEAR 0u
#define SHM_TRANSFER_SRGB 1u
typedef struct ShmDisplayParams {   /* 96 bytes; offsets in the comments */
    uint32_t source;            /*  0: SHM_DISPLAY_SOURCE_* (the CPU twin takes its film as an argument and only checks the value) */
    uint32_t tonemap;           /*  4: SHM_TONEMAP_* */
    uint32_t transfer;          /*  8: SHM_TRANSFER_* */
    uint32_t auto_exposure;     /* 12: 0: scale = exposure; otherwise the histogram's exposure, adapted, times `exposure` as a compensation */
    uint32_t dither;            /* 16: 0 or not 0 */
    float exposure;             /* 20: > 0 */
    float key;                  /* 24: > 0: the luminance the metered mean is brought to */
    float white;                /* 28: > 0: SHM_TONEMAP_REINHARD's white point */
    float log2_min, log2_max;   /* 32, 36: the histogram's range, log2_min < log2_max */
    float percentile_low, percentile_high;   /* 40, 44: 0 <= low < high <= 1 */
    float adaptation_rate;      /* 48: per second; <= 0: no adaptation */
    float dt;                   /* 52: seconds since the previous frame; <= 0: no adaptation */
    float output_rgb_from_sensor_rgb[9];   /* 56: row-major 3x3, as shm_film_get_image takes it */
    uint32_t reserved[1];       /* 92 */
} ShmDisplayParams;
typedef struct ShmDisplayState {   /* 32 bytes */
    float log2_target;     /*  0: what the last auto-exposed frame metered */
    float log2_exposure;   /*  4: the adapted exposure: what the next frame adapts from */
    float scale;           /*  8: what that frame's colours were multiplied by */
    uint32_t counted;      /* 12: the pixels its histogram counted */
    uint32_t valid;        /* 16: 0: no auto-exposed frame yet (the next one jumps to its target) */
    uint32_t reserved[3];  /* 20 */
} ShmDisplayState;
/* source FILM, tonemap ACES, transfer SRGB, auto_exposure 0, dither 0, exposure 1, key 0.18, white 4, log2_min -16, log2_max 16 (about eight bins per stop),
 * percentiles 0.10 and 0.95, adaptation_rate 3, dt 0, the identity matrix */
SHM_API int shm_display_default_params(ShmDisplayParams* out);
/* Forget the adaptation state (and zero the counts): the next auto-exposed frame jumps to its target. The first call allocates the pass's buffers — the RGBA8 image,
 * the histogram's per-workgroup slabs, the 256 counts and the state — which shm_scene_destroy frees. Blocking. */
SHM_API int shm_display_clear(ShmScene* scene);
/* One frame: params->source into the scene's RGBA8 image, three launches with no host round trip between them (one with auto_exposure = 0). None of the three sources is
 * written. Blocking; state_out (may be NULL) receives the state as the call leaves it, ms_out (may be NULL) the HIP-event time of the launches.
 * SHM_ERR_INVALID_ARGUMENT, with the cause in shm_last_error(): a source that holds no result; a parameter outside its range. */
SHM_API int shm_display_device(ShmScene* scene, const ShmDisplayParams* params, ShmDisplayState* state_out, double* ms_out);
/* Copy the last image (one uint32_t per pixel: R | G << 8 | B << 16 | 255 << 24, pixel_bounds-sized, row-major) or the counts of the last auto-exposed frame to the host
 * (SHM_ERR_INVALID_ARGUMENT before the first shm_display_device). */
SHM_API int shm_display_read(ShmScene* scene, uint32_t* rgba8_out);
SHM_API int shm_display_read_histogram(ShmScene* scene, uint32_t counts_out[256]);
/* The RGBA8 image's device pointer and size in bytes, as shm_film_device_ptr gives the film's: for interop (SHM_ERR_INVALID_ARGUMENT before the first
 * shm_display_device or shm_display_clear: there is no buffer yet). */
SHM_API int shm_display_device_ptr(ShmScene* scene, void** ptr_out, uint64_t* bytes_out);
/* shm_display_device and shm_display_read in one call */
SHM_API int shm_display(ShmScene* scene, const ShmDisplayParams* params, uint32_t* rgba8_out, ShmDisplayState* state_out, double* ms_out);
/* The CPU twin (no GPU needed): one frame from a read-back film. state_in_out: the state before the frame and after it (NULL: no state, and none kept); counts_out
 * (may be NULL): the frame's 256 counts. With auto_exposure = 0 neither is read or written. */
SHM_API int shm_display_host(const ShmFilmPixel* film, int32_t width, int32_t height, const ShmDisplayParams* params, ShmDisplayState* state_in_out,
                             uint32_t* counts_out, uint32_t* rgba8_out);

/* ---- multi-GPU (ABI v7) -------------------------------------------------------------------------------------------
 * Pixels are independent and tile ownership is exclusive (the reference's one parallel region, integrator.rs:242-304, relies on that
 * for its unsynchronised film writes), so the frame shards by tiles with the scene replicated per GPU and NO collective while
 * rendering; one exchange at the end brings every rank's film rows to the root. Sharding is by blocks of whole tile rows, so a
 * rank's pixels are full-width row ranges of the film: only those rows travel (33 MB per rank of the 265 MB film at 3840x2160 on 8
 * GPUs), straight from one device film into the other, and no sum is needed. */

/* Static interleaved sharding of the row-major tile list Tile::tile emits: blocks of `rows_per_block` tile rows, block b belongs to
 * rank b % world. rows_per_block 0 = the default (about 16 blocks per rank: expensive image regions are spread over all ranks).
 * idx_out (capacity n_tiles) receives this rank's tile indices in increasing order. */
SHM_API int shm_shard_tiles(uint32_t n_tiles, uint32_t tiles_per_row, int32_t rank, int32_t world, int32_t rows_per_block,
                            uint32_t* idx_out, uint32_t* n_out);

/* One process per GPU (the layout of `torchrun` / MPI launches): an RCCL communicator per scene. The host distributes the 128-byte
 * unique id from rank 0 to every rank by whatever control channel it has (MPI_Bcast, a TCP store, a file: bench.py uses a directory of
 * files, shimmer_amd/launch.py), then every rank calls shm_dist_init (collective: ncclCommInitRank on the scene's device, then rank 0's
 * shard plan — tile rows per block — is broadcast, so that per-process environments cannot make block ownership differ between ranks). */
#define SHM_DIST_ID_BYTES 128
SHM_API int shm_dist_unique_id(uint8_t id_out[SHM_DIST_ID_BYTES]);
SHM_API int shm_dist_init(ShmScene* scene, int32_t rank, int32_t world, const uint8_t id[SHM_DIST_ID_BYTES]);
SHM_API int shm_dist_finalize(ShmScene* scene);   /* also done by shm_scene_destroy */
/* Whole ImageTileIntegrator::render of the scene's frame on `world` GPUs (collective): clears the device film, renders all spp-waves
 * of THIS rank's tiles (Tile::tile(pixel_bounds, 8, 8) sharded with shm_shard_tiles), then gathers the film rows of every rank into
 * rank 0's device film with one RCCL group (ncclRecv per block on the root, ncclSend on the owners; each peer -> root transfer rides its
 * own xGMI link). On return rank 0's device film (shm_film_read / shm_film_device_ptr) holds the complete frame, bit-identical to a
 * single-GPU render; the other ranks hold their own rows. stats (may be NULL) is this rank's. Without shm_dist_init it renders the
 * whole frame on this GPU (world = 1). */
SHM_API int shm_render_sharded(ShmScene* scene, const ShmRenderParams* params, ShmStats* stats);
/* Small collectives on the scene's communicator, so that a host needs NO second communication stack beside this library (bench.py runs
 * its barrier and its max-over-ranks clock through these; the only thing the host carries itself is the 128-byte id). Host values in,
 * host values out; they go through a 32 KB device scratch and ncclAllReduce / ncclAllGather on the render stream. Every wait polls the
 * stream and ncclCommGetAsyncError instead of blocking: a peer that died or never arrives becomes SHM_ERR_DEVICE after SHM_DIST_TIMEOUT_S
 * (default 900 s), and the communicator is aborted so that the other ranks' pending operations fail too. Without shm_dist_init (or with
 * a world of 1) they are the identity. */
enum { SHM_REDUCE_SUM = 0, SHM_REDUCE_MAX = 1, SHM_REDUCE_MIN = 2 };
SHM_API int shm_dist_barrier(ShmScene* scene);   /* this rank's streams drained, then one all-reduce: every rank arrived */
SHM_API int shm_dist_allreduce_f64(ShmScene* scene, double* values /* in / out */, uint32_t n /* <= 4096 */, int32_t op /* SHM_REDUCE_* */);
SHM_API int shm_dist_allgather_f64(ShmScene* scene, const double* mine, uint32_t n, double* all_out /* world * n <= 4096, rank-major */);
/* What this process runs on: the communicator as RCCL sees it and the shared objects the two runtimes were mapped from (a host process that
 * imported another ROCm stack before this library would show up here). scene may be NULL (library-wide fields only). */
typedef struct ShmDistInfo {
    int32_t rank, world;             /* as given to shm_dist_init (0, 1 without) */
    int32_t rccl_ranks;              /* ncclCommCount of the communicator (0 without one) */
    int32_t rccl_device;             /* ncclCommCuDevice */
    int32_t rccl_version;            /* ncclGetVersion: e.g. 22707 */
    int32_t hip_runtime_version;     /* hipRuntimeGetVersion */
    int32_t rows_per_block;          /* tile rows per shard block in use (rank 0's, broadcast at shm_dist_init) */
    uint32_t n_my_tiles;             /* tiles this rank owns */
    char librccl_path[256];          /* dladdr of ncclGetVersion */
    char libamdhip_path[256];        /* dladdr of hipRuntimeGetVersion */
} ShmDistInfo;
SHM_API int shm_dist_info(ShmScene* scene, ShmDistInfo* out);
SHM_API int shm_device_synchronize(int32_t device);   /* hipDeviceSynchronize on that ordinal */
/* Test entry: sends this rank's film rows to ITSELF through the same RCCL send / recv group into a scratch film and compares
 * (exercises the RCCL transport on a one-GPU box). SHM_OK when every byte matches. */
SHM_API int shm_dist_selftest(ShmScene* scene);

/* One process, n devices: the same frame with one host thread and one scene replica per entry of `devices` (HIP ordinals; an ordinal may
 * repeat, which shares that GPU between two replicas — used by the tests on a one-GPU box), tiles sharded as above, film rows gathered
 * into the first device's film with hipMemcpyPeerAsync over xGMI, then read back. film_out: pixel_bounds-sized, overwritten.
 * stats_per_device: n_devices entries or NULL. A C-only caller renders on every GPU of a node with this one call. */
SHM_API int shm_render_multi(const ShmSceneDesc* desc, const int32_t* devices, int32_t n_devices, const ShmRenderParams* params,
                             ShmFilmPixel* film_out, ShmStats* stats_per_device);

SHM_API const char* shm_last_error(void);   /* thread-local, never NULL */
SHM_API int shm_device_count(void);

/* ---- host-side mirror of the reference's scene-construction steps (no GPU needed) ------------- */

/* BvhAggregate::new (aggregate.rs:207-467): recursive build (split_method 0 = middle, 1 = equal counts),
 * 1-primitive leaves, DFS flatten.  prim_bounds: 6 floats (min xyz, max xyz) per input primitive.
 * nodes_out capacity 2*n-1; prim_order_out[n] receives, per leaf-order slot, the input primitive index. */
SHM_API int shm_bvh_build(const float* prim_bounds, uint32_t n, int split_method, ShmBvhNode* nodes_out,
                  uint32_t* n_nodes_out, uint32_t* prim_order_out);
/* Test entry: the Bounds3f operations the builder is made of (union, union_point, surface_area, volume, max_dimension; bounding_box.rs:394-446),
 * for the reference's own vectors (bounding_box.rs:699-733, 950-995). a, b: {min xyz, max xyz}. out[16]: union(a, b) min, max | union_point(a, p)
 * min, max | surface_area(a), volume(a), max_dimension(a), 0. */
SHM_API int shm_bounds3_probe(const float a[6], const float b[6], const float p[3], float out[16]);
/* (The DEVICE test entry of rounds 4-5, shm_debug_eval_leaf, lives in the test library libshimmer_hip_probe.so since round 6: include/shimmer_hip_probe.h.) */
/* Tile::tile (tile.rs:21-104). tiles_out capacity ceil(w/tw)*ceil(h/th); returns the count via n_out. */
SHM_API int shm_tile_bounds(const int32_t pixel_bounds[4], int32_t tile_w, int32_t tile_h, ShmTile* tiles_out,
                    uint32_t* n_out);
/* PerspectiveCamera::new + CameraTransform (camera.rs:893-963, 507-523, 594-642) for a world_from_camera
 * matrix, fov (degrees), screen window derived from the aspect ratio (camera.rs:848-864). Rendering
 * coordinate system: CameraWorld (the reference default, options.rs). */
SHM_API int shm_camera_perspective(const float world_from_camera[16], float fov_deg, const int32_t full_resolution[2],
                           float lens_radius, float focal_distance, ShmCamera* out,
                           float render_from_world_out[16]);
/* OrthographicCamera::new (camera.rs:713-744) with Transform::orthographic(0, 1) and the same screen window / CameraWorld
 * conventions. lens_radius / focal_distance are stored but unused, as in the reference. */
SHM_API int shm_camera_orthographic(const float world_from_camera[16], const int32_t full_resolution[2], float lens_radius,
                            float focal_distance, ShmCamera* out, float render_from_world_out[16]);
/* The same two constructors with the rest of what Camera::create reads (camera.rs:676-705, 848-890) and the rendering space of
 * CameraTransform::new (camera.rs:507-523; Option "rendercoordsys"): */
enum { SHM_RENDER_SPACE_CAMERA_WORLD = 0, SHM_RENDER_SPACE_CAMERA = 1, SHM_RENDER_SPACE_WORLD = 2 };
typedef struct ShmCameraParams {
    uint32_t kind;                /* SHM_CAMERA_PERSPECTIVE / SHM_CAMERA_ORTHOGRAPHIC */
    uint32_t render_space;        /* SHM_RENDER_SPACE_* */
    float world_from_camera[16];  /* row-major */
    float fov_deg;                /* perspective only */
    int32_t full_resolution[2];
    float lens_radius, focal_distance;
    float frame_aspect_ratio;     /* "frameaspectratio"; 0 = x / y of the film */
    uint32_t has_screen_window;
    float screen_window[4];       /* "screenwindow" as the file gives it: x0 x1 y0 y1 */
} ShmCameraParams;
SHM_API int shm_camera_create(const ShmCameraParams* params, ShmCamera* out, float render_from_world_out[16]);
/* shm_camera_create with the render space GIVEN instead of chosen by params->render_space (which is not read): render_from_camera = render_from_world *
 * world_from_camera, in double; camera_from_render and the four minimum differentials are filled as above. For a second camera in the render space an existing
 * scene's geometry was baked in (shm_scene_set_camera). With the render_from_world a shm_camera_create call returned for the same parameters it gives that call's
 * ShmCamera bit for bit under SHM_RENDER_SPACE_CAMERA_WORLD and SHM_RENDER_SPACE_WORLD, whose matrix (a translation, the identity) is exact in float; under
 * SHM_RENDER_SPACE_CAMERA the returned matrix is a rounded inverse and the two agree to that rounding. SHM_ERR_INVALID_ARGUMENT for a singular matrix. */
SHM_API int shm_camera_create_in(const ShmCameraParams* params, const float render_from_world[16], ShmCamera* out);
/* PBRT-v4's SphericalCamera for a world_from_camera matrix: `mapping` is SHM_SPHERICAL_*, `render_space` SHM_RENDER_SPACE_* (the same CameraTransform as above). Fills
 * camera_from_raster as described at ShmCamera, camera_from_render and the four minimum differentials (the same 512-sample loop, over this camera's rays).
 * SHM_ERR_INVALID_ARGUMENT for a mapping above 1, a resolution below 1 or a render space above 2. */
SHM_API int shm_camera_spherical(const float world_from_camera[16], uint32_t mapping, const int32_t full_resolution[2], uint32_t render_space, ShmCamera* out,
                                 float render_from_world_out[16]);
/* C entry to the C++ host mirror of the reference's integrator interface (shimmer_amd/csrc/host/integrator.hpp):
 * create_integrator(name, {maxdepth, regularize, lightsampler "uniform", spp}, scene)->render(options), integrator.rs:16-42,
 * 52-54, 120-210, 226-322. `name`: "path", "simplepath" (sample_lights / sample_bsdf are its "samplelights" / "samplebsdf") or
 * "randomwalk";
 * anything else fails the way the reference panics ("Unknown integrator ..."); the message
 * is available through shm_last_error(). film_out: pixel_bounds-sized, overwritten; n_waves_out: spp-waves rendered. */
SHM_API int shm_integrator_render(const char* name, const ShmSceneDesc* scene, int device, int32_t max_depth, int regularize,
                          int sample_lights, int sample_bsdf, int32_t samples_per_pixel, int32_t seed, int disable_pixel_jitter,
                          int disable_wavelength_jitter, ShmFilmPixel* film_out, ShmStats* stats_out, int32_t* n_waves_out);
/* RgbFilm::get_image / get_pixel_rgb (film.rs:647-707, 720-738) over a read-back film: rgb = sum / weight_sum (when the
 * weight is non-zero), plus the (here always zero) splat term, times output_rgb_from_sensor_rgb (film.rs:524; row-major 3x3,
 * passed by the caller, who owns the colour space), with the reference's f16 clamp when write_fp16 is set (film.rs:676-690,
 * including its `rgb.g > max -> rgb.r = max` assignment). rgb_out: 3 floats per pixel, same order as `film`. */
SHM_API int shm_film_get_image(const ShmFilmPixel* film, uint64_t n_pixels, const float output_rgb_from_sensor_rgb[9], int write_fp16,
                       float* rgb_out);
/* Image::write_pfm (image.rs:1333-1377): RGB float, bottom-up rows, little-endian (scale -1). */
SHM_API int shm_write_pfm(const char* path, const float* rgb, int32_t width, int32_t height);
/* An 8-bit RGB PNG (colour type 2, rows top-down) of an RGBA8 image as shm_display_read gives it; the alpha byte is dropped. Stored deflate blocks: no compression and
 * no dependency. SHM_ERR_INVALID_ARGUMENT: a null argument, an empty image, a path that cannot be opened. */
SHM_API int shm_write_png(const char* path, const uint32_t* rgba8, int32_t width, int32_t height);
/* TriQuadMesh::read_ply (shape/mesh.rs:179-358; the "plymesh" shape, shape/shape.rs:97-135): vertex element with float x y z
 * [nx ny nz] [u v | s t | texture_u texture_v | texture_s texture_t], face element with an int list vertex_indices /
 * vertex_index (triangles and quads; a quad v0 v1 v2 v3 is stored in bilinear-patch order v0 v1 v3 v2) and optionally
 * face_indices. ascii, binary_little_endian and binary_big_endian. n and uv are ALWAYS n_vertices long, zero where the file has
 * no such property — the reference builds them the same way and hands both to the meshes (shape/shape.rs:104-131). Anything
 * the reference panics on (other elements, non-float vertex properties, unsigned index lists, faces that are neither triangles
 * nor quads, indices out of range) returns SHM_ERR_INVALID_ARGUMENT with the message in shm_last_error(). Free with shm_ply_free. */
typedef struct ShmPlyMesh {
    uint32_t n_vertices, n_tri_indices, n_quad_indices, n_face_indices;
    float* p;               /* 3 * n_vertices */
    float* n;               /* 3 * n_vertices */
    float* uv;              /* 2 * n_vertices */
    int32_t* tri_indices;   /* n_tri_indices  (3 per triangle) */
    int32_t* quad_indices;  /* n_quad_indices (4 per quad, patch order) */
    int32_t* face_indices;  /* n_face_indices */
} ShmPlyMesh;
SHM_API int shm_ply_read(const char* filename, ShmPlyMesh* out);
SHM_API void shm_ply_free(ShmPlyMesh* mesh);

/* ---- PBRT-v4 scene front end (ABI v7) ------------------------------------------------------------------------------
 * The reference's loader (loading/tokenizer.rs, parser.rs:216-351, parser_target.rs:50-184, scene.rs:1221-2033) restated in C++ for the
 * directive set the repository's scenes use: transforms (LookAt Translate Scale Rotate Identity Transform ConcatTransform CoordinateSystem
 * CoordSysTransform ReverseOrientation), Camera (perspective / orthographic, incl. frameaspectratio / screenwindow), Film (rgb, whitebalance),
 * Attribute, Option (incl. rendercoordsys), Sampler (independent / zsobol), PixelFilter (box gaussian mitchell sinc triangle),
 * Integrator (path / simplepath / randomwalk), Option, WorldBegin, AttributeBegin / End, Material / MakeNamedMaterial / NamedMaterial
 * (diffuse conductor dielectric thindielectric coateddiffuse coatedconductor mix, "normalmap"), Texture (float / spectrum: constant scale
 * mix directionmix imagemap — with the uv / spherical / cylindrical / planar mappings —, PBRT-v4's procedural checkerboard dots (float / spectrum) fbm windy bilerp (float);
 * marble, ptex, spectrum bilerp: SHM_ERR_UNSUPPORTED), AreaLightSource (diffuse), LightSource (point,
 * spot, distant — the two as PBRT-v4 defines them —, infinite: uniform or an environment image), Shape (trianglemesh bilinearmesh sphere plymesh), ObjectBegin / ObjectEnd / ObjectInstance,
 * Include — with the reference's parameter names and defaults. Spectra: "float", "spectrum" (lambda / value pairs, a named spectrum or a
 * spectrum file), "blackbody", and "rgb" as RgbAlbedo / RgbUnbounded / RgbIlluminantSpectrum by the slot that reads it (paramdict.rs:605-656)
 * through the sRGB rgb2spec coefficient table — the `.spec` file the reference loads from rgbtospec/srgb.spec (rgb_to_spectra.rs:27-31),
 * looked for in $SHM_RGB2SPEC_SRGB, <scene dir>/rgbtospec/srgb.spec, ./rgbtospec/srgb.spec, then the table tools/gen_rgb2spec.py writes
 * beside this library. Image files are PNG, the one format the reference reads (image.rs:1140-1311), decoded and turned into MIP pyramids
 * exactly as Image::read / MIPMap::create_from_file / Image::generate_pyramid do (host/image_io.hpp). What the reference leaves todo!() or
 * this backend does not take (media, Import, portals, animated transforms, other colour spaces) is SHM_ERR_UNSUPPORTED: nothing is silently
 * rendered as something else. Errors carry file:line in shm_last_error(). The returned description owns every array it points to; free
 * it with shm_pbrt_free. */
typedef struct ShmPbrtScene {
    ShmSceneDesc desc;          /* ready for shm_scene_create */
    ShmRenderParams params;     /* Sampler "pixelsamples" / "seed", Integrator "maxdepth" / "regularize" / "samplelights" / "samplebsdf", Option flags */
    char integrator[32];        /* "path" (default), "simplepath", "randomwalk": the name create_integrator receives */
    char output_filename[256];  /* Film "filename" (default "shimmer.pfm", film.rs:232-243) */
    void* owner;                /* the loader's storage */
    float output_rgb_from_sensor_rgb[9]; /* RgbFilm::new (film.rs:524): rgb_from_xyz of sRGB (from its primaries and the D65 white, colorspace.rs:38-72)
                                   times the sensor's matrix — the identity, or the von Kries white balance of Film "whitebalance" (color.rs:404-416,
                                   the illuminant from DenselySampledSpectrum::d, spectrum.rs:215-262). Row-major; what shm_film_get_image takes. */
} ShmPbrtScene;
SHM_API int shm_scene_load_pbrt(const char* path, ShmPbrtScene** out);
/* The same from a string; base_dir (may be NULL) resolves Include and plymesh file names. */
SHM_API int shm_scene_parse_pbrt(const char* text, const char* base_dir, ShmPbrtScene** out);
SHM_API void shm_pbrt_free(ShmPbrtScene* scene);
/* Test entries (the front end's own tokenizer and parameter-list parser, exposed so that the reference's in-source vectors —
 * loading/tokenizer.rs:126-260, token.rs:218-290, param.rs:214-260, parser.rs:656-870 — can be replayed against them):
 * shm_pbrt_tokenize writes every token as <kind letter><token text as the reference's Token holds it, quotes kept><NUL>; kinds: D a
 * directive name (Token::is_directive), W another bare word, S a quoted string (Token::is_quote), B a bracket, Q an opening quote without
 * its partner (the rest of the input, as tokenizer.rs yields it; the loader proper reports it as an error, as the reference's parser does).
 * shm_pbrt_parse_params parses a parameter list (`"type name" value | [ values ]` ...) and writes it as JSON:
 * [{"type", "name", "floats", "ints", "bools", "strings"}] (ParsedParameter, paramdict.rs). */
SHM_API int shm_pbrt_tokenize(const char* text, char* out, uint64_t capacity, uint32_t* n_tokens);
SHM_API int shm_pbrt_parse_params(const char* text, char* out_json, uint64_t capacity);
/* Two pieces of the front end the scene generators of this repository share with the loader, so that both hand the library bit-identical
 * inputs: DenselySampledSpectrum::new(BlackbodySpectrum::new(T)) at 360..=830 nm (spectra/spectrum.rs:430-489) and the world_from_camera
 * matrix of Transform::look_at (transform.rs:270-303), both in f32 as the reference computes them. */
SHM_API int shm_blackbody_dense(float temperature_kelvin, float out471[471]);
SHM_API int shm_look_at(const float eye[3], const float look[3], const float up[3], float world_from_camera_out[16]);
/* The image side of the front end for hosts that fill ShmSceneDesc themselves: Image::read (PNG; `encoding` "sRGB" / "linear" / "gamma <g>",
 * NULL = "sRGB"; image.rs:1140-1311, color.rs:487-525), then — with build_pyramid — MIPMap::create_from_file's channel selection and
 * Image::generate_pyramid for the wrap mode (mipmap.rs:42-99, image.rs:699-802, 1007-1138). Levels come finest first with texel offsets
 * relative to `texels`; channels: 1 ("Y") or 3 (R, G, B; an alpha plane is dropped — file_channels says what the file held, 4 with
 * build_pyramid meaning the alpha was not all ones). has_color_space: the RGB PNG's sRGB colour space (ImageMetadata::color_space). */
typedef struct ShmLoadedImage {
    uint32_t n_levels, n_channels, file_channels, has_color_space;
    uint64_t n_texel_floats;
    ShmImageLevel* levels;
    float* texels;
} ShmLoadedImage;
SHM_API int shm_image_load_png(const char* path, const char* encoding, uint32_t wrap /* SHM_WRAP_* */, int build_pyramid, ShmLoadedImage* out);
SHM_API void shm_image_free(ShmLoadedImage* image);

#ifdef __cplusplus
}
#endif
#endif /* SHIMMER_HIP_H */
