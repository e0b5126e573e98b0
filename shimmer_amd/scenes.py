"""Seeded synthetic scenes for the BASELINE.json configs (the reference's own scenes live in an external repo
and are not available offline; SURVEY §8d defines these stand-ins).

  S1 sphere_light   unit diffuse sphere + one-sided quad area light            (C1, 128x128x4)
  S2 cornell_box    Cornell-style box, 32 triangles                            (C2, 512x512x64)
  S3 ganesha_proxy  displaced cube-sphere, 4 305 612 tris + room (16 tris)     (C3/C5, 1024x1024x256 / 4K)
  S4 crown_proxy    dispersive dielectric icospheres + rough gold + floor      (C4, maxdepth 32)
  three_spheres     the reference's own BVH known-answer scene (aggregate.rs:631-702)

All geometry is generated in world space and moved to render space with the camera-world translation
(camera.rs:507-523), as TriangleMesh::new does at load time (shape/mesh.rs:43-46).

Every builder takes `film`: keyword arguments for SceneBuilder.set_film, e.g. film=dict(filter="gaussian") or
film=dict(filter="mitchell", filter_radius=(2.0, 1.5), filter_params=(0.5, 0.25)); the default is the box filter.
"""
import functools
from types import SimpleNamespace

import numpy as np

from . import abi
from .scene import SceneBuilder, blackbody_dense, f32


def _to_render(p, rfw):
    """render_from_world is a pure translation here: apply_point_helper in f32 (transform.rs:742-752)."""
    p = np.asarray(p, np.float32)
    t = rfw[:3, 3].astype(np.float32)
    return (p + t[None, :]).astype(np.float32)


def _quad(p0, p1, p2, p3):
    """Two triangles (p0,p1,p2), (p0,p2,p3)."""
    return np.array([p0, p1, p2, p3], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def _merge(parts):
    ps, vis, base = [], [], 0
    for p, vi in parts:
        ps.append(p)
        vis.append(vi + base)
        base += p.shape[0]
    return np.concatenate(ps).astype(np.float32), np.concatenate(vis).astype(np.uint32)


def _box(lo, hi, faces="xXyYzZ"):
    """Axis-aligned box faces with outward normals (counter-clockwise seen from outside)."""
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    f = {
        "x": [(x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)],
        "X": [(x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)],
        "y": [(x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)],
        "Y": [(x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)],
        "z": [(x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)],
        "Z": [(x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)],
    }
    return _merge([_quad(*f[c]) for c in faces])


def _finish(b, lib, extra_lights=None, rfw=None, **extra):
    """`extra_lights(builder, render_from_world)` (the generators' optional argument) appends lights AFTER the scene's own; absent, the description is
    byte for byte what the generator always produced."""
    if extra_lights is not None:
        extra_lights(b, rfw)
    desc, info = b.build(lib)
    return SimpleNamespace(desc=desc, builder=b, info=info, **extra)


def _set_camera(b, lib, camera, pos, look_at, up, fov):
    """The generators' optional `camera=` argument REPLACES the scene's own camera (given here as pos, look_at, up, fov); absent, the description is byte for byte
    what the generator always produced. A dict: "type" — "spherical" (PBRT-v4's SphericalCamera, with "mapping": "equalarea" | "equirectangular"), "perspective" or
    "orthographic" —, and optionally "pos", "look_at", "up" (world space; default: the scene's own), "fov", "lens_radius", "focal_distance" (the projective two)."""
    if camera is None:
        return b.set_camera_look_at(lib, pos, look_at, up, fov)
    unknown = set(camera) - {"type", "pos", "look_at", "up", "mapping", "fov", "lens_radius", "focal_distance"}
    if unknown or camera.get("type") not in ("spherical", "perspective", "orthographic"):
        raise ValueError(f"camera: unknown key(s) {sorted(unknown)} or type {camera.get('type')!r} (spherical, perspective, orthographic)")
    pos, look_at, up = camera.get("pos", pos), camera.get("look_at", look_at), camera.get("up", up)
    if camera["type"] == "spherical":
        return b.set_camera_spherical(lib, pos, look_at, up, mapping=camera.get("mapping", "equalarea"))
    return b.set_camera_look_at(lib, pos, look_at, up, camera.get("fov", fov), lens_radius=camera.get("lens_radius", 0.0), focal_distance=camera.get("focal_distance", 1e6),
                                orthographic=camera["type"] == "orthographic")


def spot_and_distant(spot_from=(0.4, 1.6, 0.6), spot_to=(0.0, 0.0, 0.0), coneangle=35.0, conedelta=10.0, spot_scale=8.0, sun_from=(1.0, 2.0, 1.5), sun_to=(0.0, 0.0, 0.0),
                     sun_scale=1.5, spot=True, distant=True):
    """An `extra_lights` argument for the generators below: PBRT-v4's spot light and / or distant light, given in WORLD space."""
    def add(b, rfw):
        if spot:
            b.light_spot(spot_from, spot_to, blackbody_dense(3200.0), scale=spot_scale, coneangle=coneangle, conedelta=conedelta, render_from_object=rfw)
        if distant:
            b.light_distant(blackbody_dense(5500.0), scale=sun_scale, frm=sun_from, to=sun_to, render_from_object=rfw)
    return add


def sphere_light(lib, width=128, height=128, film=None):
    """S1 (config C1)."""
    b = SceneBuilder()
    b.set_film(width, height, **(film or {}))
    rfw = b.set_camera_look_at(lib, (0, 1, 5), (0, 0, 0), (0, 1, 0), 40.0)
    grey = b.material_diffuse(0.5)
    black = b.material_diffuse(0.0)
    rfo = np.eye(4, dtype=np.float32)
    rfo[:3, 3] = rfw[:3, 3]
    b.add_sphere(1.0, grey, render_from_object=rfo)
    # 2x2 quad at y=3 facing -y (one-sided): winding chosen so that normalize(dp02 x dp12) points down
    p, vi = _quad((-1, 3, -1), (1, 3, -1), (1, 3, 1), (-1, 3, 1))
    b.add_mesh(_to_render(p, rfw), vi, black, emission=blackbody_dense(6500.0), emission_scale=10.0)
    # a floor so that paths do more than one bounce
    pf, vif = _quad((-4, -1, -4), (-4, -1, 4), (4, -1, 4), (4, -1, -4))
    b.add_mesh(_to_render(pf, rfw), vif, grey)
    return _finish(b, lib, name="S1 sphere+area light")


def _two_point_spectrum(b, lo, hi):
    """Red/green walls as 2-knot piecewise-linear reflectances."""
    return b.spectrum_piecewise(np.array([359.0, 831.0], np.float32), np.array([lo, hi], np.float32))


def test_image(size=64, channels=3, seed=7):
    """A deterministic float test image (row 0 = top): a checker of soft colours modulated by value noise, every value in
    [0.05, 0.95] (no exact zeros: rgb2spec's published fetch divides by the largest component)."""
    y, x = np.mgrid[0:size, 0:size]
    checker = (((x // max(1, size // 8)) + (y // max(1, size // 8))) & 1).astype(np.float64)
    pts = np.stack([x.ravel() / size, y.ravel() / size, np.zeros(size * size)], axis=1)
    noise = _value_noise(pts, seed, octaves=2).reshape(size, size)
    base = np.stack([0.15 + 0.7 * checker, 0.25 + 0.5 * (x / (size - 1.0)), 0.8 - 0.6 * checker * (y / (size - 1.0))], axis=2)
    img = np.clip(base + 0.25 * noise[..., None], 0.05, 0.95).astype(np.float32)
    return img[..., 1].copy() if channels == 1 else img


def cornell_box(lib, width=512, height=512, coated=False, mix=False, patches=False, patch_skew=0.0, textured=False,
                texture_filter=None, textured_coated_ceiling=True, glass=False, emitter_reflects=False, environment=None, glass_too=False, film=None, extra_lights=None,
                diffuse_transmission=None, camera=None):
    """S2 (config C2): 5 walls x 2 + 2 boxes x 5 faces x 2 + light 2 = 32 triangles.
    coated=True: the tall box becomes CoatedConductor (rough interface, Cu), the short one CoatedDiffuse with a scattering
    medium between the interfaces, the floor CoatedDiffuse with a smooth interface (SURVEY §8f-1 materials).
    diffuse_transmission: PBRT-v4's diffuse transmission material (absent, the description is byte for byte what the generator always produced) — a string of words:
      "sheet"     a back-lit sheet hangs between the camera and the boxes (wavelength-dependent R and T)
      "textured"  ... its transmittance an image texture, its reflectance a checkerboard, both under a `scale` of 0.9
      "mixed"     ... the sheet is a MixMaterial of two diffuse transmission materials
      "tall"      the tall box is diffuse transmission
      "gold"      the short box is a rough gold conductor
      "sphere"    a diffuse transmission sphere stands on the short box
      "all"       every DiffuseMaterial of the room — walls, boxes, the emitter's — is diffuse transmission instead: no plain diffuse material is left"""
    dt = set((diffuse_transmission or "").split())
    assert dt <= {"sheet", "textured", "mixed", "tall", "gold", "sphere", "all"}
    b = SceneBuilder()
    b.set_film(width, height, **(film or {}))
    rfw = _set_camera(b, lib, camera, (0, 1, 3.4), (0, 1, 0), (0, 1, 0), 39.0)
    if "all" in dt:
        white = b.material_diffuse_transmission(0.6, 0.15)
        red = b.material_diffuse_transmission(_two_point_spectrum(b, 0.05, 0.6), _two_point_spectrum(b, 0.0, 0.15))
        green = b.material_diffuse_transmission(_two_point_spectrum(b, 0.5, 0.08), 0.1)
        black = b.material_diffuse_transmission(0.0, 0.0)
    else:
        white = b.material_diffuse(0.75)
        red = b.material_diffuse(_two_point_spectrum(b, 0.05, 0.75))
        green = b.material_diffuse(_two_point_spectrum(b, 0.6, 0.08))
        black = b.material_diffuse(0.0)
    tall_m = short_m = floor_m = white
    if coated:
        tall_m = b.material_coated_conductor(interface_roughness=0.05, conductor_roughness=0.2, thickness=0.02)
        short_m = b.material_coated_diffuse(reflectance=_two_point_spectrum(b, 0.1, 0.7), roughness=0.1, thickness=0.05, albedo=0.6, g=0.3)
        floor_m = b.material_coated_diffuse(reflectance=0.6, roughness=0.0, eta=b.spectrum_named("glass-BK7"))
    if glass:  # every kind of dielectric interface in one scene: smooth + dispersive, rough, index-matched, thin (the specular / rough scatter kernels)
        tall_m = b.material_dielectric(b.spectrum_named("glass-BK7"))
        short_m = b.material_dielectric(1.5, roughness=0.3)
        floor_m = b.material_mix(white, b.material_dielectric(1.0, roughness=0.2), 0.7)
    if mix:  # MixMaterial (material.rs:1288-1330): a plain two-way mix, and a nested one whose leaves include a coated material
        gold = b.material_conductor(b.spectrum_named("metal-Au-eta"), b.spectrum_named("metal-Au-k"), roughness=0.3)
        short_m = b.material_mix(white, gold, 0.5)
        tall_m = b.material_mix(b.material_mix(red, green, 0.3), b.material_coated_diffuse(reflectance=0.7, roughness=0.1), 0.6)
        floor_m = b.material_mix(white, black, 0.0)  # amount <= 0: always the first
    ceil_m, back_m, left_m, right_m = white, white, red, green
    if "tall" in dt:
        tall_m = b.material_diffuse_transmission(_two_point_spectrum(b, 0.1, 0.5), _two_point_spectrum(b, 0.6, 0.2))
    if "gold" in dt:
        short_m = b.material_conductor(b.spectrum_named("metal-Au-eta"), b.spectrum_named("metal-Au-k"), roughness=0.3)
    if glass_too:  # beside whatever else the scene holds (coated boxes, ...): a smooth glass short box and a rough dielectric left wall — the dielectric class's specular AND general kernels
        short_m = b.material_dielectric(1.5)
        left_m = b.material_dielectric(1.5, roughness=0.3)
    if glass:
        left_m = b.material_mix(red, b.material_dielectric(1.33, thin=True), 0.5)
    if textured:
        # SpectrumImageTexture on every wall, one combination of mapping / filter / wrap / spectrum type each; the
        # tall box is a mirror and the short one glass so that specular reflection AND transmission differentials reach textures
        tf = (lambda default: texture_filter or default)
        img3, img1 = test_image(64, 3), test_image(32, 1, seed=11)
        to_render = np.asarray(rfw, np.float32).reshape(4, 4)
        floor_m = b.material_diffuse(b.add_image_texture(img3, filter=tf("ewa"), wrap="repeat", su=3.0, sv=3.0))
        back_m = b.material_diffuse(b.add_image_texture(img1, filter=tf("trilinear"), wrap="clamp", color_space=False))
        left_m = b.material_diffuse(b.add_image_texture(img3, filter=tf("point"), wrap="repeat", spectrum_type="unbounded", scale=0.9,
                                                        mapping="planar", vs=(0.0, 0.5, 0.0), vt=(0.0, 0.0, 0.5), du=0.1, dv=0.2,
                                                        texture_from_render=np.linalg.inv(to_render.astype(np.float64))))
        right_tex = b.add_image_texture(img3, filter=tf("bilinear"), wrap="black", spectrum_type="illuminant", scale=0.8,
                                        mapping="spherical", texture_from_render=np.linalg.inv(to_render.astype(np.float64)))
        # a composite spectrum texture (texture.rs:536-687): the image mixed with a smooth spectrum by a float image, then dimmed by direction
        right_m = b.material_diffuse(b.stex_direction_mix(b.stex_mix(right_tex, _two_point_spectrum(b, 0.6, 0.08), b.ftex_image(img1, filter=tf("point"))),
                                                          b.stex_scaled(0.5, 0.5), dir=(1.0, 0.0, 0.0)))
        ceil_tex = b.add_image_texture(img3, filter=tf("ewa"), invert=True, mapping="cylindrical", max_anisotropy=4.0, wrap="octahedralsphere",
                                       texture_from_render=np.linalg.inv(to_render.astype(np.float64)))
        if textured_coated_ceiling:
            ceil_m = b.material_coated_diffuse(reflectance=ceil_tex, roughness=0.2, albedo=b.add_image_texture(img1, filter=tf("bilinear")), thickness=0.05)
        else:  # no LayeredBxDF anywhere: the scene class of the lighter textured shade instantiation
            ceil_m = b.material_conductor(b.spectrum_named("metal-Al-eta"), b.spectrum_named("metal-Al-k"), roughness=0.3)
        tall_m = b.material_conductor(b.spectrum_named("metal-Ag-eta"), b.spectrum_named("metal-Ag-k"), roughness=0.0)
        short_m = b.material_dielectric(1.5)
        # float textures (texture.rs:88-403) on the float parameters, a bump map and a normal map (interaction.rs:223-245):
        bump = b.ftex_scaled(b.ftex_image(img1, filter=tf("bilinear"), su=2.0, sv=2.0), 0.03)
        b.set_float_texture(floor_m, abi.SHM_FLOATSLOT_DISPLACEMENT, bump)              # every DiffuseMaterial has a displacement slot
        b.set_float_texture(back_m, abi.SHM_FLOATSLOT_DISPLACEMENT, b.ftex_image(img3, filter=tf("ewa"), scale=0.02))  # RGB image as a float: channel 0 / average
        rough = b.ftex_mix(0.05, b.ftex_image(img1, filter=tf("trilinear"), invert=True), b.ftex_direction_mix(0.2, 0.8, dir=(0.0, -1.0, 0.0)))
        b.set_float_texture(ceil_m, abi.SHM_FLOATSLOT_U_ROUGHNESS, rough)
        b.set_float_texture(ceil_m, abi.SHM_FLOATSLOT_THICKNESS, b.ftex_scaled(b.ftex_image(img1, filter=tf("point")), 0.1))
        b.set_float_texture(ceil_m, abi.SHM_FLOATSLOT_G, b.ftex_constant(0.3))
        nm = np.stack([0.5 + 0.25 * np.sin(np.arange(16) * 0.8)[None, :].repeat(16, 0), 0.5 + 0.25 * np.cos(np.arange(16) * 0.5)[:, None].repeat(16, 1),
                       np.full((16, 16), 0.9)], axis=2).astype(np.float32)
        b.set_normal_map(tall_m, nm)                                                      # conductor: no displacement, so the normal map is reached
        gold = b.material_conductor(b.spectrum_named("metal-Au-eta"), b.spectrum_named("metal-Au-k"), roughness=0.3)
        b.set_float_texture(gold, abi.SHM_FLOATSLOT_V_ROUGHNESS, b.ftex_image(img1, filter=tf("bilinear"), scale=0.5))
        left_m = b.material_mix(left_m, gold, 0.5)
        b.set_float_texture(left_m, abi.SHM_FLOATSLOT_MIX_AMOUNT, b.ftex_image(img1, filter=tf("point"), su=2.0, sv=3.0, mapping="planar",
                                                                                 vs=(0.0, 1.0, 0.0), vt=(0.0, 0.0, 1.0),
                                                                                 texture_from_render=np.linalg.inv(to_render.astype(np.float64))))
    # room [-1,1] x [0,2] x [-1,1], open towards +z (camera side); inward-facing windings via reversed quads
    def inward(q):
        p, vi = q
        return p, vi[:, ::-1].copy()
    floor = inward(_quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1)))
    ceil_ = _quad((-1, 2, -1), (1, 2, -1), (1, 2, 1), (-1, 2, 1))
    back = _quad((-1, 0, -1), (-1, 2, -1), (1, 2, -1), (1, 0, -1))
    left = _quad((-1, 0, -1), (-1, 0, 1), (-1, 2, 1), (-1, 2, -1))
    right = inward(_quad((1, 0, -1), (1, 0, 1), (1, 2, 1), (1, 2, -1)))
    quad_uv = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32) if textured else None
    if textured:
        b.add_mesh(_to_render(ceil_[0], rfw), ceil_[1], ceil_m)
        b.add_mesh(_to_render(back[0], rfw), back[1], back_m, uv=quad_uv)
    else:
        p, vi = _merge([ceil_, back])
        b.add_mesh(_to_render(p, rfw), vi, white)
    b.add_mesh(_to_render(floor[0], rfw), floor[1], floor_m, uv=quad_uv)
    p, vi = left
    b.add_mesh(_to_render(p, rfw), vi, left_m)
    p, vi = right
    b.add_mesh(_to_render(p, rfw), vi, right_m)
    # two boxes, 5 faces each (no bottom), the tall one rotated about y
    def rot_y(p, deg, centre):
        a = np.deg2rad(deg)
        c, s = np.cos(a), np.sin(a)
        q = p - centre
        out = np.stack([c * q[:, 0] + s * q[:, 2], q[:, 1], -s * q[:, 0] + c * q[:, 2]], axis=1)
        return (out + centre).astype(np.float32)
    p, vi = _box((-0.75, 0.0, -0.65), (-0.15, 1.2, -0.05), faces="xXYzZ")
    b.add_mesh(_to_render(rot_y(p, 18.0, np.array([-0.45, 0, -0.35], np.float32)), rfw), vi, tall_m)
    p, vi = _box((0.1, 0.0, 0.0), (0.7, 0.6, 0.6), faces="xXYzZ")
    b.add_mesh(_to_render(rot_y(p, -17.0, np.array([0.4, 0, 0.3], np.float32)), rfw), vi, short_m)
    # ceiling light, facing down
    if patches:
        # the light is ONE rectangular bilinear patch (spherical-rectangle sampling, bilinear_patch.rs:681-737), and
        # a curved (non-planar) diffuse patch leans against the back wall (area sampling, quadratic intersection)
        # (patch_skew lifts p11 out of the plane: is_rectangle fails and the same emitter is sampled by area instead)
        q = np.array([(-0.3, 1.98, -0.3), (0.3, 1.98, -0.3), (-0.3, 1.98, 0.3), (0.3, 1.98 - patch_skew, 0.3)], np.float32)  # p00 p10 p01 p11
        b.add_patch_mesh(_to_render(q, rfw), [[0, 1, 2, 3]], black, emission=blackbody_dense(6500.0), emission_scale=20.0)
        q = np.array([(-0.9, 0.9, -0.95), (-0.2, 1.1, -0.7), (-0.9, 1.7, -0.95), (-0.2, 1.6, -0.95)], np.float32)
        b.add_patch_mesh(_to_render(q, rfw), [[0, 1, 2, 3]], green, reverse_orientation=True)
    else:
        p, vi = _quad((-0.3, 1.98, -0.3), (0.3, 1.98, -0.3), (0.3, 1.98, 0.3), (-0.3, 1.98, 0.3))
        # emitter_reflects: the emitter's own material is white instead of black, so a path that hits it goes ON (emission at a vertex whose state the vertex
        # kernel overwrites: the deferred evaluation of k_emit_jobs reads its side copies), and it emits from both sides
        b.add_mesh(_to_render(p, rfw), vi, white if emitter_reflects else black, emission=blackbody_dense(6500.0), emission_scale=20.0, two_sided=bool(emitter_reflects))
    if "sheet" in dt:
        # the sheet leans a little, so that no ray meets it edge-on; the ceiling light is behind it as the camera sees it
        if "textured" in dt:
            sheet_m = b.material_diffuse_transmission(b.stex_checkerboard(_two_point_spectrum(b, 0.1, 0.4), 0.05, b.add_texture_mapping("uv", su=4.0, sv=4.0)),
                                                      b.add_image_texture(test_image(32, 3), filter="trilinear"), scale=0.9)
        elif "mixed" in dt:
            sheet_m = b.material_mix(b.material_diffuse_transmission(0.1, _two_point_spectrum(b, 0.7, 0.2)), b.material_diffuse_transmission(0.5, 0.0), 0.4)
        else:
            sheet_m = b.material_diffuse_transmission(_two_point_spectrum(b, 0.05, 0.3), _two_point_spectrum(b, 0.65, 0.35))
        p, vi = _quad((-0.7, 0.25, 0.55), (0.7, 0.25, 0.55), (0.7, 1.75, 0.85), (-0.7, 1.75, 0.85))
        b.add_mesh(_to_render(p, rfw), vi, sheet_m, uv=np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32) if "textured" in dt else None)
    if "sphere" in dt:
        rfo = np.asarray(rfw, np.float32).reshape(4, 4) @ np.array([[1, 0, 0, 0.4], [0, 1, 0, 0.85], [0, 0, 1, 0.3], [0, 0, 0, 1]], np.float32)
        b.add_sphere(0.25, b.material_diffuse_transmission(0.2, _two_point_spectrum(b, 0.3, 0.7)), render_from_object=rfo.astype(np.float32))
    if environment is not None:  # an ImageInfinitelight shines in through the open front (round 5: the K_ENV_LIGHT units of the staged kernels)
        rot = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float32)
        b.light_image_infinite(environment, scale=0.5, render_from_light=rot)
    return _finish(b, lib, extra_lights=extra_lights, rfw=rfw, name="S2 cornell box" + (" (diffuse transmission: %s)" % diffuse_transmission if dt else "") + (" (environment map)" if environment is not None else "") + (" (coated)" if coated else "") + (" (mix)" if mix else "") + (" (patches)" if patches else "") + (" (textured)" if textured else "") + (" (glass)" if glass else "") + (" (+ glass)" if glass_too else ""))


def procedural_cornell(lib, width=33, height=31, which="checker", film=None, extra_lights=None):
    """The Cornell box with PBRT-v4's procedural textures (no image anywhere: a scene whose only textures are procedural is a textured scene).
    which = "checker": a spectrum checkerboard on the floor (planar mapping), spectrum dots on the back wall (spherical mapping), a float bilerp (cylindrical mapping) scaling
                       the right wall, a float checkerboard in its child form (3-D point mapping) on the tall box's conductor roughness; every other surface is plain
                       diffuse (the split pass of a textured scene);
            "general": as "checker", plus a sphere with a 3-D spectrum checkerboard, a curved bilinear patch with spectrum dots (uv mapping) and a patch light;
            "coated":  a coated-diffuse floor whose bump map is `wrinkled`, whose interface roughness is driven by `fbm` and whose thickness by `windy` (the LayeredBxDF stages)."""
    b = SceneBuilder()
    b.set_film(width, height, **(film or {}))
    rfw = b.set_camera_look_at(lib, (0, 1, 3.4), (0, 1, 0), (0, 1, 0), 39.0)
    world_from_render = np.linalg.inv(np.asarray(rfw, np.float64).reshape(4, 4))

    def mapping(kind, scale=1.0, centre=(0.0, 0.0, 0.0), **kw):  # texture space = scale * (world - centre)
        m = np.diag([scale, scale, scale, 1.0])
        m[:3, 3] = [-scale * c for c in centre]
        return b.add_texture_mapping(kind, texture_from_render=m @ world_from_render, **kw)
    white, black = b.material_diffuse(0.75), b.material_diffuse(0.0)
    red, green_spec = b.material_diffuse(_two_point_spectrum(b, 0.05, 0.75)), _two_point_spectrum(b, 0.6, 0.08)
    floor_m = b.material_diffuse(b.stex_checkerboard(0.7, _two_point_spectrum(b, 0.3, 0.05), mapping("planar", vs=(2.0, 0.0, 0.0), vt=(0.0, 0.0, 2.0), du=0.25, dv=0.25)))
    back_m = b.material_diffuse(b.stex_dots(_two_point_spectrum(b, 0.1, 0.6), 0.7, mapping("spherical", centre=(0.0, 1.0, 0.5))))
    right_m = b.material_diffuse(b.stex_scaled(green_spec, b.ftex_bilerp(0.2, 1.0, 0.6, 0.3, mapping("cylindrical", centre=(0.0, 0.0, 0.0)))))
    tall_m = b.material_conductor(b.spectrum_named("metal-Al-eta"), b.spectrum_named("metal-Al-k"), roughness=0.1)
    b.set_float_texture(tall_m, abi.SHM_FLOATSLOT_U_ROUGHNESS, b.ftex_checkerboard(0.05, 0.3, mapping("point3d", scale=5.0)))
    short_m = white
    if which == "coated":
        floor_m = b.material_coated_diffuse(reflectance=0.6, roughness=0.1, thickness=0.05, albedo=0.3, g=0.2)
        noise_space = mapping("point3d", scale=6.0)
        b.set_float_texture(floor_m, abi.SHM_FLOATSLOT_DISPLACEMENT, b.ftex_scaled(b.ftex_wrinkled(6, 0.6, noise_space), 0.05))
        rough = b.ftex_mix(0.3, 0.1, b.ftex_scaled(b.ftex_fbm(5, 0.5, noise_space), 0.3))  # 0.3 - 0.2 * (0.3 fbm): stays positive
        b.set_float_texture(floor_m, abi.SHM_FLOATSLOT_U_ROUGHNESS, rough)
        b.set_float_texture(floor_m, abi.SHM_FLOATSLOT_V_ROUGHNESS, rough)
        b.set_float_texture(floor_m, abi.SHM_FLOATSLOT_THICKNESS, b.ftex_mix(0.05, 0.07, b.ftex_windy(mapping("point3d", scale=3.0))))

    def inward(q):
        p, vi = q
        return p, vi[:, ::-1].copy()
    quad_uv = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32)
    for quad, m in ((_quad((-1, 2, -1), (1, 2, -1), (1, 2, 1), (-1, 2, 1)), white), (_quad((-1, 0, -1), (-1, 2, -1), (1, 2, -1), (1, 0, -1)), back_m),
                    (inward(_quad((-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1))), floor_m), (_quad((-1, 0, -1), (-1, 0, 1), (-1, 2, 1), (-1, 2, -1)), red),
                    (inward(_quad((1, 0, -1), (1, 0, 1), (1, 2, 1), (1, 2, -1))), right_m)):
        b.add_mesh(_to_render(quad[0], rfw), quad[1], m, uv=quad_uv)
    p, vi = _box((-0.75, 0.0, -0.65), (-0.15, 1.2, -0.05), faces="xXYzZ")
    b.add_mesh(_to_render(p, rfw), vi, tall_m)
    if which == "general":
        rfo = np.eye(4, dtype=np.float32)
        rfo[:3, 3] = _to_render([(0.4, 0.35, 0.3)], rfw)[0]
        b.add_sphere(0.35, b.material_diffuse(b.stex_checkerboard(0.8, 0.1, mapping("point3d", scale=4.0))), render_from_object=rfo)
        q = np.array([(-0.9, 0.9, -0.95), (-0.2, 1.1, -0.7), (-0.9, 1.7, -0.95), (-0.2, 1.6, -0.95)], np.float32)
        dots_m = b.material_diffuse(b.stex_dots(0.1, green_spec, b.add_texture_mapping("uv", su=4.0, sv=4.0)))
        b.add_patch_mesh(_to_render(q, rfw), [[0, 1, 2, 3]], dots_m, reverse_orientation=True)
        q = np.array([(-0.3, 1.98, -0.3), (0.3, 1.98, -0.3), (-0.3, 1.98, 0.3), (0.3, 1.98, 0.3)], np.float32)
        b.add_patch_mesh(_to_render(q, rfw), [[0, 1, 2, 3]], black, emission=blackbody_dense(6500.0), emission_scale=20.0)
    else:
        p, vi = _box((0.1, 0.0, 0.0), (0.7, 0.6, 0.6), faces="xXYzZ")
        b.add_mesh(_to_render(p, rfw), vi, short_m)
        p, vi = _quad((-0.3, 1.98, -0.3), (0.3, 1.98, -0.3), (0.3, 1.98, 0.3), (-0.3, 1.98, 0.3))
        b.add_mesh(_to_render(p, rfw), vi, black, emission=blackbody_dense(6500.0), emission_scale=20.0)
    return _finish(b, lib, extra_lights=extra_lights, rfw=rfw, name=f"S2 cornell box (procedural textures: {which})")


def _hash3(ix, iy, iz, seed):
    """Integer lattice hash -> [0,1) float64 (vectorised, wraps like uint64)."""
    with np.errstate(over="ignore"):
        h = (ix.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ (iy.astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F)) ^ (
            iz.astype(np.uint64) * np.uint64(0x165667B19E3779F9)) ^ np.uint64(seed)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
    return (h >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def _value_noise(p, seed, octaves=3):
    """Seeded value noise on R^3 (trilinear, smoothstep), summed over octaves."""
    total = np.zeros(p.shape[0], np.float64)
    amp, freq = 1.0, 3.0
    for o in range(octaves):
        q = p.astype(np.float64) * freq + 100.0
        i = np.floor(q).astype(np.int64)
        f = q - i
        f = f * f * (3.0 - 2.0 * f)
        acc = 0.0
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    w = (f[:, 0] if dx else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dz else 1 - f[:, 2])
                    acc = acc + w * _hash3(i[:, 0] + dx, i[:, 1] + dy, i[:, 2] + dz, seed + o)
        total += amp * (acc - 0.5)
        amp *= 0.5
        freq *= 2.0
    return total


@functools.lru_cache(maxsize=2)
def cube_sphere(n, seed=1234, amplitude=0.15, shuffle_seed=99, as_quads=False, quad_fraction=None):
    """Closed genus-0 cube-sphere: 6 faces x n x n quads x 2 triangles with shared vertices (6 n^2 + 2), unit radius,
    radially displaced by value noise; triangle order randomised (seeded Fisher-Yates / permutation)."""
    m = n + 1
    # unique lattice points on the cube surface, indexed through a dict-free scheme: generate all 6 faces then unify
    g = np.arange(m, dtype=np.int64)
    u, v = np.meshgrid(g, g, indexing="ij")
    u, v = u.ravel(), v.ravel()
    faces = []
    zeros, full = np.zeros_like(u), np.full_like(u, n)
    faces.append(np.stack([full, u, v], 1))    # +x
    faces.append(np.stack([zeros, v, u], 1))   # -x
    faces.append(np.stack([v, full, u], 1))    # +y
    faces.append(np.stack([u, zeros, v], 1))   # -y
    faces.append(np.stack([u, v, full], 1))    # +z
    faces.append(np.stack([v, u, zeros], 1))   # -z
    allp = np.concatenate(faces)               # integer lattice coords in [0,n]^3 on the surface
    key = (allp[:, 0] * (m * m) + allp[:, 1] * m + allp[:, 2])
    uniq, inverse = np.unique(key, return_inverse=True)
    coords = np.stack([uniq // (m * m), (uniq // m) % m, uniq % m], 1).astype(np.float64)
    cube = coords / n * 2.0 - 1.0
    # tangent-warp for more uniform cells, then normalise to the sphere
    cube = np.tan(cube * (np.pi / 4.0))
    sph = cube / np.linalg.norm(cube, axis=1, keepdims=True)
    r = 1.0 + amplitude * _value_noise(sph, seed) * 2.0
    verts = (sph * r[:, None]).astype(np.float32)
    tris, quads = [], []
    cell_i, cell_j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    cell_i, cell_j = cell_i.ravel(), cell_j.ravel()
    for fi in range(6):
        idx = inverse[fi * m * m:(fi + 1) * m * m].reshape(m, m)
        a, b_, c, d = idx[cell_i, cell_j], idx[cell_i + 1, cell_j], idx[cell_i + 1, cell_j + 1], idx[cell_i, cell_j + 1]
        tris.append(np.stack([a, b_, c], 1))
        tris.append(np.stack([a, c, d], 1))
        quads.append(np.stack([a, b_, d, c], 1))  # p00, p10, p01, p11 (bilinear_patch.rs:87-98): the same cell as ONE bilinear patch
    rng = np.random.Generator(np.random.PCG64(shuffle_seed))
    if quad_fraction is not None:  # (development: a MIXED object — this share of the cells as patches, the others as triangle pairs; returns verts, tris, quads)
        quads = np.concatenate(quads).astype(np.uint32)
        perm = rng.permutation(quads.shape[0])
        nq = int(round(quad_fraction * quads.shape[0]))
        q_cells, t_cells = perm[:nq], perm[nq:]
        qq = quads[q_cells]
        cells = quads[t_cells]  # a, b, d, c
        tt = np.concatenate([np.stack([cells[:, 0], cells[:, 1], cells[:, 3]], 1), np.stack([cells[:, 0], cells[:, 3], cells[:, 2]], 1)]).astype(np.uint32)
        return verts, tt[rng.permutation(tt.shape[0])], qq
    if as_quads:  # what the reference makes of a PLY file's quad faces (shape/mesh.rs:233-256): 6 n^2 bilinear patches over the same vertices, order randomised alike
        quads = np.concatenate(quads).astype(np.uint32)
        return verts, quads[rng.permutation(quads.shape[0])]
    tris = np.concatenate(tris).astype(np.uint32)
    tris = tris[rng.permutation(tris.shape[0])]
    return verts, tris


def ganesha_proxy(lib, width=1024, height=1024, n=599, with_room=True, coated=False, variant=None, floor_filter="ewa", quad_fraction=None, object_material=None, film=None, extra_lights=None, camera=None,
                  cutout_fraction=None, cutout_alpha=True):
    """S3 (configs C3/C5): n=599 gives 6*599^2*2 = 4 305 612 triangles and 2 152 808 vertices.
    coated=True: the object is CoatedDiffuse (the material of the reference's Ganesha render, images/shimmer-ganesha-1.png).
    variant (round 5: the shapes a real PBRT-v4 scene mixes into its triangles; same camera, room and object):
      "patch_emitter"  the window emitter is ONE bilinear patch — what a quad face of a PLY file becomes (shape/shape.rs:119-134, shape/mesh.rs:233-256)
      "one_sphere"     a diffuse sphere stands on the floor beside the object (shape/sphere.rs)
      "one_disk", "one_cylinder"  PBRT-v4's disk (hovering where that sphere's centre is) / cylinder (standing where it stands) in its place
      "instanced"      the object is an object definition placed once through a TransformedPrimitive (primitive.rs:136-176)
      "textured_floor" the ground plane's reflectance is an image texture (EWA-filtered, repeated): ONE textured material among plain ones
      "mesh_emitter"   (round 6) the window emitter tessellated into 64 x 64 x 2 = 8 192 emissive triangles: one DiffuseAreaLight per triangle (light.rs:632-684), the uniform
                       light sampler picks among 8 192 lights — the light table, the emitters' records and the per-light data no longer fit the kernels' LDS tables
      "smooth"         (round 6) the object's mesh carries per-vertex normals and uv coordinates, as every production mesh does (triangle.rs:380-504: the shading frame from
                       interpolated normals, dndu / dndv): the headline scene's object has neither
      "instance_grid"  (round 6) the object is ONE small object definition (the same displaced sphere at n // 4: a sixteenth of the triangles) placed 4 x 4 x 4 times through
                       TransformedPrimitives in the object's place — the class instancing exists for: most rays cross several instance boxes, each a transformed sub-traversal
      "quads"          (round 6) the object's 6 n^2 cells as bilinear patches instead of 12 n^2 triangles: what a quad PLY file becomes in the reference
      "environment"    no room and no window: the object on its ground plane under an ImageInfinitelight (light.rs:805-981) — escaped rays look the map up, next-event
                       estimation samples its (compensated) piecewise-constant distribution
    cutout_fraction (no variant): that share of the object's triangles — every k-th one — as a second mesh with uv coordinates and, with `cutout_alpha`, PBRT-v4's shape
    alpha: a 64 x 32 checkerboard over the sphere's (longitude, latitude). `cutout_alpha=False`: the same two meshes uncut (the workload's partner in a measurement)."""
    assert variant in (None, "patch_emitter", "one_sphere", "instanced", "environment", "textured_floor", "textured_hidden", "quads", "smooth", "mesh_emitter", "textured_object", "instance_grid", "one_disk", "one_cylinder")
    b = SceneBuilder()
    b.set_film(width, height, **(film or {}))
    rfw = _set_camera(b, lib, camera, (0.0, 0.6, 4.2), (0.0, 0.0, 0.0), (0, 1, 0), 38.0)
    obj = b.material_coated_diffuse(reflectance=0.4, roughness=0.05, thickness=0.01) if coated else b.material_diffuse(0.4)
    if object_material == "gold":  # (round 6 class probes) a rough conductor / a dispersive glass / a coated conductor object
        obj = b.material_conductor(b.spectrum_named("metal-Au-eta"), b.spectrum_named("metal-Au-k"), roughness=0.2)
    elif object_material == "glass":
        obj = b.material_dielectric(b.spectrum_named("glass-BK7"))
    elif object_material == "coated_conductor":
        obj = b.material_coated_conductor(interface_roughness=0.05, conductor_roughness=0.2, thickness=0.02)
    elif object_material == "diffuse_transmission":  # (reflectance as the plain object's, plus a transmitted lobe)
        obj = b.material_diffuse_transmission(0.4, 0.4)
    wall = b.material_diffuse(0.6)
    black = b.material_diffuse(0.0)
    if quad_fraction is not None:  # (development: where the five-wave traversal kernels start to pay — a share of the object's cells as patches, the rest as triangles)
        verts, tris, quads = cube_sphere(n, quad_fraction=quad_fraction)
        b.add_mesh(_to_render(verts, rfw), tris, obj)
        if quads.shape[0]:
            b.add_patch_mesh(_to_render(verts, rfw), quads, obj)
    else:
        verts, tris = cube_sphere(n, as_quads=variant == "quads")
    if quad_fraction is not None:
        pass
    elif cutout_fraction is not None:
        assert variant is None and 0.0 < cutout_fraction <= 1.0
        cut = (np.arange(tris.shape[0]) * float(cutout_fraction)).astype(np.int64)
        cut = np.concatenate([[True], cut[1:] != cut[:-1]])  # every k-th triangle, spread over the whole object
        vr = _to_render(verts, rfw)
        d = verts / np.linalg.norm(verts, axis=1, keepdims=True)
        uv = np.stack([0.5 + np.arctan2(d[:, 2], d[:, 0]) / (2 * np.pi), 0.5 - np.arcsin(np.clip(d[:, 1], -1, 1)) / np.pi], 1).astype(np.float32)
        if (~cut).any():
            b.add_mesh(vr, tris[~cut], obj)
        holes = b.ftex_checkerboard(None, None, mapping=b.add_texture_mapping("uv", su=64.0, sv=32.0)) if cutout_alpha else None
        b.add_mesh(vr, tris[cut], obj, uv=uv, alpha=holes)
    elif variant == "quads":
        # (round 6) the object as 6 n^2 BILINEAR PATCHES — the reference turns every quad face of a PLY file into one (shape/shape.rs:97-137), and the showcase Ganesha is
        # a quad PLY: the class a real scene's traversal runs in, every leaf a parked non-triangle test
        b.add_patch_mesh(_to_render(verts, rfw), tris, obj)
    elif variant == "instanced":
        b.begin_object("object")
        b.add_mesh(verts, tris, obj)  # object space
        b.end_object()
        b.add_instance("object", rfw)  # render_from_instance = render_from_world x identity (loading/scene.rs:855-866)
    elif variant == "instance_grid":
        sv, st = cube_sphere(max(2, n // 4))
        b.begin_object("cell")
        b.add_mesh(sv, st, obj)
        b.end_object()
        for ix in range(4):
            for iy in range(4):
                for iz in range(4):
                    m = np.eye(4, dtype=np.float32)
                    m[0, 0] = m[1, 1] = m[2, 2] = 0.27  # (cells of 0.5: neighbouring spheres' boxes overlap a little, as a scattered placement's do)
                    m[:3, 3] = (-0.75 + 0.5 * ix, -0.75 + 0.5 * iy, -0.75 + 0.5 * iz)
                    b.add_instance("cell", (np.asarray(rfw, np.float32).reshape(4, 4) @ m).astype(np.float32))
    elif variant in ("smooth", "textured_object"):
        if variant == "textured_object":  # (round 6) ... and its reflectance is an image texture (trilinear, repeated) over that uv: EVERY hit on the object is a textured vertex
            obj = b.material_diffuse(b.add_image_texture(test_image(256, 3), filter="trilinear", wrap="repeat", su=8.0, sv=8.0))
        vr = _to_render(verts, rfw)
        centre = _to_render(np.zeros((1, 3), np.float32), rfw)[0]
        nrm = vr - centre  # (radial: a smoothed version of the displaced sphere's normals — any unit field serves the arithmetic)
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
        d = verts / np.linalg.norm(verts, axis=1, keepdims=True)
        uv = np.stack([0.5 + np.arctan2(d[:, 2], d[:, 0]) / (2 * np.pi), 0.5 - np.arcsin(np.clip(d[:, 1], -1, 1)) / np.pi], 1).astype(np.float32)
        b.add_mesh(vr, tris, obj, n=nrm, uv=uv)
    else:
        b.add_mesh(_to_render(verts, rfw), tris, obj)
    if variant == "one_sphere":
        rfo = np.eye(4, dtype=np.float32)
        rfo[:3, 3] = _to_render(np.array([[0.7, -0.8, 1.7]], np.float32), rfw)[0]  # (in front of the object, to the right: in the camera's view)
        b.add_sphere(0.45, wall, render_from_object=rfo)
    if variant in ("one_disk", "one_cylinder"):  # PBRT-v4's disk / cylinder where "one_sphere" has its sphere: the extended kernels and k_trace_quadrics.hip's on the S3 frame
        rfo = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float32)  # the shape's +z is the world's +y
        rfo[:3, 3] = _to_render(np.array([[0.7, -0.8 if variant == "one_disk" else -1.25, 1.7]], np.float32), rfw)[0]
        if variant == "one_disk":
            b.add_disk(0.45, wall, render_from_object=rfo)
        else:
            b.add_cylinder(0.45, wall, z_min=0.0, z_max=0.9, render_from_object=rfo)
    if variant == "textured_hidden":  # (development: a textured material nobody sees — the textured class's fixed cost)
        tm = b.material_diffuse(b.add_image_texture(test_image(64, 3), filter="bilinear", wrap="repeat"))
        p, vi = _quad((-0.1, -50.0, -0.1), (-0.1, -50.0, 0.1), (0.1, -50.0, 0.1), (0.1, -50.0, -0.1))
        b.add_mesh(_to_render(p, rfw), vi, tm, uv=np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32))
    if variant == "environment":
        p, vi = _quad((-4, -1.25, -4), (-4, -1.25, 6), (4, -1.25, 6), (4, -1.25, -4))
        b.add_mesh(_to_render(p, rfw), vi, wall)
        rot = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float32)  # +z of the map is the world's +y (as in three_spheres)
        b.light_image_infinite(environment_image(64), scale=1.0, render_from_light=rot)
    elif with_room:
        # ground (2) + open room (10: back, left, right, ceiling, front-top strip) + window emitter (2)
        p, vi = _quad((-4, -1.25, -4), (-4, -1.25, 6), (4, -1.25, 6), (4, -1.25, -4))
        if variant == "textured_floor":
            floor_m = b.material_diffuse(b.add_image_texture(test_image(64, 3), filter=floor_filter, wrap="repeat", su=4.0, sv=4.0))
            b.add_mesh(_to_render(p, rfw), vi, floor_m, uv=np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32))
        else:
            b.add_mesh(_to_render(p, rfw), vi, wall)
        room = _merge([
            _quad((-4, -1.25, -4), (4, -1.25, -4), (4, 4, -4), (-4, 4, -4)),      # back
            _quad((-4, -1.25, -4), (-4, 4, -4), (-4, 4, 6), (-4, -1.25, 6)),      # left
            _quad((4, -1.25, -4), (4, -1.25, 6), (4, 4, 6), (4, 4, -4)),          # right
            _quad((-4, 4, -4), (4, 4, -4), (4, 4, 6), (-4, 4, 6)),                # ceiling
            _quad((-4, -1.25, 6), (-4, 4, 6), (4, 4, 6), (4, -1.25, 6)),          # behind camera
        ])
        b.add_mesh(_to_render(room[0], rfw), room[1], wall)
        # window emitter high on the left, facing +x/-y into the room (one-sided)
        p, vi = _quad((-3.9, 1.0, -1.5), (-3.9, 3.0, -1.5), (-3.9, 3.0, 1.5), (-3.9, 1.0, 1.5))
        if variant == "mesh_emitter":
            m = 64
            g = np.linspace(0.0, 1.0, m + 1)
            yy, zz = np.meshgrid(1.0 + 2.0 * g, -1.5 + 3.0 * g, indexing="ij")
            pv = np.stack([np.full(yy.size, -3.9), yy.ravel(), zz.ravel()], 1).astype(np.float32)
            ii, jj = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
            a, b_, c, d = (ii * (m + 1) + jj).ravel(), ((ii + 1) * (m + 1) + jj).ravel(), ((ii + 1) * (m + 1) + jj + 1).ravel(), (ii * (m + 1) + jj + 1).ravel()
            tv = np.concatenate([np.stack([a, b_, c], 1), np.stack([a, c, d], 1)]).astype(np.uint32)  # the same winding as the two-triangle quad: (p0, p1, p2), (p0, p2, p3)
            # per-vertex normals (+x, into the room): without them the reference's Triangle::sample FLIPS the area-sampled normal (triangle.rs:558-560: `n * -1.0` whenever
            # the mesh has no normals) and a one-sided emitter of small triangles — solid angle below 3e-4 sr: sampled by area — sends its light samples the wrong way
            nv = (_to_render(np.array([[1.0, 0.0, 0.0]], np.float32), rfw) - _to_render(np.zeros((1, 3), np.float32), rfw))[0]
            b.add_mesh(_to_render(pv, rfw), tv, black, n=np.tile(nv / np.linalg.norm(nv), (pv.shape[0], 1)).astype(np.float32), emission=blackbody_dense(6500.0), emission_scale=40.0)
        elif variant == "patch_emitter":  # p00, p10, p01, p11 (bilinear_patch.rs:87-98): the same quad, the same side emitting
            b.add_patch_mesh(_to_render(p, rfw), [[0, 1, 3, 2]], black, emission=blackbody_dense(6500.0), emission_scale=40.0)
        else:
            b.add_mesh(_to_render(p, rfw), vi, black, emission=blackbody_dense(6500.0), emission_scale=40.0)
    return _finish(b, lib, extra_lights=extra_lights, rfw=rfw, name=f"S3 ganesha-proxy n={n}" + (" (coated)" if coated else "") + (f" [{variant}]" if variant else ""))


def icosphere(level):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10],
                  [8, 6, 7], [9, 8, 1]], np.int64)
    for _ in range(level):
        edges = {}
        verts = list(v)

        def mid(a, b_):
            k = (min(a, b_), max(a, b_))
            if k not in edges:
                m = verts[a] + verts[b_]
                verts.append(m / np.linalg.norm(m))
                edges[k] = len(verts) - 1
            return edges[k]

        nf = []
        for a, b_, c in f:
            ab, bc, ca = mid(a, b_), mid(b_, c), mid(c, a)
            nf += [[a, ab, ca], [b_, bc, ab], [c, ca, bc], [ab, bc, ca]]
        v, f = np.array(verts), np.array(nf, np.int64)
    return v.astype(np.float32), f.astype(np.uint32)


def crown_proxy(lib, width=1000, height=1400, level=4, n_glass=64, n_gold=16, seed=4242, environment=None, film=None, extra_lights=None, camera=None):
    """S4 (config C4): dispersive smooth dielectric icospheres (BK7 eta table -> terminate_secondary), rough gold
    conductors, diffuse floor, one quad emitter; render with max_depth=32."""
    b = SceneBuilder()
    b.set_film(width, height, **(film or {}))
    rfw = _set_camera(b, lib, camera, (0.0, 2.2, 7.5), (0.0, 1.2, 0.0), (0, 1, 0), 32.0)
    glass = b.material_dielectric(b.spectrum_named("glass-BK7"))
    gold = b.material_conductor(b.spectrum_named("metal-Au-eta"), b.spectrum_named("metal-Au-k"), roughness=0.01)  # alpha = sqrt(0.01) = 0.1
    floor = b.material_diffuse(0.5)
    black = b.material_diffuse(0.0)
    sv, sf = icosphere(level)
    rng = np.random.Generator(np.random.PCG64(seed))
    k = n_glass + n_gold
    ring = np.arange(k)
    ang = ring * (2 * np.pi / 16.0) + (ring // 16) * 0.2
    rad = 1.0 + 0.35 * (ring // 16)
    centres = np.stack([rad * np.cos(ang), 0.35 + 0.55 * (ring // 16) + 0.1 * rng.random(k), rad * np.sin(ang)], 1)
    radii = 0.18 + 0.1 * rng.random(k)
    order = rng.permutation(k)
    for j, idx in enumerate(order):
        verts = sv * f32(radii[idx]) + centres[idx].astype(np.float32)[None, :]
        b.add_mesh(_to_render(verts, rfw), sf, glass if j < n_glass else gold)
    p, vi = _quad((-6, 0, -6), (-6, 0, 8), (6, 0, 8), (6, 0, -6))
    b.add_mesh(_to_render(p, rfw), vi, floor)
    p, vi = _quad((-2, 5, -2), (2, 5, -2), (2, 5, 2), (-2, 5, 2))
    b.add_mesh(_to_render(p, rfw), vi, black, emission=blackbody_dense(6500.0), emission_scale=30.0)
    if environment is not None:  # glass and metal under an ImageInfinitelight as well (round 5: the sorted fused kernel's ENV_LIGHT instantiation)
        rot = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float32)
        b.light_image_infinite(environment, scale=1.0, render_from_light=rot)
    return _finish(b, lib, extra_lights=extra_lights, rfw=rfw, name="S4 crown-proxy" + ("" if environment is None else " (environment map)"))


def environment_image(n=32, sun=(0.3, 0.5, 0.81), sun_radiance=40.0):
    """A small synthetic environment map in the equal-area octahedral layout (math.rs:456-485): blue-ish sky fading to a warm
    horizon, a dim ground, and a sun — bright enough that the compensated distribution (light.rs:948-955) differs from the plain one."""
    y, x = np.mgrid[0:n, 0:n]
    u, v = 2.0 * (x + 0.5) / n - 1.0, 2.0 * (y + 0.5) / n - 1.0
    up, vp = np.abs(u), np.abs(v)
    sd = 1.0 - (up + vp)
    r = 1.0 - np.abs(sd)
    phi = np.where(r == 0, 1.0, (vp - up) / np.where(r == 0, 1.0, r) + 1.0) * np.pi / 4
    z = np.copysign(1.0 - r * r, sd)
    d = np.stack([np.copysign(np.cos(phi), u) * r * np.sqrt(2.0 - r * r), np.copysign(np.sin(phi), v) * r * np.sqrt(2.0 - r * r), z], axis=-1)
    s = np.asarray(sun, np.float64)
    s /= np.linalg.norm(s)
    t = np.clip(d[..., 2], 0.0, 1.0)[..., None]
    sky = (1.0 - t) * np.array([0.9, 0.7, 0.5]) + t * np.array([0.25, 0.45, 0.9])
    img = np.where(d[..., 2:3] >= 0.0, sky, np.array([0.12, 0.1, 0.08]))
    img = img + sun_radiance * np.array([1.0, 0.9, 0.7]) * (np.einsum("ijk,k->ij", d, s) > 0.97)[..., None]
    return img.astype(np.float32)


def environment_from_probe(image):
    """The film of an equal-area spherical camera (linear RGB, row 0 first; the camera's up = the world's +y) as the `environment=` image of the generators here, so
    that what the probe saw in a world direction is what the map shows in that direction. The camera's swap of y and z is a REFLECTION ((x, y, z) -> (x, z, y)) and the
    generators turn their map by a ROTATION ((x, y, z) -> (x, z, -y)); with the look-at frame's right = cross(up, dir) pointing along -x for a probe that looks down -z,
    what is left between the two is a mirror in u: the film flipped left to right. (Negative values, which a filter with negative lobes may leave, are clamped.)"""
    return np.ascontiguousarray(np.maximum(np.asarray(image, np.float32)[:, ::-1], 0.0))


def three_spheres(lib, width=32, height=32, offsets=(-3.5, 0.0, 5.0), camera=(0.0, 0.0, 0.0), environment=None, film=None, extra_lights=None):
    """The reference's set_of_spheres BVH test scene (aggregate.rs:631-702): unit spheres at x = -3.5, 0, 5.
    With the default camera at the origin world == render space, as the reference's unit tests assume (rays are given
    in render space); pass a camera position outside the spheres to render it — or, like the other generators, a dict that replaces the camera (_set_camera)."""
    b = SceneBuilder()
    b.set_film(width, height, **(film or {}))
    spec = camera if isinstance(camera, dict) else None
    cam = np.asarray((0.0, 0.0, 0.0) if spec is not None else camera, np.float64)
    rfw = _set_camera(b, lib, spec, cam, cam + np.array([0.0, 0.0, -1.0]), (0, 1, 0), 60.0)
    m = b.material_diffuse(0.5)
    for x in offsets:
        rfo = np.eye(4, dtype=np.float32)
        rfo[:3, 3] = rfw[:3, 3]
        rfo[0, 3] += np.float32(x)
        b.add_sphere(1.0, m, render_from_object=rfo)
    # a uniform environment (UniformInfiniteLight, light.rs:692-816): exercises the escaped-ray branch of
    # PathIntegrator::li (integrator.rs:776-794)
    if environment is None:
        b.light_uniform_infinite(np.ones(471, np.float32), scale=1.0)
    else:  # ImageInfinitelight (light.rs:805-981), turned so that +z of the map is the world's +y
        rot = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float32)
        b.light_image_infinite(environment, scale=0.01, render_from_light=rot)
    return _finish(b, lib, extra_lights=extra_lights, rfw=rfw, name="three spheres" + ("" if environment is None else " (environment map)"))


def instanced_scene(lib, width=64, height=48, n_instances=5, only_object=False, baked=False, environment=None, film=None, extra_lights=None, diffuse_transmission=False, camera=None):
    """Object instancing: one object definition (an icosphere with per-vertex normals, a partial sphere and a curved
    bilinear patch, three materials) placed several times with rotated, non-uniformly scaled transforms over a floor lit by a quad
    light and a point light. `only_object`: just the object's shapes at top level, untransformed, no floor. `baked`: the same
    placements as explicitly transformed triangle copies (icosphere only) instead of instances — for cross-checks."""
    rng = np.random.Generator(np.random.PCG64(77))
    b = SceneBuilder()
    b.set_film(width, height, **(film or {}))
    rfw = _set_camera(b, lib, camera, (0.0, 2.2, 7.0), (0.0, 0.8, 0.0), (0, 1, 0), 40.0)
    # (diffuse_transmission: the object's icosphere is PBRT-v4's diffuse transmission material instead of a DiffuseMaterial)
    mats = [b.material_diffuse_transmission(_two_point_spectrum(b, 0.3, 0.1), _two_point_spectrum(b, 0.2, 0.6)) if diffuse_transmission else b.material_diffuse(_two_point_spectrum(b, 0.7, 0.2)), b.material_conductor(b.spectrum_named("metal-Cu-eta"), b.spectrum_named("metal-Cu-k"), roughness=0.2),
            b.material_coated_diffuse(reflectance=0.5, roughness=0.1)]
    sv, sf = icosphere(1)
    nrm = (sv / np.linalg.norm(sv, axis=1, keepdims=True)).astype(np.float32)

    def object_shapes(to_render=None, ico_only=False):
        p = (sv * np.float32(0.6)).astype(np.float32)
        if to_render is not None:
            p = (np.c_[p.astype(np.float64), np.ones(len(p))] @ to_render.T)[:, :3].astype(np.float32)
        b.add_mesh(p, sf, mats[0], n=None if to_render is not None else nrm)
        if ico_only:
            return
        rfo = np.eye(4, dtype=np.float32)
        rfo[:3, 3] = (0.9, 0.1, 0.0)
        b.add_sphere(0.35, mats[1], render_from_object=rfo, z_min=-0.2, z_max=0.3, phi_max=270.0)
        q = np.array([(-0.9, -0.4, 0.2), (-0.3, -0.4, 0.4), (-0.9, 0.5, 0.1), (-0.3, 0.4, 0.6)], np.float32)
        b.add_patch_mesh(q, [[0, 1, 2, 3]], mats[2])

    placements = []
    for i in range(n_instances):
        ang, axis = rng.uniform(0, 2 * np.pi), rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        rot = np.eye(3) + np.sin(ang) * k + (1 - np.cos(ang)) * (k @ k)
        m = np.eye(4)
        m[:3, :3] = rot @ np.diag(rng.uniform(0.6, 1.4, 3))
        m[:3, 3] = (rng.uniform(-2.5, 2.5), rng.uniform(0.8, 1.6), rng.uniform(-1.5, 1.5))
        placements.append((np.asarray(rfw, np.float64).reshape(4, 4) @ m))
    if only_object:
        object_shapes()
        b.light_point((0.0, 0.0, 0.0), blackbody_dense(5000.0), scale=1.0)
        return _finish(b, lib, extra_lights=extra_lights, rfw=rfw, name="instanced object alone")
    if baked:
        for m in placements:
            object_shapes(to_render=m, ico_only=True)
    else:
        b.begin_object("blob")
        object_shapes()
        b.end_object()
        for m in placements:
            b.add_instance("blob", m.astype(np.float32))
    floor_m = b.material_diffuse(0.6)
    p, vi = _quad((-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6))
    b.add_mesh(_to_render(p, rfw), vi, floor_m)
    black = b.material_diffuse(0.0)
    p, vi = _quad((-1.5, 5.0, -1.5), (1.5, 5.0, -1.5), (1.5, 5.0, 1.5), (-1.5, 5.0, 1.5))
    b.add_mesh(_to_render(p, rfw), vi, black, emission=blackbody_dense(6500.0), emission_scale=12.0)
    b.light_point((rfw @ np.array([3.0, 4.0, 4.0, 1.0], np.float32))[:3], blackbody_dense(4000.0), scale=30.0)
    if environment is not None:
        rot = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float32)
        b.light_image_infinite(environment, scale=0.5, render_from_light=rot)
    sc = _finish(b, lib, extra_lights=extra_lights, rfw=rfw, name="instanced objects" + (" (baked)" if baked else "") + ("" if environment is None else " (environment map)"))
    sc.placements = placements
    return sc


def random_scene(lib, seed, width=40, height=32, film=None, extra_lights=None):
    """A seeded random scene for parity fuzzing: every shape kind (triangle meshes with and without per-vertex N / S / uv,
    full and partial transformed spheres, flat and curved bilinear patches), every material kind (including nested mixes
    and both coated ones), area lights on every shape kind, a point light, optionally a uniform infinite light, and a
    thin-lens camera for odd seeds. Nothing here is tuned to look good; it is tuned to reach code."""
    rng = np.random.Generator(np.random.PCG64(seed))
    b = SceneBuilder()
    b.set_film(width, height, **(film or {}))
    lens = 0.05 if seed % 2 else 0.0
    # every fourth seed looks through an OrthographicCamera (camera.rs:658-840; its screen window spans [-aspect, aspect] x [-1, 1]
    # world units, so it sees the middle of the scene)
    # (the reference's OrthographicCamera::generate_ray_differential leaves its rays in camera space, camera.rs:769-792: such a
    # camera only sees the scene if its axes are the world's, so the orthographic seeds look down +z with y up, from just in front of the back wall)
    ortho = bool(seed % 4 == 2)
    rfw = b.set_camera_look_at(lib, (0.0, 1.0, -2.9) if ortho else (0.0, 1.2, 6.0), (0.0, 1.0, 0.0) if ortho else (0.0, 0.8, 0.0), (0, 1, 0), 42.0,
                               lens_radius=lens, focal_distance=6.0, orthographic=ortho)

    # seeds >= 12 bind image textures to about half of the spectrum-texture slots, options drawn from their own
    # generator so that the scenes of the earlier seeds stay what they were
    trng = np.random.Generator(np.random.PCG64(1000 + seed))
    world_from_render = np.linalg.inv(np.asarray(rfw, np.float64).reshape(4, 4))

    def spec():
        if seed >= 12 and trng.random() < 0.5:
            nc = int(trng.choice([1, 3]))
            return b.add_image_texture(test_image(int(trng.choice([8, 16, 32])), nc, seed=int(trng.integers(0, 99))),
                                       filter=str(trng.choice(["point", "bilinear", "trilinear", "ewa"])),
                                       wrap=str(trng.choice(["black", "clamp", "repeat", "octahedralsphere"])),
                                       scale=float(trng.uniform(0.5, 1.2)), invert=bool(trng.random() < 0.3),
                                       spectrum_type=str(trng.choice(["albedo", "unbounded", "illuminant"])),
                                       mapping=str(trng.choice(["uv", "uv", "planar", "spherical", "cylindrical"])),
                                       su=float(trng.uniform(0.5, 4.0)), sv=float(trng.uniform(0.5, 4.0)), du=float(trng.uniform(0, 1)),
                                       dv=float(trng.uniform(0, 1)), max_anisotropy=float(trng.choice([1.0, 4.0, 8.0, 16.0])),
                                       vs=tuple(trng.uniform(-0.5, 0.5, 3)), vt=tuple(trng.uniform(-0.5, 0.5, 3)),
                                       texture_from_render=world_from_render, color_space=bool(nc == 3 or trng.random() < 0.5))
        k = rng.integers(0, 4)
        if k == 0:
            return float(rng.uniform(0.1, 0.9))
        if k == 3:  # RgbAlbedoSpectrum from sigmoid coefficients: x = c0 l^2 + c1 l + c2 stays within a few units over 360..830 nm
            c0 = float(rng.uniform(-2e-5, 2e-5))
            return b.spectrum_rgb((c0, float(rng.uniform(-6e-3, 6e-3)) - 1190.0 * c0, float(rng.uniform(-1.5, 1.5))))
        return _two_point_spectrum(b, float(rng.uniform(0.05, 0.9)), float(rng.uniform(0.05, 0.9)))

    singles = [
        b.material_diffuse(spec()),
        b.material_diffuse(spec()),
        b.material_conductor(b.spectrum_named("metal-Cu-eta"), b.spectrum_named("metal-Cu-k"), roughness=float(rng.uniform(0.0, 0.4))),
        b.material_conductor(b.spectrum_named("metal-Ag-eta"), b.spectrum_named("metal-Ag-k"), roughness=0.0),
        b.material_dielectric(1.5, roughness=float(rng.uniform(0.0, 0.3))),
        b.material_dielectric(b.spectrum_named("glass-F11"), roughness=0.0),
        b.material_dielectric(1.33, thin=True),
        b.material_coated_diffuse(reflectance=spec(), roughness=float(rng.uniform(0.0, 0.3)), thickness=float(rng.uniform(0.005, 0.1)),
                                  albedo=float(rng.choice([0.0, 0.5])), g=float(rng.uniform(-0.5, 0.5))),
        b.material_coated_conductor(interface_roughness=float(rng.uniform(0.0, 0.2)), conductor_roughness=float(rng.uniform(0.0, 0.3)),
                                    reflectance=(0.8 if rng.random() < 0.5 else None)),
    ]
    # (soak seeds only — seeds below 16 are pinned by golden films: an index-matched interface with a rough distribution, which BxDF::flags calls GLOSSY although
    #  every f and pdf of it is zero; found the one bug of round 3's specular / rough scatter split)
    if seed >= 16 and seed % 3 == 0:
        singles.append(b.material_dielectric(1.0, roughness=float(rng.uniform(0.05, 0.3))))
    mixes = [b.material_mix(int(rng.choice(singles)), int(rng.choice(singles)), float(rng.uniform(0.2, 0.8)))]
    mixes.append(b.material_mix(mixes[0], int(rng.choice(singles)), float(rng.uniform(0.2, 0.8))))
    mats = singles + mixes
    black = b.material_diffuse(0.0)
    emit = blackbody_dense(float(rng.uniform(3000.0, 7000.0)))

    def pick():
        return int(rng.choice(mats))

    # a floor and a back wall so that paths bounce
    p, vi = _quad((-5, 0, -5), (-5, 0, 7), (5, 0, 7), (5, 0, -5))
    b.add_mesh(_to_render(p, rfw), vi, singles[0])
    p, vi = _quad((-5, 0, -3), (5, 0, -3), (5, 5, -3), (-5, 5, -3))
    b.add_mesh(_to_render(p, rfw), vi, singles[1])
    # random triangle meshes: icospheres (with per-vertex normals / tangents / uv in some) and a triangle soup
    for k in range(3):
        sv, sf = icosphere(int(rng.integers(0, 3)))
        c = np.array([rng.uniform(-2.5, 2.5), rng.uniform(0.4, 2.0), rng.uniform(-1.5, 2.0)], np.float32)
        r = f32(rng.uniform(0.3, 0.8))
        verts = sv * r + c[None]
        kw = {}
        if k != 1:
            kw["n"] = sv / np.linalg.norm(sv, axis=1, keepdims=True)
        if k == 2:
            t = np.cross(sv, np.array([0.0, 1.0, 0.0], np.float32)) + np.float32(1e-3)
            kw["s"] = (t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.float32)
            kw["uv"] = np.stack([np.arctan2(sv[:, 2], sv[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(sv[:, 1], -1, 1)) / np.pi], 1).astype(np.float32)
        b.add_mesh(_to_render(verts, rfw), sf, pick(), reverse_orientation=bool(k == 1), **kw)
    soup = rng.uniform(-1.0, 1.0, size=(24, 3)).astype(np.float32) * np.array([2.5, 1.0, 1.5], np.float32) + np.array([0.0, 1.5, 0.5], np.float32)
    b.add_mesh(_to_render(soup, rfw), np.arange(24).reshape(8, 3), pick())
    # spheres: full, partial (z clip + phi), scaled / rotated
    for k in range(3):
        ang = rng.uniform(0, 2 * np.pi)
        rot = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], np.float32)
        rfo = np.eye(4, dtype=np.float32)
        rfo[:3, :3] = rot * (np.float32(rng.uniform(0.7, 1.3)) if k == 2 else np.float32(1.0))
        rfo[:3, 3] = np.array([rng.uniform(-3, 3), rng.uniform(0.6, 2.2), rng.uniform(-1, 2.5)], np.float32)
        rfo = (rfw @ rfo).astype(np.float32)
        kw = dict(z_min=-0.3, z_max=0.45, phi_max=float(rng.uniform(120, 300))) if k == 1 else {}
        b.add_sphere(0.5, pick(), render_from_object=rfo, reverse_orientation=bool(k == 2), **kw)
    # bilinear patches: a flat skewed quad and a saddle
    q = np.array([(-3.0, 0.2, 2.0), (-1.8, 0.2, 2.2), (-3.1, 1.4, 1.6), (-1.7, 1.6, 2.1)], np.float32) + rng.uniform(-0.1, 0.1, (4, 3)).astype(np.float32)
    b.add_patch_mesh(_to_render(q, rfw), [[0, 1, 2, 3]], pick(), reverse_orientation=bool(seed % 3 == 0))
    q = np.array([(1.5, 0.1, 2.5), (3.0, 0.1, 2.5), (1.5, 0.1, 3.6), (3.0, 0.1, 3.6)], np.float32)
    q[:, 1] += rng.uniform(0.0, 0.6, 4).astype(np.float32)
    # the saddle carries per-vertex uv (a sheared, scaled (s, t) frame) and, for some seeds, per-vertex shading normals
    uv = np.array([(0.0, 0.0), (2.0, 0.3), (0.2, 1.5), (2.3, 1.9)], np.float32)
    nn = None
    if seed % 2 == 0:
        nn = np.array([(0.2, 1.0, 0.1), (-0.1, 1.0, 0.2), (0.1, 1.0, -0.2), (-0.2, 1.0, -0.1)], np.float32)
        nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    b.add_patch_mesh(_to_render(q, rfw), [[0, 1, 2, 3]], pick(), n=nn, uv=uv)
    # lights: a triangle pair, a sphere, a rectangular patch and a skewed patch, a point light, sometimes the sky
    p, vi = _quad((-1, 4.5, -1), (1, 4.5, -1), (1, 4.5, 1), (-1, 4.5, 1))
    b.add_mesh(_to_render(p, rfw), vi, black, emission=emit, emission_scale=float(rng.uniform(5, 20)), two_sided=bool(seed % 2))
    rfo = np.eye(4, dtype=np.float32)
    rfo[:3, 3] = np.array([2.5, 3.0, 1.0], np.float32)
    b.add_sphere(0.25, black, render_from_object=(rfw @ rfo).astype(np.float32), emission=emit, emission_scale=8.0)
    q = np.array([(-3.5, 3.0, 0.0), (-2.5, 3.0, 0.0), (-3.5, 3.0, 1.0), (-2.5, 3.0, 1.0)], np.float32)  # faces down
    down = np.tile(np.array([[0.0, -1.0, 0.0]], np.float32), (4, 1))
    b.add_patch_mesh(_to_render(q, rfw), [[0, 1, 2, 3]], black, n=(down if seed % 3 == 2 else None), emission=emit, emission_scale=10.0)
    q = q + np.array([5.5, 0.3, 0.5], np.float32)
    q[3, 1] -= np.float32(0.05)
    b.add_patch_mesh(_to_render(q, rfw), [[0, 1, 2, 3]], black, emission=emit, emission_scale=10.0, two_sided=True)
    pos = (rfw @ np.array([0.0, 3.5, 3.0, 1.0], np.float32))[:3]
    b.light_point(pos, emit, scale=float(rng.uniform(2, 10)))
    if seed % 3 == 1:
        b.light_uniform_infinite(blackbody_dense(6500.0), scale=0.3)
    if seed >= 12 and seed % 2 == 1:  # object instancing (primitive.rs:136-176): every shape kind inside, a mirrored placement among them
        b.begin_object("thing")
        sv2, sf2 = icosphere(1)
        b.add_mesh((sv2 * np.float32(0.4)).astype(np.float32), sf2, int(trng.choice(mats)), n=(sv2 / np.linalg.norm(sv2, axis=1, keepdims=True)).astype(np.float32))
        rfo = np.eye(4, dtype=np.float32)
        rfo[:3, 3] = (0.6, 0.0, 0.1)
        b.add_sphere(0.3, int(trng.choice(mats)), render_from_object=rfo, z_min=-0.2, z_max=0.25, phi_max=250.0)
        q = np.array([(-0.7, -0.3, 0.1), (-0.2, -0.3, 0.3), (-0.7, 0.4, 0.0), (-0.2, 0.3, 0.5)], np.float32)
        b.add_patch_mesh(q, [[0, 1, 2, 3]], int(trng.choice(mats)))
        b.end_object()
        for k in range(3):
            a = trng.normal(size=3)
            a /= np.linalg.norm(a)
            ang = trng.uniform(0, 2 * np.pi)
            kk = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            m = np.eye(4)
            m[:3, :3] = (np.eye(3) + np.sin(ang) * kk + (1 - np.cos(ang)) * (kk @ kk)) @ np.diag(trng.uniform(0.7, 1.5, 3) * np.array([-1.0 if k == 2 else 1.0, 1.0, 1.0]))
            m[:3, 3] = (trng.uniform(-3, 3), trng.uniform(0.8, 2.5), trng.uniform(-1, 3))
            b.add_instance("thing", (np.asarray(rfw, np.float64).reshape(4, 4) @ m).astype(np.float32))
    if seed >= 12 and seed % 2 == 0:  # an ImageInfinitelight under a random rotation (even beside the uniform sky: two infinite lights)
        a = trng.normal(size=3)
        a /= np.linalg.norm(a)
        ang = trng.uniform(0, 2 * np.pi)
        k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        rot = np.eye(4)
        rot[:3, :3] = np.eye(3) + np.sin(ang) * k + (1 - np.cos(ang)) * (k @ k)
        b.light_image_infinite(environment_image(int(trng.choice([8, 16])), sun=tuple(trng.normal(size=3)), sun_radiance=float(trng.uniform(5, 60))),
                               scale=float(trng.uniform(0.002, 0.01)), render_from_light=rot)
    return _finish(b, lib, extra_lights=extra_lights, rfw=rfw, name=f"random scene {seed}")


def disk_and_cylinder(emissive_disk=True, glass_cylinder=False):
    """An `extra_lights`-style argument for the generators above — it is called at the same place, with (builder, render_from_world) — that appends SHAPES: PBRT-v4's
    disk and cylinder, given in WORLD space around the origin (a sector of an annulus lying flat at y = 0.3, an upright partial cylinder of radius 0.25 beside it) and,
    with `emissive_disk`, a small one-sided disk emitter above them that shines downwards. Their lights come after the scene's own."""
    def add(b, rfw):
        rfw = np.asarray(rfw, np.float32).reshape(4, 4)
        up = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float32)  # the object's +z is the world's +y
        down = np.array([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float32)  # ... the world's -y
        def place(rot, x, y, z):
            m = rot.copy()
            m[:3, 3] = (x, y, z)
            return (rfw @ m).astype(np.float32)
        b.add_disk(0.4, b.material_diffuse(0.6), height=0.0, inner_radius=0.15, phi_max=300.0, render_from_object=place(up, -0.45, 0.3, 0.2))
        cyl_m = b.material_dielectric(1.5) if glass_cylinder else b.material_conductor(b.spectrum_named("metal-Cu-eta"), b.spectrum_named("metal-Cu-k"), roughness=0.3)
        b.add_cylinder(0.25, cyl_m, z_min=0.0, z_max=0.7, phi_max=360.0 if glass_cylinder else 250.0, render_from_object=place(up, 0.45, 0.0, 0.1))
        if emissive_disk:
            b.add_disk(0.3, b.material_diffuse(0.0), render_from_object=place(down, 0.0, 1.6, 0.3), emission=blackbody_dense(5000.0), emission_scale=6.0)
    return add


def quadric_scene(lib, variant="lean", width=40, height=32, film=None, n_disks=96, as_spheres=False):
    """PBRT-v4's disk and cylinder (ShmSphere.quadric) in one small scene per scene class the general kernels serve. A floor of two triangles with a disk lying ON a
    triangle pair of the same centroid (a BVH leaf that holds a quadric together with triangles), an upright cylinder, a tilted and non-uniformly scaled annulus sector,
    a mirrored disk and a one-sided disk emitter overhead. `variant`:
      "lean"         every material a DiffuseMaterial
      "glass"        the cylinder is smooth glass: the material-sorted fused kernel
      "coated"       the floor a coated diffuse material: the staged LayeredBxDF kernels
      "textured"     the lying disk carries an image texture by its (u, v)
      "environment"  an environment map beside the emitter
      "instances"    a cylinder and a disk inside an object that is instanced three times, one cylinder at top level
      "many_disks"   `n_disks` small disks over the floor: quadrics are a twelfth of the primitive records or more, the five-wave traversal row
    `as_spheres`: the same records with quadric = 0 (what a build without the shapes would render) — for tests that the byte is read."""
    assert variant in ("lean", "glass", "coated", "textured", "environment", "instances", "many_disks")
    b = SceneBuilder()
    b.set_film(width, height, **(film or {}))
    rfw = np.asarray(b.set_camera_look_at(lib, (0.0, 1.5, 3.5), (0.0, 0.5, 0.0), (0, 1, 0), 38.0), np.float32).reshape(4, 4)
    up = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float64)    # object +z -> world +y
    down = np.array([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)  # object +z -> world -y

    def place(m, at):
        m = np.array(m, np.float64)
        m[:3, 3] = at
        return (rfw.astype(np.float64) @ m).astype(np.float32)

    grey = b.material_diffuse(0.55)
    floor_m = b.material_coated_diffuse(reflectance=0.5, roughness=0.1) if variant == "coated" else b.material_diffuse(_two_point_spectrum(b, 0.3, 0.6))
    p, vi = _quad((-3, 0, -3), (-3, 0, 3), (3, 0, 3), (3, 0, -3))
    b.add_mesh(_to_render(p, rfw), vi, floor_m)
    # a square plate as two triangles, each with the square's own bounding box, and the disk inscribed in it: three primitives with ONE centroid, which the builder
    # leaves in one leaf (aggregate.rs:345-356) — every coordinate a dyadic fraction, so that the three boxes are the same floats
    p, vi = _quad((-0.5, 0.25, -0.5), (-0.5, 0.25, 0.5), (0.5, 0.25, 0.5), (0.5, 0.25, -0.5))
    b.add_mesh(_to_render(p, rfw), vi, grey)
    if variant == "textured":
        disk_m = b.material_diffuse(b.add_image_texture(test_image(16, 3), filter="bilinear"))
    else:
        disk_m = b.material_diffuse(_two_point_spectrum(b, 0.7, 0.2))
    b.add_disk(0.5, disk_m, inner_radius=0.125, render_from_object=place(up, (0.0, 0.25, 0.0)))
    cyl_m = b.material_dielectric(1.5) if variant == "glass" else grey
    b.add_cylinder(0.25, cyl_m, z_min=0.0, z_max=0.8, phi_max=360.0 if variant == "glass" else 280.0, render_from_object=place(up, (0.9, 0.0, -0.2)))
    tilt = up.copy()
    c, s = np.cos(0.6), np.sin(0.6)
    tilt[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ up[:3, :3] @ np.diag([1.3, 0.7, 1.0])
    b.add_disk(0.45, grey, height=0.1, inner_radius=0.2, phi_max=250.0, render_from_object=place(tilt, (-0.95, 0.5, -0.1)))
    mirror = up.copy()
    mirror[:3, :3] = up[:3, :3] @ np.diag([-1.0, 1.0, 1.0])
    b.add_disk(0.3, grey, render_from_object=place(mirror, (0.2, 0.7, -0.9)), reverse_orientation=True)
    b.add_disk(0.35, b.material_diffuse(0.0), render_from_object=place(down, (0.0, 2.2, 0.2)), emission=blackbody_dense(5500.0), emission_scale=9.0)
    if variant == "environment":
        rot = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float32)
        b.light_image_infinite(environment_image(16), scale=0.3, render_from_light=rot)
    if variant == "instances":
        b.begin_object("post")
        b.add_cylinder(0.12, grey, z_min=0.0, z_max=0.6, render_from_object=up.astype(np.float32))
        cap = up.copy()
        cap[:3, 3] = (0.0, 0.6, 0.0)
        b.add_disk(0.2, disk_m, render_from_object=cap.astype(np.float32))
        b.end_object()
        for k, (x, z, sy) in enumerate(((-1.5, 0.6, 1.0), (1.5, 0.7, 1.4), (0.3, 1.2, 0.7))):
            m = np.diag([1.0, sy, 1.0, 1.0])
            a = 0.5 * k
            m[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ m[:3, :3]
            b.add_instance("post", place(m, (x, 0.0, z)))
    if variant == "many_disks":
        rng = np.random.Generator(np.random.PCG64(5))
        for _ in range(n_disks):
            b.add_disk(float(rng.uniform(0.05, 0.12)), grey, inner_radius=float(rng.uniform(0.0, 0.04)), phi_max=float(rng.uniform(120.0, 360.0)),
                       render_from_object=place(up, (rng.uniform(-1.6, 1.6), rng.uniform(0.05, 0.5), rng.uniform(-1.2, 1.2))))
    if as_spheres:
        for s in b.spheres:
            s.quadric = abi.SHM_QUADRIC_SPHERE
    return _finish(b, lib, rfw=rfw, name=f"disks and cylinders ({variant})" + (" as spheres" if as_spheres else ""))


def cutout_scene(lib, variant="lean", width=32, height=32, film=None, alpha="checker", disk=False, n_leaves=0, cut=True):
    """PBRT-v4's shape alpha (`alpha=` of the SceneBuilder's shapes) in one small scene per scene class: an open box lit by a quad emitter overhead and in front, and in
    front of its back wall a quad of two triangles cut by a 4 x 4 checkerboard over its (u, v) — seen directly, and as the shadow it casts on the wall —, a bilinear patch
    cut by dots, and a sphere cut by a checkerboard over its (phi, theta). `variant`:
      "lean"         every material a DiffuseMaterial
      "glass"        the cut sphere is smooth glass: the material-sorted fused kernel
      "coated"       the floor a coated diffuse material: the staged LayeredBxDF kernels
      "textured"     the cut quad's reflectance is an image texture over the same (u, v)
      "environment"  an environment map beside the emitter
      "instances"    a cut quad and a cut sphere inside an object that is instanced twice
    `alpha`: the quad's texture — "checker", a number (a constant) or None; `disk`: a cut annulus as well (PBRT-v4's disk: the extended kernels); `n_leaves`: that many
    small cut triangles scattered in front of the wall; `cut=False`: the same shapes without any alpha (what a build that ignores the field would render)."""
    assert variant in ("lean", "glass", "coated", "textured", "environment", "instances")
    b = SceneBuilder()
    b.set_film(width, height, **(film or {}))
    rfw = np.asarray(b.set_camera_look_at(lib, (0.0, 1.0, 3.6), (0.0, 0.9, 0.0), (0, 1, 0), 40.0), np.float32).reshape(4, 4)

    def place(m, at):
        m = np.array(m, np.float64)
        m[:3, 3] = at
        return (rfw.astype(np.float64) @ m).astype(np.float32)

    def a(tex):
        return tex if cut else None

    grey = b.material_diffuse(0.55)
    floor_m = b.material_coated_diffuse(reflectance=0.5, roughness=0.1) if variant == "coated" else b.material_diffuse(_two_point_spectrum(b, 0.3, 0.6))
    p, vi = _box((-1.6, 0.0, -1.5), (1.6, 2.4, 1.5), faces="xXz")
    b.add_mesh(_to_render(p, rfw), vi, b.material_diffuse(_two_point_spectrum(b, 0.6, 0.4)))
    p, vi = _quad((-1.6, 0.0, -1.5), (-1.6, 0.0, 1.5), (1.6, 0.0, 1.5), (1.6, 0.0, -1.5))
    b.add_mesh(_to_render(p, rfw), vi, floor_m)
    p, vi = _quad((-0.4, 2.3, 0.6), (0.4, 2.3, 0.6), (0.4, 2.3, 1.2), (-0.4, 2.3, 1.2))
    b.add_mesh(_to_render(p, rfw), vi, b.material_diffuse(0.0), emission=blackbody_dense(5500.0), emission_scale=14.0)
    # the cut quad: (u, v) = (0, 0) .. (1, 1) over it, four cells each way
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    checker4 = b.ftex_checkerboard(None, None, mapping=b.add_texture_mapping("uv", su=4.0, sv=4.0))
    quad_alpha = checker4 if alpha == "checker" else alpha
    quad_m = b.material_diffuse(b.add_image_texture(test_image(16, 3), filter="bilinear")) if variant == "textured" else b.material_diffuse(_two_point_spectrum(b, 0.7, 0.2))
    p, vi = _quad((-0.9, 0.3, -0.6), (0.3, 0.3, -0.6), (0.3, 1.7, -0.6), (-0.9, 1.7, -0.6))
    b.add_mesh(_to_render(p, rfw), vi, quad_m, uv=uv, alpha=a(quad_alpha))
    # a skewed bilinear patch cut by dots, eight cells each way
    dots = b.ftex_dots(0.0, 1.0, mapping=b.add_texture_mapping("uv", su=6.0, sv=6.0))
    pp = np.array([(0.5, 0.2, 0.2), (1.3, 0.2, -0.1), (0.5, 1.1, 0.0), (1.3, 1.3, -0.4)], np.float32)
    b.add_patch_mesh(_to_render(pp, rfw), np.array([[0, 1, 2, 3]], np.uint32), grey, uv=np.array([[0, 0], [1, 0], [0, 1], [1, 1]], np.float32), alpha=a(dots))
    # a sphere cut by a checkerboard over (phi / phi_max, theta): a cage
    cage = b.ftex_checkerboard(None, None, mapping=b.add_texture_mapping("uv", su=8.0, sv=4.0))
    up = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float64)  # object +z -> world +y
    b.add_sphere(0.4, b.material_dielectric(1.5) if variant == "glass" else grey, render_from_object=place(up, (-0.2, 0.45, 0.5)), alpha=a(cage))
    if disk:
        b.add_disk(0.45, grey, inner_radius=0.1, phi_max=300.0, render_from_object=place(np.eye(4), (0.9, 1.8, -0.9)), alpha=a(0.5))
    if n_leaves:
        rng = np.random.Generator(np.random.PCG64(17))
        leaf = b.ftex_checkerboard(None, None, mapping=b.add_texture_mapping("uv", su=2.0, sv=2.0))
        ps, vis = [], []
        for k in range(n_leaves):
            c = np.array([rng.uniform(-1.4, 1.4), rng.uniform(0.2, 2.1), rng.uniform(-1.3, -0.8)])
            e0, e1 = rng.uniform(-0.15, 0.15, 3), rng.uniform(-0.15, 0.15, 3)
            ps += [c, c + e0, c + e1]
            vis.append([3 * k, 3 * k + 1, 3 * k + 2])
        b.add_mesh(_to_render(np.array(ps, np.float32), rfw), np.array(vis, np.uint32), grey, uv=np.tile(np.array([[0, 0], [1, 0], [0, 1]], np.float32), (n_leaves, 1)), alpha=a(leaf))
    if variant == "environment":
        rot = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], np.float32)
        b.light_image_infinite(environment_image(16), scale=0.3, render_from_light=rot)
    if variant == "instances":
        b.begin_object("fence")
        p, vi = _quad((-0.3, 0.0, 0.0), (0.3, 0.0, 0.0), (0.3, 0.8, 0.0), (-0.3, 0.8, 0.0))
        b.add_mesh(p, vi, quad_m, uv=uv, alpha=a(quad_alpha))
        ball = up.copy()
        ball[:3, 3] = (0.0, 1.0, 0.0)
        b.add_sphere(0.2, grey, render_from_object=ball.astype(np.float32), alpha=a(cage))
        b.end_object()
        for k, (x, z, sy) in enumerate(((-1.1, 0.7, 1.0), (1.0, 0.9, 1.3))):
            m = np.diag([1.0, sy, 1.0, 1.0])
            ang = 0.4 + 0.7 * k
            m[:3, :3] = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]) @ m[:3, :3]
            b.add_instance("fence", place(m, (x, 0.0, z)))
    return _finish(b, lib, rfw=rfw, name=f"cutouts ({variant})" + ("" if cut else " uncut"))
