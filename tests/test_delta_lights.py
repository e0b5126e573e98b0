"""PBRT-v4's distant and spot lights (SHM_LIGHT_DISTANT, SHM_LIGHT_SPOT; shm/path.h) on the CPU oracle: leaf values against a float64 restatement of the
semantics, deterministic renders of a diffuse floor (spot == point * smoothstep per pixel; distant == (R / pi) cos(theta) L in absolute terms, shadow edges),
linearity in the emitters under the uniform light sampler, the PBRT front end's parameters, and the ABI.

float32 error model used for the bounds below (U = 2^-24, the relative error of one correctly rounded operation):
  * cos(theta) of a spot light is (M w).z / |M w| with w = -wi a normalised difference: w carries 4 U per component (subtract, three squares and two sums, sqrt,
    divide); a row's dot product adds 4 U |row| |w| to the 4 U it inherits: 8 U KAPPA relative to |M w| with KAPPA = |M| |w| / |M w| (1 for a rigid light
    transform); the quotient z / len doubles it and adds two roundings: COS_ERR = 16 U KAPPA + 2 U;
  * the ramp t = (cos - cos_end) / (cos_start - cos_end) divides that by the ramp's width and adds three roundings;
  * smoothstep's slope is at most 1.5, and its own evaluation adds four roundings;
  * I / d^2 with the spectrum sample and the scale adds six more.
So |L - L64| <= L_axis * (1.5 * (COS_ERR / width + 3 U) + 10 U) where L_axis = scale * spectrum / d^2 is the unattenuated value."""
import ctypes as C
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_py
from shimmer_amd import abi, render, scene as scn
from shimmer_amd.scenes import _quad, _to_render, blackbody_dense

ROOT = Path(__file__).resolve().parents[1]
F, FP = C.c_float, C.POINTER(C.c_float)
U = 2.0 ** -24
LAMBDA = (451.3, 520.0, 611.8, 700.2)
ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -2  # (include/shimmer_hip.h)


def fa(v):
    v = np.asarray(v, np.float32).ravel()
    return (F * len(v))(*[float(x) for x in v])


def smoothstep64(x, a, b):
    if a == b:
        return 0.0 if x < a else 1.0
    t = min(max((x - a) / (b - a), 0.0), 1.0)
    return t * t * (3.0 - 2.0 * t)


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = c * np.eye(3) + s * k + (1 - c) * np.outer(a, a)
    return m


def leaf_tolerance(kappa, width):
    cos_err = 16 * U * kappa + 2 * U
    return cos_err, (1.5 * (cos_err / width + 3 * U) + 10 * U) if width > 0 else 10 * U


def spot_expected(light, spot, dense, ctx=(0.0, 0.0, 0.0)):
    """Section 1 of the semantics in float64 from the float32 fields of the ABI records: (wi, cos, L_axis[4], falloff, kappa)."""
    p_l = np.array(light.position[:], np.float64)
    d = p_l - np.asarray(ctx, np.float64)
    d2 = float(d @ d)
    wi = d / math.sqrt(d2)
    m3 = np.array(spot.light_from_render[:], np.float64).reshape(4, 4)[:3, :3]
    wl = m3 @ (-wi)
    cos = float(wl[2] / np.linalg.norm(wl))
    spec = np.array([float(dense[int(round(l)) - 360]) for l in LAMBDA])
    kappa = float(np.linalg.norm(m3, 2) / np.linalg.norm(wl))
    return wi, cos, float(light.scale) * spec / d2, smoothstep64(cos, float(spot.cos_falloff_end), float(spot.cos_falloff_start)), kappa


def sample_li(o, index):
    out = (F * 8)()
    ok = o.lib.orc_fn_light_sample_li(o.handle, index, fa((0.5, 0.5)), 1, fa(LAMBDA), out)
    return ok, np.array(out[:], np.float64)


def leaf_scene(lib):
    """A floor and the grid of lights of test 1, all seen from the render-space origin (the context of orc_fn_light_sample_li). Returns the builder (kept alive),
    the description and per light what the test expects of it."""
    b = scn.SceneBuilder()
    b.set_film(4, 4)
    b.set_camera_look_at(lib, (0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0)
    p, vi = _quad((-4, -1, -4), (-4, -1, 4), (4, -1, 4), (4, -1, -4))
    b.add_mesh(p, vi, b.material_diffuse(0.5))
    dense = blackbody_dense(4500.0)
    cases = []
    # spot lights: apex, target, cone
    for frm, to, cone, delta, note in (
            ((0.0, 2.0, 0.0), (0.0, 0.0, 0.0), 30.0, 5.0, "on the axis"),
            ((0.3, 2.0, -0.2), (0.0, -1.0, 0.5), 40.0, 15.0, "inside the ramp"),
            ((1.0, 2.0, 0.0), (1.0, 0.0, 0.0), 30.0, 5.0, "in the ramp (26.6 degrees off the axis)"),
            ((1.1, 2.0, 0.0), (1.1, 0.0, 0.0), 30.0, 2.0, "in a narrow ramp"),
            ((2.0, 2.0, 0.0), (2.0, 0.0, 0.0), 30.0, 5.0, "outside the cone"),
            ((0.0, 2.0, 0.0), (0.0, 4.0, 0.0), 60.0, 10.0, "behind the light"),
            ((0.5, 2.0, 0.0), (0.5, 0.0, 0.0), 25.0, 0.0, "conedelta 0, inside"),
            ((1.5, 2.0, 0.0), (1.5, 0.0, 0.0), 25.0, 0.0, "conedelta 0, outside"),
            ((-0.7, 1.5, 2.5), (0.2, -1.0, -0.3), 170.0, 160.0, "a wide cone"),
    ):
        b.light_spot(frm, to, dense, scale=7.0, coneangle=cone, conedelta=delta)
        cases.append(("spot", note))
    # a non-uniformly scaled, rotated light transform: PBRT-v4 takes -wi to light space by the INVERSE matrix
    m = rot((1, 2, 3), 40.0) @ np.diag([1.0, 2.5, 0.4, 1.0])
    m[:3, 3] = (0.4, 1.8, -0.6)
    u = np.linalg.inv(m[:3, :3]) @ -m[:3, 3]  # the origin of render space seen from the apex, in the light's object space ...
    u = u / np.linalg.norm(u)
    v = np.cross(u, (0.0, 0.0, 1.0))
    to = math.cos(math.radians(40.0)) * u + math.sin(math.radians(40.0)) * v / np.linalg.norm(v)  # ... and an axis 40 degrees off it THERE: inside the ramp (30 .. 50)
    b.light_spot((0.0, 0.0, 0.0), to, dense, scale=3.0, coneangle=50.0, conedelta=20.0, render_from_object=m.astype(np.float32))
    cases.append(("spot", "non-uniform scale"))
    # exactly on cos_end: light space = render space mirrored in z, apex (0, 3, 4): -wi = (0, -0.6f, -0.8f), whose float32 cosine is restated here operation by operation
    f32 = np.float32
    wy, wz = f32(3.0) / f32(5.0), f32(4.0) / f32(5.0)
    cos_edge = wz / np.sqrt(f32(f32(f32(0.0) + wy * wy) + wz * wz))
    for delta_zero in (False, True):
        b.light_spot((0.0, 3.0, 4.0), (0.0, 3.0, 3.0), dense, scale=5.0, coneangle=30.0, conedelta=5.0)
        sp = b.spot_lights[-1]
        sp.light_from_render[:] = [1, 0, 0, 0, 0, 1, 0, -3, 0, 0, -1, 4, 0, 0, 0, 1]
        sp.render_from_light[:] = [1, 0, 0, 0, 0, 1, 0, 3, 0, 0, -1, 4, 0, 0, 0, 1]
        sp.cos_falloff_end = float(cos_edge)
        sp.cos_falloff_start = float(cos_edge) if delta_zero else 0.95
        cases.append(("spot-edge", "cos == cos_end" + (" == cos_start" if delta_zero else "")))
    for frm, to, m in (((0, 0, 0), (0, 0, 1), None), ((1.0, 3.0, -2.0), (0.0, 0.0, 0.0), None), ((0, 1, 0), (0, 0, 0), rot((0, 0, 1), 25.0) @ np.diag([1.0, 3.0, 0.5, 1.0]))):
        b.light_distant(dense, scale=2.5, frm=frm, to=to, render_from_object=None if m is None else m.astype(np.float32))
        w = np.asarray(frm, np.float64) - np.asarray(to, np.float64)
        w = w / np.linalg.norm(w)
        if m is not None:
            w = m[:3, :3] @ w
            w = w / np.linalg.norm(w)
        cases.append(("distant", w))
    desc, _ = b.build(lib)
    return b, desc, dense, cases


def test_leaf_values_against_float64(lib):
    b, desc, dense, cases = leaf_scene(lib)
    o = oracle_py.Oracle(desc)
    o.lib.orc_fn_light_sample_li.restype, o.lib.orc_fn_light_sample_li.argtypes = C.c_int, [C.c_void_p, C.c_uint32, FP, C.c_int, FP, FP]
    seen = set()
    for i, (kind, note) in enumerate(cases):
        light = desc.lights[i]
        ok, out = sample_li(o, i)
        if kind == "distant":
            assert light.kind == abi.SHM_LIGHT_DISTANT
            w32 = np.array(light.position[:], np.float64)
            assert np.allclose(w32, note, atol=8 * U) and abs(np.linalg.norm(w32) - 1.0) < 4 * U
            spec = np.array([float(dense[int(round(l)) - 360]) for l in LAMBDA])
            assert ok == 1 and np.array_equal(out[:3], w32) and out[3] == 1.0  # wi IS the stored vector
            assert np.allclose(out[4:], float(light.scale) * spec, rtol=2 * U, atol=0), (out[4:], float(light.scale) * spec)
            continue
        assert light.kind == abi.SHM_LIGHT_SPOT
        spot = b.spot_lights[light.primitive]
        wi, cos, l_axis, falloff, kappa = spot_expected(light, spot, dense)
        width = float(spot.cos_falloff_start) - float(spot.cos_falloff_end)
        cos_err, tol = leaf_tolerance(kappa, width)
        if kind == "spot-edge":
            want_sample = width == 0.0  # x == a == b -> 1; on a ramp t = 0 -> I = 0 -> no sample
            assert ok == (1 if want_sample else 0), note
            if want_sample:
                assert np.allclose(out[4:], l_axis, rtol=10 * U, atol=0)
            seen.add(note)
            continue
        # (a case must not sit within the rounding of cos(theta) of an edge of its ramp, where "no sample" itself would be ambiguous)
        assert abs(cos - float(spot.cos_falloff_end)) > 4 * cos_err, note
        if falloff == 0.0:
            assert ok == 0, note  # exactly "no sample"
            seen.add("none")
            continue
        assert ok == 1, note
        assert np.allclose(out[:3], wi, atol=4 * U) and out[3] == 1.0, note
        print(f"{note}: cos {cos:.7f} falloff {falloff:.6f} kappa {kappa:.2f} max |L - L64| / L_axis = {np.max(np.abs(out[4:] - falloff * l_axis) / l_axis):.3e} (bound {tol:.3e})")
        assert np.all(np.abs(out[4:] - falloff * l_axis) <= tol * l_axis), note
        seen.add("full" if falloff == 1.0 else "ramp")
        if note == "non-uniform scale":  # (a transformed AXIS would put this context at another angle: the test sees the difference)
            assert 0.0 < falloff < 1.0 and kappa > 1.5
            axis_render = np.array(spot.render_from_light[:], np.float64).reshape(4, 4)[:3, 2]
            assert abs(float(-wi @ axis_render / np.linalg.norm(axis_render)) - cos) > 0.02
    assert {"none", "full", "ramp", "cos == cos_end", "cos == cos_end == cos_start"} <= seen
    # delta lights: pdf_li = 0 for any direction
    o.lib.orc_fn_image_light_pdf.restype, o.lib.orc_fn_image_light_pdf.argtypes = F, [C.c_void_p, C.c_uint32, FP, C.c_int]
    for i in (0, len(cases) - 1):
        assert o.lib.orc_fn_image_light_pdf(o.handle, i, fa((0.0, 1.0, 0.0)), 1) == 0.0
    o.close()


# ---- the floor renders -----------------------------------------------------------------------------------------------------------------
R, W = 0.5, 24


def floor_builder(lib):
    b = scn.SceneBuilder()
    b.set_film(W, W)
    rfw = b.set_camera_look_at(lib, (0.0, 1.2, 4.0), (0.0, 0.0, 0.3), (0, 1, 0), 30.0)
    p, vi = _quad((-40, 0, -40), (-40, 0, 40), (40, 0, 40), (40, 0, -40))
    b.add_mesh(_to_render(p, rfw), vi, b.material_diffuse(R))
    return b, rfw


def floor_points(o, desc, rfw):
    """the floor point of every pixel centre (world space): its camera ray met with the plane y = 0, float64"""
    o.lib.orc_fn_camera_ray_differential.restype, o.lib.orc_fn_camera_ray_differential.argtypes = None, [C.c_void_p, FP, FP, FP]
    cam_pos = -np.asarray(rfw, np.float64).reshape(4, 4)[:3, 3]
    pts = np.zeros((W, W, 3))
    for y in range(W):
        for x in range(W):
            out = (F * 18)()
            o.lib.orc_fn_camera_ray_differential(C.byref(desc.camera), fa((x + 0.5, y + 0.5)), fa((0.5, 0.5)), out)
            org, d = np.array(out[0:3], np.float64) + cam_pos, np.array(out[3:6], np.float64)
            assert d[1] < -1e-3  # the camera sees only floor
            pts[y, x] = org + (-org[1] / d[1]) * d
    return pts


def render_floor(lib, add_lights, seed=11, spp=4, max_depth=1, jitter=False, with_points=True):
    b, rfw = floor_builder(lib)
    add_lights(b, rfw)
    desc, _ = b.build(lib)
    o = oracle_py.Oracle(desc)
    film, stats = o.render(render.make_params(seed=seed, spp=spp, max_depth=max_depth, disable_pixel_jitter=not jitter), n_threads=8)
    pts = floor_points(o, desc, rfw) if with_points else None
    o.close()
    return render.film_to_rgb(film).astype(np.float64), stats, pts, (b, desc)


def test_spot_is_the_point_light_times_the_smoothstep_per_pixel(lib):
    apex, target, cone, delta = np.array([0.2, 2.0, 0.4]), np.array([0.1, 0.0, 0.2]), 28.0, 12.0
    dense = blackbody_dense(4000.0)
    spp = 4
    point, st_p, pts, _ = render_floor(lib, lambda b, rfw: b.light_point(_to_render(apex[None], rfw)[0], dense, scale=9.0), spp=spp)
    spot, st_s, _, (b, desc) = render_floor(lib, lambda b, rfw: b.light_spot(apex, target, dense, scale=9.0, coneangle=cone, conedelta=delta, render_from_object=rfw), spp=spp)
    sp = b.spot_lights[0]
    assert desc.lights[0].scale == pytest.approx(9.0 / float(scn.spectrum_to_photometric(dense)), rel=4 * U)
    axis = (target - apex) / np.linalg.norm(target - apex)
    cos_start, cos_end = float(sp.cos_falloff_start), float(sp.cos_falloff_end)
    # the floor point itself is a float32 intersection (its error bound is a few gamma(n) |p|: 16 U |p| taken here, with |p| <= 8 in render space) seen from
    # at least 2 away: that moves cos(theta) by up to 16 U * 8 / 2 on top of the leaf's own error
    cos_err = 64 * U + leaf_tolerance(1.0, cos_start - cos_end)[0]
    tol = 1.5 * (cos_err / (cos_start - cos_end) + 3 * U) + 16 * U
    n_inside = 0
    worst = 0.0
    for y in range(W):
        for x in range(W):
            d = pts[y, x] - apex
            cos = float(d @ axis / np.linalg.norm(d))
            assert abs(cos - cos_end) > 4 * cos_err  # (no pixel centre sits on the cone's edge: inside / outside is decided)
            s = smoothstep64(cos, cos_end, cos_start)
            assert np.all(point[y, x] > 0)
            if s == 0.0:
                assert np.all(spot[y, x] == 0.0), (x, y)
            else:
                n_inside += 1
                err = float(np.max(np.abs(spot[y, x] - s * point[y, x]) / point[y, x]))
                worst = max(worst, err)
                assert err <= tol, (x, y, cos, s, err, tol)
    print(f"spot == point * smoothstep: {n_inside} of {W * W} pixels inside the cone, worst relative error {worst:.3e} (bound {tol:.3e})")
    assert 0 < n_inside < W * W
    # at maxdepth 1 only the first vertex estimates direct lighting, and a vertex outside the cone queues no shadow ray
    assert st_p["rays_any"] == W * W * spp and st_s["rays_any"] == n_inside * spp and st_s["rays_any"] < st_p["rays_any"]


def calibration_film(lib, dense, scale, seed, spp):
    """The film value of radiance scale * spectrum: a render that looks straight into an emitter of that spectrum and scale, same film size, same seed, no jitter."""
    b = scn.SceneBuilder()
    b.set_film(W, W)
    rfw = b.set_camera_look_at(lib, (0, 0, 0), (0, 0, -1), (0, 1, 0), 30.0)
    p, vi = _quad((-50, -50, -1), (50, -50, -1), (50, 50, -1), (-50, 50, -1))
    b.add_mesh(_to_render(p, rfw), vi, b.material_diffuse(0.0), emission=dense, emission_scale=scale)
    desc, _ = b.build(lib)
    o = oracle_py.Oracle(desc)
    film, _ = o.render(render.make_params(seed=seed, spp=spp, max_depth=0, disable_pixel_jitter=True), n_threads=4)
    o.close()
    return render.film_to_rgb(film).astype(np.float64)


def test_distant_light_in_absolute_terms_and_its_shadow(lib):
    dense, scale, seed, spp = blackbody_dense(5500.0), 1.5, 23, 4
    le = calibration_film(lib, dense, scale, seed, spp)
    assert np.all(le > 0)
    for frm in ((0.0, 1.0, 0.0), (1.0, 2.0, 0.5), (-3.0, 1.0, 2.0)):
        w = np.asarray(frm, np.float64) / np.linalg.norm(frm)
        rgb, stats, _, _ = render_floor(lib, lambda b, rfw: b.light_distant(dense, scale=scale, frm=frm, to=(0, 0, 0), render_from_object=rfw), seed=seed, spp=spp, with_points=False)
        want = (R / math.pi) * w[1] * le
        # per sample: f = R * (1 / pi), |wi . n|, the product with L and with beta, then the same film arithmetic on a value scaled by a constant: 12 roundings
        # on top of the 4 U of the stored direction
        err = float(np.max(np.abs(rgb - want) / want))
        print(f"distant light from {frm}: cos(theta) {w[1]:.4f}, worst relative error {err:.3e} (bound {16 * U:.3e})")
        assert err <= 16 * U
        assert stats["rays_any"] == W * W * spp
    # at and beyond 90 degrees of incidence the floor is black
    for frm in ((1.0, 0.0, 0.0), (1.0, -0.5, 0.0)):
        rgb, _, _, _ = render_floor(lib, lambda b, rfw: b.light_distant(dense, scale=scale, frm=frm, to=(0, 0, 0), render_from_object=rfw), seed=seed, spp=spp, with_points=False)
        assert np.all(rgb == 0.0)
    # an occluder: a rectangle at height h casts the rectangle moved by -(h / w.y) w
    frm, h, lo, hi = (1.0, 2.0, 0.5), 0.5, np.array([-0.6, -0.2]), np.array([0.5, 0.9])
    w = np.asarray(frm, np.float64) / np.linalg.norm(frm)

    def lights(b, rfw):
        b.light_distant(dense, scale=scale, frm=frm, to=(0, 0, 0), render_from_object=rfw)
        p, vi = _quad((lo[0], h, lo[1]), (hi[0], h, lo[1]), (hi[0], h, hi[1]), (lo[0], h, hi[1]))
        b.add_mesh(_to_render(p, rfw), vi, b.material_diffuse(0.0))
    rgb, _, pts, _ = render_floor(lib, lights, seed=seed, spp=spp)
    want = (R / math.pi) * w[1] * le
    n_dark = n_lit = 0
    for y in range(1, W - 1):
        for x in range(1, W - 1):
            # the camera must see the floor point itself, not the occluder in front of it: the camera ray passes the height h at this point
            cam = np.array([0.0, 1.2, 4.0])
            t = (h - cam[1]) / (pts[y, x][1] - cam[1])
            via = cam + t * (pts[y, x] - cam)
            if np.all(via[[0, 2]] > lo - 0.05) and np.all(via[[0, 2]] < hi + 0.05):
                continue
            up = pts[y, x] + (h / w[1]) * w  # where the shadow ray passes the occluder's plane
            margin = max(np.linalg.norm(pts[y, x] - pts[y, x + 1]), np.linalg.norm(pts[y, x] - pts[y + 1, x]), np.linalg.norm(pts[y, x] - pts[y - 1, x]))  # one pixel on the floor
            q = up[[0, 2]]
            if np.all(q > lo + margin) and np.all(q < hi - margin):
                assert np.all(rgb[y, x] == 0.0), (x, y)
                n_dark += 1
            elif np.any(q < lo - margin) or np.any(q > hi + margin):
                assert np.all(np.abs(rgb[y, x] - want[y, x]) <= 16 * U * want[y, x]), (x, y)
                n_lit += 1
    assert n_dark >= 4 and n_lit >= 100, (n_dark, n_lit)


def test_an_area_light_and_a_spot_light_add_up(lib):
    """Transport is linear in the emitters and the uniform light sampler divides by its pmf (1/2 with two lights... three here: the emitter is two triangles), so
    the combined image is the sum of the single-light images in expectation, at any depth. Means over the image and over 2 x 2 blocks; per seed the combined render is
    compared with the pair of single-light renders at 4x the samples; the margin is 4 standard errors of the mean difference, estimated over the seeds."""
    dense_a, dense_s = blackbody_dense(6500.0), blackbody_dense(3000.0)

    def area(b, rfw):
        p, vi = _quad((-0.4, 2.0, -0.4), (0.4, 2.0, -0.4), (0.4, 2.0, 0.4), (-0.4, 2.0, 0.4))
        b.add_mesh(_to_render(p, rfw), vi, b.material_diffuse(0.0), emission=dense_a, emission_scale=6.0)
        # a wall, so that deeper paths matter
        p, vi = _quad((-2, 0, -1.5), (2, 0, -1.5), (2, 3, -1.5), (-2, 3, -1.5))
        b.add_mesh(_to_render(p, rfw), vi, b.material_diffuse(0.7))

    def spot(b, rfw, with_geometry=False):
        if with_geometry:  # (the same scene without the emission: a black quad in the emitter's place)
            p, vi = _quad((-0.4, 2.0, -0.4), (0.4, 2.0, -0.4), (0.4, 2.0, 0.4), (-0.4, 2.0, 0.4))
            b.add_mesh(_to_render(p, rfw), vi, b.material_diffuse(0.0))
            p, vi = _quad((-2, 0, -1.5), (2, 0, -1.5), (2, 3, -1.5), (-2, 3, -1.5))
            b.add_mesh(_to_render(p, rfw), vi, b.material_diffuse(0.7))
        b.light_spot((1.0, 1.5, 1.0), (0.0, 0.0, -0.3), dense_s, scale=12.0, coneangle=35.0, conedelta=15.0, render_from_object=rfw)

    def both(b, rfw):
        area(b, rfw)
        spot(b, rfw)

    for depth in (1, 4):
        diffs = []
        for seed in range(12):
            kw = dict(max_depth=depth, jitter=True, with_points=False)
            c = render_floor(lib, both, seed=100 + seed, spp=16, **kw)[0]
            a = render_floor(lib, area, seed=300 + seed, spp=64, **kw)[0]
            s = render_floor(lib, lambda b, rfw: spot(b, rfw, True), seed=500 + seed, spp=64, **kw)[0]
            d = (c - (a + s))[..., 1]
            diffs.append([d.mean()] + [d[y0:y0 + W // 2, x0:x0 + W // 2].mean() for y0 in (0, W // 2) for x0 in (0, W // 2)])
            level = (a + s)[..., 1].mean()
        diffs = np.array(diffs)
        mean, se = diffs.mean(axis=0), diffs.std(axis=0, ddof=1) / math.sqrt(len(diffs))
        print(f"maxdepth {depth}: level {level:.4e}, mean difference / 4 SE per region: {(np.abs(mean) / (4 * se)).round(3).tolist()}")
        assert np.all(se < 0.05 * level)  # (the comparison has the power to see a wrong pmf: a factor 2/3 or 3/2 would be > 10 SE)
        assert np.all(np.abs(mean) <= 4 * se), (mean, se)


# ---- the PBRT front end -----------------------------------------------------------------------------------------------------------------
HEAD = ('LookAt 0 0 0  0 0 -1  0 1 0\nCamera "perspective" "float fov" 40\nFilm "rgb" "integer xresolution" 8 "integer yresolution" 8\n'
        'WorldBegin\nShape "trianglemesh" "point3 P" [ -4 -1 -4  -4 -1 4  4 -1 4  4 -1 -4 ] "integer indices" [ 0 1 2 0 2 3 ]\n')


def load(lib, tmp_path, text, name="s.pbrt"):
    (tmp_path / name).write_text(text)
    out = C.POINTER(abi.ShmPbrtScene)()
    rc = lib.shm_scene_load_pbrt(str(tmp_path / name).encode(), C.byref(out))
    return rc, out


def test_loader_defaults_transforms_and_photometric_parameters(lib, tmp_path):
    ctm = rot((0, 1, 0), 30.0) @ np.diag([1.0, 2.0, 0.5, 1.0])
    text = HEAD + ('LightSource "point"\nLightSource "distant"\nLightSource "spot"\n'
                   'AttributeBegin\nRotate 30 0 1 0\nScale 1 2 0.5\n'
                   'LightSource "distant" "point3 from" [ 1 2 3 ] "point3 to" [ 0 1 -1 ] "blackbody L" 5500 "float scale" 2 "float illuminance" 700\n'
                   'LightSource "spot" "point3 from" [ 1 2 3 ] "point3 to" [ 0 -1 1 ] "blackbody I" 3200 "float coneangle" 40 "float conedelta" 12 "float power" 900 "float scale" 3\n'
                   'AttributeEnd\n')
    rc, out = load(lib, tmp_path, text)
    assert rc == 0, lib.shm_last_error().decode()
    d = out.contents.desc
    assert d.n_lights == 5 and d.n_spot_lights == 2
    pt, dist0, spot0, dist1, spot1 = (d.lights[i] for i in range(5))
    assert [l.kind for l in (pt, dist0, spot0, dist1, spot1)] == [abi.SHM_LIGHT_POINT, abi.SHM_LIGHT_DISTANT, abi.SHM_LIGHT_SPOT, abi.SHM_LIGHT_DISTANT, abi.SHM_LIGHT_SPOT]
    spec = np.ctypeslib.as_array(d.spectrum_data, (d.n_spectrum_floats,))

    def table(l):
        assert l.spectrum.kind == abi.SHM_SPECTRUM_DENSE
        return spec[l.spectrum.offset:l.spectrum.offset + l.spectrum.n].copy()
    # defaults: the colour space's illuminant as the point light's I, scale = 1 / its photometric integral; from 0 0 0 to 0 0 1: light arrives from -z, the spot shines along +z
    for l in (dist0, spot0):
        assert np.array_equal(table(l), table(pt)) and l.scale == pt.scale
    assert tuple(dist0.position) == (0.0, 0.0, -1.0)
    sp = d.spot_lights[spot0.primitive]
    assert tuple(spot0.position) == (0.0, 0.0, 0.0)
    assert sp.cos_falloff_end == pytest.approx(math.cos(math.radians(30.0)), abs=2 * U) and sp.cos_falloff_start == pytest.approx(math.cos(math.radians(25.0)), abs=2 * U)
    m = np.array(sp.render_from_light[:]).reshape(4, 4)
    assert np.allclose(m[:3, 2], (0, 0, 1), atol=2 * U) and np.allclose(m @ np.array(sp.light_from_render[:]).reshape(4, 4), np.eye(4), atol=8 * U)
    # under the CTM
    w = ctm[:3, :3] @ (np.array([1.0, 1.0, 4.0]) / np.linalg.norm([1.0, 1.0, 4.0]))
    assert np.allclose(np.array(dist1.position[:]), w / np.linalg.norm(w), atol=16 * U)
    bb = blackbody_dense(5500.0)
    assert np.allclose(table(dist1), bb, rtol=4 * U)
    assert dist1.scale == pytest.approx(2.0 / float(scn.spectrum_to_photometric(table(dist1))) * 700.0, rel=8 * U)
    sp = d.spot_lights[spot1.primitive]
    m, mi = np.array(sp.render_from_light[:], np.float64).reshape(4, 4), np.array(sp.light_from_render[:], np.float64).reshape(4, 4)
    assert np.allclose(np.array(spot1.position[:]), (ctm @ np.array([1.0, 2.0, 3.0, 1.0]))[:3], atol=32 * U) and np.allclose(m[:3, 3], spot1.position[:])
    axis = np.array([-1.0, -3.0, -2.0]) / np.linalg.norm([1.0, 3.0, 2.0])
    assert np.allclose(m[:3, 2], ctm[:3, :3] @ axis, atol=16 * U)
    lin = np.linalg.inv(ctm[:3, :3]) @ m[:3, :3]  # the frame itself: orthonormal, z = the axis
    assert np.allclose(lin.T @ lin, np.eye(3), atol=64 * U) and np.allclose(m @ mi, np.eye(4), atol=64 * U)
    cs, ce = math.cos(math.radians(28.0)), math.cos(math.radians(40.0))
    assert sp.cos_falloff_start == pytest.approx(cs, abs=2 * U) and sp.cos_falloff_end == pytest.approx(ce, abs=2 * U)
    k_e = 2 * math.pi * ((1 - cs) + (cs - ce) / 2)
    photometric = float(scn.spectrum_to_photometric(table(spot1)))
    assert spot1.scale == pytest.approx(3.0 / photometric * 900.0 / k_e, rel=32 * U)

    # the power, back from the light itself: Phi_v = photometric * scale * 2 pi Int smoothstep dcos, the integral as a midpoint rule over the lights' own sample_li
    # (apex at distance 1 from the origin of render space: L = I). The ramp is a cubic in cos: the midpoint rule's error is below width^3 / (24 n^2) * max|s''| = 6 / width^2.
    n = 256
    b = scn.SceneBuilder()
    b.set_film(4, 4)
    b.set_camera_look_at(lib, (0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0)
    p, vi = _quad((-4, -2, -4), (-4, -2, 4), (4, -2, 4), (4, -2, -4))
    b.add_mesh(p, vi, b.material_diffuse(0.5))
    dense = table(spot1)
    cosines = ce + (np.arange(n) + 0.5) / n * (1.0 - ce)
    for c in cosines:  # the origin seen from the apex at the angle acos(c) off the axis (0, -1, 0)
        s = math.sqrt(1 - c * c)
        apex = np.array([-s, c, 0.0])
        b.light_spot(apex, apex + (0.0, -1.0, 0.0), dense, scale=3.0, coneangle=40.0, conedelta=12.0, power=900.0)
    desc, _ = b.build(lib)
    assert desc.lights[0].scale == pytest.approx(spot1.scale, rel=8 * U)  # the builder's formula == the loader's
    o = oracle_py.Oracle(desc)
    o.lib.orc_fn_light_sample_li.restype, o.lib.orc_fn_light_sample_li.argtypes = C.c_int, [C.c_void_p, C.c_uint32, FP, C.c_int, FP, FP]
    total = 0.0
    for i in range(n):
        ok, outv = sample_li(o, i)
        total += outv[4 + 1] if ok else 0.0
    o.close()
    intensity_integral = 2 * math.pi * total * (1.0 - ce) / n
    power_back = intensity_integral / float(dense[int(round(LAMBDA[1])) - 360]) * photometric
    print(f"power from the quadrature of I(w): {power_back:.4f} lm (3 x 900: PBRT-v4 multiplies \"scale\" on top of \"power\")")
    assert power_back == pytest.approx(3.0 * 900.0, rel=1e-4)
    lib.shm_pbrt_free(out)


def test_loader_rejects_the_lights_it_does_not_have_with_file_and_line(lib, tmp_path):
    for kind in ("goniometric", "projection"):
        rc, out = load(lib, tmp_path, HEAD + f'\nLightSource "{kind}"\n', name=f"{kind}.pbrt")
        msg = lib.shm_last_error().decode()
        assert rc == ERR_UNSUPPORTED and not out
        assert f"{kind}.pbrt:7" in msg and "(point, spot, distant, infinite)" in msg, msg
    rc, out = load(lib, tmp_path, HEAD + 'LightSource "spot" "float coneangle" 190 "float conedelta" 5\n', name="cone.pbrt")
    assert rc == ERR_INVALID_ARGUMENT and "cone.pbrt:6" in lib.shm_last_error().decode()


def test_scene_file_round_trip_equals_the_builder(lib, tmp_path):
    text = HEAD + ('LightSource "distant" "point3 from" [ 1 3 2 ] "point3 to" [ 0 0 0 ] "blackbody L" 5000 "float scale" 2\n'
                   'LightSource "spot" "point3 from" [ 0.5 2 1 ] "point3 to" [ 0 -1 0 ] "blackbody I" 3000 "float scale" 4 "float coneangle" 35 "float conedelta" 10\n')
    rc, out = load(lib, tmp_path, text)
    assert rc == 0, lib.shm_last_error().decode()
    d = out.contents.desc
    b = scn.SceneBuilder()
    b.light_distant(blackbody_dense(5000.0), scale=2.0, frm=(1, 3, 2), to=(0, 0, 0))
    b.light_spot((0.5, 2, 1), (0, -1, 0), blackbody_dense(3000.0), scale=4.0, coneangle=35.0, conedelta=10.0)
    for i in range(2):
        got, want = d.lights[i], b.lights[i]
        assert (got.kind, got.primitive, got.two_sided, got.area) == (want.kind, want.primitive, want.two_sided, want.area)
        assert tuple(got.position) == tuple(want.position)
        assert got.scale == pytest.approx(want.scale, rel=2 * U)  # (the two photometric sums run over tables that may differ in the last bit)
    got, want = d.spot_lights[0], b.spot_lights[0]
    assert tuple(got.render_from_light) == tuple(want.render_from_light) and tuple(got.light_from_render) == tuple(want.light_from_render)
    # (cosf against the float64 cosine rounded once: within one unit in the last place)
    assert got.cos_falloff_start == pytest.approx(want.cos_falloff_start, abs=2 * U) and got.cos_falloff_end == pytest.approx(want.cos_falloff_end, abs=2 * U)
    lib.shm_pbrt_free(out)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_header_agrees_with_abi_py_on_the_new_lights(tmp_path):
    assert abi.SHM_ABI_VERSION == 10 and C.sizeof(abi.ShmLight) == 64 and (abi.SHM_LIGHT_DISTANT, abi.SHM_LIGHT_SPOT) == (4, 5)
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "shimmer_hip.h"\nint main(void) {\n'
           '  printf("%d %zu %zu %zu %zu %zu %zu %zu %d %d\\n", SHM_ABI_VERSION, sizeof(ShmLight), sizeof(ShmSpotLight), offsetof(ShmSpotLight, light_from_render),'
           ' offsetof(ShmSpotLight, cos_falloff_end), sizeof(ShmSceneDesc), offsetof(ShmSceneDesc, n_spot_lights), offsetof(ShmSceneDesc, spot_lights),'
           ' SHM_LIGHT_DISTANT, SHM_LIGHT_SPOT);\n  return 0;\n}\n')
    (tmp_path / "p.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "p.c"), "-o", str(tmp_path / "p")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "p")], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [10, 64, C.sizeof(abi.ShmSpotLight), abi.ShmSpotLight.light_from_render.offset, abi.ShmSpotLight.cos_falloff_end.offset, C.sizeof(abi.ShmSceneDesc),
                   abi.ShmSceneDesc.n_spot_lights.offset, abi.ShmSceneDesc.spot_lights.offset, 4, 5]
    assert C.sizeof(abi.ShmSpotLight) == 144 and abi.ShmSceneDesc.spot_lights.offset == C.sizeof(abi.ShmSceneDesc) - 8  # appended at the end


def test_flatten_scene_rejects_malformed_lights_with_a_message(lib):
    def attempt(mutate):
        b = scn.SceneBuilder()
        b.set_film(4, 4)
        b.set_camera_look_at(lib, (0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0)
        p, vi = _quad((-4, -1, -4), (-4, -1, 4), (4, -1, 4), (4, -1, -4))
        b.add_mesh(p, vi, b.material_diffuse(0.5))
        b.light_distant(blackbody_dense(5000.0), frm=(0, 1, 0), to=(0, 0, 0))
        b.light_spot((0, 2, 0), (0, 0, 0), blackbody_dense(5000.0))
        desc, _ = b.build(lib)
        mutate(b, desc)
        handle = C.c_void_p()
        rc = oracle_py.load().orc_scene_create(C.byref(desc), C.byref(handle))
        msg = oracle_py.load().orc_last_error().decode() if rc != 0 else ""
        if rc == 0:
            oracle_py.load().orc_scene_destroy(handle)
        return rc, msg

    assert attempt(lambda b, d: None)[0] == 0
    spots = lambda d: d.spot_lights  # noqa: E731

    def set_dir(v):
        def f(b, d):
            d.lights[0].position[:] = v
        return f

    def set_spot(**kw):
        def f(b, d):
            for k, v in kw.items():
                if k == "m":
                    spots(d)[0].light_from_render[5] = v
                else:
                    setattr(spots(d)[0], k, v)
        return f

    def set_light(i, **kw):
        def f(b, d):
            for k, v in kw.items():
                setattr(d.lights[i], k, v)
        return f
    for mutate, word in ((set_dir((0.0, 2.0, 0.0)), "unit vector"), (set_dir((0.0, float("nan"), 0.0)), "not finite"), (set_dir((0.0, 0.0, 0.0)), "unit vector"),
                         (set_light(1, primitive=1), "spot light index out of range"), (set_spot(cos_falloff_start=0.5, cos_falloff_end=0.8), "cos_falloff_end <= cos_falloff_start"),
                         (set_spot(cos_falloff_start=1.5), "cos_falloff_end <= cos_falloff_start"), (set_spot(cos_falloff_end=-1.5), "cos_falloff_end <= cos_falloff_start"),
                         (set_spot(cos_falloff_end=float("nan")), "cos_falloff_end <= cos_falloff_start"), (set_spot(m=float("inf")), "transform is not finite"),
                         (set_light(1, scale=float("inf")), "scale is not finite")):
        rc, msg = attempt(mutate)
        assert rc == ERR_INVALID_ARGUMENT and word in msg, (rc, msg, word)
    # a spectrum that is not densely sampled, as for the other lights
    def constant_spectrum(b, d):
        d.lights[1].spectrum.kind = abi.SHM_SPECTRUM_CONSTANT
    rc, msg = attempt(constant_spectrum)
    assert rc == ERR_INVALID_ARGUMENT and "densely sampled" in msg
    rc, msg = attempt(set_light(0, kind=6))
    assert rc == ERR_UNSUPPORTED and "unsupported light kind" in msg
