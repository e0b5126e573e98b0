"""PBRT-v4's disk and cylinder (ShmSphere.quadric = SHM_QUADRIC_DISK / SHM_QUADRIC_CYLINDER; shm/shapes.h, quadric_*) on the CPU oracle: the leaves against a float64
restatement (tests/quadric_cases.py), the densities against the solid angle they integrate to, direct lighting by a disk emitter in absolute terms, the PBRT front
end, flatten_scene's rejections, the ABI, and the films of scenes without such a shape as the parent commit rendered them.

Tolerances of the leaf comparisons are those of tests/test_leaf_golden.py::test_sphere_sample_and_pdf_with_context for the same quantities of the sphere — a point (and
here a distance along the ray, an object-space point, an angle): 2e-5 * max(1, |value|) absolute; a unit normal's component: 2e-5 absolute; a density: 2e-4 relative."""
import ctypes as C
import json
import math
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_py
import quadric_cases as qc
from shimmer_amd import abi, render, scene as scn, scenes
from shimmer_amd.scenes import _quad, _to_render, blackbody_dense

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests" / "golden"))
F, FP = C.c_float, C.POINTER(C.c_float)
ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -2  # (include/shimmer_hip.h)
P_ATOL, N_ATOL, PDF_RTOL = 2e-5, 2e-5, 2e-4    # (tests/test_leaf_golden.py::test_sphere_sample_and_pdf_with_context)


def fa(v):
    v = np.asarray(v, np.float32).ravel()
    return (F * len(v))(*[float(x) for x in v])


def near(got, want, atol):
    want = np.asarray(want, np.float64)
    return bool(np.all(np.abs(np.asarray(got, np.float64) - want) <= atol * max(1.0, float(np.max(np.abs(want))))))


def one_shape_scene(lib, rec):
    """A scene whose only primitive is the record (render space = world space: the camera sits at the origin)."""
    b = scn.SceneBuilder()
    b.set_film(4, 4)
    b.set_camera_look_at(lib, (0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0)
    b.add_disk(1.0, b.material_diffuse(0.5))
    b.spheres[0] = rec
    desc, _ = b.build(lib)
    return b, desc


def oracle_hit(o, ro, rd, t_max):
    ray = abi.ShmRay()
    ray.o[:], ray.d[:], ray.t_max = [float(x) for x in ro], [float(x) for x in rd], t_max
    out, hit = (F * 12)(), abi.ShmHit()
    if o.lib.orc_fn_hit_interaction(o.handle, C.byref(ray), out, C.byref(hit)) != 1:
        return None
    return dict(t=hit.t, p_obj=(hit.b0, hit.b1, hit.b2), phi=hit.phi, p=list(out[0:3]), n=list(out[3:6]), ns=list(out[6:9]), dpdu=list(out[9:12]))


@pytest.fixture(scope="module")
def olib():
    lib = oracle_py.load()
    lib.orc_fn_sphere_sample_with_context.restype = C.c_int
    lib.orc_fn_sphere_sample_with_context.argtypes = [C.POINTER(abi.ShmSphere), FP, FP, FP, FP, FP]
    lib.orc_fn_sphere_pdf_with_context.restype, lib.orc_fn_sphere_pdf_with_context.argtypes = F, [C.POINTER(abi.ShmSphere), FP, FP, FP, FP]
    return lib


# ---- leaves ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(qc.HIT_CASES))
def test_intersection_and_interaction_against_float64(lib, name):
    rec, ro, rd, t_max, expect_hit = qc.HIT_CASES[name]
    want = qc.intersect(rec, ro, rd, t_max)
    assert (want is not None) == expect_hit  # (the restatement itself agrees with what the case is named for)
    b, desc = one_shape_scene(lib, rec)
    o = oracle_py.Oracle(desc)
    try:
        got = oracle_hit(o, ro, rd, t_max)
        occ, _ = o.trace(np.array([[*ro, *rd, t_max, 0]], np.float32), any_hit=True)
    finally:
        o.close()
    assert (got is not None) == expect_hit and bool(occ[0]) == expect_hit, (name, got)
    if not expect_hit:
        return
    t, p_obj, phi = want
    it = qc.interaction(rec, p_obj, phi)
    assert near(got["t"], t, P_ATOL) and near(got["p_obj"], p_obj, P_ATOL) and near(got["phi"], phi, P_ATOL), (name, got, want)
    assert near(got["p"], it["p"], P_ATOL), (name, got["p"], it["p"])
    assert np.all(np.abs(np.array(got["n"]) - it["n"]) <= N_ATOL) and np.all(np.abs(np.array(got["ns"]) - it["n"]) <= N_ATOL), (name, got["n"], it["n"])
    assert near(got["dpdu"], it["dpdu"], P_ATOL), (name, got["dpdu"], it["dpdu"])


def test_the_quadric_byte_is_read(lib):
    """The same records with quadric = 0 are spheres: a film with the shapes differs from the film a build without them would render (a test that fails on the parent,
    where the byte is padding)."""
    films = []
    for as_spheres in (False, True):
        sc = scenes.quadric_scene(lib, "lean", 24, 20, as_spheres=as_spheres)
        o = oracle_py.Oracle(sc.desc)
        film, _ = o.render(render.make_params(seed=3, spp=2, max_depth=3), n_threads=8)
        o.close()
        films.append(render.film_to_rgb(film))
    assert np.isfinite(films[0]).all() and films[0].max() > 0
    assert not np.array_equal(films[0], films[1])
    assert np.mean(np.any(films[0] != films[1], axis=-1)) > 0.25  # (not a pixel or two: the scene is made of these shapes)


# ---- densities ---------------------------------------------------------------------------------------------------------------------------
def draw(olib, rec, ctx_p, u):
    out = (F * 7)()
    zero = fa([0.0, 0.0, 0.0])
    if olib.orc_fn_sphere_sample_with_context(C.byref(rec), fa(ctx_p), zero, zero, fa(u), out) != 1:
        return None
    return np.array(out[0:3], np.float64), np.array(out[3:6], np.float64), float(out[6])


@pytest.mark.parametrize("name", list(qc.SAMPLE_CASES))
def test_samples_against_float64_and_pdf_of_a_drawn_sample(olib, name):
    """sample_with_context against the restatement, and pdf_with_context(wi) of a drawn direction equals the sample's density — for every sample that is the first
    thing its direction meets (a cylinder seen from outside also draws points of its far side, which the ray towards them finds behind the near one)."""
    rec, ctx_p = qc.SAMPLE_CASES[name]
    rng = np.random.Generator(np.random.PCG64(17))
    zero = fa([0.0, 0.0, 0.0])
    checked = 0
    for u in rng.random((128, 2)):
        got, want = draw(olib, rec, ctx_p, u), qc.sample_with_context(rec, ctx_p, u)
        assert (got is None) == (want is None)
        if got is None:
            continue
        assert near(got[0], want[0], P_ATOL) and np.all(np.abs(got[1] - want[1]) <= N_ATOL), (name, u, got, want)
        assert abs(got[2] - want[2]) <= PDF_RTOL * want[2], (name, u, got[2], want[2])
        wi = got[0] - np.asarray(ctx_p, np.float64)
        dist = np.linalg.norm(wi)
        wi /= dist
        first = qc.intersect(rec, ctx_p, wi)
        if first is None or abs(first[0] - dist) > 1e-3 * dist or abs(float(got[1] @ wi)) < 0.05:  # (not the first hit; or grazing, where the hit point's rounding moves the cosine)
            continue
        pdf = olib.orc_fn_sphere_pdf_with_context(C.byref(rec), fa(ctx_p), zero, zero, fa(wi))
        assert abs(pdf - got[2]) <= PDF_RTOL * got[2], (name, u, pdf, got[2])
        assert abs(pdf - qc.pdf_with_context(rec, ctx_p, wi)) <= PDF_RTOL * pdf
        checked += 1
    assert checked >= 24, checked
    assert olib.orc_fn_sphere_pdf_with_context(C.byref(rec), fa(ctx_p), zero, zero, fa(-wi)) == 0.0 or name.endswith("inside")  # away from the shape: no density


def cap(h, r):
    return 2.0 * math.pi * (1.0 - h / math.sqrt(h * h + r * r))


def quadrature(rec, ctx_p, n=1024):
    """Int |cos| / d^2 dA over the surface in float64 (midpoint rule over the area sample's own (u0, u1) square: the sample is uniform in area)."""
    c = (np.arange(n) + 0.5) / n
    total = 0.0
    for u0 in c[:: n // 256]:
        for u1 in c[:: n // 256]:
            s = qc.sample_with_context(rec, ctx_p, (u0, u1))
            total += 0.0 if s is None else 1.0 / s[2]
    return total / 256 ** 2


SOLID_ANGLES = {
    "disk on its axis": lambda rec, p: cap(p[2], 0.6),
    "annulus on its axis": lambda rec, p: cap(p[2], 0.6) - cap(p[2], 0.25),
    "sector on its axis": lambda rec, p: cap(p[2], 0.6) * rec.phi_max / (2.0 * math.pi),
    "cylinder from outside": quadrature,
    "cylinder sector from inside": quadrature,
}


@pytest.mark.parametrize("name", list(SOLID_ANGLES))
def test_mean_of_one_over_pdf_is_the_solid_angle(olib, name):
    """E[1 / pdf] over the area samples = Int |cos| / d^2 dA: the solid angle the shape subtends (counted once per sheet a direction crosses: twice for the cylinder seen
    from outside, which the quadrature counts the same way). Rigid placements only: PBRT-v4's area density 1 / area is the object-space one.
    Criterion: within 4 standard errors of the test's own sample mean, the sample count chosen so that the standard error is below 1 % of the value."""
    rec, ctx_p = qc.SAMPLE_CASES[name]
    want = SOLID_ANGLES[name](rec, ctx_p)
    rng = np.random.Generator(np.random.PCG64(23))
    n = 8192
    vals = np.zeros(n)
    for i, u in enumerate(rng.random((n, 2))):
        s = draw(olib, rec, ctx_p, u)
        vals[i] = 0.0 if s is None else 1.0 / s[2]
    mean, se = vals.mean(), vals.std(ddof=1) / math.sqrt(n)
    print(f"{name}: solid angle {want:.6f}, mean of 1/pdf {mean:.6f}, standard error {se:.2e} ({100 * se / want:.3f} % of the value), off by {abs(mean - want) / se:.2f} SE")
    assert se < 0.01 * want
    assert abs(mean - want) <= 4 * se


# ---- direct lighting ---------------------------------------------------------------------------------------------------------------------
def test_direct_lighting_by_a_disk_emitter_is_the_radiometric_integral(lib):
    """A one-sided Lambertian disk emitter of radius r at height h, parallel to a diffuse floor of reflectance R: the floor point on its axis receives the irradiance
    E = pi L r^2 / (h^2 + r^2) and shows L_o = R / pi * E. As tests/test_direct_lighting_analytic.py: maxdepth 1, L in film units from a render that looks into the same
    emission, the same criterion (the mean within 1 %) — with the standard error of that mean measured and held below a quarter of the criterion. The view is 0.5 degrees
    wide: its footprint on the floor stays within 0.07 of the axis, where the irradiance is within 2 rho^2 / h^2 = 0.25 % of the axis value."""
    R, H, RAD, W = 0.5, 2.0, 0.5, 8
    em = dict(emission=blackbody_dense(6500.0), emission_scale=5.0)
    b = scn.SceneBuilder()
    b.set_film(W, W)
    rfw = np.asarray(b.set_camera_look_at(lib, (0.0, 1.2, 4.0), (0.0, 0.0, 0.0), (0, 1, 0), 0.5), np.float32).reshape(4, 4)
    p, vi = _quad((-40, 0, -40), (-40, 0, 40), (40, 0, 40), (40, 0, -40))
    b.add_mesh(_to_render(p, rfw), vi, b.material_diffuse(R))
    down = np.array([[1, 0, 0, 0], [0, 0, -1, H], [0, 1, 0, 0], [0, 0, 0, 1]], np.float32)  # the disk's +z is the world's -y, its centre at height H
    b.add_disk(RAD, b.material_diffuse(0.0), render_from_object=(rfw @ down).astype(np.float32), **em)
    desc, _ = b.build(lib)
    o = oracle_py.Oracle(desc)
    film, _ = o.render(render.make_params(seed=4, spp=768, max_depth=1), n_threads=8)
    o.close()
    rgb = render.film_to_rgb(film).reshape(-1, 3)
    # calibration: a wall of the same emission filling the view
    c = scn.SceneBuilder()
    c.set_film(8, 8)
    crfw = c.set_camera_look_at(lib, (0, 0, 0), (0, 0, -1), (0, 1, 0), 30.0)
    p, vi = _quad((-50, -50, -1), (50, -50, -1), (50, 50, -1), (-50, 50, -1))
    c.add_mesh(_to_render(p, crfw), vi, c.material_diffuse(0.0), **em)
    cdesc, _ = c.build(lib)
    o = oracle_py.Oracle(cdesc)
    cfilm, _ = o.render(render.make_params(seed=1, spp=64, max_depth=0), n_threads=4)
    o.close()
    le = render.film_to_rgb(cfilm).reshape(-1, 3).mean(axis=0)
    assert np.all(le > 0)
    want = R * RAD ** 2 / (H ** 2 + RAD ** 2)
    ratios = (rgb / le / want).mean(axis=1)  # per pixel, the three channels averaged
    mean, se = float(ratios.mean()), float(ratios.std(ddof=1) / math.sqrt(len(ratios)))
    print(f"disk emitter: floor radiance / (R L r^2 / (h^2 + r^2)) = {mean:.5f}, standard error {se:.5f}")
    assert se < 0.0025
    assert abs(mean - 1.0) < 0.01


def test_quirks_switch_changes_nothing_for_these_shapes(lib):
    """There is no reference behaviour to keep for a disk or a cylinder: a scene made of them (and of triangles that emit nothing) renders the same film with
    ShmRenderParams::disable_reference_quirks 0 and 1."""
    sc = scenes.quadric_scene(lib, "lean", 24, 20)
    o = oracle_py.Oracle(sc.desc)
    a, sa = o.render(render.make_params(seed=9, spp=4, max_depth=4, reference_quirks=True), n_threads=8)
    b, sb = o.render(render.make_params(seed=9, spp=4, max_depth=4, reference_quirks=False), n_threads=8)
    o.close()
    assert np.array_equal(a, b) and all(sa[k] == sb[k] for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"))


# ---- the PBRT front end ------------------------------------------------------------------------------------------------------------------
HEAD = ('LookAt 0 0 0  0 0 -1  0 1 0\nCamera "perspective" "float fov" 40\nFilm "rgb" "integer xresolution" 8 "integer yresolution" 8\n'
        'WorldBegin\nShape "trianglemesh" "point3 P" [ -4 -1 -4  -4 -1 4  4 -1 4  4 -1 -4 ] "integer indices" [ 0 1 2 0 2 3 ]\n')
FIELDS = ("radius", "z_min", "z_max", "theta_z_min", "theta_z_max", "phi_max", "reverse_orientation", "transform_swaps_handedness", "quadric")


def load(lib, tmp_path, text, name="s.pbrt"):
    (tmp_path / name).write_text(text)
    out = C.POINTER(abi.ShmPbrtScene)()
    rc = lib.shm_scene_load_pbrt(str(tmp_path / name).encode(), C.byref(out))
    return rc, out


def same_record(got, want):
    for f in FIELDS:
        assert getattr(got, f) == getattr(want, f), (f, getattr(got, f), getattr(want, f))
    assert tuple(got.render_from_object) == tuple(want.render_from_object) and tuple(got.object_from_render) == tuple(want.object_from_render)
    assert bytes(got.pad) == bytes(5)


def test_loader_equals_the_builder_field_by_field(lib, tmp_path):
    text = HEAD + ('Shape "disk"\nShape "cylinder"\n'
                   'AttributeBegin\nTranslate 0.5 -0.25 -3\nScale 2 2 -2\n'
                   'Shape "disk" "float height" 0.25 "float radius" 0.75 "float innerradius" 0.125 "float phimax" 270\n'
                   'ReverseOrientation\nShape "cylinder" "float radius" 0.5 "float zmin" 1.5 "float zmax" -0.5 "float phimax" 400\n'
                   'AttributeEnd\n'
                   'AttributeBegin\nTranslate 0 2 -3\nAreaLightSource "diffuse" "blackbody L" 5000 "float scale" 2\n'
                   'Shape "disk" "float radius" 0.5 "float innerradius" 0.25 "float phimax" 180\nShape "cylinder" "float radius" 0.25 "float zmin" 0 "float zmax" 0.5\nAttributeEnd\n')
    rc, out = load(lib, tmp_path, text)
    assert rc == 0, lib.shm_last_error().decode()
    d = out.contents.desc
    b = scn.SceneBuilder()
    m = b.material_diffuse(0.5)
    b.add_disk(1.0, m)           # PBRT-v4's defaults: height 0, radius 1, innerradius 0, phimax 360
    b.add_cylinder(1.0, m)       # radius 1, zmin -1, zmax 1, phimax 360
    ctm = np.diag([2.0, 2.0, -2.0, 1.0])
    ctm[:3, 3] = (0.5, -0.25, -3.0)
    b.add_disk(0.75, m, height=0.25, inner_radius=0.125, phi_max=270.0, render_from_object=ctm)
    b.add_cylinder(0.5, m, z_min=1.5, z_max=-0.5, phi_max=400.0, render_from_object=ctm, reverse_orientation=True)  # zmin / zmax ordered, phimax clamped to 360
    up = np.eye(4)
    up[:3, 3] = (0.0, 2.0, -3.0)
    em = dict(emission=blackbody_dense(5000.0), emission_scale=2.0)
    b.add_disk(0.5, m, inner_radius=0.25, phi_max=180.0, render_from_object=up, **em)
    b.add_cylinder(0.25, m, z_min=0.0, z_max=0.5, render_from_object=up, **em)
    assert d.n_spheres == 6 and len(b.spheres) == 6
    for i in range(6):
        same_record(d.spheres[i], b.spheres[i])
    dflt_disk, dflt_cyl, _, clamped = (d.spheres[i] for i in range(4))
    assert (dflt_disk.quadric, dflt_disk.radius, dflt_disk.z_min, dflt_disk.z_max, dflt_disk.theta_z_min) == (abi.SHM_QUADRIC_DISK, 1.0, 0.0, 0.0, 0.0)
    assert (dflt_cyl.quadric, dflt_cyl.radius, dflt_cyl.z_min, dflt_cyl.z_max) == (abi.SHM_QUADRIC_CYLINDER, 1.0, -1.0, 1.0)
    assert dflt_disk.phi_max == dflt_cyl.phi_max == clamped.phi_max == float(np.float32(np.pi / 180.0) * np.float32(360.0))
    assert (clamped.z_min, clamped.z_max, clamped.reverse_orientation, clamped.transform_swaps_handedness) == (-0.5, 1.5, 1, 1)
    # every one of them is a SHM_SHAPE_SPHERE primitive; the two emitters are diffuse area lights with the shapes' areas
    prims = [d.primitives[i] for i in range(d.n_primitives)]
    assert sorted(p.shape_index for p in prims if p.shape_kind == abi.SHM_SHAPE_SPHERE) == list(range(6))
    lights = {p.shape_index: d.lights[p.area_light] for p in prims if p.shape_kind == abi.SHM_SHAPE_SPHERE and p.area_light >= 0}
    assert sorted(lights) == [4, 5] and all(l.kind == abi.SHM_LIGHT_DIFFUSE_AREA for l in lights.values())
    want = {4: b.lights[0], 5: b.lights[1]}
    for k in (4, 5):
        assert lights[k].area == want[k].area and lights[k].two_sided == want[k].two_sided
        assert lights[k].scale == pytest.approx(want[k].scale, rel=2 * 2.0 ** -24)
    assert lights[4].area == pytest.approx(math.pi * (0.25 - 0.0625) / 2.0, rel=1e-6) and lights[5].area == pytest.approx(0.5 * 0.25 * 2 * math.pi, rel=1e-6)
    # the loaded scene renders
    o = oracle_py.Oracle(d)
    film, _ = o.render(render.make_params(seed=1, spp=1, max_depth=2), n_threads=4)
    o.close()
    assert np.isfinite(film["rgb_sum"]).all()
    lib.shm_pbrt_free(out)


def test_loader_still_rejects_the_shapes_it_does_not_have(lib, tmp_path):
    rc, out = load(lib, tmp_path, HEAD + '\nShape "curve"\n', name="curve.pbrt")
    msg = lib.shm_last_error().decode()
    assert rc == ERR_UNSUPPORTED and not out
    assert "curve.pbrt:7" in msg and "not supported" in msg and "(sphere, disk, cylinder, trianglemesh, bilinearmesh, plymesh)" in msg, msg


def test_example_scene_loads(lib):
    out = C.POINTER(abi.ShmPbrtScene)()
    rc = lib.shm_scene_load_pbrt(str(ROOT / "examples" / "scenes" / "disk_and_cylinder.pbrt").encode(), C.byref(out))
    assert rc == 0, lib.shm_last_error().decode()
    d = out.contents.desc
    kinds = sorted(d.spheres[i].quadric for i in range(d.n_spheres))
    assert abi.SHM_QUADRIC_DISK in kinds and abi.SHM_QUADRIC_CYLINDER in kinds
    lib.shm_pbrt_free(out)


# ---- flatten_scene -----------------------------------------------------------------------------------------------------------------------
def test_flatten_scene_rejects_malformed_records_with_a_message(lib):
    orc = oracle_py.load()

    def attempt(kind, **kw):
        rec = qc.record(kind, 0.5, -0.5, 0.5) if kind == "cylinder" else qc.record("disk", 0.5, 0.25, inner=0.1)
        b, desc = one_shape_scene(lib, rec)
        for k, v in kw.items():
            if k == "m":
                desc.spheres[0].object_from_render[5] = v
            else:
                setattr(desc.spheres[0], k, v)
        handle = C.c_void_p()
        rc = orc.orc_scene_create(C.byref(desc), C.byref(handle))
        msg = orc.orc_last_error().decode() if rc != 0 else ""
        if rc == 0:
            orc.orc_scene_destroy(handle)
        return rc, msg

    assert attempt("disk")[0] == 0 and attempt("cylinder")[0] == 0
    assert attempt("disk", phi_max=float(np.float32(2 * np.pi)))[0] == 0  # (2 pi itself, as the builders round it, is inside)
    rc, msg = attempt("disk", quadric=3)
    assert rc == ERR_UNSUPPORTED and "unsupported quadric kind" in msg, (rc, msg)
    for kind, kw, word in (("disk", dict(radius=float("nan")), "not finite"), ("cylinder", dict(z_max=float("inf")), "not finite"), ("disk", dict(m=float("nan")), "not finite"),
                           ("disk", dict(radius=0.0), "radius must be positive"), ("disk", dict(radius=-1.0), "radius must be positive"),
                           ("disk", dict(theta_z_min=-0.1), "inner radius"), ("disk", dict(theta_z_min=0.5), "inner radius"), ("disk", dict(theta_z_min=0.75), "inner radius"),
                           ("cylinder", dict(radius=0.0), "radius must be positive"), ("cylinder", dict(z_min=0.5), "z_min < z_max"), ("cylinder", dict(z_min=0.75), "z_min < z_max"),
                           ("disk", dict(phi_max=0.0), "phi_max"), ("disk", dict(phi_max=-1.0), "phi_max"), ("cylinder", dict(phi_max=6.5), "phi_max"),
                           ("cylinder", dict(phi_max=float("nan")), "not finite")):
        rc, msg = attempt(kind, **kw)
        assert rc == ERR_INVALID_ARGUMENT and word in msg and kind in msg, (kind, kw, rc, msg)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_header_agrees_with_abi_py_on_the_record(tmp_path):
    assert abi.SHM_ABI_VERSION == 10 and C.sizeof(abi.ShmSphere) == 160 and abi.ShmSphere.quadric.offset == 154 and C.sizeof(abi.ShmSceneDesc) == 640
    assert (abi.SHM_QUADRIC_SPHERE, abi.SHM_QUADRIC_DISK, abi.SHM_QUADRIC_CYLINDER) == (0, 1, 2)
    assert abi.ShmSphere().quadric == 0  # a zeroed record is a sphere
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "shimmer_hip.h"\nint main(void) {\n'
           '  printf("%d %zu %zu %zu %zu %zu %zu %d %d %d %d\\n", SHM_ABI_VERSION, sizeof(ShmSphere), offsetof(ShmSphere, quadric), offsetof(ShmSphere, pad),'
           ' offsetof(ShmSphere, reverse_orientation), offsetof(ShmSphere, phi_max), sizeof(ShmSceneDesc), SHM_QUADRIC_SPHERE, SHM_QUADRIC_DISK, SHM_QUADRIC_CYLINDER,'
           ' SHM_SHAPE_SPHERE);\n  return 0;\n}\n')
    (tmp_path / "p.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "p.c"), "-o", str(tmp_path / "p")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "p")], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [10, 160, abi.ShmSphere.quadric.offset, abi.ShmSphere.pad.offset, abi.ShmSphere.reverse_orientation.offset, abi.ShmSphere.phi_max.offset, 640, 0, 1, 2,
                   abi.SHM_SHAPE_SPHERE]


# ---- before and after --------------------------------------------------------------------------------------------------------------------
def test_scenes_without_the_shapes_render_what_the_parent_commit_rendered(lib):
    """tests/golden/quadrics_before.json (gen_quadrics_before.py, run on the parent commit): the oracle's films and counters of three_spheres, instanced_scene and the
    Cornell box as patches under both samplers — every sphere record of theirs has quadric = 0, and the sphere's functions return what they returned."""
    import gen_quadrics_before as gen
    before = json.loads((ROOT / "tests" / "golden" / "quadrics_before.json").read_text())
    assert len(before["films"]) == len(gen.CASES) == 6
    for rec in before["films"]:
        case = {k: rec[k] for k in ("scene", "sampler", "seed", "spp", "max_depth")}
        assert case in gen.CASES
        film, st = gen.film_of(lib, case)
        assert gen.film_sha256(film) == rec["sha256"], case
        assert [int(st[k]) for k in gen.STATS] == rec["stats"], case


def test_plan_takes_the_extended_kernels_for_exactly_the_scenes_with_the_shapes(lib):
    """scene_facts ORs has_quadric_kinds into `extended` (column 6 of orc_fn_scene_facts): the *_dl shading kernels, which know the shapes — and no scene without one
    reaches a kernel it did not reach before."""
    for sc, want in ((scenes.quadric_scene(lib, "lean", 8, 8), 1), (scenes.quadric_scene(lib, "lean", 8, 8, as_spheres=True), 0), (scenes.three_spheres(lib, 8, 8), 0)):
        o = oracle_py.Oracle(sc.desc)
        facts = o.scene_facts()
        o.close()
        assert facts["extended"] == want and facts["has_spheres"] == 1
