"""The G-buffer pass's CPU twin (shm_gbuffer_camera_rays / shm_gbuffer_samples_host / shm_gbuffer_rho_host, host/host_mirror.cpp over shm/gbuffer.h) and its host
helpers, without a GPU: twin rays -> the oracle's closest hits -> the twin's per-sample records. DESIGN.md section 4i is the definition the checks restate."""
import ctypes as C
import hashlib
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gbuffer_cases as gc
import oracle_py
from shimmer_amd import abi, render, scenes
from shimmer_amd.scene import SceneBuilder

ROOT = Path(__file__).resolve().parents[1]
EPS = 2.0 ** -24
F32 = np.float32

# BSDF::rho_hd's fixed points, as the definition writes them
REV4 = [int(format(i, "04b")[::-1], 2) for i in range(16)]
U2 = [(F32((i + 0.5) / 16), F32((REV4[i] + 0.5) / 16)) for i in range(16)]
UC = [F32((((5 * i) % 16) + 0.5) / 16) for i in range(16)]


class Chain:
    """One scene through the chain, every sample of the film: rays, the oracle's hits, the twin's records in render space."""

    def __init__(self, lib, sc, params, space=abi.SHM_GBUFFER_SPACE_RENDER):
        self.lib, self.sc, self.desc, self.params = lib, sc, sc.desc, params
        pb = tuple(sc.desc.film.pixel_bounds)
        self.n_pixels = (pb[2] - pb[0]) * (pb[3] - pb[1])
        self.pix, self.idx = gc.all_samples(pb, params.samples_per_pixel)
        self.rays = gc.twin_rays(lib, self.desc, params, self.pix, self.idx)
        self.orc = oracle_py.Oracle(self.desc)
        self.hits, _ = self.orc.trace(self.rays)
        self.samples = self.records(space)
        self.hit = self.hits["prim"] >= 0
        self.wo = -self.rays[:, 3:6].astype(np.float64)

    def records(self, space):
        return gc.twin_samples(self.lib, self.desc, self.params, space, self.pix, self.idx, self.hits)

    def rho(self):
        return gc.twin_rho(self.lib, self.desc, self.params, self.pix, self.idx, self.hits)


@pytest.fixture(scope="module")
def cornell(lib):
    return Chain(lib, gc.make_scene(lib, "cornell"), gc.params_for())


def _plane(lib, material, reverse=False, w=gc.W, h=gc.H):
    """A 4 x 4 quad in the plane z = 0 of render space's axes, seen from (0.3, 0.2, 3): shading frames are the axes themselves."""
    b = SceneBuilder()
    b.set_film(w, h)
    rfw = b.set_camera_look_at(lib, (0.3, 0.2, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0)
    p, vi = scenes._quad((-2, -2, 0), (2, -2, 0), (2, 2, 0), (-2, 2, 0))
    if reverse:
        vi = vi[:, ::-1].copy()
    # (uv along the quad's edges: dpdu is render space's x axis, not the diagonal a triangle without uv gets)
    b.add_mesh(scenes._to_render(p, rfw), vi, material(b), uv=np.array([(0, 0), (1, 0), (1, 1), (0, 1)], F32))
    return scenes._finish(b, lib)


def _leaf_kinds(desc, material):
    """The material kinds a hit on `material` can resolve to: a MixMaterial's leaves."""
    m = desc.materials[material]
    if m.kind != abi.SHM_MATERIAL_MIX:
        return {m.kind}
    return _leaf_kinds(desc, m.mix_material[0]) | _leaf_kinds(desc, m.mix_material[1])


def _room(lib, reflectance, n=32):
    """The camera inside a closed box of one DiffuseMaterial: every ray hits it."""
    b = SceneBuilder()
    b.set_film(n, n)
    rfw = b.set_camera_look_at(lib, (0.1, 0.2, 0.5), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 70.0)
    p, vi = scenes._box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    b.add_mesh(scenes._to_render(p, rfw), vi, b.material_diffuse(reflectance))
    return scenes._finish(b, lib)


def _sensor(desc):
    f = desc.film
    return [np.ctypeslib.as_array(t, shape=(471,)).astype(F32) for t in (f.sensor_r_bar, f.sensor_g_bar, f.sensor_b_bar)]


def _sensor_weighting(desc, rho, lam, pdf):
    """a_c of one sample at unit exposure, in float32 as the pass computes it: average(table_c[round(lambda) - 360] * safe_div(rho, pdf))."""
    r = np.array([rho[i] / pdf[i] if pdf[i] != 0 else F32(0) for i in range(4)], F32)
    out = []
    for table in _sensor(desc):
        s = F32(0)
        for i in range(4):
            off = int(np.floor(lam[i] + F32(0.5))) - 360
            t = table[off] if 0 <= off < 471 else F32(0)
            s = F32(s + F32(t * r[i]))
        out.append(F32(s / F32(4)))
    return np.array(out, F32)


# ---- camera rays ----
def test_camera_rays_are_the_oracles_independent_sampler(lib, cornell):
    c = cornell
    out = (C.c_float * 14)()
    for k in range(0, len(c.idx), 7):
        c.orc.lib.orc_fn_camera_ray(c.orc.handle, int(c.pix[k, 0]), int(c.pix[k, 1]), int(c.idx[k]), c.params.seed, out)
        assert np.array_equal(np.array(out[:6], F32).view(np.uint32), c.rays[k, :6].view(np.uint32)), k
    assert np.all(np.isinf(c.rays[:, 6])) and not c.rays[:, 7].any()


@pytest.mark.parametrize("kw", [dict(), dict(disable_pixel_jitter=True), dict(randomization="none")], ids=str)
def test_camera_rays_are_the_oracles_zsobol(lib, kw):
    sc = gc.make_scene(lib, "cornell", "gaussian")
    params = gc.params_for("zsobol", **kw)
    pix, idx = gc.all_samples(tuple(sc.desc.film.pixel_bounds), gc.SPP)
    rays = gc.twin_rays(lib, sc.desc, params, pix, idx)
    o = oracle_py.Oracle(sc.desc)
    try:
        for k in range(0, len(idx), 5):
            ref = o.camera_ray_zs(int(pix[k, 0]), int(pix[k, 1]), int(idx[k]), params.seed, gc.SPP, none=kw.get("randomization") == "none",
                                  disable_pixel_jitter=kw.get("disable_pixel_jitter", False))
            assert np.array_equal(ref["o"].view(np.uint32), rays[k, 0:3].view(np.uint32)) and np.array_equal(ref["d"].view(np.uint32), rays[k, 3:6].view(np.uint32)), k
    finally:
        o.close()


# ---- position, normals, uv ----
@pytest.mark.parametrize("scene", ["cornell", "textured"])
def test_position_and_uv_against_float64_interpolation(lib, scene, cornell):
    c = cornell if scene == "cornell" else Chain(lib, gc.make_scene(lib, scene), gc.params_for())
    assert c.hit.mean() > 0.5
    checked_uv_mesh = False
    for k in np.flatnonzero(c.hit)[::3]:
        h = c.hits[k]
        if c.desc.primitives[int(h["prim"])].shape_kind != abi.SHM_SHAPE_TRIANGLE or h["instance"]:
            continue
        pts, uv, _ = gc.triangle_of(c.desc, int(h["prim"]))
        b = np.array([h["b0"], h["b1"], h["b2"]], np.float64)
        want = b @ pts.astype(np.float64)
        # three products and two sums, each rounded once, with slack for the rounded weights
        assert np.abs(c.samples[k, 0:3] - want).max() <= 8 * EPS * np.abs(pts).max(), (k, c.samples[k, 0:3], want)
        tri_uv = uv.astype(np.float64) if uv is not None else np.array([[0, 0], [1, 0], [1, 1]], np.float64)  # (a mesh without uv: Triangle's own corners)
        checked_uv_mesh = checked_uv_mesh or uv is not None
        assert np.abs(c.samples[k, 9:11] - b @ tri_uv).max() <= 8 * EPS * max(1.0, np.abs(tri_uv).max()), (k, c.samples[k, 9:11], b @ tri_uv)
    assert checked_uv_mesh == (scene == "textured")


@pytest.mark.parametrize("scene", ["cornell", "textured", "coated"])
def test_normals_are_unit_and_face_the_ray(lib, scene, cornell):
    c = cornell if scene == "cornell" else Chain(lib, gc.make_scene(lib, scene), gc.params_for())
    s = c.samples[c.hit]
    wo = c.wo[c.hit]
    for name, cols in (("n", slice(3, 6)), ("ns", slice(6, 9))):
        v = s[:, cols]
        assert np.abs(np.linalg.norm(v, axis=1) - 1.0).max() <= 4 * EPS, name
        assert (np.einsum("ij,ij->i", v.astype(F32), wo.astype(F32)) >= 0).all(), name
    assert (s[:, 14] == 1.0).all() and (s[:, 15] == 1.0).all()  # box filter: weight 1, every sample a hit


def test_a_one_sided_quad_seen_from_behind_shows_the_negated_normal(lib):
    seen = []
    for reverse in (False, True):
        c = Chain(lib, _plane(lib, lambda b: b.material_diffuse(0.5), reverse=reverse), gc.params_for())
        k = int(np.flatnonzero(c.hit)[0])
        pts, _, mesh = gc.triangle_of(c.desc, int(c.hits[k]["prim"]))
        assert not mesh.reverse_orientation and not mesh.transform_swaps_handedness
        p = pts.astype(np.float64)
        stored = np.cross(p[0] - p[2], p[1] - p[2])
        stored /= np.linalg.norm(stored)
        behind = float(stored @ c.wo[k]) < 0
        seen.append(behind)
        want = -stored if behind else stored
        for kk in np.flatnonzero(c.hit)[::17]:
            assert np.abs(c.samples[kk, 3:6] - want).max() <= 4 * EPS
            assert c.samples[kk, 3:6] @ c.wo[kk] > 0
    assert sorted(seen) == [False, True], "one of the two windings must face away from the camera"


# ---- albedo ----
@pytest.mark.parametrize("R", [0.5, 0.75, 1.0])
def test_constant_diffuse_albedo(lib, R):
    c = Chain(lib, _room(lib, R, n=8), gc.params_for(spp=2))
    assert c.hit.all()
    rho = c.rho()
    # four roundings per term and a 16-term sum
    assert np.abs(rho[:, 0:4].astype(np.float64) - R).max() <= 32 * EPS * R
    for k in range(0, len(c.idx), 5):
        a = _sensor_weighting(c.desc, rho[k, 0:4], rho[k, 4:8], rho[k, 8:12])
        assert np.array_equal(a.astype(np.float64).view(np.uint64), c.samples[k, 11:14].view(np.uint64)), (k, a, c.samples[k, 11:14])


@pytest.mark.parametrize("R", [1.0, 0.5])
def test_albedo_normalisation(lib, R):
    """A room of reflectance R over 32 x 32 x 16 samples resolves to R per channel, within 5 standard errors (from the twin's own per-sample values)."""
    sc = _room(lib, R, n=32)
    c = Chain(lib, sc, gc.params_for(spp=16))
    assert c.hit.all()
    white = render.gbuffer_white(lib, sc.desc)
    g = gc.pixel_sums(c.samples, c.n_pixels, 16).view(render.GBUFFER_DTYPE).reshape(-1)
    img = render.gbuffer_resolve(lib, g, white)
    assert (img["coverage"] == 1.0).all()
    per_sample = c.samples[:, 11:14] / white
    se = per_sample.std(axis=0, ddof=1) / np.sqrt(len(per_sample))
    mean = img["albedo"].astype(np.float64).mean(axis=0)
    assert (np.abs(mean - R) <= 5 * se).all(), (mean, R, se)


def _restated_rho(orc, kind, r4, k4, eta, alpha, wo_local):
    """BSDF::rho_hd over the fixed points through the oracle's BxDF::sample_f probe, in float32 and in the stated order."""
    FP = C.POINTER(C.c_float)
    fa = lambda a: np.ascontiguousarray(a, F32).ctypes.data_as(FP)
    r = np.zeros(4, F32)
    if wo_local[2] == 0:
        return r
    out = np.zeros(10, F32)
    for i in range(16):
        ok = orc.lib.orc_fn_bxdf_sample_f(kind, fa(r4), fa(k4), float(eta), float(alpha), float(alpha), fa(wo_local), float(UC[i]), fa(np.array(U2[i], F32)), out.ctypes.data_as(FP))
        if ok and out[7] > 0:
            r = (r + (out[0:4] * np.abs(out[6])) / out[7]).astype(F32)
    return (r / F32(16)).astype(F32)


@pytest.mark.parametrize("kind", ["conductor", "dielectric"])
def test_conductor_and_dielectric_rho_restated(lib, kind):
    if kind == "conductor":
        mat = lambda b: b.material_conductor(b.spectrum_constant(0.2), b.spectrum_constant(3.5), roughness=0.3, remap=False)
        args = (abi.SHM_MATERIAL_CONDUCTOR, [0.2] * 4, [3.5] * 4, 1.0, 0.3)
    else:
        mat = lambda b: b.material_dielectric(1.5, roughness=0.3, remap=False)
        args = (abi.SHM_MATERIAL_DIELECTRIC, [0.0] * 4, [0.0] * 4, 1.5, 0.3)
    c = Chain(lib, _plane(lib, mat), gc.params_for())
    rho = c.rho()
    out12, n_checked = (C.c_float * 12)(), 0
    for k in np.flatnonzero(c.hit)[::11]:
        ray = abi.ShmRay()
        ray.o[:], ray.d[:], ray.t_max = [float(v) for v in c.rays[k, 0:3]], [float(v) for v in c.rays[k, 3:6]], float("inf")
        assert c.orc.lib.orc_fn_hit_interaction(c.orc.handle, C.byref(ray), out12, None)
        ns, dpdu = np.array(out12[6:9], F32), np.array(out12[9:12], F32)
        x = dpdu / np.linalg.norm(dpdu)
        assert sorted(np.abs(x)) == [0, 0, 1] and sorted(np.abs(ns)) == [0, 0, 1], "the plane's shading frame is render space's axes: to_local is exact"
        y = np.cross(ns, x)
        wo = -c.rays[k, 3:6]
        wo_local = np.array([x @ wo, y @ wo, ns @ wo], F32)
        want = _restated_rho(c.orc, *args, wo_local)
        assert np.array_equal(want.view(np.uint32), rho[k, 0:4].view(np.uint32)), (k, want, rho[k, 0:4])
        assert want.any()
        n_checked += 1
    assert n_checked > 20


def test_rho_bounds_of_every_material(lib):
    kinds = set()
    for scene in ("materials", "coated", "diffuse_transmission"):
        c = Chain(lib, gc.make_scene(lib, scene), gc.params_for())
        rho = c.rho()[:, 0:4]
        assert np.isfinite(rho).all() and rho.min() >= 0 and rho.max() <= 1 + 64 * EPS, (scene, rho.min(), rho.max())
        kinds |= set().union(*(_leaf_kinds(c.desc, c.desc.primitives[int(p)].material) for p in np.unique(c.hits["prim"][c.hit])))
    # what the camera rays of the three scenes meet between them: every material kind but the one a MixMaterial resolves away
    assert kinds >= {abi.SHM_MATERIAL_DIFFUSE, abi.SHM_MATERIAL_CONDUCTOR, abi.SHM_MATERIAL_DIELECTRIC, abi.SHM_MATERIAL_THIN_DIELECTRIC, abi.SHM_MATERIAL_COATED_DIFFUSE,
                     abi.SHM_MATERIAL_COATED_CONDUCTOR, abi.SHM_MATERIAL_DIFFUSE_TRANSMISSION}, kinds


# ---- camera space ----
def test_camera_space_is_the_render_space_result_transformed(lib):
    sc = gc.make_scene(lib, "tilted")  # (camera_from_render is a general rotation under this camera's look-at)
    c = Chain(lib, sc, gc.params_for())
    cam = c.records(abi.SHM_GBUFFER_SPACE_CAMERA)
    FP = C.POINTER(C.c_float)
    m = np.array(sc.desc.camera.camera_from_render[:], F32)
    m_inv = np.array(sc.desc.camera.render_from_camera[:], F32)
    out = np.zeros(3, F32)
    apply = lambda kind, v: (c.orc.lib.orc_fn_transform_apply(kind, 0, m.ctypes.data_as(FP), m_inv.ctypes.data_as(FP), np.ascontiguousarray(v, F32).ctypes.data_as(FP),
                                                              out.ctypes.data_as(FP)), out.copy())[1]
    assert c.hit.any()
    for k in np.flatnonzero(c.hit)[::13]:
        r = c.samples[k].astype(F32)  # (box filter: the records are the float values themselves)
        assert np.array_equal(apply(0, r[0:3]).astype(np.float64), cam[k, 0:3])
        assert np.array_equal(apply(2, r[3:6]).astype(np.float64), cam[k, 3:6])
        assert np.array_equal(apply(2, r[6:9]).astype(np.float64), cam[k, 6:9])
        assert np.array_equal(c.samples[k, 9:16], cam[k, 9:16])
    assert not np.array_equal(cam[:, 0:3], c.samples[:, 0:3])


# ---- host helpers ----
def test_white_is_the_float64_sum_of_the_sensor_tables(lib, cornell):
    white = render.gbuffer_white(lib, cornell.desc)
    want = [float(np.sum(t.astype(np.float64))) for t in _sensor(cornell.desc)]
    assert np.allclose(white, want, rtol=1e-14, atol=0) and (white > 0).all()


def test_resolve_against_numpy(lib):
    rng = np.random.default_rng(5)
    g = np.zeros(6, render.GBUFFER_DTYPE)
    rows = g.view(np.float64).reshape(6, 16)
    rows[:] = rng.uniform(-2.0, 2.0, rows.shape)
    rows[:, 11:14] = rng.uniform(0.0, 50.0, (6, 3))
    rows[:, 14] = rng.uniform(0.5, 3.0, 6)
    rows[:, 15] = rows[:, 14] + rng.uniform(0.0, 1.0, 6)
    rows[2, 14] = 0.0  # a pixel no sample hit
    white = np.array([106.9, 106.8, 106.7])
    for m in (None, render.SRGB_FROM_XYZ):
        img = render.gbuffer_resolve(lib, g, white, m)
        mm = np.eye(3) if m is None else m.astype(np.float64)
        for i in range(6):
            if rows[i, 14] == 0:
                assert not any(img[k][i].any() for k in img)
                continue
            w = rows[i, 14]
            assert np.allclose(img["p"][i], rows[i, 0:3] / w, rtol=1e-6) and np.allclose(img["n"][i], rows[i, 3:6] / w, rtol=1e-6)
            assert np.allclose(img["ns"][i], rows[i, 6:9] / w, rtol=1e-6) and np.allclose(img["uv"][i], rows[i, 9:11] / w, rtol=1e-6)
            assert np.allclose(img["albedo"][i], (mm @ (rows[i, 11:14] / w)) / (mm @ white), rtol=1e-6)
            assert np.isclose(img["coverage"][i], w / rows[i, 15], rtol=1e-6)


def test_abi_probe(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    fields = [n for n, _ in abi.ShmGBufferPixel._fields_]
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"shimmer_hip.h\"\nint main(void) {\n"
           "  printf(\"%zu %d %zu %d %d\\n\", sizeof(ShmGBufferPixel), SHM_ABI_VERSION, sizeof(ShmSceneDesc), SHM_GBUFFER_SPACE_RENDER, SHM_GBUFFER_SPACE_CAMERA);\n"
           + "".join(f"  printf(\"{f} %zu\\n\", offsetof(ShmGBufferPixel, {f}));\n" for f in fields) + "  return 0;\n}\n")
    (tmp_path / "probe.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")], check=True)
    lines = subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert lines[0].split() == ["128", "10", "640", "0", "1"]
    assert C.sizeof(abi.ShmGBufferPixel) == 128 and C.sizeof(abi.ShmSceneDesc) == 640 and abi.SHM_ABI_VERSION == 10
    for line in lines[1:]:
        name, off = line.split()
        assert getattr(abi.ShmGBufferPixel, name).offset == int(off), name
    assert render.GBUFFER_DTYPE.itemsize == 128 and [render.GBUFFER_DTYPE.fields[f][1] for f in fields] == [getattr(abi.ShmGBufferPixel, f).offset for f in fields]


def test_force_diffuse_films_are_what_they_were(lib):
    """bsdf_rho_hd stands beside bsdf_force_diffuse in shm/bxdf.h since the G-buffer pass: the oracle's force_diffuse films of two scenes, hashed at the commit before
    it (tests/golden/gbuffer_force_diffuse.json), are unchanged."""
    recorded = json.loads((ROOT / "tests" / "golden" / "gbuffer_force_diffuse.json").read_text())
    for scene, want in recorded.items():
        sc = gc.make_scene(lib, scene)
        o = oracle_py.Oracle(sc.desc)
        try:
            film, _ = o.render(render.make_params(seed=5, spp=4, max_depth=5, force_diffuse=True), n_threads=4)
        finally:
            o.close()
        assert hashlib.sha256(np.ascontiguousarray(film).tobytes()).hexdigest() == want, scene
