"""The per-primitive shading records of flat triangles (shimmer_amd/csrc/shm/tri_shade.h): a triangle whose mesh has neither normals nor tangents, on a material that is
no mix and binds no displacement texture or normal map, has its normal and BSDF frame computed once at scene creation; the TRI_ONLY no-texture vertex kernels (k_shade,
k_emit_jobs, k_vertex) fetch them. One small scene holds every kind of triangle the record code distinguishes, beside triangles that get no record, and is rendered
against the CPU oracle (which knows nothing of records) and against the same library with SHM_TRI_SHADE=0 (no records: every hit takes the full interaction): f64 film
sums and all seven counters, bit for bit.

Two kinds of triangle cannot be hit reliably by camera rays at this size — one so large that set_shading_geometry's rescale loop runs, and a needle whose
cross(dpdu, dpdv) underflows to zero. The records are built on the device by running triangle_interaction + get_bsdf themselves, so those two are covered by
construction only: the stored values are that code's output whatever branch it took."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")
W = H = 32
SPP, DEPTH, SEED = 8, 5, 13


def _tilted_quad(cx, cy, cz=0.0, half=0.24, yaw=0.35, pitch=0.2):
    """A quad facing the camera (+z in world space), turned a little about y and x so that no normal component is 0."""
    c, s, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    local = np.array([[-half, -half, 0], [half, -half, 0], [half, half, 0], [-half, half, 0]], np.float64)
    p = local @ (ry @ rx).T + np.array([cx, cy, cz])
    return p.astype(np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def _scene(lib, scenes, variant="diffuse"):
    """variant: "diffuse" (all-diffuse: the lean fused kernel + k_emit_jobs), "spot" (the same + a spot light: the *_dl builds), "staged" (a conductor and a coated
    material beside the diffuse ones: the staged k_vertex with the lean diversion), "fused" (the conductor alone beside them: the material-sorted fused kernel, which
    keeps the full interaction — no records are built for its scenes). Returns the scene and, per special mesh, a world-space point on it."""
    from shimmer_amd.scene import SceneBuilder, blackbody_dense
    b = SceneBuilder()
    b.set_film(W, H)
    rfw = b.set_camera_look_at(lib, (0, 1, 3.4), (0, 1, 0), (0, 1, 0), 39.0)
    white = b.material_diffuse(0.7)             # the reference's DiffuseMaterial: a constant displacement of 0 (the bump map runs)
    bumped = b.material_diffuse(0.6)
    b.materials[bumped].displacement = 0.05     # a non-zero constant displacement
    plain = b.material_diffuse(0.5)
    b.materials[plain].has_displacement = 0     # no displacement at all: get_bsdf leaves the shading geometry alone
    m_flip, m_uv, m_uv0 = bumped, white, plain
    if variant in ("staged", "fused"):
        m_flip = b.material_conductor(b.spectrum_named("metal-Cu-eta"), b.spectrum_named("metal-Cu-k"), roughness=0.3)
    if variant == "staged":
        m_uv0 = b.material_coated_diffuse(reflectance=0.6, roughness=0.2, thickness=0.02)
    targets = {}

    def add(name, p, vi, material, **kw):
        b.add_mesh(scenes._to_render(p, rfw), vi, material, **kw)
        targets[name] = p[vi[0]].astype(np.float64).mean(0)

    # axis-aligned faces: normal components exactly +-0 through the flip and face_forward
    room_p, room_vi = scenes._box((-1, 0, -1), (1, 2, 1), faces="xXyYz")
    add("room", room_p, room_vi, white)
    # a MESH_FLIP mesh (wound so that the flipped normal faces the camera or not: both are shaded, the surface is two-sided for a BSDF)
    p, vi = _tilted_quad(-0.6, 0.45)
    add("flip", p, vi, m_flip, reverse_orientation=True)
    # a mesh with uv
    p, vi = _tilted_quad(0.0, 0.45, yaw=-0.3)
    add("uv", p, vi, m_uv, uv=np.array([[0.1, 0.2], [0.9, 0.1], [1.0, 0.8], [0.0, 1.0]], np.float32))
    # a mesh whose three uv coincide: the coordinate_system fallback
    p, vi = _tilted_quad(0.6, 0.45, yaw=0.5)
    add("uv_coincident", p, vi, m_uv0, uv=np.full((4, 2), 0.3, np.float32))
    # beside the flat ones: a mesh with normals and one with tangents (no record: the full interaction, in the same waves)
    p, vi = _tilted_quad(-0.6, 1.15, yaw=0.0, pitch=0.0)
    n = np.array([[-0.3, -0.3, 1], [0.3, -0.3, 1], [0.3, 0.3, 1], [-0.3, 0.3, 1]], np.float64)
    add("normals", p, vi, white, n=(n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32))
    p, vi = _tilted_quad(0.0, 1.15, yaw=0.25)
    add("tangents", p, vi, bumped, s=np.array([[1, 0.2, 0], [1, 0.1, 0.1], [0.9, 0, 0.2], [1, -0.1, 0]], np.float32))
    # a flat mesh on the material without a displacement
    p, vi = _tilted_quad(0.6, 1.15, yaw=-0.45, pitch=-0.25)
    add("no_displacement", p, vi, plain)
    # the emitter: reachable after a diffuse bounce (k_emit_jobs: the hit itself, and the previous vertex rebuilt from its hit record); reflecting, so that paths go on from it
    p, vi = scenes._quad((-0.35, 1.98, -0.35), (0.35, 1.98, -0.35), (0.35, 1.98, 0.35), (-0.35, 1.98, 0.35))
    b.add_mesh(scenes._to_render(p, rfw), vi, b.material_diffuse(0.4), emission=blackbody_dense(6500.0), emission_scale=12.0)
    if variant == "spot":
        b.light_spot((0.4, 1.7, 0.9), (0.0, 0.6, 0.0), blackbody_dense(3200.0), scale=6.0, coneangle=40.0, conedelta=10.0, render_from_object=rfw)
    desc, _ = b.build(lib)
    desc.keepalive = b  # (the description points into the builder's arrays)
    return desc, targets, rfw


@pytest.fixture(scope="module")
def env(gpu_lib):
    import oracle_py
    from shimmer_amd import render, scenes
    return gpu_lib, oracle_py, render, scenes


@pytest.fixture(scope="module")
def oracle_results(env):
    """The oracle's film and counters per scene variant, rendered once and shared; checked here, on the CPU, to be finite and to see every special mesh."""
    lib, oracle_py, render, scenes = env
    cache = {}

    def get(variant):
        if variant not in cache:
            desc, targets, rfw = _scene(lib, scenes, variant)
            orc = oracle_py.Oracle(desc)
            # every special mesh is seen from the camera (the origin of render space): a ray at its first triangle's centroid ends there
            t = np.array([targets[k] + rfw[:3, 3] for k in targets], np.float64)
            dist = np.linalg.norm(t, axis=1)
            rays = np.zeros((len(t), 8), np.float32)
            rays[:, 3:6], rays[:, 6] = t / dist[:, None], np.inf
            hits, _ = orc.trace(rays)
            assert (hits["prim"] >= 0).all() and np.allclose(hits["t"], dist, rtol=1e-4), dict(zip(targets, hits["t"] - dist))
            film, stats = orc.render(render.make_params(seed=SEED, spp=SPP, max_depth=DEPTH), n_threads=min(16, os.cpu_count() or 1))
            orc.close()
            assert np.isfinite(film["rgb_sum"]).all() and film["rgb_sum"].max() > 0
            cache[variant] = (film, stats)
        return cache[variant]
    return get


# flat triangles of the scene (24 primitives; the meshes with normals and with tangents, two triangles each, get no record) per variant, with the switch on: the scene
# class "fused" (no coated material: the material-sorted fused kernel shades it, which reads no records) builds none
N_RECORDS = {"diffuse": 20, "spot": 20, "staged": 20, "fused": 0}


def _gpu_render(env, variant, **params):
    lib, oracle_py, render, scenes = env
    desc, _, _ = _scene(lib, scenes, variant)
    gpu = render.Renderer(lib, desc, 0)
    # the records were built, or not, as the switch says: parity alone would also hold if every hit silently took the full interaction
    assert gpu.shading_records()[0] == (0 if os.environ.get("SHM_TRI_SHADE") == "0" else N_RECORDS[variant])
    film, stats = gpu.render(render.make_params(seed=SEED, spp=SPP, max_depth=DEPTH, **params))
    gpu.close()
    return film, stats


def _same(a, b):
    (fa, sa), (fb, sb) = a, b
    assert np.array_equal(fa.view(np.uint8), fb.view(np.uint8))
    for k in COUNTERS:
        assert sa[k] == sb[k], k


def test_records_equal_the_oracle(env, oracle_results, monkeypatch):
    """Records on (the default): the all-diffuse scene through the lean fused kernel and k_emit_jobs equals the oracle bit for bit."""
    monkeypatch.delenv("SHM_TRI_SHADE", raising=False)
    got = _gpu_render(env, "diffuse")
    assert got[1]["rays_any"] > 1000  # (next-event estimation ran)
    _same(got, oracle_results("diffuse"))


def test_records_on_equal_records_off(env, monkeypatch):
    """The same scene from two fresh scene objects, without records (SHM_TRI_SHADE=0, read at scene creation) and with them: identical films and counters."""
    monkeypatch.setenv("SHM_TRI_SHADE", "0")
    off = _gpu_render(env, "diffuse")
    monkeypatch.delenv("SHM_TRI_SHADE")
    on = _gpu_render(env, "diffuse")
    _same(on, off)


def test_records_under_zsobol(env, monkeypatch):
    """The *_zs builds of the same kernels: with records, the library without them and the oracle agree."""
    monkeypatch.setenv("SHM_TRI_SHADE", "0")
    off = _gpu_render(env, "diffuse", sampler="zsobol")
    monkeypatch.delenv("SHM_TRI_SHADE")
    on = _gpu_render(env, "diffuse", sampler="zsobol")
    _same(on, off)
    lib, _, render, scenes = env
    import zsobol_cases as zc
    zc.assert_equals_oracle(_scene(lib, scenes, "diffuse")[0], render.make_params(seed=SEED, spp=SPP, max_depth=DEPTH, sampler="zsobol"), on[0], on[1], "diffuse")
    assert not np.array_equal(on[0]["rgb_sum"], _gpu_render(env, "diffuse")[0]["rgb_sum"])  # (it was another sampler)


def test_records_with_a_spot_light(env, oracle_results, monkeypatch):
    """The *_dl builds (a scene with a spot light) against the oracle."""
    monkeypatch.delenv("SHM_TRI_SHADE", raising=False)
    _same(_gpu_render(env, "spot"), oracle_results("spot"))


@pytest.mark.parametrize("variant", ["staged", "fused"])
def test_records_in_the_staged_class(env, oracle_results, monkeypatch, variant):
    """A conductor and a coated material beside the diffuse ones: the staged k_vertex (coated materials keep the scene on the staged pipeline, plain diffuse hits are
    diverted to the lean kernel); without the coated one: the material-sorted fused kernel, whose scenes get no records. Against the oracle, with the switch on and off."""
    monkeypatch.delenv("SHM_TRI_SHADE", raising=False)
    on = _gpu_render(env, variant)
    _same(on, oracle_results(variant))
    monkeypatch.setenv("SHM_TRI_SHADE", "0")
    _same(_gpu_render(env, variant), on)
