"""PBRT-v4's distant and spot lights on the device: the *_dl kernels (wavefront.h, K_DELTA_LIGHTS) of every scene class against the CPU oracle bit for bit — film and
the seven counters —, the other integrators, ZSobol against the oracle and by decomposition invariance, scenes lit by delta lights alone, the leaf probe on
tests/test_delta_lights.py's vectors, and a sweep over the scene classes, options and pipelines that the remaining *_dl kernels serve."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_py
import test_delta_lights as dl
import zsobol_cases as zc
from shimmer_amd import abi, render, scene as scn, scenes
from shimmer_amd.scenes import _box, _quad, _to_render, blackbody_dense
from test_gpu_zsobol import probe_op

pytestmark = pytest.mark.gpu
STATS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")
# per scene: where the spot light stands and what it and the sun aim at (world space), so that both reach what the camera sees
CORNELL = dict(spot_from=(0.5, 1.7, 0.8), spot_to=(-0.2, 0.3, -0.2), sun_from=(0.3, 0.4, 3.0), sun_to=(0.0, 0.8, 0.0))
PROXY = dict(spot_from=(2.0, 2.5, 2.5), spot_to=(0.0, -0.5, 0.0), coneangle=30.0, conedelta=8.0, spot_scale=60.0, sun_from=(1.0, 1.5, 4.0), sun_to=(0.0, 0.0, 0.0))
CROWN = dict(spot_from=(2.5, 4.0, 3.0), spot_to=(0.0, 1.0, 0.0), coneangle=30.0, conedelta=8.0, spot_scale=80.0, sun_from=(-1.0, 2.0, 3.0), sun_to=(0.0, 1.0, 0.0))
SPHERES = dict(spot_from=(0.0, 4.0, 6.0), spot_to=(0.5, 0.0, 0.0), coneangle=40.0, conedelta=10.0, spot_scale=60.0, sun_from=(1.0, 2.0, 3.0), sun_to=(0.0, 0.0, 0.0))
INSTANCES = dict(spot_from=(-2.0, 5.0, 3.0), spot_to=(0.0, 0.5, 0.0), coneangle=35.0, conedelta=10.0, spot_scale=80.0, sun_from=(1.0, 3.0, 2.0), sun_to=(0.0, 0.0, 0.0))


def class_scene(lib, which, lights=True, **only):
    def x(kw):
        return scenes.spot_and_distant(**kw, **only) if lights else None
    if which == "lean":  # the Cornell box: all-diffuse triangles, the fused lean kernel
        return scenes.cornell_box(lib, 40, 40, extra_lights=x(CORNELL)), 6, 5
    if which == "sorted_fused":  # glass and metal: the material-sorted fused all-materials kernel
        return scenes.crown_proxy(lib, 30, 42, level=1, n_glass=6, n_gold=2, extra_lights=x(CROWN)), 4, 6
    if which == "staged_coated":  # the coated S3 proxy at small size: k_vertex -> k_scatter<class>, the LayeredBxDF stages
        return scenes.ganesha_proxy(lib, 48, 48, n=24, coated=True, extra_lights=x(PROXY)), 4, 5
    if which == "textured":
        return scenes.cornell_box(lib, 32, 32, textured=True, extra_lights=x(CORNELL)), 4, 5
    if which == "environment":  # distant + image infinite: a delta direction beside an infinite light
        return scenes.three_spheres(lib, 40, 30, camera=(0.75, 0.5, 9.0), environment=scenes.environment_image(32), extra_lights=x(SPHERES)), 4, 5
    if which == "general":  # bilinear patches and glass: the general-geometry kernels
        return scenes.cornell_box(lib, 32, 32, glass=True, patches=True, extra_lights=x(CORNELL)), 4, 5
    assert which == "instances"
    return scenes.instanced_scene(lib, 40, 30, extra_lights=x(INSTANCES)), 4, 5


def gpu_render(lib, desc, p):
    g = render.Renderer(lib, desc, 0)
    out = g.render(p)
    g.close()
    return out


def assert_equals_oracle(lib, sc, p, what):
    f_gpu, s_gpu = gpu_render(lib, sc.desc, p)
    orc = oracle_py.Oracle(sc.desc)
    f_cpu, s_cpu = orc.render(p, n_threads=min(16, os.cpu_count() or 1))
    orc.close()
    for field in ("rgb_sum", "weight_sum"):
        assert np.array_equal(f_gpu[field], f_cpu[field]), (what, field)
    for k in STATS:
        assert s_gpu[k] == s_cpu[k], (what, k)
    assert np.isfinite(f_gpu["rgb_sum"]).all()
    return f_gpu, s_gpu


CLASSES = ["lean", "sorted_fused", "staged_coated", "textured", "environment", "general", "instances"]


@pytest.mark.parametrize("which", CLASSES)
def test_film_and_counters_equal_the_oracle(gpu_lib, which):
    sc, spp, depth = class_scene(gpu_lib, which)
    assert [l.kind for l in sc.builder.lights[-2:]] == [abi.SHM_LIGHT_SPOT, abi.SHM_LIGHT_DISTANT]
    p = render.make_params(seed=13, spp=spp, max_depth=depth)
    f_gpu, s_gpu = assert_equals_oracle(gpu_lib, sc, p, which)
    # the lights are used — each of them: the film differs from the scene without them and from the scene with either one alone
    for kw in (dict(lights=False), dict(spot=False), dict(distant=False)):
        other, _, _ = class_scene(gpu_lib, which, **kw)
        f_other, _ = gpu_render(gpu_lib, other.desc, p)
        assert not np.array_equal(f_other["rgb_sum"], f_gpu["rgb_sum"]), (which, kw)


def test_with_the_reference_quirks_off(gpu_lib):
    for which in ("lean", "general"):
        sc, spp, depth = class_scene(gpu_lib, which)
        p = render.make_params(seed=17, spp=spp, max_depth=depth, reference_quirks=False)
        f_gpu, _ = assert_equals_oracle(gpu_lib, sc, p, which)
        plain, _, _ = class_scene(gpu_lib, which, lights=False)
        assert not np.array_equal(gpu_render(gpu_lib, plain.desc, p)[0]["rgb_sum"], f_gpu["rgb_sum"]), which  # (the lights are used)


@pytest.mark.parametrize("integrator, lights, bsdf", [("simplepath", True, True), ("simplepath", True, False), ("simplepath", False, True), ("simplepath", False, False),
                                                      ("randomwalk", True, True)])
def test_the_other_integrators_equal_the_oracle(gpu_lib, integrator, lights, bsdf):
    for which in ("lean", "general"):
        sc, spp, depth = class_scene(gpu_lib, which)
        p = render.make_params(seed=3, spp=spp, max_depth=4, integrator=integrator, sample_lights=lights, sample_bsdf=bsdf)
        f_gpu, _ = assert_equals_oracle(gpu_lib, sc, p, (which, integrator, lights, bsdf))
        if integrator == "simplepath" and lights:  # (without light sampling a delta light is never found: the film is the plain scene's)
            plain, _, _ = class_scene(gpu_lib, which, lights=False)
            assert not np.array_equal(gpu_render(gpu_lib, plain.desc, p)[0]["rgb_sum"], f_gpu["rgb_sum"])


@pytest.mark.parametrize("which", ["lean", "general"])
def test_the_other_integrators_under_zsobol(gpu_lib, which):
    """k_shade_simple_zs_dl (RandomWalk samples no light and has no _dl build: k_shade_randomwalk_zs serves the scene). The renders equal the oracle's, are
    repeatable, independent of how the work is cut up, use the lights, and agree with independent sampling in the mean (as tests/test_gpu_zsobol.py has it for the plain kernels)."""
    sc, _, _ = class_scene(gpu_lib, which)
    plain, _, _ = class_scene(gpu_lib, which, lights=False)
    g = render.Renderer(gpu_lib, sc.desc, 0)
    for integ, kw in (("simplepath", dict()), ("simplepath", dict(sample_bsdf=False)), ("randomwalk", dict())):
        pz = render.make_params(seed=3, spp=256, max_depth=4, integrator=integ, sampler="zsobol", **kw)
        fz, sz = g.render(pz)
        zc.assert_equals_oracle(sc.desc, pz, fz, sz, (which, integ, kw))
        fz2, _ = g.render(pz)
        assert np.array_equal(fz, fz2) and np.isfinite(fz["rgb_sum"]).all(), integ
        g.clear()
        idx = np.arange(g.n_tiles)
        for ws, we in scn.wave_schedule(256):
            g.render_waves(pz, tile_indices=idx[idx % 2 == 1], waves=[(ws, we)])
            g.render_waves(pz, tile_indices=idx[idx % 2 == 0], waves=[(ws, we)])
        assert np.array_equal(g.read_film(), fz), integ
        if which == "lean":  # (spp and margin of tests/test_gpu_zsobol.py's check of the plain kernels on the same box; the glass scene's caustics are too noisy for it)
            fi, _ = g.render(render.make_params(seed=3, spp=1024, max_depth=4, integrator=integ, **kw))
            a, b = render.film_to_rgb(fz).mean(), render.film_to_rgb(fi).mean()
            assert abs(a / b - 1.0) < 0.03, (integ, a, b)
        if integ == "simplepath":  # (a delta light is found by light sampling alone)
            assert not np.array_equal(gpu_render(gpu_lib, plain.desc, pz)[0]["rgb_sum"], fz["rgb_sum"])
    g.close()


def delta_only_scene(lib, coated, **only):
    """No emitter, no infinite light: a floor, a wall and a box under a spot and a distant light."""
    b = scn.SceneBuilder()
    b.set_film(36, 30)
    rfw = b.set_camera_look_at(lib, (0.0, 1.5, 4.5), (0.0, 0.5, 0.0), (0, 1, 0), 35.0)
    grey = b.material_diffuse(0.6)
    p, vi = _quad((-5, 0, -5), (-5, 0, 5), (5, 0, 5), (5, 0, -5))
    b.add_mesh(_to_render(p, rfw), vi, grey)
    p, vi = _quad((-5, 0, -2), (5, 0, -2), (5, 5, -2), (-5, 5, -2))
    b.add_mesh(_to_render(p, rfw), vi, b.material_diffuse(0.4))
    box_m = b.material_coated_diffuse(0.5, roughness=0.1) if coated else b.material_diffuse(0.8)
    p, vi = _box((-0.5, 0.0, -0.5), (0.5, 1.0, 0.5))
    b.add_mesh(_to_render(p, rfw), vi, box_m)
    scenes.spot_and_distant(spot_from=(1.5, 3.0, 2.0), spot_to=(0.0, 0.5, 0.0), coneangle=30.0, conedelta=10.0, spot_scale=40.0, sun_from=(-1.0, 2.0, 1.5), sun_to=(0, 0, 0), **only)(b, rfw)
    desc, _ = b.build(lib)
    return b, desc


@pytest.mark.parametrize("coated", [False, True])
def test_a_scene_lit_by_delta_lights_alone(gpu_lib, coated):
    from types import SimpleNamespace
    b, desc = delta_only_scene(gpu_lib, coated)
    f, s = assert_equals_oracle(gpu_lib, SimpleNamespace(desc=desc), render.make_params(seed=29, spp=4, max_depth=4), coated)
    assert f["rgb_sum"].max() > 0 and s["rays_any"] > 0
    # the lights are used, each of them: without either one the film differs (there is no scene "without the lights" to compare with: it would be black)
    for kw in (dict(spot=False), dict(distant=False)):
        _, other = delta_only_scene(gpu_lib, coated, **kw)
        assert not np.array_equal(gpu_render(gpu_lib, other, render.make_params(seed=29, spp=4, max_depth=4))[0]["rgb_sum"], f["rgb_sum"]), kw


@pytest.mark.parametrize("which", ["lean", "staged_coated", "sorted_fused"])
def test_zsobol_decomposition_invariance(gpu_lib, which):
    """The *_zs_dl kernels: the oracle's film and counters, and a film that does not depend on how the work is cut up."""
    sc, spp, depth = class_scene(gpu_lib, which)
    p = render.make_params(seed=21, spp=8, max_depth=depth, sampler="zsobol")
    gpu = render.Renderer(gpu_lib, sc.desc, 0)
    f1, s1 = gpu.render(p)
    f2, _ = gpu.render(p)
    assert np.array_equal(f1, f2) and (f1["weight_sum"] == 8.0).all() and np.isfinite(f1["rgb_sum"]).all()
    zc.assert_equals_oracle(sc.desc, p, f1, s1, which)
    f_ind, _ = gpu.render(render.make_params(seed=21, spp=8, max_depth=depth))
    assert not np.array_equal(f1, f_ind)
    gpu.clear()
    idx = np.arange(gpu.n_tiles)
    for ws, we in scn.wave_schedule(8):
        gpu.render_waves(p, tile_indices=idx[idx % 3 != 0], waves=[(ws, we)])
        gpu.render_waves(p, tile_indices=idx[idx % 3 == 0], waves=[(ws, we)])
    assert np.array_equal(gpu.read_film(), f1)
    gpu.clear()
    gpu.render_device(p)
    assert np.array_equal(gpu.read_film(), f1)
    gpu.close()
    plain, _, _ = class_scene(gpu_lib, which, lights=False)
    assert not np.array_equal(gpu_render(gpu_lib, plain.desc, p)[0]["rgb_sum"], f1["rgb_sum"])
    # ... and the image is the independent sampler's in the mean (the same lights, the same estimator)
    a = render.film_to_rgb(gpu_render(gpu_lib, sc.desc, render.make_params(seed=2, spp=64, max_depth=depth, sampler="zsobol"))[0]).mean()
    c = render.film_to_rgb(gpu_render(gpu_lib, sc.desc, render.make_params(seed=2, spp=64, max_depth=depth))[0]).mean()
    assert abs(a / c - 1.0) < 0.05, (a, c)


def test_a_scene_without_the_new_lights_renders_what_it_rendered(gpu_lib):
    """Before / after: the instanced scene (an area light, a point light, no distant or spot light) renders the film that the library before this change rendered —
    by its CPU oracle, which its device path equals bit for bit; the SHA-256 is recorded in tests/golden/delta_lights_before.json — through the kernels built without the new lights, which are instruction-identical
    to that library's (tools/kernel_isa_diff.py)."""
    import hashlib
    import json
    before = json.loads((dl.ROOT / "tests" / "golden" / "delta_lights_before.json").read_text())
    sc = scenes.instanced_scene(gpu_lib, 40, 30)
    assert any(l.kind == abi.SHM_LIGHT_POINT for l in sc.builder.lights) and sc.desc.n_spot_lights == 0
    for case in before["films"]:
        p = render.make_params(seed=case["seed"], spp=case["spp"], max_depth=case["max_depth"], sampler=case["sampler"])
        f, st = gpu_render(gpu_lib, sc.desc, p)
        assert hashlib.sha256(np.ascontiguousarray(f).tobytes()).hexdigest() == case["sha256"], case
        assert [st[k] for k in STATS] == case["stats"], case


def test_the_probe_replays_the_leaf_vectors(gpu_lib):
    """tests/test_delta_lights.py's grid of lights through PROBE_LIGHT_SAMPLE_LI: the device's own light_sample_li against the float64 restatement at that test's
    tolerance, and bit-equal to the oracle's; also at a context point away from the origin."""
    plib = abi.load_probe_library()
    op = probe_op("LIGHT_SAMPLE_LI")
    b, desc, dense, cases = dl.leaf_scene(gpu_lib)
    o = oracle_py.Oracle(desc)
    o.lib.orc_fn_light_sample_li.restype, o.lib.orc_fn_light_sample_li.argtypes = C.c_int, [C.c_void_p, C.c_uint32, dl.FP, C.c_int, dl.FP, dl.FP]
    fb = lambda v: int(np.float32(v).view(np.uint32))  # noqa: E731

    def probe(light, spot, ctx):
        m = np.array(spot.light_from_render[:], np.float32).reshape(4, 4)[:3, :3].ravel() if spot is not None else np.zeros(9, np.float32)
        words = [light.kind, fb(light.scale)] + [fb(v) for v in light.position] + [fb(v) for v in m]
        words += [fb(spot.cos_falloff_start if spot is not None else 0.0), fb(spot.cos_falloff_end if spot is not None else 0.0), len(dense), 360]
        words += [fb(v) for v in ctx] + [fb(3.0)] + [fb(v) for v in dl.LAMBDA] + [fb(v) for v in dense]
        a = (C.c_uint32 * len(words))(*words)
        out = (C.c_uint32 * 8)()
        res = C.c_int()
        abi.check(plib, plib.shm_debug_eval_leaf(0, op, a, len(words), out, 8, C.byref(res)), "shm_debug_eval_leaf")
        return res.value, np.frombuffer(bytes(out), np.float32).astype(np.float64)

    n_checked = 0
    for i, (kind, note) in enumerate(cases):
        light = desc.lights[i]
        spot = b.spot_lights[light.primitive] if light.kind == abi.SHM_LIGHT_SPOT else None
        ok_d, out_d = probe(light, spot, (0.0, 0.0, 0.0))
        ok_c, out_c = dl.sample_li(o, i)
        assert ok_d == ok_c, note
        if ok_c:
            assert np.array_equal(out_d, out_c), note  # the device == the oracle, bit for bit
        if kind != "spot":
            continue
        for ctx in ((0.0, 0.0, 0.0), (0.3, -0.4, 0.25)):
            ok, out = probe(light, spot, ctx)
            wi, cos, l_axis, falloff, kappa = dl.spot_expected(light, spot, dense, ctx)
            width = float(spot.cos_falloff_start) - float(spot.cos_falloff_end)
            cos_err, tol = dl.leaf_tolerance(kappa, width)
            if abs(cos - float(spot.cos_falloff_end)) <= 4 * cos_err:
                continue
            if falloff == 0.0:
                assert ok == 0, (note, ctx)
                continue
            assert ok == 1 and np.allclose(out[:3], wi, atol=4 * dl.U) and out[3] == 1.0, (note, ctx)
            assert np.all(np.abs(out[4:] - falloff * l_axis) <= tol * l_axis), (note, ctx)
            n_checked += 1
    o.close()
    assert n_checked >= 10


def test_every_delta_light_kernel_runs_and_the_pipelines_agree(gpu_lib, monkeypatch):
    """The remaining *_dl kernels — the general scatter kernels under force_diffuse / regularize, the *_env units, rough dielectrics, the split pass and the lean
    diversion, both samplers: the staged pipeline from the camera ray on (SHM_TAIL_FUSED_BOUNCE=-1) against the default, and the split pass off against on,
    give the same bits and counters; under ZSobol the default's are also the oracle's (under the independent sampler the tests above hold the classes to it). (Which *_dl kernels a run of this file launches is what tools/kernel_coverage.py shows of a kernel trace: profiles/delta_lights.md.)"""
    lib = gpu_lib
    env = scenes.environment_image(32)
    c, cr, sp, ins = scenes.spot_and_distant(**CORNELL), scenes.spot_and_distant(**CROWN), scenes.spot_and_distant(**SPHERES), scenes.spot_and_distant(**INSTANCES)
    cases = [scenes.crown_proxy(lib, 30, 42, level=1, n_glass=6, n_gold=2, extra_lights=cr), scenes.crown_proxy(lib, 30, 42, level=1, n_glass=6, n_gold=2, environment=env, extra_lights=cr),
             scenes.cornell_box(lib, 32, 32, textured=True, extra_lights=c), scenes.cornell_box(lib, 32, 32, glass=True, environment=env, extra_lights=c),
             scenes.cornell_box(lib, 32, 32, coated=True, environment=env, extra_lights=c), scenes.three_spheres(lib, 40, 30, camera=(0.75, 0.5, 9.0), environment=env, extra_lights=sp),
             scenes.instanced_scene(lib, 40, 30, environment=env, extra_lights=ins), scenes.cornell_box(lib, 32, 32, coated=True, extra_lights=c),
             scenes.cornell_box(lib, 32, 32, glass_too=True, extra_lights=c), scenes.cornell_box(lib, 32, 32, glass_too=True, environment=env, extra_lights=c),
             scenes.cornell_box(lib, 32, 32, glass=True, patches=True, extra_lights=c), scenes.cornell_box(lib, 32, 32, glass=True, patches=True, environment=env, extra_lights=c),
             scenes.cornell_box(lib, 32, 32, patches=True, extra_lights=c), scenes.cornell_box(lib, 32, 32, patches=True, environment=env, extra_lights=c),
             scenes.cornell_box(lib, 32, 32, environment=env, extra_lights=c),
             scenes.cornell_box(lib, 32, 32, textured=True, textured_coated_ceiling=False, patches=True, extra_lights=c)] + [scenes.random_scene(lib, k, extra_lights=ins) for k in (1, 3, 11, 13)]
    variants = ((None, None), ("SHM_TAIL_FUSED_BOUNCE", "-1"), ("SHM_TAIL_FUSED_BOUNCE", "3"), ("SHM_SPLIT_PASS", "0"), ("SHM_SPLIT_PASS", "1"))
    for sc in cases:
        assert any(l.kind == abi.SHM_LIGHT_SPOT for l in sc.builder.lights)
        for sampler in ("independent", "zsobol"):
            for kw in (dict(), dict(force_diffuse=True), dict(regularize=True)):
                p = render.make_params(seed=9, spp=2, max_depth=5, sampler=sampler, **kw)
                out = []
                for var, val in variants if not kw else variants[:2]:
                    for v in ("SHM_TAIL_FUSED_BOUNCE", "SHM_SPLIT_PASS"):
                        monkeypatch.delenv(v, raising=False)
                    if var:
                        monkeypatch.setenv(var, val)
                    out.append(gpu_render(lib, sc.desc, p))
                for v in ("SHM_TAIL_FUSED_BOUNCE", "SHM_SPLIT_PASS"):
                    monkeypatch.delenv(v, raising=False)
                assert np.isfinite(render.film_to_rgb(out[0][0])).all(), (sc.name, sampler, kw)
                if sampler == "zsobol":
                    zc.assert_equals_oracle(sc.desc, p, out[0][0], out[0][1], (sc.name, kw))
                for f, s in out[1:]:
                    assert np.array_equal(f, out[0][0]), (sc.name, sampler, kw)
                    for k in STATS:
                        assert s[k] == out[0][1][k], (sc.name, sampler, kw, k)
