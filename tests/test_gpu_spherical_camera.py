"""PBRT-v4's spherical camera on the device: the generate kernels of k_generate_spherical.hip (K_SPHERICAL_CAMERA, wavefront.h) in every scene class, with both
mappings, against the CPU oracle bit for bit — film and the seven counters —; ZSobol, the wider pixel filters (border pixels sample outside the film and take the wrap),
pixel centres, the quirks switch, the other integrators, decomposition invariance, the leaf probe on tests/test_spherical_camera.py's vectors, and that file's
irradiance probe rendered by the device. Film sizes are ragged on purpose: 40 x 40, 48 x 24, 33 x 17."""
import numpy as np
import pytest

import test_spherical_camera as sph
import zsobol_cases as zc
from device_leaves import DeviceLeaves
from shimmer_amd import abi, render, scene as scn, scenes
from test_gpu_delta_lights import assert_equals_oracle, gpu_render

pytestmark = pytest.mark.gpu
SIZES = [(40, 40), (48, 24), (33, 17)]
CLASSES = ["lean", "sorted_fused", "staged_coated", "textured", "environment", "general", "instances"]


def class_scene(lib, which, size, mapping=None, film=None):
    """(scene, spp, depth); mapping None: the scene under its own perspective camera. The probe stands INSIDE the scene."""
    w, h = size
    def cam(pos, look_at):
        return None if mapping is None else dict(type="spherical", mapping=mapping, pos=pos, look_at=look_at)
    kw = dict(film=film) if film else {}
    if which == "lean":  # the Cornell box: all-diffuse triangles, the fused lean kernel, k_generate<false, LEAN>
        return scenes.cornell_box(lib, w, h, camera=cam((0.1, 1.1, 0.4), (0, 1, -1)), **kw), 6, 5
    if which == "sorted_fused":
        return scenes.crown_proxy(lib, w, h, level=1, n_glass=6, n_gold=2, camera=cam((0.0, 1.4, 3.0), (0.0, 1.2, 0.0)), **kw), 4, 5
    if which == "staged_coated":
        return scenes.ganesha_proxy(lib, w, h, n=24, coated=True, camera=cam((0.0, 0.4, 2.2), (0.0, 0.0, 0.0)), **kw), 4, 5
    if which == "textured":  # k_generate<true, false>: the finite-difference auxiliary rays
        return scenes.cornell_box(lib, w, h, textured=True, camera=cam((0.1, 1.1, 0.4), (0, 1, -1)), **kw), 4, 5
    if which == "environment":  # most rays escape
        env = scenes.environment_image(32)
        if mapping is None:
            return scenes.three_spheres(lib, w, h, camera=(0.75, 0.5, 9.0), environment=env, **kw), 4, 5
        return scenes.three_spheres(lib, w, h, camera=cam((0.75, 0.5, 3.0), (0.0, 0.0, 0.0)), environment=env, **kw), 4, 5
    if which == "general":
        return scenes.cornell_box(lib, w, h, glass=True, patches=True, camera=cam((0.1, 1.1, 0.4), (0, 1, -1)), **kw), 4, 5
    assert which == "instances"
    return scenes.instanced_scene(lib, w, h, camera=cam((0.0, 1.5, 3.0), (0.0, 0.8, 0.0)), **kw), 4, 5


@pytest.mark.parametrize("mapping", ["equalarea", "equirectangular"])
@pytest.mark.parametrize("which", CLASSES)
def test_film_and_counters_equal_the_oracle(gpu_lib, which, mapping):
    size = SIZES[(CLASSES.index(which) + (mapping == "equirectangular")) % 3]
    sc, spp, depth = class_scene(gpu_lib, which, size, mapping)
    assert sc.desc.camera.kind == abi.SHM_CAMERA_SPHERICAL
    p = render.make_params(seed=13, spp=spp, max_depth=depth)
    f_gpu, _ = assert_equals_oracle(gpu_lib, sc, p, (which, mapping))
    assert f_gpu["rgb_sum"].max() > 0
    plain, _, _ = class_scene(gpu_lib, which, size)
    assert not np.array_equal(gpu_render(gpu_lib, plain.desc, p)[0]["rgb_sum"], f_gpu["rgb_sum"]), (which, mapping)  # (the camera is used)


@pytest.mark.parametrize("which", ["lean", "textured"])
def test_zsobol(gpu_lib, which):
    for mapping, size in (("equalarea", (33, 17)), ("equirectangular", (40, 40))):
        sc, _, depth = class_scene(gpu_lib, which, size, mapping)
        p = render.make_params(seed=21, spp=8, max_depth=depth, sampler="zsobol")
        f, s = gpu_render(gpu_lib, sc.desc, p)
        zc.assert_equals_oracle(sc.desc, p, f, s, (which, mapping))


@pytest.mark.parametrize("film", [dict(filter="gaussian", filter_radius=(1.5, 1.5)), dict(filter="mitchell"), dict(filter="triangle")])
def test_wider_pixel_filters_take_the_wrap(gpu_lib, film):
    for mapping, size in (("equalarea", (33, 17)), ("equirectangular", (48, 24))):
        sc, spp, depth = class_scene(gpu_lib, "lean", size, mapping, film=film)
        assert_equals_oracle(gpu_lib, sc, render.make_params(seed=5, spp=spp, max_depth=depth), (film, mapping))
    sc, spp, depth = class_scene(gpu_lib, "textured", (33, 17), "equalarea", film=film)
    assert_equals_oracle(gpu_lib, sc, render.make_params(seed=5, spp=spp, max_depth=depth), (film, "textured"))


def test_pixel_centres_and_the_quirks_switch(gpu_lib):
    for which in ("lean", "textured"):
        for mapping, size in (("equalarea", (40, 40)), ("equirectangular", (33, 17))):
            sc, spp, depth = class_scene(gpu_lib, which, size, mapping)
            assert_equals_oracle(gpu_lib, sc, render.make_params(seed=7, spp=spp, max_depth=depth, disable_pixel_jitter=True), (which, mapping, "centres"))
            assert_equals_oracle(gpu_lib, sc, render.make_params(seed=7, spp=spp, max_depth=depth, reference_quirks=False), (which, mapping, "quirks off"))


@pytest.mark.parametrize("integrator", ["simplepath", "randomwalk"])
def test_the_other_integrators(gpu_lib, integrator):
    for mapping, size in (("equalarea", (48, 24)), ("equirectangular", (33, 17))):
        sc, spp, _ = class_scene(gpu_lib, "lean", size, mapping)
        assert_equals_oracle(gpu_lib, sc, render.make_params(seed=3, spp=spp, max_depth=4, integrator=integrator), (integrator, mapping))


@pytest.mark.parametrize("sampler", ["independent", "zsobol"])
def test_decomposition_invariance(gpu_lib, sampler):
    """Odd and even tiles rendered separately, wave by wave, give the film of one call."""
    sc, _, depth = class_scene(gpu_lib, "lean", (33, 17), "equalarea")
    p = render.make_params(seed=11, spp=8, max_depth=depth, sampler=sampler)
    g = render.Renderer(gpu_lib, sc.desc, 0)
    f1, _ = g.render(p)
    g.clear()
    idx = np.arange(g.n_tiles)
    for ws, we in scn.wave_schedule(8):
        g.render_waves(p, tile_indices=idx[idx % 2 == 1], waves=[(ws, we)])
        g.render_waves(p, tile_indices=idx[idx % 2 == 0], waves=[(ws, we)])
    assert np.array_equal(g.read_film(), f1)
    g.close()


def test_the_probe_replays_the_leaf_vectors(gpu_lib, orc):
    """Every vector of tests/test_spherical_camera.py's leaf test — both mappings, the three resolutions, all 65 film points each — through the device's own
    camera_generate_ray_differential (the leaf probe): the float64 restatement at the CPU test's tolerance, and the oracle's bits."""
    dev = DeviceLeaves(gpu_lib)
    cases = sph.leaf_cases(gpu_lib)
    assert len(cases) == 2 * 3 * 65
    for cam, res, p in cases:
        got = sph.leaf32(dev, cam, p)
        sph.assert_leaf(got, sph.leaf64(cam, res, p), (cam.mapping, res, p))
        assert np.array_equal(got, sph.leaf32(orc, cam, p)), (cam.mapping, res, p)


def test_irradiance_probe_on_the_device(gpu_lib, orc):
    """tests/test_spherical_camera.py's irradiance probe against the diffuse patch, rendered by the device, under the same allowance."""
    def renderer(desc, p):
        return gpu_render(gpu_lib, desc, p)[0]
    sph.assert_probe(sph.probe_measurement(gpu_lib, orc, renderer, sph.quadrature_rel(gpu_lib, orc)))
