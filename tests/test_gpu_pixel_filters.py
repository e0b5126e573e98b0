"""The pixel filters on the device: films and counters bit for bit against the oracle in every scene class, ZSobol films equal to the oracle's and invariant under every decomposition of the
work, the probe's Filter::Sample against the host build of shm/filter.h, and the step-edge scene (signed weights, weight sums of either sign) against the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_py
import test_pixel_filters as pf
import zsobol_cases as zc
from shimmer_amd import abi, render, scene as scn, scenes
from test_gpu_zsobol import probe_op

pytestmark = pytest.mark.gpu
STATS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")
NEW_FILTERS = ("gaussian", "mitchell", "sinc", "triangle")
host_filter = pf.host_filter  # (the module's fixture: the g++ build of shm/filter.h)


def class_scene(lib, which, film):
    if which == "lean":  # the Cornell box: all-diffuse triangles, k_generate<., LEAN>
        return scenes.cornell_box(lib, 40, 40, film=film), 6, 5
    if which == "staged":  # the coated S3 proxy at small size
        return scenes.ganesha_proxy(lib, 48, 48, n=24, coated=True, film=film), 4, 5
    if which == "textured":  # the filter's offset feeds the camera ray's differentials
        return scenes.cornell_box(lib, 32, 32, textured=True, film=film), 4, 5
    if which == "environment":
        return scenes.three_spheres(lib, 40, 30, camera=(0.75, 0.5, 9.0), environment=scenes.environment_image(32), film=film), 4, 5
    return scenes.instanced_scene(lib, 40, 30, film=film), 4, 5


@pytest.mark.parametrize("which", ["lean", "staged", "textured", "environment", "instances"])
@pytest.mark.parametrize("name", NEW_FILTERS)
def test_film_and_counters_equal_the_oracle(gpu_lib, name, which):
    sc, spp, depth = class_scene(gpu_lib, which, dict(filter=name))
    p = render.make_params(seed=13, spp=spp, max_depth=depth)
    gpu = render.Renderer(gpu_lib, sc.desc, 0)
    f_gpu, s_gpu = gpu.render(p)
    gpu.close()
    orc = oracle_py.Oracle(sc.desc)
    f_cpu, s_cpu = orc.render(p, n_threads=os.cpu_count() or 1)
    orc.close()
    for field in ("rgb_sum", "weight_sum"):
        assert np.array_equal(f_gpu[field], f_cpu[field]), (name, which, field)
    for k in STATS:
        assert s_gpu[k] == s_cpu[k], (name, which, k)
    box, _, _ = class_scene(gpu_lib, which, None)
    gpu = render.Renderer(gpu_lib, box.desc, 0)
    f_box, _ = gpu.render(p)
    gpu.close()
    assert (f_box["weight_sum"] == spp).all() and not np.array_equal(f_box["rgb_sum"], f_gpu["rgb_sum"])  # (the filter is used)


@pytest.mark.parametrize("name", NEW_FILTERS)
def test_without_pixel_jitter_the_device_film_is_the_box_film(gpu_lib, name):
    p = render.make_params(seed=13, spp=4, max_depth=4, disable_pixel_jitter=True)
    films = []
    for film in (None, dict(filter=name)):
        sc = scenes.cornell_box(gpu_lib, 24, 24, film=film)
        gpu = render.Renderer(gpu_lib, sc.desc, 0)
        films.append(gpu.render(p)[0])
        gpu.close()
    assert np.array_equal(films[0], films[1]) and (films[1]["weight_sum"] == 4).all()


@pytest.mark.parametrize("name", ["gaussian", "mitchell"])
def test_zsobol_filtered_film_decomposition_invariance(gpu_lib, monkeypatch, name):
    """The decomposition set of test_zsobol_film_decomposition_invariance under a pixel filter, and the film and counters of the oracle."""
    sc = scenes.ganesha_proxy(gpu_lib, 160, 120, n=64, film=dict(filter=name))
    p = render.make_params(seed=21, spp=12, max_depth=5, sampler="zsobol")
    gpu = render.Renderer(gpu_lib, sc.desc, 0)
    f1, s1 = gpu.render(p)
    f2, _ = gpu.render(p)
    assert np.array_equal(f1, f2)
    zc.assert_equals_oracle(sc.desc, p, f1, s1, name)
    f_ind, _ = gpu.render(render.make_params(seed=21, spp=12, max_depth=5))
    assert not np.array_equal(f1, f_ind)  # (the sampler is used ...)
    box = scenes.ganesha_proxy(gpu_lib, 160, 120, n=64)
    g_box = render.Renderer(gpu_lib, box.desc, 0)
    f_box, _ = g_box.render(p)
    g_box.close()
    assert not np.array_equal(f1["rgb_sum"], f_box["rgb_sum"]) and not np.array_equal(f1["weight_sum"], f_box["weight_sum"])  # (... and so is the filter)
    gpu.clear()
    idx = np.arange(gpu.n_tiles)
    for ws, we in scn.wave_schedule(12):
        gpu.render_waves(p, tile_indices=idx[idx % 3 != 0], waves=[(ws, we)])
        gpu.render_waves(p, tile_indices=idx[idx % 3 == 0], waves=[(ws, we)])
    assert np.array_equal(gpu.read_film(), f1)
    gpu.clear()
    gpu.render_device(p)
    assert np.array_equal(gpu.read_film(), f1)
    gpu.clear()
    uid = gpu.dist_unique_id()
    gpu.dist_init(0, 1, uid)
    gpu.render_sharded(p)
    assert np.array_equal(gpu.read_film(), f1)
    abi.check(gpu_lib, gpu_lib.shm_dist_finalize(gpu.handle), "shm_dist_finalize")
    gpu.close()
    for var, val in (("SHM_BATCH_PATHS", "8192"), ("SHM_OVERLAP_PATHS", "0")):
        monkeypatch.setenv(var, val)
        g = render.Renderer(gpu_lib, sc.desc, 0)
        f3, s3 = g.render(p)
        g.close()
        monkeypatch.delenv(var)
        assert np.array_equal(f3, f1), var
        assert s3["rays_any"] == s1["rays_any"], var


def probe_filter(plib, name, rx, ry, params, u):
    words = pf.filter_words(name, rx, ry, params, u)
    n_out = 3 * len(u)
    a = (C.c_uint32 * len(words))(*words)
    out = (C.c_uint32 * n_out)()
    res = C.c_int()
    abi.check(plib, plib.shm_debug_eval_leaf(0, probe_op("FILTER_SAMPLE"), a, len(words), out, n_out, C.byref(res)), "shm_debug_eval_leaf")
    assert res.value == len(u)
    w = np.frombuffer(out, np.uint32).view(np.float32).reshape(-1, 3)
    return w[:, :2].copy(), w[:, 2].copy()


def test_device_sampler_equals_the_host_build(gpu_lib, host_filter):
    plib = abi.load_probe_library()
    u = pf.draws()
    cases = list(pf.sampler_cases()) + [("triangle", 2.0, 2.0, ()), ("triangle", 1.25, 3.0, ()), ("box", 0.5, 0.5, ()), ("box", 0.75, 1.5, ())]
    for name, rx, ry, params in cases:
        _, p_host, w_host = host_filter(name, rx, ry, params, u)
        p_dev, w_dev = probe_filter(plib, name, rx, ry, params, u)
        assert np.array_equal(p_dev.view(np.uint32), p_host.view(np.uint32)), (name, rx, ry)
        assert np.array_equal(w_dev.view(np.uint32), w_host.view(np.uint32)), (name, rx, ry)


@pytest.mark.parametrize("name", list(pf.KIND))
def test_step_edge_on_the_device_equals_the_oracle(gpu_lib, name):
    """The scene of test_step_edge_is_the_scene_convolved_with_the_filter: orthographic camera, negative weights, pixels whose weight_sum is of either sign."""
    desc, keep = pf.step_edge_scene(gpu_lib, name)
    p = pf.edge_params()
    gpu = render.Renderer(gpu_lib, desc, 0)
    f_gpu, s_gpu = gpu.render(p)
    gpu.close()
    orc = oracle_py.Oracle(desc)
    f_cpu, s_cpu = orc.render(p, n_threads=os.cpu_count() or 1)
    orc.close()
    assert np.array_equal(f_gpu["rgb_sum"], f_cpu["rgb_sum"]) and np.array_equal(f_gpu["weight_sum"], f_cpu["weight_sum"])
    for k in STATS:
        assert s_gpu[k] == s_cpu[k], k
    if name in ("mitchell", "sinc"):
        col = pf.pooled_columns(f_gpu)
        assert col[14] < 0  # (the pixel column centred 1.2 px outside the edge)


def test_pbrt_file_with_a_gaussian_filter_renders_as_the_oracle(gpu_lib):
    out = C.POINTER(abi.ShmPbrtScene)()
    path = pf.ROOT / "examples" / "scenes" / "gaussian_filter.pbrt"
    abi.check(gpu_lib, gpu_lib.shm_scene_load_pbrt(str(path).encode(), C.byref(out)), "shm_scene_load_pbrt")
    ps = out.contents
    g = render.Renderer(gpu_lib, ps.desc, 0)
    f_gpu, _ = g.render(ps.params)
    g.close()
    orc = oracle_py.Oracle(ps.desc)
    f_cpu, _ = orc.render(ps.params, n_threads=os.cpu_count() or 1)
    orc.close()
    gpu_lib.shm_pbrt_free(out)
    assert np.array_equal(f_gpu, f_cpu)
