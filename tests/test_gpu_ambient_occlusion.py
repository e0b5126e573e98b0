"""PBRT-v4's ambient occlusion integrator on the device (SHM_INTEGRATOR_AMBIENT_OCCLUSION: k_shade_ao in render_batch's loop) against the CPU chain
of tests/ao_cases.py — twin camera rays, the oracle's two traversals, shm_ao_samples_host, the film's rule — bit for bit, films and counters; its invariance under how
a render is cut into calls; the passes behind the film on an AO film; and what it leaves behind for the other integrators. Films of 37 x 27: partial tiles and waves."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import ao_cases as ao
import oracle_py
import temporal_cases as tc
from shimmer_amd import abi, render, scenes

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
W, H, SPP = 37, 27, 5

# scene class -> (generator, disable_reference_quirks, the finite distance: some occlusion rays must end before the occluder they would otherwise hit)
SCENES = {
    "cornell": (lambda lib: scenes.cornell_box(lib, W, H), False, 0.5),
    "three_spheres": (lambda lib: scenes.three_spheres(lib, W, H, camera=(0.0, 0.0, 8.0)), False, 2.5),
    "patches": (lambda lib: scenes.cornell_box(lib, W, H, patches=True, patch_skew=0.1), False, 0.5),
    "quadrics": (lambda lib: scenes.quadric_scene(lib, width=W, height=H), False, 0.3),
    "instanced": (lambda lib: scenes.instanced_scene(lib, W, H), False, 0.5),
    "instanced_strict": (lambda lib: scenes.instanced_scene(lib, W, H), True, 0.5),
    "cutout": (lambda lib: scenes.cutout_scene(lib, width=W, height=H), False, 0.4),
    "fuzz1": (lambda lib: scenes.random_scene(lib, 1, W, H), False, 0.5),
    "fuzz2": (lambda lib: scenes.random_scene(lib, 2, W, H), False, 0.5),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_film_and_counters_equal_the_cpu_chain(gpu_lib, name):
    make, quirks_off, distance = SCENES[name]
    sc = make(gpu_lib)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        for sampler in ("independent", "zsobol"):
            for uniform in (False, True):
                chains = {}
                for d in (0.0, distance):
                    params = ao.params_for(sampler, spp=SPP, uniform=uniform, max_distance=d, reference_quirks=not quirks_off)
                    ch = chains[d] = ao.Chain(gpu_lib, sc.desc, params)
                    film, stats = r.render(params)
                    case = (name, sampler, uniform, d)
                    assert film.tobytes() == ch.film().tobytes(), case
                    assert not ao.stats_equal(stats, ch.stats), (case, ao.stats_equal(stats, ch.stats))
                    assert stats["paths"] == stats["rays_closest"] == W * H * SPP and stats["rays_any"] == int(ch.queued.sum())
                # the finite distance does both: it ends some rays before the occluder they hit when unbounded, and leaves others occluded
                inf, fin = chains[0.0], chains[distance]
                assert np.array_equal(inf.occ_rays[:, :6], fin.occ_rays[:, :6])
                assert (inf.occluded & ~fin.occluded).any() and fin.occluded.any(), (name, sampler, uniform)
    finally:
        r.close()


def test_decomposition_invariance(gpu_lib):
    sc = scenes.cornell_box(gpu_lib, W, H)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        for sampler in ("independent", "zsobol"):
            params = ao.params_for(sampler, spp=8, max_distance=0.8)
            r.clear()
            r.render_waves(params, waves=[(0, 8)])
            whole = r.read_film()
            assert whole.tobytes() == ao.Chain(gpu_lib, sc.desc, params).film().tobytes()
            r.clear()
            r.render_waves(params, waves=[(0, 3), (3, 8)])
            assert r.read_film().tobytes() == whole.tobytes()
            r.clear()
            tiles = list(range(r.n_tiles))
            r.render_waves(params, tile_indices=tiles[1::2], waves=[(0, 8)])
            r.render_waves(params, tile_indices=tiles[0::2], waves=[(0, 8)])
            assert r.read_film().tobytes() == whole.tobytes()
            for depth in (0, 1, 5):
                params.max_depth = depth
                film, stats = r.render(params)  # (the reference's wave schedule: 1, 1, 2, 4)
                assert film.tobytes() == whole.tobytes() and stats["rays_any"] > 0, depth
            r.clear()
            r.render_device(params)  # (the fused schedule)
            assert r.read_film().tobytes() == whole.tobytes()
        # the sharded entry point takes the integrator through shm_render_device: this rank's shard (all tiles in a world of one) and its gather
        r.render_sharded(params)
        assert r.read_film().tobytes() == whole.tobytes()
        assert gpu_lib.shm_dist_finalize(r.handle) == 0
        # ... and the two shards a world of two would own (shm_shard_tiles), rendered one after the other, add up to the same film
        r.clear()
        shards = [render.shard_tiles(r.n_tiles, r.tiles_per_row, rank, 2, lib=gpu_lib) for rank in (0, 1)]
        assert sorted(int(i) for sh in shards for i in sh) == list(range(r.n_tiles)) and all(len(sh) for sh in shards)
        for sh in shards:
            r.render_device(params, tile_indices=list(sh))
        assert r.read_film().tobytes() == whole.tobytes()
    finally:
        r.close()


def test_the_passes_behind_the_film_take_an_ao_film(gpu_lib):
    """Moments, denoiser, temporal accumulation under a moved camera and the display pass on an AO film, each against its own CPU twin fed with that film."""
    lib = gpu_lib
    sc = scenes.cornell_box(lib, W, H)
    white = render.gbuffer_white(lib, sc.desc)
    params = ao.params_for("zsobol", spp=8, max_distance=1.0)
    r = render.Renderer(lib, sc.desc)
    try:
        # moments: four batches of two samples
        ap = render.make_adaptive_params(lib, min_spp=4, batch_spp=2)
        r.clear()
        r.moments_clear()
        host = np.zeros((H, W), dtype=render.MOMENTS_DTYPE)
        for wave in ((0, 2), (2, 4), (4, 6), (6, 8)):
            r.render_waves(params, waves=[wave])
            err = r.moments_update(ap)
            want = render.moments_update_host(lib, r.read_film(), host, r.tiles, ap, n_tiles=r.n_tiles)
            assert err.tobytes() == want.tobytes() and r.read_moments().tobytes() == host.tobytes()
        film = r.read_film()
        assert film.tobytes() == ao.Chain(lib, sc.desc, params).film().tobytes()
        # the denoiser
        g, _ = r.gbuffer(params)
        assert r.denoise().tobytes() == render.denoise_host(lib, film, g, white).tobytes()
        # temporal accumulation: the scene's camera, then an orbit
        r.temporal_clear()
        r.temporal_accumulate()
        rec1, out1 = render.temporal_accumulate_host(lib, film, g, white, sc.desc.camera)
        assert r.read_temporal_history().tobytes() == rec1.tobytes() and r.read_temporal().tobytes() == out1.tobytes()
        view = tc.VIEWS["cornell"]
        cam2 = render.camera_in_scene(lib, sc.builder, *tc.orbit(view, 4.0), (0.0, 1.0, 0.0), fov=view[2])
        r.set_camera(cam2)
        film2, _ = r.render(params)
        g2, _ = r.gbuffer(params)
        assert film2.tobytes() != film.tobytes()
        r.temporal_accumulate()
        rec2, out2 = render.temporal_accumulate_host(lib, film2, g2, white, cam2, history=rec1, previous_camera=sc.desc.camera)
        assert r.read_temporal_history().tobytes() == rec2.tobytes() and r.read_temporal().tobytes() == out2.tobytes()
        assert (rec2["length"] > 1).any()  # some history survived the reprojection
        # the display pass, auto-exposed, over the film and over the temporal result
        for source, src_film in ((abi.SHM_DISPLAY_SOURCE_FILM, film2), (abi.SHM_DISPLAY_SOURCE_TEMPORAL, out2)):
            dp = render.make_display_params(lib, source=source, auto_exposure=1)
            r.display_clear()
            image, state = r.display(dp, return_state=True)
            want_image, counts, want_state = render.display_host(lib, src_film, W, H, dp)
            assert image.tobytes() == want_image.tobytes() and r.read_display_histogram().tobytes() == counts.tobytes() and state == want_state.as_dict()
            assert image[..., :3].max() > 0
    finally:
        r.close()


def test_the_other_integrators_after_an_ao_render(gpu_lib):
    """A path render (and a simple-path one) of a ShmScene that has just rendered AO equals the oracle byte for byte — nothing of the shadow buffers or the queues
    leaks — and with the AO fields set to valid garbage too."""
    sc = scenes.cornell_box(gpu_lib, W, H, glass=True, mix=True)
    o = oracle_py.Oracle(sc.desc)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        for integrator in ("path", "simplepath"):
            r.render(ao.params_for("zsobol", spp=SPP, uniform=True, max_distance=0.7))
            params = render.make_params(seed=9, spp=3, max_depth=4, integrator=integrator, ao_uniform_sample=True, ao_max_distance=0.37)
            film, stats = r.render(params)
            plain = render.make_params(seed=9, spp=3, max_depth=4, integrator=integrator)
            want, want_stats = o.render(plain, n_threads=8)
            assert film.tobytes() == want.tobytes(), integrator
            assert stats["rays_closest"] == want_stats["rays_closest"] and stats["rays_any"] == want_stats["rays_any"]
    finally:
        r.close()
        o.close()


def test_dispatch_checks(gpu_lib):
    lib = gpu_lib
    sc = scenes.cornell_box(lib, 16, 12)
    r = render.Renderer(lib, sc.desc)
    try:
        stats = abi.ShmStats()
        args = (r.tiles, r.n_tiles, 0, 1, C.byref(stats))
        for bad in (-1.0, float("nan")):
            p = ao.params_for(max_distance=bad)
            assert lib.shm_render_wave(r.handle, C.byref(p), *args) == -1 and b"ao_max_distance" in lib.shm_last_error()
            p.integrator = abi.SHM_INTEGRATOR_PATH  # ... which no other integrator reads
            assert lib.shm_render_wave(r.handle, C.byref(p), *args) == 0
        p = ao.params_for()
        p.integrator = 9
        assert lib.shm_render_wave(r.handle, C.byref(p), *args) == -2 and b"unknown integrator" in lib.shm_last_error()
    finally:
        r.close()
    keep = sc.desc.color_space.illuminant
    sc.desc.color_space.illuminant = None
    r = render.Renderer(lib, sc.desc)
    sc.desc.color_space.illuminant = keep
    try:
        p = ao.params_for()
        assert lib.shm_render_wave(r.handle, C.byref(p), r.tiles, r.n_tiles, 0, 1, None) == -1 and b"illuminant" in lib.shm_last_error()
        assert r.render(render.make_params(spp=1))[0]["rgb_sum"].sum() > 0  # the scene itself is fine
    finally:
        r.close()


def test_the_example_scene_renders(gpu_lib):
    lib = gpu_lib
    out = C.POINTER(abi.ShmPbrtScene)()
    abi.check(lib, lib.shm_scene_load_pbrt(str(ROOT / "examples" / "scenes" / "integrators" / "ambient_occlusion.pbrt").encode(), C.byref(out)), "ambient_occlusion.pbrt")
    try:
        s = out.contents
        params = abi.ShmRenderParams.from_buffer_copy(bytes(s.params))
        params.samples_per_pixel = 4
        r = render.Renderer(lib, s.desc)
        try:
            film, stats = r.render(params)
        finally:
            r.close()
        assert film.tobytes() == ao.Chain(lib, s.desc, params).film().tobytes()
        assert stats["rays_any"] > 0 and film["rgb_sum"].sum() > 0 and np.all(film["weight_sum"] == 4.0)
    finally:
        lib.shm_pbrt_free(out)
