"""The G-buffer pass on the device (shm_gbuffer_*) against its CPU twin, bit for bit.

The expected value of a pixel is built from the host twin: its camera rays, traced by the GPU's own shm_trace_closest, fed back into shm_gbuffer_samples_host — the same
shared arithmetic (shm/gbuffer.h) compiled for the host — and added in sample order in float64. Film 24 x 20 (no multiple of a tile), 3 samples per pixel."""
import ctypes as C

import numpy as np
import pytest

import gbuffer_cases as gc
from shimmer_amd import abi, render

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT = -1  # SHM_ERR_INVALID_ARGUMENT (include/shimmer_hip.h)


def _expected(lib, r, sc, params, space):
    pix, idx = gc.all_samples(r.pixel_bounds, params.samples_per_pixel)
    rays = gc.twin_rays(lib, sc.desc, params, pix, idx)
    hits, _ = r.trace(rays)
    return gc.twin_samples(lib, sc.desc, params, space, pix, idx, hits), hits


@pytest.mark.parametrize("scene,sampler,filt,space", gc.gpu_rows(), ids=lambda v: str(v))
def test_gbuffer_matches_the_host_twin_bit_for_bit(gpu_lib, scene, sampler, filt, space):
    sc = gc.make_scene(gpu_lib, scene, filt)
    params = gc.params_for(sampler)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        samples, hits = _expected(gpu_lib, r, sc, params, space)
        want = gc.pixel_sums(samples, r.width * r.height, gc.SPP)
        g, stats = r.gbuffer(params, space=space)
        got = gc.gbuffer_as_rows(g)
        assert (hits["prim"] >= 0).any(), "the scene is out of the camera's sight: the case checks nothing"
        assert stats["rays_closest"] == r.width * r.height * gc.SPP and stats["paths"] == stats["rays_closest"]
        assert np.isfinite(got).all()
        bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
        assert bad.size == 0, (scene, sampler, filt, space, bad[:8], got[bad[:1]], want[bad[:1]])
        if filt == "mitchell":
            assert (samples[:, 15] < 0).any(), "no negative filter weight among the samples: the signed path is not exercised"
    finally:
        r.close()


@pytest.mark.parametrize("scene", ["cornell", "textured"])
def test_wave_split_and_tile_split_equal_one_call(gpu_lib, scene):
    sc = gc.make_scene(gpu_lib, scene, "mitchell")
    params = gc.params_for("zsobol")
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        whole, _ = r.gbuffer(params)
        r.gbuffer_clear()
        r.gbuffer_wave(params, 0, 1)
        r.gbuffer_wave(params, 1, 3)
        waves = r.read_gbuffer()
        assert whole.tobytes() == waves.tobytes()
        r.gbuffer_clear()
        odd, even = list(range(1, r.n_tiles, 2)), list(range(0, r.n_tiles, 2))
        r.gbuffer_wave(params, 0, 3, tile_indices=odd)
        part = r.read_gbuffer()
        assert part.tobytes() != whole.tobytes()
        r.gbuffer_wave(params, 0, 3, tile_indices=even)
        assert r.read_gbuffer().tobytes() == whole.tobytes()
    finally:
        r.close()


@pytest.mark.parametrize("scene", ["cornell", "textured"])
def test_a_batched_pass_equals_the_unbatched_one(gpu_lib, monkeypatch, scene):
    """The pass's batch loop, more than once round: 40 x 36 x 3 = 4 320 paths against a workspace of 4 096 (SHM_BATCH_PATHS) are two batches, of 1 344 pixels (1 365
    rounded down to whole 8 x 8 tiles) and of 96. Mitchell's signed weights are indexed by path slot, and a slot depends on its batch's pixel count; the textured box
    runs the HAS_TEX K1 with its auxiliary rays."""
    sc = gc.make_scene(gpu_lib, scene, "mitchell", size=(40, 36))
    params = gc.params_for("zsobol")
    monkeypatch.delenv("SHM_BATCH_PATHS", raising=False)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        whole, _ = r.gbuffer(params)
    finally:
        r.close()
    monkeypatch.setenv("SHM_BATCH_PATHS", "4096")
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        batched, stats = r.gbuffer(params)
    finally:
        r.close()
    assert gc.gbuffer_as_rows(whole).any()
    assert batched.tobytes() == whole.tobytes()
    assert stats["paths"] == stats["rays_closest"] == 4320


@pytest.mark.parametrize("scene", ["cornell", "coated", "textured"])
def test_a_gbuffer_pass_leaves_the_beauty_render_alone(gpu_lib, scene):
    sc = gc.make_scene(gpu_lib, scene)
    params = gc.params_for("independent")
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        before, _ = r.render(params)
        r.gbuffer(params, space=abi.SHM_GBUFFER_SPACE_CAMERA)
        assert r.read_film().tobytes() == before.tobytes(), "the pass wrote into the film"
        after, _ = r.render(params)
        assert after.tobytes() == before.tobytes()
    finally:
        r.close()


def test_rejections(gpu_lib):
    sc = gc.make_scene(gpu_lib, "cornell")
    params = gc.params_for()
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        overlap = (abi.ShmTile * 2)(abi.ShmTile(0, 0, 8, 8), abi.ShmTile(4, 4, 12, 12))
        st = abi.ShmStats()
        rc = gpu_lib.shm_gbuffer_render_wave(r.handle, C.byref(params), abi.SHM_GBUFFER_SPACE_RENDER, overlap, 2, 0, 1, C.byref(st))
        assert rc == INVALID_ARGUMENT and b"overlap" in gpu_lib.shm_last_error()
        rc = gpu_lib.shm_gbuffer_render_wave(r.handle, C.byref(params), 2, r.tiles, r.n_tiles, 0, 1, C.byref(st))
        assert rc == INVALID_ARGUMENT and b"space" in gpu_lib.shm_last_error()
        outside = (abi.ShmTile * 1)(abi.ShmTile(16, 16, 32, 24))
        assert gpu_lib.shm_gbuffer_render_wave(r.handle, C.byref(params), 0, outside, 1, 0, 1, C.byref(st)) == INVALID_ARGUMENT
        # nothing was added by the refused calls
        assert not gc.gbuffer_as_rows(r.read_gbuffer()).any()
    finally:
        r.close()
