"""The moments pass and the adaptive render on the device (shm_moments_*, shm_render_adaptive): the pass against its CPU twin bit for bit — the twin
fed with the film read back after every batch — the adaptive render against plain renders of the sample ranges it claims to have spent, and the variance against numpy's
over separately rendered one-sample films. Films: 24 x 20 (3 x 2.5 tiles: clipped edge tiles) and 70 x 45."""
import ctypes as C

import numpy as np
import pytest

import gbuffer_cases as gc
import moments_cases as mc
from shimmer_amd import abi, render, scenes

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT = -1  # SHM_ERR_INVALID_ARGUMENT (include/shimmer_hip.h)
SPP = 6


def _film(filt):
    return None if filt == "box" else {"filter": filt}


SCENES = {
    "cornell": lambda lib, w, h, film: scenes.cornell_box(lib, w, h, film=film),
    "coated": lambda lib, w, h, film: scenes.cornell_box(lib, w, h, coated=True, glass_too=True, film=film),
    "escaped": lambda lib, w, h, film: scenes.three_spheres(lib, w, h, camera=(0.0, 0.0, 8.0), environment=scenes.environment_image(16), film=film),
}
# (scene, sampler, filter, width, height, tile): the product at 24 x 20 under the renderer's 8x8 tiling; the 70 x 45 film; a 16x16 tiling of the caller's own, over which
# a wave's lanes stride four times (and twice, and once with idle lanes, over its clipped tiles)
ROWS = [(sc, sa, f, 24, 20, 8) for sc in SCENES for sa in gc.SAMPLERS for f in ("box", "mitchell")]
ROWS += [("cornell", "zsobol", "box", 70, 45, 8), ("escaped", "independent", "mitchell", 24, 20, 16)]


def _params(sampler, spp=SPP, seed=5):
    return render.make_params(seed=seed, spp=spp, max_depth=5, sampler=sampler)


@pytest.mark.parametrize("scene,sampler,filt,w,h,tile", ROWS, ids=lambda v: str(v))
def test_device_matches_the_host_twin_bit_for_bit(gpu_lib, scene, sampler, filt, w, h, tile):
    sc = SCENES[scene](gpu_lib, w, h, _film(filt))
    params = _params(sampler)
    batch = 1 if filt == "mitchell" else 2  # one sample a batch under the signed filter: some pixel's batch then has no positive weight
    a = render.make_adaptive_params(gpu_lib, min_spp=2 * batch, batch_spp=batch, threshold=0.1)
    boxes = mc.tile_boxes(w, h, tile)
    tiles = render.make_tiles(boxes)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        r.clear()
        r.moments_clear()
        twin = mc.clear(r.read_film())
        assert mc.same_bits(r.read_moments(), twin) and not twin.view(np.float64).any()
        skipped, prev_w = False, np.zeros((h, w))
        for b in range(SPP // batch):
            r.render_waves(params, waves=[(b * batch, (b + 1) * batch)])
            got = r.moments_update(a, tiles=tiles) if tile != 8 else r.moments_update(a)
            film = r.read_film()
            want = render.moments_update_host(gpu_lib, film, twin, tiles, a, n_tiles=len(boxes))
            assert mc.same_bits(got, want), (b, got[:4], want[:4])
            skipped = skipped or bool((film["weight_sum"] - prev_w <= 0).any())
            prev_w = film["weight_sum"]
        records = r.read_moments()
        bad = np.flatnonzero((records.view(np.uint64).reshape(-1, 12) != twin.view(np.uint64).reshape(-1, 12)).any(axis=1))
        assert bad.size == 0, (bad[:8], records.ravel()[bad[:1]], twin.ravel()[bad[:1]])
        assert (records["batches"] >= 2).any() and (records["m2"] > 0).any(), "nothing was measured: the case checks nothing"
        assert int(got["unconverged"].sum()) == int((~mc.converged(records, a.floor, a.threshold, 2)).sum())
        if filt == "mitchell":
            assert skipped and (records["batches"] < SPP).any(), "no batch had dw <= 0: the signed case checks nothing more than the box"
        else:
            assert (records["batches"] == SPP // batch).all()
    finally:
        r.close()


def test_the_pass_is_invisible_and_counts_from_its_clear(gpu_lib):
    sc = SCENES["cornell"](gpu_lib, 24, 20, None)
    params = _params("independent")
    a = render.make_adaptive_params(gpu_lib, min_spp=2, batch_spp=1)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        r.clear()
        r.render_waves(params, waves=[(0, 2), (2, 4), (4, 6)])
        plain = r.read_film()
        r.clear()
        r.moments_clear()
        for wave in [(0, 2), (2, 4)]:
            r.render_waves(params, waves=[wave])
            r.moments_update(a)
        first = r.read_moments()
        r.moments_clear()  # in the middle of a render: the records count from here
        mid = r.read_film()
        assert mc.same_bits(r.read_moments(), mc.clear(mid))
        r.render_waves(params, waves=[(4, 6)])
        r.moments_update(a)
        assert mc.same_bits(r.read_film(), plain), "the moments pass changed the film"
        m = r.read_moments()
        assert (first["batches"] == 2).all() and (m["batches"] == 1).all() and (m["weight"] == 2).all()
        assert np.allclose(m["mean"], (plain["rgb_sum"] - mid["rgb_sum"]) / 2.0, rtol=1e-12, atol=0)
    finally:
        r.close()


@pytest.mark.parametrize("sampler,cap", [("independent", 8), ("zsobol", 7)])
def test_threshold_zero_is_a_plain_render(gpu_lib, sampler, cap):
    """Nothing converges at threshold 0: every tile receives the cap, and the film is the plain render's — with a cap that is no multiple of batch_spp too."""
    sc = SCENES["cornell"](gpu_lib, 24, 20, None)
    params = _params(sampler, spp=cap)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        r.clear()
        r.render_device(params)
        plain = r.read_film()
        film, tile_spp, moments, stats = render.render_adaptive(gpu_lib, sc.desc, params, render.make_adaptive_params(gpu_lib, min_spp=4, batch_spp=2, threshold=0.0), renderer=r)
        assert mc.same_bits(film, plain) and (tile_spp == cap).all() and tile_spp.shape == (9,)
        assert stats["paths"] == 24 * 20 * cap and (moments["batches"] == (cap + 1) // 2).all() and (moments["weight"] == cap).all()
    finally:
        r.close()


def test_threshold_infinity_stops_at_min_spp(gpu_lib):
    sc = SCENES["coated"](gpu_lib, 24, 20, None)
    params = _params("zsobol", spp=16)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        r.clear()
        r.render_waves(params, waves=[(0, 6)])
        plain = r.read_film()
        tile_spp, stats = r.render_adaptive(params, render.make_adaptive_params(gpu_lib, min_spp=6, batch_spp=3, threshold=float("inf")))
        assert mc.same_bits(r.read_film(), plain) and (tile_spp == 6).all() and stats["paths"] == 24 * 20 * 6
    finally:
        r.close()


def test_it_adapts(gpu_lib):
    """A sphere on a floor under an area light, no environment: above the floor's far edge the camera rays escape into black, every batch of such a pixel is exactly 0 and
    its e2 exactly 0, so the tiles of the top corners stop at min_spp while lit tiles go on. Every tile holds the bits of a plain render of the samples it received."""
    w, h, cap = 70, 45, 16
    sc = scenes.sphere_light(gpu_lib, w, h)
    params = _params("independent", spp=cap)
    a = render.make_adaptive_params(gpu_lib, min_spp=4, batch_spp=2, threshold=0.3)  # (coarse, so that lit tiles stop at every stage between min_spp and the cap)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        film, tile_spp, moments, stats = render.render_adaptive(gpu_lib, sc.desc, params, a, renderer=r)
        print("tile_spp:", np.unique(tile_spp, return_counts=True))
        assert tile_spp.min() == 4 and tile_spp.max() > 4 and set(np.unique(tile_spp)) <= set(range(4, cap + 1, 2))
        assert ((tile_spp > 4) & (tile_spp < cap)).any(), "no tile stopped between min_spp and the cap: the comparison below sees the two plain renders only"
        per_pixel = render.tile_spp_image(tile_spp, w, h)
        assert np.array_equal(film["weight_sum"], per_pixel.astype(np.float64)), "a pixel's weight_sum is not its tile's spp (box filter)"
        assert stats["paths"] == int(per_pixel.sum())
        black = (film["rgb_sum"] == 0).all(axis=-1)
        assert black[:8, :8].all() and not black.all()
        assert (per_pixel[:8, :8] == 4).all(), "a tile of unlit background went on past min_spp"
        res = render.moments_resolve(gpu_lib, moments, a.floor)
        assert not res["e2"][:8, :8].any() and (res["e2"][per_pixel > 4] >= 0).all()
        for s in np.unique(tile_spp):
            r.clear()
            r.render_waves(params, waves=[(0, int(s))])
            plain = r.read_film()
            here = per_pixel == s
            assert mc.same_bits(film[here], plain[here]), f"tiles that stopped at {s} differ from a plain render of [0, {s})"
        r.clear()
        r.render_device(params)
        capped = per_pixel == cap
        if capped.any():
            assert mc.same_bits(film[capped], r.read_film()[capped])
        # a tile that stopped below the cap is converged in every pixel (its records were not touched since)
        assert mc.converged(moments, a.floor, a.threshold, 2)[per_pixel < cap].all()
    finally:
        r.close()


def test_the_variance_is_a_variance(gpu_lib):
    """s2 of a batch_spp = 1 moments run over N = 16 samples against numpy's var(ddof = 1) of the same 16 samples rendered as separate one-sample films (box filter: a
    one-sample film's rgb_sum is the sample itself, x_b).
    Tolerance, per pixel and channel, with SS = sum (x_b - m)^2 and eps = 2^-53. The pass sees x_b' = F_b - F_(b-1): F_b carries the rounding of its own accumulation, at
    most eps |F_b| <= eps sum |x_b|, and the subtraction rounds once more, so |x_b' - x_b| <= delta = 2 eps sum |x_b| (the cancellation in F - prev: the error is relative
    to the film's sum, not to the batch). Perturbing every x_b by at most delta moves SS by at most 2 delta sum |x_b - m| + N delta^2 <= 2 delta sqrt(N SS) + N delta^2.
    The recurrence itself is within 16 N eps sum x_b^2 of the exact SS of what it was given (tests/test_moments.py derives that), and numpy's two-pass variance within the
    same bound. Divided by N - 1."""
    N = 16
    sc = SCENES["cornell"](gpu_lib, 24, 20, None)
    params = _params("independent", spp=N)
    a = render.make_adaptive_params(gpu_lib, min_spp=2, batch_spp=1)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        xs = []
        for b in range(N):
            r.clear()
            r.render_waves(params, waves=[(b, b + 1)])
            f = r.read_film()
            assert (f["weight_sum"] == 1.0).all()
            xs.append(f["rgb_sum"].copy())
        xs = np.array(xs)
        r.clear()
        r.moments_clear()
        for b in range(N):
            r.render_waves(params, waves=[(b, b + 1)])
            r.moments_update(a)
        m = r.read_moments()
    finally:
        r.close()
    assert (m["batches"] == N).all() and (m["weight"] == N).all()
    s2 = m["m2"] / (N - 1.0)
    want = xs.var(axis=0, ddof=1)
    ss = ((xs - xs.mean(axis=0)) ** 2).sum(axis=0)
    delta = 2 * mc.EPS * np.abs(xs).sum(axis=0)
    tol = (2 * delta * np.sqrt(N * ss) + N * delta ** 2 + 32 * N * mc.EPS * (xs ** 2).sum(axis=0)) / (N - 1)
    print("variance: max |s2 - var| / tol =", float(np.max(np.abs(s2 - want) / np.where(tol > 0, tol, 1.0))), "; max relative", float(np.max(np.abs(s2 - want) / np.where(want > 0, want, 1.0))))
    assert (np.abs(s2 - want) <= tol).all()
    assert (want > 0).mean() > 0.9 and np.allclose(m["mean"], xs.mean(axis=0), rtol=1e-12, atol=0)
    res = render.moments_resolve(gpu_lib, m, a.floor)
    assert np.allclose(res["s2"], want, rtol=1e-6) and np.allclose(res["v"], want / N, rtol=1e-6)


# ---- the denoiser's measured variance source (ShmDenoiseParams::variance_source) ----
DENOISE_SCENES = dict(SCENES, textured=lambda lib, w, h, film: scenes.cornell_box(lib, w, h, textured=True, film=film))
# the denoise suite's 24 x 20 rows — scene x sampler x filter x iterations x demodulate — under the measured source
DENOISE_ROWS = [(sc, sa, f, it, dm) for sc in ("cornell", "coated", "textured", "escaped") for sa in gc.SAMPLERS for f in ("box", "mitchell") for it in (1, 5) for dm in (0, 1)]


@pytest.mark.parametrize("scene,sampler,filt,iterations,demodulate", DENOISE_ROWS, ids=lambda v: str(v))
def test_measured_variance_device_matches_the_host_twin_bit_for_bit(gpu_lib, scene, sampler, filt, iterations, demodulate):
    sc = DENOISE_SCENES[scene](gpu_lib, 24, 20, _film(filt))
    params = gc.params_for(sampler)
    a = render.make_adaptive_params(gpu_lib, min_spp=2, batch_spp=1, threshold=0.0)
    measured = render.make_denoise_params(gpu_lib, iterations=iterations, demodulate=demodulate, variance_source=abi.SHM_DENOISE_VARIANCE_MEASURED)
    spatial = render.make_denoise_params(gpu_lib, iterations=iterations, demodulate=demodulate)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        plain, _ = r.render(params)
        r.clear()
        r.moments_clear()
        for b in range(gc.SPP):  # one sample a batch: the records of a plain render
            r.render_waves(params, waves=[(b, b + 1)])
            r.moments_update(a)
        film, m = r.read_film(), r.read_moments()
        assert mc.same_bits(film, plain)
        g, _ = r.gbuffer(params)
        white = render.gbuffer_white(gpu_lib, sc.desc)
        got = r.denoise(measured)
        want = render.denoise_host(gpu_lib, film, g, white, measured, moments=m)
        assert mc.same_bits(got, want)
        # the spatial source is what it was: the twin without records, whatever records the scene holds
        base = r.denoise(spatial)
        assert mc.same_bits(base, render.denoise_host(gpu_lib, film, g, white, spatial))
        covered = (g["weight_hit"] > 0) & (film["weight_sum"] > 0) & (m["batches"] >= 2)
        assert covered.any() and not mc.same_bits(got, base), "the measured source changed nothing: the case checks nothing"
    finally:
        r.close()


def test_measured_variance_needs_moments(gpu_lib):
    sc = SCENES["cornell"](gpu_lib, 24, 20, None)
    params = gc.params_for()
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        r.render(params)
        r.gbuffer(params)
        with pytest.raises(abi.ShimmerHipError, match="no moments"):
            r.denoise(render.make_denoise_params(gpu_lib, variance_source=abi.SHM_DENOISE_VARIANCE_MEASURED))
        with pytest.raises(abi.ShimmerHipError, match="unknown variance_source"):
            r.denoise(render.make_denoise_params(gpu_lib, variance_source=2))
        base = r.denoise()
        r.moments_clear()  # records without a batch: every pixel keeps the spatial estimate
        assert mc.same_bits(r.denoise(render.make_denoise_params(gpu_lib, variance_source=abi.SHM_DENOISE_VARIANCE_MEASURED)), base)
    finally:
        r.close()


def test_rejections(gpu_lib):
    sc = SCENES["cornell"](gpu_lib, 24, 20, None)
    params = _params("independent", spp=8)
    a = render.make_adaptive_params(gpu_lib)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        out = np.zeros(r.n_tiles, render.TILE_ERROR_DTYPE)
        rec = np.zeros((20, 24), render.MOMENTS_DTYPE)
        upd = lambda ap, tiles=r.tiles, n=r.n_tiles: gpu_lib.shm_moments_update(r.handle, tiles, n, C.byref(ap), out.ctypes.data_as(C.c_void_p))
        assert upd(a) == INVALID_ARGUMENT and b"shm_moments_clear" in gpu_lib.shm_last_error()
        assert gpu_lib.shm_moments_read(r.handle, rec.ctypes.data_as(C.c_void_p)) == INVALID_ARGUMENT and b"shm_moments_clear" in gpu_lib.shm_last_error()
        r.moments_clear()
        assert upd(a) == 0
        assert upd(render.make_adaptive_params(gpu_lib, min_spp=10)) == INVALID_ARGUMENT and b"multiple" in gpu_lib.shm_last_error()
        assert upd(a, render.make_tiles([(0, 0, 8, 8), (7, 7, 9, 9)]), 2) == INVALID_ARGUMENT and b"overlap" in gpu_lib.shm_last_error()
        assert upd(a, render.make_tiles([(16, 16, 24, 21)]), 1) == INVALID_ARGUMENT and b"outside" in gpu_lib.shm_last_error()
        assert upd(a, n=0) == INVALID_ARGUMENT
        with pytest.raises(abi.ShimmerHipError, match="below min_spp"):
            r.render_adaptive(params, a)  # the cap, 8, is below min_spp, 16
        with pytest.raises(abi.ShimmerHipError, match="threshold"):
            r.render_adaptive(params, render.make_adaptive_params(gpu_lib, min_spp=4, batch_spp=2, threshold=-1.0))
        tile_spp, _ = r.render_adaptive(params, render.make_adaptive_params(gpu_lib, min_spp=8, batch_spp=4))  # cap == min_spp: the base batches and no round
        assert (tile_spp == 8).all()
        # tile_spp_out and stats may be NULL
        assert gpu_lib.shm_render_adaptive(r.handle, C.byref(params), r.tiles, r.n_tiles, C.byref(render.make_adaptive_params(gpu_lib, min_spp=4, batch_spp=2)), None, None) == 0
    finally:
        r.close()


def test_the_example_writes_the_sample_count_and_the_variance(gpu_lib, tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "cornell.pfm"
    subprocess.run([sys.executable, os.path.join(root, "examples", "render_scene.py"), "cornell", "--spp", "16", "--res", "64", "--adaptive", "0.1", "--min-spp", "4",
                    "--batch-spp", "2", "--denoise", "-o", str(out)], check=True, timeout=120)
    for name in ("cornell.pfm", "cornell.png", "cornell.spp.pfm", "cornell.variance.pfm", "cornell.denoised.pfm"):
        assert (tmp_path / name).stat().st_size > 0, name
