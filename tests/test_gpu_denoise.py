"""The denoiser on the device (shm_denoise*) against its CPU twin, bit for bit — the twin fed with the film and the G-buffer read back from the same
scene — and against a 1024-spp render: does it denoise. Films: 24 x 20 at 3 spp (every pixel of the last two iterations has taps outside the film) and one 70 x 45."""
import ctypes as C

import numpy as np
import pytest

import gbuffer_cases as gc
from shimmer_amd import abi, render, scenes

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT = -1  # SHM_ERR_INVALID_ARGUMENT (include/shimmer_hip.h)


def _film(filt):
    return None if filt == "box" else {"filter": filt}


SCENES = {
    "cornell": lambda lib, w, h, film: scenes.cornell_box(lib, w, h, film=film),
    "coated": lambda lib, w, h, film: scenes.cornell_box(lib, w, h, coated=True, glass_too=True, film=film),
    "textured": lambda lib, w, h, film: scenes.cornell_box(lib, w, h, textured=True, film=film),
    "escaped": lambda lib, w, h, film: scenes.three_spheres(lib, w, h, camera=(0.0, 0.0, 8.0), environment=scenes.environment_image(16), film=film),  # seen from outside: rays pass between the spheres
}
# (the first three are gbuffer_cases' rows of those names, at a size of this suite's choosing)

# (scene, sampler, filter, iterations, demodulate, width, height): the whole product at 24 x 20, and the 70 x 45 film — several workgroups both ways, a multiple of
# nothing — with and without pass-through pixels
ROWS = [(sc, sa, f, it, dm, 24, 20) for sc in SCENES for sa in gc.SAMPLERS for f in ("box", "mitchell") for it in (1, 5) for dm in (0, 1)]
ROWS += [("cornell", "independent", "box", 5, 1, 70, 45), ("escaped", "zsobol", "mitchell", 5, 1, 70, 45)]


def _differing(a, b):
    return np.flatnonzero((np.ascontiguousarray(a).view(np.uint64).reshape(-1, 4) != np.ascontiguousarray(b).view(np.uint64).reshape(-1, 4)).any(axis=1))


@pytest.mark.parametrize("scene,sampler,filt,iterations,demodulate,w,h", ROWS, ids=lambda v: str(v))
def test_device_matches_the_host_twin_bit_for_bit(gpu_lib, scene, sampler, filt, iterations, demodulate, w, h):
    sc = SCENES[scene](gpu_lib, w, h, _film(filt))
    params = gc.params_for(sampler)
    d = render.make_denoise_params(gpu_lib, iterations=iterations, demodulate=demodulate)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        film, _ = r.render(params)
        g, _ = r.gbuffer(params)
        got = r.denoise(d)
        want = render.denoise_host(gpu_lib, film, g, render.gbuffer_white(gpu_lib, sc.desc), d)
        bad = _differing(got, want)
        assert bad.size == 0, (scene, sampler, filt, iterations, demodulate, bad[:8], got.ravel()[bad[:1]], want.ravel()[bad[:1]])
        covered = (g["weight_hit"] > 0) & (film["weight_sum"] > 0)
        assert covered.any(), "no pixel has a guide: the case checks nothing"
        assert _differing(got, film).size > 0 and np.isfinite(got["rgb_sum"][covered]).all()
        if scene == "escaped":
            assert (~covered).any(), "no pass-through pixel"
            c = render.film_to_rgb(film)
            assert np.array_equal(got["rgb_sum"].astype(np.float32)[~covered].view(np.uint32), c[~covered].view(np.uint32))
        if filt == "mitchell":  # the signed path: one sample per pixel shows the weight's magnitude, and some pixel's three samples do not add up to three of it
            r.gbuffer_clear()
            r.gbuffer_wave(params, 0, 1)
            one = np.abs(r.read_gbuffer()["weight_sum"])
            assert one.min() > 0 and np.allclose(one, one.max(), rtol=1e-6, atol=0), "a sample's filter weight is not plus or minus one constant"
            assert (g["weight_hit"] <= 0).any() or (g["weight_sum"] < gc.SPP * one.max() * (1 - 1e-6)).any(), "no negative filter weight among the samples"
    finally:
        r.close()


@pytest.mark.parametrize("scene", ["cornell", "textured"])
def test_denoise_leaves_its_inputs_alone(gpu_lib, scene):
    sc = SCENES[scene](gpu_lib, 24, 20, None)
    params = gc.params_for("independent")
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        film, _ = r.render(params)
        g, _ = r.gbuffer(params)
        first = r.denoise()
        assert r.read_film().tobytes() == film.tobytes(), "the denoiser wrote into the film"
        assert r.read_gbuffer().tobytes() == g.tobytes(), "the denoiser wrote into the G-buffer"
        assert r.denoise().tobytes() == first.tobytes()
        again, _ = r.render(params)
        assert again.tobytes() == film.tobytes()
        assert r.denoise().tobytes() == first.tobytes()
    finally:
        r.close()


def test_rejections(gpu_lib):
    sc = SCENES["cornell"](gpu_lib, 24, 20, None)
    params = gc.params_for()
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        r.render(params)
        d = render.make_denoise_params(gpu_lib)
        ms = C.c_double(0.0)
        assert gpu_lib.shm_denoise_device(r.handle, C.byref(d), C.byref(ms)) == INVALID_ARGUMENT and b"G-buffer" in gpu_lib.shm_last_error()
        r.gbuffer(params)
        assert gpu_lib.shm_denoise_device(r.handle, C.byref(d), None) == 0
        r.gbuffer_clear()
        assert gpu_lib.shm_denoise_device(r.handle, C.byref(d), C.byref(ms)) == INVALID_ARGUMENT and b"G-buffer" in gpu_lib.shm_last_error()
        r.gbuffer_wave(params, 0, 1)
        bad = render.make_denoise_params(gpu_lib, iterations=9)
        assert gpu_lib.shm_denoise_device(r.handle, C.byref(bad), C.byref(ms)) == INVALID_ARGUMENT and b"iterations" in gpu_lib.shm_last_error()
        with pytest.raises(abi.ShimmerHipError, match="sigma_plane"):
            r.denoise(render.make_denoise_params(gpu_lib, sigma_plane=0.0))
        assert gpu_lib.shm_denoise_device(r.handle, C.byref(d), C.byref(ms)) == 0 and ms.value > 0.0
    finally:
        r.close()


_TRUTH = {}


def _mse_case(lib, textured):
    """(noisy, truth, renderer kept open for the denoiser, coverage mask) of the 64 x 64 Cornell box at 4 spp, zsobol, depth 5; the truth is 1024 spp of the same scene."""
    sc = scenes.cornell_box(lib, 64, 64, textured=textured)
    r = render.Renderer(lib, sc.desc)
    if textured not in _TRUTH:
        truth_film, _ = r.render(render.make_params(seed=3, spp=1024, max_depth=5, sampler="zsobol"))
        _TRUTH[textured] = render.film_get_image(lib, truth_film, render.SRGB_FROM_XYZ).astype(np.float64)
    p = render.make_params(seed=7, spp=4, max_depth=5, sampler="zsobol")
    film, _ = r.render(p)
    g, _ = r.gbuffer(p)
    return r, film, g, _TRUTH[textured]


@pytest.mark.parametrize("textured", [False, True], ids=["cornell", "textured"])
def test_it_denoises(gpu_lib, textured):
    """MSE(denoised, truth) < MSE(noisy, truth) on the output-matrix image over the pixels with coverage; the textured box with demodulate = 1 (the default)."""
    r, film, g, truth = _mse_case(gpu_lib, textured)
    try:
        covered = g["weight_hit"] > 0
        assert covered.mean() > 0.5
        mse = lambda f: float(((render.film_get_image(gpu_lib, f, render.SRGB_FROM_XYZ).astype(np.float64) - truth)[covered] ** 2).mean())
        noisy, den = mse(film), mse(r.denoise(render.make_denoise_params(gpu_lib, demodulate=1)))
        flat = mse(r.denoise(render.make_denoise_params(gpu_lib, demodulate=0)))
        print(f"{'textured' if textured else 'cornell'} 64x64 4 spp: MSE noisy {noisy:.5e}, denoised {den:.5e} (ratio {den / noisy:.4f}), demodulate 0 {flat:.5e} "
              f"(ratio {flat / noisy:.4f}; demodulate 1 / 0 = {den / flat:.4f})")
        assert den < noisy
    finally:
        r.close()


def test_render_denoised_is_render_gbuffer_and_denoise(gpu_lib):
    sc = SCENES["textured"](gpu_lib, 24, 20, None)
    params = gc.params_for("zsobol")
    d = render.make_denoise_params(gpu_lib, iterations=3)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        res = render.render_denoised(gpu_lib, sc.desc, params, d, matrix=render.SRGB_FROM_XYZ, renderer=r)
        assert res["denoised"].tobytes() == r.denoise(d).tobytes()  # (the renderer still holds the film and the G-buffer of the call)
        assert res["film"].tobytes() == r.read_film().tobytes() and res["gbuffer"].tobytes() == r.read_gbuffer().tobytes()
        assert np.array_equal(res["image"], render.film_get_image(gpu_lib, res["denoised"], render.SRGB_FROM_XYZ))
        assert np.array_equal(res["noisy"], render.film_get_image(gpu_lib, res["film"], render.SRGB_FROM_XYZ)) and not np.array_equal(res["image"], res["noisy"])
        assert res["denoise_ms"] > 0.0
    finally:
        r.close()
    own = render.render_denoised(gpu_lib, sc.desc, params, d)  # a scene of the call's own
    assert own["denoised"].tobytes() == res["denoised"].tobytes()


def test_the_example_writes_the_denoised_image(gpu_lib, tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "cornell.pfm"
    subprocess.run([sys.executable, os.path.join(root, "examples", "render_scene.py"), "cornell", "--spp", "16", "--res", "64", "--denoise", "-o", str(out)], check=True, timeout=120)
    for name in ("cornell.pfm", "cornell.png", "cornell.denoised.pfm", "cornell.denoised.png"):
        assert (tmp_path / name).stat().st_size > 0, name
    assert (tmp_path / "cornell.denoised.pfm").read_bytes() != out.read_bytes()
