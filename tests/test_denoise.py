"""The denoiser's CPU twin (shm_denoise_host: shm/denoise.h compiled for the host) on synthetic films and G-buffers built in numpy, against
properties the definition implies and against a float64 restatement of it (tests/denoise_cases.py). Films: 24 x 20 and 37 x 70. No GPU."""
import ctypes as C

import numpy as np
import pytest

import denoise_cases as dc
from shimmer_amd import render

INVALID_ARGUMENT = -1


def _params(lib, **kw):
    return render.make_denoise_params(lib, **kw)


def _run(lib, film, g, **kw):
    return dc.result_rgb(render.denoise_host(lib, film, g, dc.WHITE, _params(lib, **kw)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("size", dc.SIZES)
def test_zero_iterations_is_the_identity(lib, size):
    rng = np.random.default_rng(1)
    film, g = dc.make_inputs(*size, rng)
    film["weight_sum"][3, 4] = 0.0
    film["rgb_sum"][3, 4] = 0.0
    out = render.denoise_host(lib, film, g, dc.WHITE, _params(lib, iterations=0))
    with np.errstate(all="ignore"):
        want = np.where((film["weight_sum"] != 0)[..., None], film["rgb_sum"] / film["weight_sum"][..., None], 0.0).astype(np.float32)
    assert np.array_equal(_bits(dc.result_rgb(out)), _bits(want))             # float32(rgb_sum / weight_sum) ...
    assert np.array_equal(_bits(want), _bits(dc.colour_of(film)))              # ... which for these inputs is also shm_film_get_image's float32 / float32
    assert out["weight_sum"][3, 4] == 0.0 and (out["weight_sum"].ravel().tolist().count(1.0) == out.size - 1)
    # the result goes through shm_film_get_image like a film
    assert np.array_equal(_bits(render.film_get_image(lib, out)), _bits(render.film_get_image(lib, film)))


def _with_pass_through(film, g, rng):
    """Four kinds of pass-through pixel, scattered; returns their mask."""
    h, w = film.shape
    mask = np.zeros((h, w), bool)
    spots = [(2, 3), (5, 5), (h - 1, w - 1), (h // 2, w // 2), (0, 0), (7, 11), (h - 3, 2), (9, w - 2)]
    for k, (y, x) in enumerate(spots):
        mask[y, x] = True
        kind = k % 4
        if kind == 0:
            g["weight_hit"][y, x] = -0.25 if k % 8 == 0 else 0.0
        elif kind == 1:
            film["weight_sum"][y, x] = 0.0; film["rgb_sum"][y, x] = 0.0
        elif kind == 2:
            g["ns"][y, x] = 0.0
        else:
            film["rgb_sum"][y, x, 1] = np.inf if k % 8 == 3 else np.nan
    return mask


@pytest.mark.parametrize("size", dc.SIZES)
@pytest.mark.parametrize("iterations", [1, 2, 5, 8])
def test_pass_through_pixels_keep_their_colour_and_touch_nobody(lib, size, iterations):
    rng = np.random.default_rng(2)
    n, p, albedo, cov = dc.bumpy_guides(*size, rng)
    film, g = dc.make_inputs(*size, rng, normal=n, position=p, albedo=albedo, coverage=cov)
    mask = _with_pass_through(film, g, rng)
    out = _run(lib, film, g, iterations=iterations)
    assert np.array_equal(_bits(out[mask]), _bits(dc.colour_of(film)[mask]))
    assert np.isfinite(out[~mask]).all()
    film2 = film.copy()
    film2["rgb_sum"][mask, 0] = film["rgb_sum"][mask, 0] * 37.0 + 5.0  # every kind stays what it is: channel 0 is finite in all of them, and no guide moves
    out2 = _run(lib, film2, g, iterations=iterations)
    assert np.array_equal(_bits(out2[~mask]), _bits(out[~mask])), "a pass-through pixel's colour reached a neighbour"


@pytest.mark.parametrize("size", dc.SIZES)
@pytest.mark.parametrize("iterations", [1, 5, 8])
def test_partition_of_unity(lib, size, iterations):
    """Constant e over arbitrary valid guides stays constant within (26 N + 4) 2^-24 relative: dc.unity_bound says where each term comes from."""
    rng = np.random.default_rng(3)
    n, p, albedo, cov = dc.bumpy_guides(*size, rng)
    E = 0.7391
    film, g = dc.make_inputs(*size, rng, colour=np.ones(size[::-1] + (3,)), normal=n, position=p, albedo=albedo, coverage=cov)
    # c = E a_eff, with a_eff as the twin computes it from these sums (float32 throughout)
    ws, wh = film["weight_sum"].astype(np.float32), g["weight_hit"].astype(np.float32)
    covf = np.clip(wh / ws, np.float32(0), np.float32(1))[..., None]
    a = g["albedo"].astype(np.float32) / wh[..., None] / dc.WHITE.astype(np.float32)
    a_eff = covf * a + (np.float32(1) - covf)
    assert (a_eff >= np.float32(0.01)).all()  # (nothing below the floor, where a channel is not demodulated)
    film["rgb_sum"] = (np.float32(E) * a_eff).astype(np.float64) * film["weight_sum"][..., None]
    film["rgb_sum"] = film["rgb_sum"].astype(np.float32).astype(np.float64)
    out = _run(lib, film, g, iterations=iterations)
    rel = np.abs(out.astype(np.float64) / a_eff.astype(np.float64) / E - 1.0).max()
    bound = dc.unity_bound(iterations)
    print(f"partition of unity {size} N={iterations}: max relative deviation {rel:.3e}, bound {bound:.3e}")
    assert rel <= bound


@pytest.mark.parametrize("size", dc.SIZES)
def test_a_hard_edge_separates_the_halves(lib, size):
    w, h = size
    rng = np.random.default_rng(4)
    n = np.zeros((h, w, 3)); n[:, : w // 2, 2] = 1.0; n[:, w // 2:, 0] = 1.0  # exactly orthogonal, axis-aligned: n_p . n_q = 0 across the edge, so w_n = 0
    film, g = dc.make_inputs(w, h, rng, normal=n)
    out = _run(lib, film, g)
    film2 = film.copy()
    film2["rgb_sum"][:, w // 2:] = (film["rgb_sum"][:, w // 2:] * 3.0 + 1.0).astype(np.float32)
    out2 = _run(lib, film2, g)
    assert np.array_equal(_bits(out2[:, : w // 2]), _bits(out[:, : w // 2]))
    assert not np.array_equal(_bits(out2[:, w // 2:]), _bits(out[:, w // 2:]))
    assert not np.array_equal(_bits(out[:, : w // 2]), _bits(dc.colour_of(film)[:, : w // 2])), "the filter did nothing"


def test_taps_outside_the_film_are_skipped(lib):
    """A single bright pixel in a corner of a 24 x 20 film, sigma_luminance = inf, five iterations, against the float64 restatement (which skips outside taps and
    renormalises; clamping or mirroring would put more of the bright pixel's weight back into the corner). Tolerance: the partition-of-unity bound times the input range."""
    w, h = dc.SIZES[0]
    rng = np.random.default_rng(5)
    colour = np.full((h, w, 3), 0.25); colour[0, 0] = 64.0
    film, g = dc.make_inputs(w, h, rng, colour=colour)
    d = _params(lib, sigma_luminance=float("inf"), iterations=5)
    out = dc.result_rgb(render.denoise_host(lib, film, g, dc.WHITE, d))
    ref = dc.reference(film, g, dc.WHITE, dc.params_dict(d))
    tol = dc.unity_bound(5) * 64.0
    err = np.abs(out - ref).max()
    print(f"border case: max |twin - float64| {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    # the restatement does tell the border rules apart here: a clamped 5x5 B3 pass would leave the corner (11/16)^2 of the bright pixel, a skipped one 36/121
    one = dc.reference(film, g, dc.WHITE, dict(dc.params_dict(d), iterations=1, demodulate=0))
    assert abs(one[0, 0, 0] - (0.25 + (64.0 - 0.25) * 36.0 / 121.0)) < 1e-9


def _composed_kernel(iterations):
    k = np.ones((1, 1))
    for i in range(iterations):
        s = 1 << i
        h1 = np.zeros(4 * s + 1); h1[::s] = np.array([1, 4, 6, 4, 1]) / 16.0
        h = np.outer(h1, h1)
        full = np.zeros((k.shape[0] + h.shape[0] - 1,) * 2)
        for y in range(h.shape[0]):
            for x in range(h.shape[1]):
                if h[y, x]:
                    full[y:y + k.shape[0], x:x + k.shape[1]] += h[y, x] * k
        k = full
    return k


def test_the_linear_case_against_float64_and_the_variance_it_leaves(lib):
    """One plane, iid noise, sigma_luminance = inf, demodulate = 0: the filter is the linear one."""
    w, h = dc.SIZES[1]
    rng = np.random.default_rng(6)
    sigma = 0.1
    noise = rng.normal(0.0, sigma, (h, w))
    colour = np.repeat((1.0 + noise)[..., None], 3, axis=-1)
    film, g = dc.make_inputs(w, h, rng, colour=colour)
    for iterations in (2, 5):
        d = _params(lib, sigma_luminance=float("inf"), demodulate=0, iterations=iterations)
        out = dc.result_rgb(render.denoise_host(lib, film, g, dc.WHITE, d))
        ref = dc.reference(film, g, dc.WHITE, dc.params_dict(d))
        tol = dc.unity_bound(iterations) * float(np.abs(dc.colour_of(film)).max())
        err = np.abs(out - ref).max()
        print(f"linear case N={iterations}: max |twin - float64| {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol
    # two iterations reach 6 pixels: the interior is where the composed kernel K lies inside the film. There Var(out) = sigma_in^2 sum K^2, and the sample variance of N
    # correlated Gaussian values has the standard error sqrt(2 / N sum_d rho(d)^2) Var(out), rho the output's autocorrelation (K correlated with itself, normalised).
    d = _params(lib, sigma_luminance=float("inf"), demodulate=0, iterations=2)
    out = dc.result_rgb(render.denoise_host(lib, film, g, dc.WHITE, d))[..., 0].astype(np.float64)
    K = _composed_kernel(2)
    r = K.shape[0] // 2
    interior = out[r:h - r, r:w - r]
    sigma_in2 = float(np.var(dc.colour_of(film)[..., 0].astype(np.float64), ddof=1))  # the noise as the film holds it
    expect = sigma_in2 * float((K ** 2).sum())
    pad = np.pad(K, K.shape[0] - 1)
    rho = np.array([[(pad[y:y + K.shape[0], x:x + K.shape[1]] * K).sum() for x in range(pad.shape[1] - K.shape[1] + 1)] for y in range(pad.shape[0] - K.shape[0] + 1)])
    rho /= rho.max()
    N = interior.size
    se = expect * np.sqrt(2.0 / N * float((rho ** 2).sum()))
    got = float(np.var(interior, ddof=1))
    print(f"variance after 2 iterations over {N} interior pixels: {got:.4e}, expected {expect:.4e}, standard error {se:.3e} (the margin)")
    assert abs(got - expect) <= se


def test_demodulation_keeps_texture(lib):
    """A checkerboard albedo over constant irradiance plus noise: out / a_eff is the filtered irradiance, and the contrast across an albedo edge is the albedo ratio."""
    w, h = dc.SIZES[1]
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:h, 0:w]
    check = ((xx // 4 + yy // 4) % 2).astype(bool)
    albedo = np.where(check[..., None], 0.75, 0.125) * np.ones(3)
    irradiance = 1.0 + rng.normal(0.0, 0.05, (h, w, 1)) * np.ones(3)
    film, g = dc.make_inputs(w, h, rng, colour=irradiance * albedo, albedo=albedo)
    n_it = 3
    d = _params(lib, sigma_luminance=float("inf"), iterations=n_it)
    out = dc.result_rgb(render.denoise_host(lib, film, g, dc.WHITE, d)).astype(np.float64)
    _, e_ref, a_eff, valid = dc.reference(film, g, dc.WHITE, dc.params_dict(d), return_parts=True)
    assert valid.all()
    tol = dc.unity_bound(n_it) * float(np.abs(irradiance).max())
    err = np.abs(out / a_eff - e_ref).max()
    print(f"demodulation: max |out / a_eff - filtered irradiance| {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol
    # across a vertical albedo edge (x = 3 | 4 on the rows of the first band): out ratio = albedo ratio (as the sums hold it) times the filtered irradiance's ratio,
    # to that same bound
    left, right = out[1, 3, 0], out[1, 4, 0]
    ratio = (right / left) / (e_ref[1, 4, 0] / e_ref[1, 3, 0])
    contrast = abs(ratio / (a_eff[1, 4, 0] / a_eff[1, 3, 0]) - 1.0)
    print(f"contrast across the albedo edge: relative deviation {contrast:.3e}, bound {dc.unity_bound(n_it):.3e}")
    assert abs(a_eff[1, 4, 0] / a_eff[1, 3, 0] - 6.0) < 1e-6 and contrast <= dc.unity_bound(n_it)
    # without demodulation the same filter smears the texture: the edge's contrast drops
    flat = dc.result_rgb(render.denoise_host(lib, film, g, dc.WHITE, _params(lib, sigma_luminance=float("inf"), iterations=n_it, demodulate=0)))
    assert flat[1, 4, 0] / flat[1, 3, 0] < 0.5 * right / left


# the full filter's measured deviation from the float64 restatement (profiles/denoise.md), relative to the input range, and the tolerance: 8 times that
FULL_FILTER_MEASURED = {(24, 20): 1.112e-06, (37, 70): 2.100e-06}


@pytest.mark.parametrize("size", dc.SIZES)
def test_the_full_filter_against_the_float64_restatement(lib, size):
    """Default parameters (finite sigma_luminance), noisy colour over bumpy guides: variance bounded away from 0, so no exponent is ill-conditioned."""
    rng = np.random.default_rng(8)
    n, p, albedo, cov = dc.bumpy_guides(*size, rng)
    colour = albedo * (1.0 + rng.normal(0.0, 0.2, size[::-1] + (1,))).clip(0.2, None)
    film, g = dc.make_inputs(*size, rng, colour=colour, normal=n, position=p, albedo=albedo, coverage=cov)
    d = _params(lib)
    out = dc.result_rgb(render.denoise_host(lib, film, g, dc.WHITE, d)).astype(np.float64)
    ref = dc.reference(film, g, dc.WHITE, dc.params_dict(d))
    dev = float(np.abs(out - ref).max() / np.abs(ref).max())
    print(f"full filter {size}: max |twin - float64| / range = {dev:.3e}")
    assert np.abs(out - dc.colour_of(film)).max() > 1e-3, "the filter did nothing"
    assert dev <= 8.0 * FULL_FILTER_MEASURED[size]


@pytest.mark.parametrize("field,value,word", [("iterations", 9, b"iterations"), ("sigma_luminance", 0.0, b"sigma_luminance"), ("sigma_luminance", float("nan"), b"sigma_luminance"),
                                              ("sigma_normal", -1.0, b"sigma_normal"), ("sigma_normal", float("nan"), b"sigma_normal"), ("sigma_plane", 0.0, b"sigma_plane"),
                                              ("sigma_plane", float("nan"), b"sigma_plane"), ("albedo_floor", 0.0, b"albedo_floor"), ("albedo_floor", 1.5, b"albedo_floor"),
                                              ("albedo_floor", float("nan"), b"albedo_floor")])
def test_the_twin_refuses_bad_parameters(lib, field, value, word):
    film, g = dc.make_inputs(*dc.SIZES[0], np.random.default_rng(9))
    d = _params(lib, **{field: value})
    out = np.zeros(film.shape, render.FILM_DTYPE)
    w = (C.c_double * 3)(*dc.WHITE)
    rc = lib.shm_denoise_host(film.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), film.shape[1], film.shape[0], w, C.byref(d), out.ctypes.data_as(C.c_void_p))
    assert rc == INVALID_ARGUMENT and word in lib.shm_last_error()
    assert not out["rgb_sum"].any()


def test_default_parameters(lib):
    d = _params(lib)
    assert (d.iterations, d.demodulate, d.sigma_luminance, d.sigma_normal, d.sigma_plane) == (5, 1, 1.5, 128.0, np.float32(0.1)) and d.albedo_floor == np.float32(0.01)
    assert _params(lib, albedo_floor=1.0).albedo_floor == 1.0  # the interval's closed end is accepted
    film, g = dc.make_inputs(*dc.SIZES[0], np.random.default_rng(9))
    render.denoise_host(lib, film, g, dc.WHITE, _params(lib, albedo_floor=1.0, iterations=1))


def test_a_channel_below_the_albedo_floor_is_not_demodulated(lib):
    """A black surface (an emitter's material, say): a_eff = 1, not the floor, so with every albedo below the floor demodulate = 1 is demodulate = 0, bit for bit."""
    rng = np.random.default_rng(10)
    w, h = dc.SIZES[0]
    film, g = dc.make_inputs(w, h, rng, albedo=np.full((h, w, 3), 0.001))
    assert np.array_equal(_bits(_run(lib, film, g, demodulate=1)), _bits(_run(lib, film, g, demodulate=0)))
    film, g = dc.make_inputs(w, h, rng, albedo=np.full((h, w, 3), 0.02))
    assert not np.array_equal(_bits(_run(lib, film, g, demodulate=1)), _bits(_run(lib, film, g, demodulate=0)))
