"""The moments pass's CPU twin (shm_moments_update_host), shm_moments_resolve and the adaptive parameters without a GPU: against a float64
restatement written from that section (tests/moments_cases.py) bit for bit, against the sums the recurrence stands for, and at the edges the section names."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import moments_cases as mc
from shimmer_amd import abi, render

ROOT = Path(__file__).resolve().parents[1]
INVALID_ARGUMENT = -1  # SHM_ERR_INVALID_ARGUMENT (include/shimmer_hip.h)


def _run_twin(lib, films, boxes, aparams, start=None):
    """The twin over a film sequence: (records, the tile errors of every batch)."""
    h, w = films[0].shape
    m = mc.clear(start if start is not None else np.zeros((h, w), render.FILM_DTYPE))
    tiles = render.make_tiles(boxes)
    errs = [render.moments_update_host(lib, f, m, tiles, aparams, n_tiles=len(boxes)).copy() for f in films]
    return m, errs


# (width, height, tile, batch weights, signed per-pixel weights): both films of the GPU suite, the 8x8 tiling with its clipped edge tiles and a 16x16 one, the
# reference's wave schedule as batch weights, and weights that are sometimes negative — some batch of some pixel is then not counted
ROWS = [(24, 20, 8, (4, 4, 4, 4, 4), False), (24, 20, 8, (1, 1, 2, 4, 8), False), (24, 20, 16, (1, 1, 1, 1, 1, 1), True), (70, 45, 8, (2, 2, 2, 2), False),
        (70, 45, 16, (1, 1, 2, 4), True)]


@pytest.mark.parametrize("w,h,tile,weights,signed", ROWS, ids=lambda v: str(v))
def test_twin_matches_the_restatement_bit_for_bit(lib, w, h, tile, weights, signed):
    rng = np.random.default_rng(w * 1000 + len(weights))
    films, _, ws = mc.film_sequence(w, h, weights, rng, per_pixel_weights=signed)
    boxes = mc.tile_boxes(w, h, tile)
    a = render.make_adaptive_params(lib, min_spp=3, batch_spp=1, threshold=0.2)
    got, got_err = _run_twin(lib, films, boxes, a)
    want = mc.clear(np.zeros((h, w), render.FILM_DTYPE))
    for b, f in enumerate(films):
        want_err = mc.update(f, want, boxes, 3, 0.2, a.floor)
        assert mc.same_bits(got_err[b], want_err), (b, got_err[b][:4], want_err[:4])
    assert mc.same_bits(got, want)
    if signed:
        assert (ws <= 0).any() and (got["batches"] < len(weights)).any(), "no batch was skipped: the signed case checks nothing more than the others"
    else:
        assert (got["batches"] == len(weights)).all()
    # the tile error is neither all-open nor all-closed at this threshold, or the comparison above saw one side only
    last = got_err[-1]
    assert (last["unconverged"] > 0).any() and np.isfinite(last["max_e2"]).all() and (last["max_e2"] > 0).all()


def test_a_partial_tile_list_updates_its_pixels_only(lib):
    rng = np.random.default_rng(5)
    films, _, _ = mc.film_sequence(24, 20, (1, 1, 1), rng)
    boxes = mc.tile_boxes(24, 20)
    some = [boxes[1], boxes[4], boxes[8]]  # (8) is a clipped edge tile: 8 x 4
    a = render.make_adaptive_params(lib, min_spp=2, batch_spp=1)
    got, errs = _run_twin(lib, films, some, a)
    want = mc.clear(np.zeros((20, 24), render.FILM_DTYPE))
    for f in films:
        want_err = mc.update(f, want, some, 2, a.threshold, a.floor)
    assert mc.same_bits(got, want) and mc.same_bits(errs[-1], want_err)
    inside = np.zeros((20, 24), bool)
    for (x0, y0, x1, y1) in some:
        inside[y0:y1, x0:x1] = True
    assert (got["batches"][inside] == 3).all() and not got.view(np.float64).reshape(20, 24, 12)[~inside].any()


@pytest.mark.parametrize("weights", [(1, 1, 2, 4, 8), (4, 4, 4, 4), (2,) * 8, (1,) * 32], ids=lambda v: f"{len(v)}batches")
def test_m2_is_the_weighted_sum_of_squared_deviations(lib, weights):
    """m2_c == sum_b w_b (x_b - m_c)^2 with m_c = sum w_b x_b / sum w_b, and mean_c == m_c, where x_b and w_b are the batch means and weights AS THE PASS SEES THEM
    (the film's differences, formed here in float64 exactly as the section forms them) and the sums are taken in extended precision.
    Tolerance: each of the B steps rounds nine times (W', dw / W', d, d r, mean', x - mean', dw d, their product, the sum into m2); a rounding perturbs the step's
    increment, or the running mean by which later increments are taken, by at most eps relative to a quantity bounded by w_b x_b^2 summed over the batches
    (m2 + W mean^2 = sum w_b x_b^2 bounds both m2 and W mean^2). Nine roundings a step, and the mean's error carried through at most B later steps with weights that
    sum to one: |m2 - direct| <= (9 + 1) B eps sum w x^2, stated here with a factor 16 for the extended-precision reference's own rounding. For B = 5 and
    sigma / mean = 1/2 that is 2e-14 relative to m2."""
    B = len(weights)
    rng = np.random.default_rng(B)
    films, _, _ = mc.film_sequence(24, 20, weights, rng)
    a = render.make_adaptive_params(lib, min_spp=2, batch_spp=1)
    got, _ = _run_twin(lib, films, mc.tile_boxes(24, 20), a)
    F = [np.zeros((20, 24, 4))] + [np.concatenate([f["rgb_sum"], f["weight_sum"][..., None]], axis=-1) for f in films]
    dw = np.array([F[b + 1][..., 3] - F[b][..., 3] for b in range(B)])
    x = np.array([(F[b + 1][..., 0:3] - F[b][..., 0:3]) / dw[b][..., None] for b in range(B)])
    xl, wl = x.astype(np.longdouble), dw.astype(np.longdouble)[..., None]
    m = (wl * xl).sum(axis=0) / wl.sum(axis=0)
    direct = (wl * (xl - m) ** 2).sum(axis=0)
    scale = (wl * xl * xl).sum(axis=0)
    tol = 16 * B * mc.EPS * scale
    assert (np.abs(got["m2"] - direct) <= tol).all(), float((np.abs(got["m2"] - direct) / tol).max())
    assert (np.abs(got["mean"] - m) <= 16 * B * mc.EPS * np.abs(xl).max(axis=0)).all()
    assert mc.same_bits(got["weight"], dw.sum(axis=0)) or np.allclose(got["weight"], dw.sum(axis=0), rtol=B * mc.EPS, atol=0)
    assert (got["m2"] > 0).all() and (got["batches"] == B).all()


def _one_pixel(values):
    """Films of a 1 x 1 image from (rgb_sum triple, weight_sum) states."""
    out = []
    for rgb, w in values:
        f = np.zeros((1, 1), render.FILM_DTYPE)
        f["rgb_sum"][0, 0] = rgb
        f["weight_sum"][0, 0] = w
        out.append(f)
    return out


@pytest.mark.parametrize("bad,why", [(((3.0, 3.0, 3.0), 2.0), "dw == 0"), (((3.0, 3.0, 3.0), 1.5), "dw < 0"), (((np.nan, 3.0, 3.0), 3.0), "a NaN"),
                                     (((3.0, np.inf, 3.0), 3.0), "an Inf"), (((3.0, 3.0, -np.inf), 3.0), "a -Inf")], ids=["dw_zero", "dw_negative", "nan", "inf", "minus_inf"])
def test_a_batch_without_weight_or_with_a_non_finite_mean_is_skipped(lib, bad, why):
    a = render.make_adaptive_params(lib, min_spp=2, batch_spp=1)
    films = _one_pixel([((1.0, 1.0, 1.0), 1.0), ((2.5, 2.0, 3.0), 2.0), bad])
    box = [(0, 0, 1, 1)]
    m, _ = _run_twin(lib, films[:2], box, a)
    before = m.copy()
    render.moments_update_host(lib, films[2], m, render.make_tiles(box), a, n_tiles=1)
    assert before["batches"][0, 0] == 2 and m["batches"][0, 0] == 2, why
    for k in ("mean", "m2", "weight"):
        assert mc.same_bits(m[k], before[k]), (why, k)
    assert mc.same_bits(m["prev"][0, 0], np.array(list(bad[0]) + [bad[1]])), "prev did not advance"
    want = before.copy()
    mc.update(films[2], want, box, 2, a.threshold, a.floor)
    assert mc.same_bits(m, want)
    # and the pass counts on from the advanced prev where that is finite
    if np.isfinite(bad[0]).all():
        nxt = _one_pixel([((bad[0][0] + 2.0, bad[0][1] + 1.0, bad[0][2] + 4.0), bad[1] + 1.0)])[0]
        render.moments_update_host(lib, nxt, m, render.make_tiles(box), a, n_tiles=1)
        assert m["batches"][0, 0] == 3 and m["weight"][0, 0] == 3.0


def test_the_comparison_is_strict(lib):
    rng = np.random.default_rng(11)
    films, _, _ = mc.film_sequence(24, 20, (1, 1, 1, 1), rng)
    films[2]["rgb_sum"][3, 5, 1] = np.nan  # from the third batch on this pixel's film is NaN: two batches counted, and no more
    films[3]["rgb_sum"][3, 5, 1] = np.nan
    boxes = mc.tile_boxes(24, 20)
    n_pix = np.array([(x1 - x0) * (y1 - y0) for (x0, y0, x1, y1) in boxes])
    # threshold 0: nothing converges, whatever the batch count
    _, errs = _run_twin(lib, films, boxes, render.make_adaptive_params(lib, min_spp=2, batch_spp=1, threshold=0.0))
    assert all((e["unconverged"] == n_pix).all() for e in errs)
    # a constant film has e2 == 0 and still does not pass 0 < 0
    flat = []
    for b in range(1, 4):
        f = np.zeros((20, 24), render.FILM_DTYPE)
        f["rgb_sum"], f["weight_sum"] = 0.5 * b, float(b)
        flat.append(f)
    _, e0 = _run_twin(lib, flat, boxes, render.make_adaptive_params(lib, min_spp=2, batch_spp=1, threshold=0.0))
    assert (e0[-1]["unconverged"] == n_pix).all() and (e0[-1]["max_e2"] == 0).all()
    # +inf: everything with B >= min_batches — nothing before the third batch, everything from it on but the pixel whose B stays 2
    m, errs = _run_twin(lib, films, boxes, render.make_adaptive_params(lib, min_spp=3, batch_spp=1, threshold=float("inf")))
    assert all((e["unconverged"] == n_pix).all() for e in errs[:2])
    tile_of_nan = [i for i, (x0, y0, x1, y1) in enumerate(boxes) if x0 <= 5 < x1 and y0 <= 3 < y1][0]
    want = np.zeros(len(boxes), np.uint32)
    want[tile_of_nan] = 1
    assert np.array_equal(errs[2]["unconverged"], want) and np.array_equal(errs[3]["unconverged"], want)
    assert m["batches"][3, 5] == 2 and (np.delete(m["batches"].ravel(), 3 * 24 + 5) == 4).all()
    # a NaN record (a NaN e2) never converges, and the tile's maximum counts it as +inf
    bad = mc.clear(np.zeros((20, 24), render.FILM_DTYPE))
    bad["batches"], bad["weight"], bad["mean"] = 5.0, 5.0, 1.0
    bad["m2"][7, 9] = np.nan
    f = np.zeros((20, 24), render.FILM_DTYPE)  # (dw == 0: the update leaves the records as they are and evaluates them)
    e = render.moments_update_host(lib, f, bad, render.make_tiles(boxes), render.make_adaptive_params(lib, min_spp=2, batch_spp=1, threshold=float("inf")), n_tiles=len(boxes))
    tile = [i for i, (x0, y0, x1, y1) in enumerate(boxes) if x0 <= 9 < x1 and y0 <= 7 < y1][0]
    assert e["unconverged"][tile] == 1 and np.isposinf(e["max_e2"][tile]) and e["unconverged"].sum() == 1
    assert (np.delete(e["max_e2"], tile) == 0).all()


def test_every_refusal_names_its_cause(lib):
    film = np.zeros((20, 24), render.FILM_DTYPE)
    m = mc.clear(film)
    tiles = render.make_tiles(mc.tile_boxes(24, 20))
    out = np.zeros(9, render.TILE_ERROR_DTYPE)

    def call(a, t=tiles, n=9, w=24, h=20):
        return lib.shm_moments_update_host(film.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), w, h, t, n, C.byref(a), out.ctypes.data_as(C.c_void_p))

    for over, word in ((dict(batch_spp=0), b"batch_spp"), (dict(min_spp=4, batch_spp=4), b"2 * batch_spp"), (dict(min_spp=10, batch_spp=4), b"multiple"),
                       (dict(threshold=-0.1), b"threshold"), (dict(threshold=float("nan")), b"threshold"), (dict(floor=0.0), b"floor"),
                       (dict(floor=float("nan")), b"floor"), (dict(floor=float("inf")), b"floor")):
        assert call(render.make_adaptive_params(lib, **over)) == INVALID_ARGUMENT and word in lib.shm_last_error(), over
    ok = render.make_adaptive_params(lib)
    assert call(ok) == 0 and call(render.make_adaptive_params(lib, threshold=float("inf"))) == 0
    assert call(ok, render.make_tiles([(0, 0, 8, 8), (4, 4, 12, 12)]), 2) == INVALID_ARGUMENT and b"overlap" in lib.shm_last_error()
    assert call(ok, render.make_tiles([(16, 16, 25, 20)]), 1) == INVALID_ARGUMENT and b"outside" in lib.shm_last_error()
    assert call(ok, render.make_tiles([(8, 8, 8, 12)]), 1) == INVALID_ARGUMENT and b"outside" in lib.shm_last_error()
    assert call(ok, n=0) == INVALID_ARGUMENT and b"no tiles" in lib.shm_last_error()
    assert call(ok, w=0) == INVALID_ARGUMENT and b"empty film" in lib.shm_last_error()
    assert not m.view(np.float64).any(), "a refused call wrote into the records"
    res = np.zeros((20, 24, 8), np.float32)
    assert lib.shm_moments_resolve(m.ctypes.data_as(C.c_void_p), m.size, -1.0, res.ctypes.data_as(abi.c_float_p)) == INVALID_ARGUMENT and b"floor" in lib.shm_last_error()
    assert lib.shm_moments_resolve(None, 1, 0.01, res.ctypes.data_as(abi.c_float_p)) == INVALID_ARGUMENT
    with pytest.raises(abi.ShimmerHipError, match="multiple"):
        render.moments_update_host(lib, film, m, tiles, render.make_adaptive_params(lib, min_spp=9, batch_spp=2))
    with pytest.raises(TypeError):
        render.make_adaptive_params(lib, spp=3)


def test_default_params(lib):
    a = render.make_adaptive_params(lib)
    assert (a.min_spp, a.batch_spp) == (16, 4) and a.threshold == np.float32(0.05) and a.floor == np.float32(0.01) and not any(a.reserved)
    assert lib.shm_adaptive_default_params(None) == INVALID_ARGUMENT


def test_resolve_against_numpy(lib):
    rng = np.random.default_rng(3)
    films, _, _ = mc.film_sequence(37, 11, (1, 1, 2, 4), rng, mean=0.02, sigma=0.05)  # means around the floor: both sides of the max are taken
    a = render.make_adaptive_params(lib, min_spp=2, batch_spp=1)
    m, _ = _run_twin(lib, films, mc.tile_boxes(37, 11), a)
    m["batches"][0, :5] = 1.0  # records with one batch resolve to zeros
    for floor in (0.01, 0.5):
        got = render.moments_resolve(lib, m, floor)
        want = mc.resolve(m, floor)
        assert mc.same_bits(np.concatenate([got["v"], got["s2"], got["batches"][..., None], got["e2"][..., None]], axis=-1), want)
        assert not got["v"][0, :5].any() and not got["s2"][0, :5].any() and not got["e2"][0, :5].any()
    mu = m["mean"].sum(axis=-1) / 3
    assert (mu > 0.01).any() and (mu < 0.01).any()
    # and in plain terms: s2 = m2 / (B - 1), v = s2 / W
    got = render.moments_resolve(lib, m, 0.01)
    assert np.allclose(got["s2"][1:], m["m2"][1:] / 3.0, rtol=1e-6) and np.allclose(got["v"][1:], m["m2"][1:] / 3.0 / 8.0, rtol=1e-6)


def test_constant_pixels_have_exactly_zero_variance(lib):
    """Dyadic constants and integer weights: every film sum and every difference is exact, so x_b is the constant itself, d is 0 from the second batch on and m2 never leaves 0."""
    films = []
    f = np.zeros((20, 24), render.FILM_DTYPE)
    yy, xx = np.mgrid[0:20, 0:24]
    c = np.stack([0.25 * (xx % 5), 0.5 + 0.125 * (yy % 7), np.full(xx.shape, 3.0)], axis=-1)  # (some channels are 0: a black background)
    for w in (1, 1, 2, 4, 8):
        f = f.copy()
        f["rgb_sum"] += c * w
        f["weight_sum"] += w
        films.append(f)
    a = render.make_adaptive_params(lib, min_spp=2, batch_spp=1, threshold=1e-6)
    m, errs = _run_twin(lib, films, mc.tile_boxes(24, 20), a)
    got = render.moments_resolve(lib, m, a.floor)
    assert not m["m2"].any() and not got["v"].any() and not got["s2"].any() and not got["e2"].any()
    assert mc.same_bits(m["mean"], c) and (m["weight"] == 16).all() and (m["batches"] == 5).all()
    assert (errs[0]["unconverged"] > 0).all() and not errs[1]["unconverged"].any() and not errs[-1]["max_e2"].any()


def test_abi_probe(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    structs = {"ShmMomentsPixel": abi.ShmMomentsPixel, "ShmTileError": abi.ShmTileError, "ShmAdaptiveParams": abi.ShmAdaptiveParams}
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"shimmer_hip.h\"\nint main(void) {\n  printf(\"%d\\n\", SHM_ABI_VERSION);\n"
    for n, t in structs.items():
        src += f'  printf("{n} %zu\\n", sizeof({n}));\n' + "".join(f'  printf("{n}.{f} %zu\\n", offsetof({n}, {f}));\n' for f, _ in t._fields_)
    (tmp_path / "probe.c").write_text(src + "  return 0;\n}\n")
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")], check=True)
    lines = subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert lines[0] == "10" == str(abi.SHM_ABI_VERSION)
    seen = 0
    for line in lines[1:]:
        name, value = line.split()
        if "." in name:
            s, f = name.split(".")
            assert getattr(structs[s], f).offset == int(value), name
        else:
            assert C.sizeof(structs[name]) == int(value), name
            seen += 1
    assert seen == 3
    assert (C.sizeof(abi.ShmMomentsPixel), C.sizeof(abi.ShmTileError), C.sizeof(abi.ShmAdaptiveParams)) == (96, 8, 32)
    fields = [f for f, _ in abi.ShmMomentsPixel._fields_]
    assert render.MOMENTS_DTYPE.itemsize == 96 and [render.MOMENTS_DTYPE.fields[f][1] for f in fields] == [getattr(abi.ShmMomentsPixel, f).offset for f in fields]
    assert [render.TILE_ERROR_DTYPE.fields[f][1] for f in ("unconverged", "max_e2")] == [0, 4]


# ---- the denoiser's measured variance source (ShmDenoiseParams::variance_source) ----
def _denoise_inputs(rng, w=24, h=20):
    import denoise_cases as dc
    n, p, albedo, coverage = dc.bumpy_guides(w, h, rng)
    film, g = dc.make_inputs(w, h, rng, normal=n, position=p, albedo=albedo, coverage=coverage)
    return film, g, dc.WHITE


def _records(film, v, batches=4.0):
    """Records whose variance of the mean is `v` (H, W, 3): W = the film's weight, B = batches, m2 = v W (B - 1)."""
    m = mc.clear(film)
    m["weight"], m["batches"] = film["weight_sum"], batches
    m["mean"] = film["rgb_sum"] / film["weight_sum"][..., None]
    m["m2"] = v * (film["weight_sum"] * (batches - 1.0))[..., None]
    return m


def test_measured_variance_source_of_the_denoiser(lib):
    rng = np.random.default_rng(21)
    film, g, white = _denoise_inputs(rng)
    spatial = render.make_denoise_params(lib, iterations=3)
    measured = render.make_denoise_params(lib, iterations=3, variance_source=abi.SHM_DENOISE_VARIANCE_MEASURED)
    assert spatial.variance_source == abi.SHM_DENOISE_VARIANCE_SPATIAL == 0
    base = render.denoise_host(lib, film, g, white, spatial)
    some = _records(film, np.full(film.shape + (3,), 0.01))
    # the spatial source does not read the records; records with fewer than two batches keep the spatial estimate
    assert mc.same_bits(render.denoise_host(lib, film, g, white, spatial, moments=some), base)
    assert mc.same_bits(render.denoise_host(lib, film, g, white, measured, moments=_records(film, np.full(film.shape + (3,), 0.01), batches=1.0)), base)
    # a measured variance of 0 closes the luminance weight on every tap whose l differs: the pixel keeps its own colour, within the rounding of e = c / a_eff and back
    import denoise_cases as dc
    zero = dc.result_rgb(render.denoise_host(lib, film, g, white, measured, moments=_records(film, np.zeros(film.shape + (3,)))))
    c = dc.colour_of(film)
    assert np.allclose(zero, c, rtol=4 * 2.0 ** -24, atol=0) and not np.allclose(dc.result_rgb(base), c, rtol=1e-3, atol=0)
    # a large one opens it: the result moves further from the input than under a small one
    dist = lambda v: float(np.abs(dc.result_rgb(render.denoise_host(lib, film, g, white, measured, moments=_records(film, np.full(film.shape + (3,), v)))) - c).mean())
    assert dist(1e-6) < dist(1e-2) < dist(1.0)
    # refusals
    out = np.zeros(film.shape, render.FILM_DTYPE)
    w3 = (C.c_double * 3)(*white)
    args = (film.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), 24, 20, w3)
    assert lib.shm_denoise_host(*args, C.byref(measured), out.ctypes.data_as(C.c_void_p)) == INVALID_ARGUMENT and b"moments" in lib.shm_last_error()
    unknown = render.make_denoise_params(lib, variance_source=2)
    assert lib.shm_denoise_host(*args, C.byref(unknown), out.ctypes.data_as(C.c_void_p)) == INVALID_ARGUMENT and b"variance_source" in lib.shm_last_error()
    assert lib.shm_denoise_host_moments(args[0], args[1], None, 24, 20, w3, C.byref(measured), out.ctypes.data_as(C.c_void_p)) == INVALID_ARGUMENT
    assert C.sizeof(abi.ShmDenoiseParams) == 32 and abi.ShmDenoiseParams.variance_source.offset == 24
