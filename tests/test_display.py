"""The display pass's CPU twin (shm_display_host, shm_write_png) against the pipeline include/shimmer_hip.h documents, on numpy-built films: no GPU.
The device is held to this twin bit for bit by tests/test_gpu_display.py."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import display_cases as dc
from shimmer_amd import abi, render

INVALID_ARGUMENT = -1  # SHM_ERR_INVALID_ARGUMENT (include/shimmer_hip.h)
HEADER = Path(__file__).resolve().parents[1] / "include" / "shimmer_hip.h"


def _rgb(image):
    return image[..., :3].astype(np.int64)


def test_defaults_and_layouts(lib):
    d = render.make_display_params(lib)
    assert (d.source, d.tonemap, d.transfer, d.auto_exposure, d.dither) == (abi.SHM_DISPLAY_SOURCE_FILM, abi.SHM_TONEMAP_ACES, abi.SHM_TRANSFER_SRGB, 0, 0)
    want = dict(exposure=1.0, key=0.18, white=4.0, log2_min=-16.0, log2_max=16.0, percentile_low=0.10, percentile_high=0.95, adaptation_rate=3.0, dt=0.0)
    for name, v in want.items():
        assert getattr(d, name) == np.float32(v), name
    assert list(d.output_rgb_from_sensor_rgb) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(d.reserved) == [0]
    # the header's documented layout: every field's offset stands in its comment
    text = HEADER.read_text()
    params = text[text.index("typedef struct ShmDisplayParams"):text.index("} ShmDisplayParams;")]
    state = text[text.index("typedef struct ShmDisplayState"):text.index("} ShmDisplayState;")]
    assert "96 bytes" in params and "32 bytes" in state
    assert C.sizeof(abi.ShmDisplayParams) == 96 and C.sizeof(abi.ShmDisplayState) == 32

    def documented(body):
        import re
        out = {}
        for names, offsets in re.findall(r"^\s+(?:uint32_t|float) ([^;]+);\s*/\*\s*([\d, ]+?)\s*(?::|\*/)", body, re.M):
            for n, o in zip([n.strip().split("[")[0] for n in names.split(",")], [int(o) for o in offsets.split(",")]):
                out[n] = o
        return out

    for struct_type, body in ((abi.ShmDisplayParams, params), (abi.ShmDisplayState, state)):
        doc = documented(body)
        assert set(doc) == {n for n, _ in struct_type._fields_}, doc
        for n, _ in struct_type._fields_:
            assert getattr(struct_type, n).offset == doc[n], n
    assert [n for n, _ in abi.ShmDisplayParams._fields_] == list(render.DISPLAY_PARAM_NAMES) + ["reserved"]
    with pytest.raises(TypeError):
        render.make_display_params(lib, gamma=2.2)


def test_the_linear_stage_is_film_get_image(lib):
    rng = np.random.default_rng(1)
    h, w = 45, 70
    film = np.zeros((h, w), dtype=render.FILM_DTYPE)
    film["rgb_sum"] = rng.uniform(0.0, 3.0, (h, w, 3))
    film["weight_sum"] = rng.uniform(0.5, 4.0, (h, w))
    film["weight_sum"][3, 5:9] = 0.0
    d = render.make_display_params(lib, tonemap=abi.SHM_TONEMAP_NONE, transfer=abi.SHM_TRANSFER_LINEAR, output_rgb_from_sensor_rgb=render.SRGB_FROM_XYZ)
    got, _, _ = render.display_host(lib, film, w, h, d)
    img = render.film_get_image(lib, film, render.SRGB_FROM_XYZ)
    want = np.floor(np.clip(img, np.float32(0), np.float32(1)) * np.float32(255) + np.float32(0.5)).astype(np.int64)
    assert want.min() == 0 and want.max() == 255 and np.unique(want).size > 100
    assert np.array_equal(_rgb(got), want)
    assert (got[..., 3] == 255).all()


def test_the_histogram_bins_the_edge_film_exactly(lib):
    film, bins, at = dc.edge_film()
    d = dc.edge_params(lib, auto_exposure=1)
    _, counts, st = render.display_host(lib, film, dc.EDGE_W, dc.EDGE_H, d)
    want = dc.counts_of(bins)
    assert np.array_equal(counts, want), np.flatnonzero(counts != want)
    assert (want[1:255] >= 1).all() and want[0] == 2 and want[255] == 2
    assert st.counted == int((bins >= 0).sum()) == int(want.sum())
    # one pixel at a time: each lands in its own bin
    for i in list(at.values()) + [0, 100, 253]:
        one = film.reshape(-1)[i:i + 1].reshape(1, 1)
        _, c1, s1 = render.display_host(lib, one, 1, 1, d)
        assert s1.counted == int(bins[i] >= 0) and (bins[i] < 0 or c1[bins[i]] == 1), (i, bins[i], np.flatnonzero(c1))
    # the default range (bins of 32 / 254 stops): its own centres
    dd = render.make_display_params(lib, auto_exposure=1)
    b = np.arange(1, 255)
    _, c2, s2 = render.display_host(lib, dc.grey_film(dc.centre(b, -16.0, 16.0), (1, 254)), 254, 1, dd)
    assert np.array_equal(c2[1:255], np.ones(254, np.uint32)) and c2[0] == 0 and c2[255] == 0 and s2.counted == 254


def test_the_histogram_matches_a_float64_binning(lib):
    rng = np.random.default_rng(2)
    h, w = 45, 70
    lum = 2.0 ** rng.uniform(-20.0, 20.0, (h, w))  # log-uniform over 40 stops: both ends outside the range
    chroma = rng.uniform(0.2, 1.0, (h, w, 3))
    rgb = (chroma / (chroma @ np.array([0.2126, 0.7152, 0.0722]))[..., None] * lum[..., None]).astype(np.float32).astype(np.float64)
    d = render.make_display_params(lib, auto_exposure=1)
    Y = 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]
    coord = (np.log2(Y) - d.log2_min) * (254.0 / (d.log2_max - d.log2_min))
    near = np.abs(coord - np.round(coord)) < 1e-4
    assert near.mean() <= 0.01, near.mean()
    keep = ~near
    film = dc.film_of(rgb)
    film["weight_sum"][near] = 0.0  # left out: a pixel without weight is not counted
    _, counts, st = render.display_host(lib, film, w, h, d)
    bins = np.where(coord < 0, 0, np.where(coord >= 254, 255, 1 + np.clip(np.floor(coord), 0, 253))).astype(np.int64)
    want = np.bincount(bins[keep], minlength=256)
    assert np.array_equal(counts, want), np.flatnonzero(counts != want)
    assert st.counted == int(keep.sum()) and want[0] > 0 and want[255] > 0 and (want[1:255] > 0).sum() > 200


@pytest.mark.parametrize("L", [2.0 ** -12.3, 0.0041, 0.18, 1.0, 37.5, 2.0 ** 13.7])
def test_the_exposure_brings_a_uniform_film_to_the_key(lib, L):
    h, w = 16, 20
    d = render.make_display_params(lib, auto_exposure=1, percentile_high=0.9)
    half_bin = 2.0 ** ((d.log2_max - d.log2_min) / 254 / 2)
    film = dc.grey_film(np.full(h * w, L), (h, w))
    _, _, st = render.display_host(lib, film, w, h, d)
    assert st.counted == h * w and st.valid == 1
    assert d.key / half_bin <= st.scale * L <= d.key * half_bin, (st.scale * L, d.key)
    assert st.scale == pytest.approx(2.0 ** st.log2_exposure, rel=1e-5)
    # 5 % of the pixels 1000 times brighter, above the high percentile: the target does not move by a bit
    v = np.full(h * w, L)
    v[::20] *= 1000.0
    _, _, st2 = render.display_host(lib, dc.grey_film(v, (h, w)), w, h, d)
    assert st2.counted == h * w
    assert np.float32(st2.log2_target).view(np.uint32) == np.float32(st.log2_target).view(np.uint32)


def test_an_empty_film_meters_nothing(lib):
    film = dc.grey_film(np.full(256, 0.5), (16, 16))
    film["weight_sum"] = 0.0
    d = render.make_display_params(lib, auto_exposure=1)
    _, counts, st = render.display_host(lib, film, 16, 16, d)
    assert st.log2_target == 0.0 and st.counted == 0 and counts.sum() == 0 and st.scale == 1.0


def test_adaptation(lib):
    h, w = 16, 16
    dark, bright = dc.grey_film(np.full(h * w, 0.01), (h, w)), dc.grey_film(np.full(h * w, 20.0), (h, w))
    rate, dt = 3.0, 1.0 / 30.0
    d = render.make_display_params(lib, auto_exposure=1, adaptation_rate=rate, dt=dt)
    st = None
    for _ in range(3):
        _, _, st = render.display_host(lib, dark, w, h, d, st)
        assert st.log2_exposure == st.log2_target  # a fresh state jumps, and then there is nowhere to go
    start, trail = st.log2_exposure, []
    for f in range(12):
        _, _, st = render.display_host(lib, bright, w, h, d, st)
        trail.append(st.log2_exposure)
        closed = start + (st.log2_target - start) * (1.0 - np.exp(-rate * dt * (f + 1)))
        assert abs(st.log2_exposure - closed) <= 1e-5 * abs(closed), (f, st.log2_exposure, closed)
        assert st.scale == pytest.approx(2.0 ** st.log2_exposure, rel=1e-5)
    target = st.log2_target
    assert target < start
    assert all(a > b for a, b in zip([start] + trail, trail)) and all(t > target for t in trail), "not monotone towards the target, or past it"
    # dt = 0, rate = 0 and a fresh state jump exactly
    for jump in (render.make_display_params(lib, auto_exposure=1, dt=0.0), render.make_display_params(lib, auto_exposure=1, dt=dt, adaptation_rate=0.0)):
        _, _, s2 = render.display_host(lib, bright, w, h, jump, st)
        assert s2.log2_exposure == s2.log2_target == target
    _, _, s3 = render.display_host(lib, bright, w, h, d, None)
    assert s3.log2_exposure == target
    # without auto-exposure the state comes back untouched
    manual = render.make_display_params(lib, auto_exposure=0, dt=dt)
    _, counts, s4 = render.display_host(lib, bright, w, h, manual, st)
    assert bytes(s4) == bytes(st) and counts.sum() == 0


def _sweep():
    rng = np.random.default_rng(3)
    grey = np.repeat(np.linspace(0.0, 16.0, 4096)[:, None], 3, axis=1)
    colours = 2.0 ** rng.uniform(-10.0, 5.0, (1024, 3))
    rgb = np.concatenate([grey, colours]).astype(np.float32).astype(np.float64)
    return rgb.reshape(80, 64, 3)


@pytest.mark.parametrize("tonemap", dc.CURVES)
@pytest.mark.parametrize("transfer", dc.TRANSFERS)
def test_curves_and_transfer_against_float64(lib, tonemap, transfer):
    rgb = _sweep()
    for exposure in (1.0, 0.37):
        d = render.make_display_params(lib, tonemap=tonemap, transfer=transfer, exposure=exposure)
        got, _, _ = render.display_host(lib, dc.film_of(rgb), 64, 80, d)
        want = dc.restate(rgb, np.float32(exposure), tonemap, transfer)
        diff = np.abs(_rgb(got) - want)
        assert diff.max() <= 1, diff.max()
        assert (diff != 0).mean() <= 1e-3, (diff != 0).mean()
        sweep = _rgb(got).reshape(-1, 3)[:4096]
        assert (np.diff(sweep, axis=0) >= 0).all(), "the codes fall somewhere along the grey sweep"
        assert sweep[0].tolist() == [0, 0, 0] and (exposure != 1.0 or sweep[-1].tolist() == [255, 255, 255])


def test_none_and_srgb_is_the_example_arithmetic(lib):
    spec = importlib.util.spec_from_file_location("render_scene_example", Path(__file__).resolve().parents[1] / "examples" / "render_scene.py")
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    rgb = _sweep()
    film = dc.film_of(rgb)
    image = render.film_get_image(lib, film)
    for e in (1.0, 0.25, 3.0):
        seen = {}
        example.write_png = lambda path, rgb8: seen.update(rgb8=rgb8)
        example.write_ldr_png("unused", image, e)
        d = render.make_display_params(lib, tonemap=abi.SHM_TONEMAP_NONE, transfer=abi.SHM_TRANSFER_SRGB, exposure=e)
        got, _, _ = render.display_host(lib, film, 64, 80, d)
        assert np.abs(_rgb(got) - seen["rgb8"].astype(np.int64)).max() <= 1


@pytest.mark.parametrize("tonemap", dc.CURVES)
def test_sanitising(lib, tonemap):
    film, bins, at = dc.edge_film()
    for transfer in dc.TRANSFERS:
        d = dc.edge_params(lib, tonemap=tonemap, transfer=transfer)
        got, _, _ = render.display_host(lib, film, dc.EDGE_W, dc.EDGE_H, d)
        px = got.reshape(-1, 4)
        assert px[at["plus_inf"]].tolist() == [255, 0, 0, 255]
        assert px[at["all_nan"]].tolist() == [0, 0, 0, 255] and px[at["negative"]].tolist() == [0, 0, 0, 255]
        # (one channel that is NaN or -inf reaches all three through the matrix, as in shm_film_get_image: 0 * inf is NaN)
        for name in ("nan", "minus_inf", "both_inf"):
            assert px[at[name]].tolist() == [0, 0, 0, 255], name
        assert px[at["mixed_negative"]][1] == 0 and px[at["mixed_negative"]][0] > 200
        assert px[at["far_above"]].tolist() == [255, 255, 255, 255] and px[at["black"]].tolist() == [0, 0, 0, 255]
        # a pixel's bytes are its own: every pixel alone gives the bytes it has in the film, the pixels without weight and their neighbours among them
        for i in (at["no_weight"] - 1, at["no_weight"], at["no_weight_black"], at["no_weight_black"] + 1, at["plus_inf"] + 1, 17):
            alone, _, _ = render.display_host(lib, film.reshape(-1)[i:i + 1].reshape(1, 1), 1, 1, d)
            assert alone.reshape(4).tolist() == px[i].tolist(), i
        # auto-exposure on: the pixels that are not counted still do not reach the others through the scale
        da = dc.edge_params(lib, tonemap=tonemap, transfer=transfer, auto_exposure=1)
        a, _, st = render.display_host(lib, film, dc.EDGE_W, dc.EDGE_H, da)
        assert np.isfinite(st.scale) and st.scale > 0
        clean = film.copy().reshape(-1)
        for name in ("nan", "all_nan", "plus_inf", "minus_inf", "both_inf", "negative", "no_weight", "no_weight_black", "black"):
            clean["weight_sum"][at[name]] = 0.0
        b, _, st_b = render.display_host(lib, clean.reshape(dc.EDGE_H, dc.EDGE_W), dc.EDGE_W, dc.EDGE_H, da)
        assert dc.state_tuple(st) == dc.state_tuple(st_b)
        assert a.reshape(-1, 4)[at["plus_inf"]].tolist() == [255, 0, 0, 255] and a.reshape(-1, 4)[at["all_nan"]].tolist() == [0, 0, 0, 255]


def test_dither(lib):
    h, w, k = 16, 24, 117
    film = dc.grey_film(np.full(h * w, (k + 0.37) / 255.0), (h, w))
    plain = render.make_display_params(lib, tonemap=abi.SHM_TONEMAP_NONE, transfer=abi.SHM_TRANSFER_LINEAR)
    dith = render.make_display_params(lib, tonemap=abi.SHM_TONEMAP_NONE, transfer=abi.SHM_TRANSFER_LINEAR, dither=1)
    got, _, _ = render.display_host(lib, film, w, h, plain)
    assert (_rgb(got) == k).all()
    got, _, _ = render.display_host(lib, film, w, h, dith)
    codes = _rgb(got)[..., 0]
    assert set(np.unique(codes)) == {k, k + 1} and np.array_equal(_rgb(got)[..., 1], codes) and np.array_equal(_rgb(got)[..., 2], codes)
    blocks = codes.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    assert (np.abs(blocks.mean(axis=1) - (k + 0.37)) <= 1 / 64).all(), blocks.mean(axis=1)
    assert (blocks == blocks[0]).all(), "the matrix does not repeat every 8 pixels"
    # the 64 thresholds of a block are distinct: at fraction (j + 1) / 64 - 1 / 256 exactly j + 1 pixels of a block round up, and each pixel's count is its own
    ups = np.zeros((h, w), np.int64)
    for j in range(64):
        f = dc.grey_film(np.full(h * w, (k + (j + 1) / 64 - 1 / 256) / 255.0), (h, w))
        c = _rgb(render.display_host(lib, f, w, h, dith)[0])[..., 0]
        assert ((c == k) | (c == k + 1)).all()
        ups += c - k
        assert int((c - k)[:8, :8].sum()) == j + 1
    assert sorted(ups[:8, :8].reshape(-1).tolist()) == list(range(1, 65))


def test_write_png(lib, tmp_path):
    rng = np.random.default_rng(4)
    h, w = 45, 70
    image = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    path = tmp_path / "picture.png"
    render.write_png(lib, path, image)
    assert np.array_equal(dc.decode_png(path.read_bytes()), image[..., :3])
    big = rng.integers(0, 256, (300, 301, 4), dtype=np.uint8)  # more than one stored block, the last one short
    render.write_png(lib, tmp_path / "big.png", big)
    assert np.array_equal(dc.decode_png((tmp_path / "big.png").read_bytes()), big[..., :3])
    loaded = abi.ShmLoadedImage()
    abi.check(lib, lib.shm_image_load_png(str(path).encode(), b"linear", abi.SHM_WRAP_REPEAT, 0, C.byref(loaded)), "shm_image_load_png")
    try:
        level = loaded.levels[0]
        assert loaded.n_channels == 3 and (level.width, level.height) == (w, h)
        texels = np.ctypeslib.as_array(loaded.texels, shape=(loaded.n_texel_floats,))[level.texel_offset:level.texel_offset + h * w * 3].reshape(h, w, 3)
        assert np.array_equal(np.round(texels * 255.0).astype(np.int64), image[..., :3].astype(np.int64))
    finally:
        lib.shm_image_free(C.byref(loaded))
    flat = np.ascontiguousarray(image).view(np.uint32)
    ptr = flat.ctypes.data_as(C.c_void_p)
    for rc in (lib.shm_write_png(None, ptr, w, h), lib.shm_write_png(str(path).encode(), None, w, h), lib.shm_write_png(str(path).encode(), ptr, 0, h),
               lib.shm_write_png(str(path).encode(), ptr, w, -1), lib.shm_write_png(str(tmp_path / "no" / "such" / "directory.png").encode(), ptr, w, h)):
        assert rc == INVALID_ARGUMENT and lib.shm_last_error()


BAD = [dict(source=3), dict(tonemap=3), dict(transfer=2), dict(log2_min=4.0, log2_max=4.0), dict(log2_min=5.0, log2_max=4.0), dict(log2_min=float("nan")),
       dict(percentile_low=-0.1), dict(percentile_low=0.5, percentile_high=0.5), dict(percentile_high=1.5), dict(percentile_low=float("nan")),
       dict(exposure=0.0), dict(exposure=-1.0), dict(exposure=float("inf")), dict(exposure=float("nan")), dict(key=0.0), dict(key=float("inf")), dict(white=0.0),
       dict(white=float("nan")), dict(dt=float("nan")), dict(dt=float("inf")), dict(adaptation_rate=float("nan")), dict(adaptation_rate=float("-inf")),
       dict(output_rgb_from_sensor_rgb=[1, 0, 0, 0, float("nan"), 0, 0, 0, 1]), dict(output_rgb_from_sensor_rgb=[1, 0, 0, 0, 1, 0, 0, 0, float("inf")])]


def test_refusals(lib):
    film = dc.grey_film(np.full(256, 0.5), (16, 16))
    out = np.zeros((16, 16), np.uint32)
    fp, op = film.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    good = render.make_display_params(lib, auto_exposure=1)
    assert lib.shm_display_host(fp, 16, 16, C.byref(good), None, None, op) == 0  # (no state and no counts asked for)
    for bad in BAD:
        d = render.make_display_params(lib, auto_exposure=1, **bad)
        assert lib.shm_display_host(fp, 16, 16, C.byref(d), None, None, op) == INVALID_ARGUMENT, bad
        assert lib.shm_last_error().startswith(b"display: "), bad
    for rc in (lib.shm_display_host(None, 16, 16, C.byref(good), None, None, op), lib.shm_display_host(fp, 16, 16, None, None, None, op),
               lib.shm_display_host(fp, 16, 16, C.byref(good), None, None, None), lib.shm_display_host(fp, 0, 16, C.byref(good), None, None, op),
               lib.shm_display_host(fp, 16, -3, C.byref(good), None, None, op)):
        assert rc == INVALID_ARGUMENT and lib.shm_last_error()
    assert lib.shm_display_default_params(None) == INVALID_ARGUMENT
