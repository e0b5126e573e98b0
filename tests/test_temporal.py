"""The temporal pass's CPU twin (shm_temporal_accumulate_host) on numpy-built films and G-buffers under cameras from shm_camera_create: the blend
against a float32 numpy restatement bit for bit, the still camera as the identity map, known motions, every rejection, degenerate input, and the documented refusals.
No GPU: tests/test_gpu_temporal.py holds the device to this twin."""
import ctypes as C

import numpy as np
import pytest

import temporal_cases as tc
from shimmer_amd import abi, render

INVALID_ARGUMENT, UNSUPPORTED = -1, -2  # SHM_ERR_* (include/shimmer_hip.h)
INF = float("inf")


def _params(lib, **kw):
    """Every tolerance explicit: nothing rejected unless the test says so."""
    base = dict(alpha_min=0.0, alpha_min_moments=0.0, max_history=32.0, normal_cos_min=-1.0, plane_tolerance=INF, albedo_floor=0.01, demodulate=0)
    base.update(kw)
    return render.make_temporal_params(lib, **base)


def _plane_frame(cam, rng, w=16, h=16, depth=4.0, colour=None, **kw):
    colour = rng.uniform(0.2, 1.5, (h, w, 3)) if colour is None else colour
    return tc.make_inputs(colour, tc.plane_points(cam, w, h, depth), **kw)


def test_default_params_are_what_the_header_says(lib):
    t = abi.ShmTemporalParams()
    assert lib.shm_temporal_default_params(C.byref(t)) == 0
    got = (t.alpha_min, t.alpha_min_moments, t.max_history, t.normal_cos_min, t.plane_tolerance, t.albedo_floor, t.demodulate, t.reserved[0])
    assert got == tuple(np.float32(v) for v in (0.2, 0.2, 32.0, 0.9, 0.02, 0.01)) + (0, 0)
    assert lib.shm_temporal_default_params(None) == INVALID_ARGUMENT


def test_struct_layouts():
    assert C.sizeof(abi.ShmTemporalParams) == 32 and C.sizeof(abi.ShmTemporalPixel) == 64
    p = abi.ShmTemporalParams
    assert [getattr(p, n).offset for n in ("alpha_min", "alpha_min_moments", "max_history", "normal_cos_min", "plane_tolerance", "albedo_floor", "demodulate", "reserved")] == list(range(0, 32, 4))
    r = abi.ShmTemporalPixel
    assert [getattr(r, n).offset for n in ("rgb", "m1", "m2", "length", "p", "ns", "pad")] == [0, 12, 16, 20, 24, 36, 48]
    assert render.TEMPORAL_DTYPE.itemsize == 64 and [render.TEMPORAL_DTYPE.fields[n][1] for n in ("rgb", "m1", "m2", "length", "p", "ns", "pad")] == [0, 12, 16, 20, 24, 36, 48]


@pytest.mark.parametrize("alpha_min,alpha_min_moments,max_history", [(0.0, 0.0, 32.0), (0.2, 0.2, 32.0), (0.0, 0.2, 3.0), (0.2, 0.0, 3.0)])
def test_the_recurrence_bit_for_bit(lib, alpha_min, alpha_min_moments, max_history):
    """Still camera, constant guide, 6 frames of random colours: rgb, m1, m2 and length after every frame are the numpy restatement's bits."""
    rng = np.random.default_rng(5)
    cam = tc.camera(lib)
    k = _params(lib, alpha_min=alpha_min, alpha_min_moments=alpha_min_moments, max_history=max_history)
    rec, want = None, None
    for f in range(6):
        film, g = _plane_frame(cam, rng)
        c = tc.colour_of(film)
        want = tc.start(c) if want is None else tc.blend(want, c, alpha_min, alpha_min_moments, max_history)
        rec, out = render.temporal_accumulate_host(lib, film, g, tc.WHITE, cam, rec, cam if rec is not None else None, k)
        tc.assert_record_is(rec, want, what=f"frame {f}")
        assert np.array_equal(tc.bits(tc.result_rgb(out)), tc.bits(want[0])) and (out["weight_sum"] == 1.0).all()  # (a_eff = 1: the result is rgb)
        assert (want[3] == min(f + 1, max_history)).all()
    assert max_history > 3 or (rec["length"] == 3.0).all()  # saturated


def test_the_recurrence_demodulated(lib):
    """demodulate = 1 under an albedo of 1/2: the history holds c / a_eff, the result is rgb a_eff; a_eff restated in float32 from the sums."""
    rng = np.random.default_rng(6)
    cam = tc.camera(lib)
    k = _params(lib, alpha_min=0.2, alpha_min_moments=0.2, demodulate=1)
    rec, want = None, None
    for f in range(4):
        film, g = _plane_frame(cam, rng, albedo=np.full((16, 16, 3), 0.5), weight=3.0)
        wh = g["weight_hit"].astype(np.float32)
        a = (g["albedo"].astype(np.float32) / wh[..., None]) / tc.WHITE.astype(np.float32)
        cov = np.clip(wh / g["weight_sum"].astype(np.float32), np.float32(0), np.float32(1))[..., None]
        a_eff = cov * a + (tc.F1 - cov)
        assert (np.abs(a_eff - 0.5) < 1e-6).all()
        c1 = tc.colour_of(film) / a_eff
        want = tc.start(c1) if want is None else tc.blend(want, c1, 0.2, 0.2, 32.0)
        rec, out = render.temporal_accumulate_host(lib, film, g, tc.WHITE, cam, rec, cam if rec is not None else None, k)
        tc.assert_record_is(rec, want, what=f"frame {f}")
        assert np.array_equal(tc.bits(tc.result_rgb(out)), tc.bits(want[0] * a_eff))


def test_identical_frames_give_the_frame(lib):
    rng = np.random.default_rng(7)
    cam = tc.camera(lib)
    film, g = _plane_frame(cam, rng)
    c = tc.colour_of(film)
    for alpha in (0.0, 0.2):
        k, rec = _params(lib, alpha_min=alpha, alpha_min_moments=alpha), None
        for f in range(5):
            rec, out = render.temporal_accumulate_host(lib, film, g, tc.WHITE, cam, rec, cam if rec is not None else None, k)
            assert np.array_equal(tc.bits(tc.result_rgb(out)), tc.bits(c)), f
        assert (rec["length"] == 5.0).all()


@pytest.mark.parametrize("kind", ["perspective", "orthographic", "tilted"])
def test_a_still_camera_is_the_identity_map(lib, kind):
    """Frame 2's history at every pixel is frame 1's record of that pixel — weights (1, 0, 0, 0) — although frame 2's P moved inside the pixel's footprint, as the mean of
    other jittered samples does: the motion vector is a difference of two projections of the same P."""
    rng = np.random.default_rng(8)
    w, h = 19, 13
    if kind == "tilted":  # a general rotation: no matrix entry is a power of two
        p = tc.camera_params(res=(w, h), fov=47.0)
        a, b = np.radians(23.0), np.radians(-11.0)
        ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        m = np.eye(4, dtype=np.float32)
        m[:3, :3] = ry @ rx
        m[:3, 3] = (0.3, -1.7, 2.9)
        p.world_from_camera[:] = [float(x) for x in m.ravel()]
        cam = tc.make_camera(lib, p)[0]
    else:
        cam = tc.camera(lib, res=(w, h), orthographic=kind == "orthographic", pos=(0.37, -0.21, 1.3))
    k = _params(lib, alpha_min=0.1, alpha_min_moments=0.3)
    normal = np.tile(-np.array(cam.render_from_camera[:], np.float64).reshape(4, 4)[:3, 2], (h, w, 1))  # facing the camera
    film1, g1 = tc.make_inputs(rng.uniform(0.2, 1.5, (h, w, 3)), tc.plane_points(cam, w, h, 4.0), normal=normal)
    rec1, _ = render.temporal_accumulate_host(lib, film1, g1, tc.WHITE, cam, None, None, k)
    film2, g2 = tc.make_inputs(rng.uniform(0.2, 1.5, (h, w, 3)), tc.plane_points(cam, w, h, 4.0, offset=rng.uniform(-0.45, 0.45, (h, w, 2))), normal=normal)
    rec2, _ = render.temporal_accumulate_host(lib, film2, g2, tc.WHITE, cam, rec1, cam, k)
    tc.assert_record_is(rec2, tc.blend(tc.record_fields(rec1), tc.colour_of(film2), 0.1, 0.3, 32.0), what=kind)
    assert (rec2["length"] == 2.0).all()
    assert np.array_equal(rec2["p"], (g2["p"] / g2["weight_hit"][..., None]).astype(np.float32))  # the record keeps THIS frame's P


@pytest.mark.parametrize("move,shift", [(0.5, 1.0), (0.25, 0.5)])
def test_known_motion(lib, move, shift):
    """A fronto-parallel plane at depth 4 under a 90-degree camera on a 16 x 16 film: one pixel is 0.5 scene units wide there. The camera steps sideways (+x) between the
    frames, so a point seen at column x was seen at column x + shift: frame 2's history is frame 1's ramp shifted by a pixel, or the mean of two neighbours."""
    w = h = 16
    cam1, cam2 = tc.camera(lib), tc.camera(lib, pos=(move, 0.0, 0.0))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ramp = np.stack([1.0 + 0.25 * xx + 0.125 * yy, 2.0 + 0.5 * xx, 0.5 + 0.0625 * yy], axis=-1)
    k = _params(lib)
    film1, g1 = tc.make_inputs(ramp, tc.plane_points(cam1, w, h, 4.0))
    rec1, _ = render.temporal_accumulate_host(lib, film1, g1, tc.WHITE, cam1, None, None, k)
    film2, g2 = tc.make_inputs(np.zeros((h, w, 3)), tc.plane_points(cam2, w, h, 4.0))  # c = 0, a = 1/2: rgb = h / 2
    rec2, _ = render.temporal_accumulate_host(lib, film2, g2, tc.WHITE, cam2, rec1, cam1, k)
    hist = 2.0 * rec2["rgb"].astype(np.float64)
    if shift == 1.0:
        assert (rec2["length"][:, :-1] == 2.0).all()
        np.testing.assert_allclose(hist[:, :-1], ramp[:, 1:], rtol=1e-4, atol=0)
        assert (rec2["length"][:, -1] == 1.0).all(), "the column whose source left the film did not start over"
        assert (rec2["rgb"][:, -1] == 0.0).all()
    else:
        assert (rec2["length"] == 2.0).all()
        np.testing.assert_allclose(hist[:, :-1], 0.5 * (ramp[:, :-1] + ramp[:, 1:]), rtol=1e-4, atol=0)
        np.testing.assert_allclose(hist[:, -1], ramp[:, -1], rtol=1e-4, atol=0)  # one tap left inside: the weights are renormalised
    # moved back the other way, two pixels: the two leftmost columns have no source
    cam3 = tc.camera(lib, pos=(-1.0, 0.0, 0.0))
    film3, g3 = tc.make_inputs(np.zeros((h, w, 3)), tc.plane_points(cam3, w, h, 4.0))
    rec3, _ = render.temporal_accumulate_host(lib, film3, g3, tc.WHITE, cam3, rec1, cam1, k)
    assert (rec3["length"][:, :2] == 1.0).all() and (rec3["length"][:, 2:] == 2.0).all()
    np.testing.assert_allclose(2.0 * rec3["rgb"][:, 2:].astype(np.float64), ramp[:, :-2], rtol=1e-4, atol=0)


def test_rejection(lib):
    """The camera steps half a pixel, so every interior pixel has two taps of weight 1/2: x and x + 1 of its row. Column 6's records are spoiled in turn."""
    w = h = 16
    cam1, cam2 = tc.camera(lib), tc.camera(lib, pos=(0.25, 0.0, 0.0))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ramp = np.stack([1.0 + xx, 1.0 + xx, 1.0 + xx], axis=-1)
    base = _params(lib)
    film1, g1 = tc.make_inputs(ramp, tc.plane_points(cam1, w, h, 4.0))
    rec1, _ = render.temporal_accumulate_host(lib, film1, g1, tc.WHITE, cam1, None, None, base)
    film2, g2 = tc.make_inputs(np.zeros((h, w, 3)), tc.plane_points(cam2, w, h, 4.0))

    def history(rec, k):
        r, _ = render.temporal_accumulate_host(lib, film2, g2, tc.WHITE, cam2, rec, cam1, k)
        return 2.0 * r["rgb"][..., 0].astype(np.float64), r["length"]

    hist, length = history(rec1, base)
    np.testing.assert_allclose(hist[:, 5], 6.5, rtol=1e-4)
    # a normal turned 60 degrees: rejected under cos >= 0.9, counted under -1
    turned = rec1.copy()
    turned["ns"][:, 6] = (np.sin(np.radians(60.0)), 0.0, -np.cos(np.radians(60.0)))
    hist, length = history(turned, _params(lib, normal_cos_min=0.9))
    np.testing.assert_allclose(hist[:, 5], 6.0, rtol=1e-4)  # column 5 keeps its own tap only
    np.testing.assert_allclose(hist[:, 6], 8.0, rtol=1e-4)  # column 6 reads 6 (spoiled) and 7
    np.testing.assert_allclose(hist[:, 4], 5.5, rtol=1e-4)
    assert (length == 2.0).all()
    hist, _ = history(turned, _params(lib, normal_cos_min=-1.0))
    np.testing.assert_allclose(hist[:, 5], 6.5, rtol=1e-4)
    hist, _ = history(turned, _params(lib, normal_cos_min=0.4))  # cos 60 = 0.5 passes
    np.testing.assert_allclose(hist[:, 5], 6.5, rtol=1e-4)
    # off the plane by 0.5 at depth 4: rejected under 0.1 (x 4 = 0.4), counted under 0.2 (0.8) and under +inf
    off = rec1.copy()
    off["p"][:, 6, 2] += 0.5
    for tol, want in ((0.1, 6.0), (0.2, 6.5), (INF, 6.5)):
        hist, _ = history(off, _params(lib, plane_tolerance=tol))
        np.testing.assert_allclose(hist[:, 5], want, rtol=1e-4, err_msg=str(tol))
    # under an orthographic camera the tolerance is absolute
    o1, o2 = tc.camera(lib, orthographic=True), tc.camera(lib, orthographic=True, pos=(0.0625, 0.0, 0.0))  # the film is 2 units wide: half a pixel
    _, go1 = tc.make_inputs(ramp, tc.plane_points(o1, w, h, 4.0))
    _, go2 = tc.make_inputs(np.zeros((h, w, 3)), tc.plane_points(o2, w, h, 4.0))
    reco, _ = render.temporal_accumulate_host(lib, film1, go1, tc.WHITE, o1, None, None, base)
    reco["p"][:, 6, 2] += 0.5
    for tol, want in ((0.4, 6.0), (0.6, 6.5)):
        r, _ = render.temporal_accumulate_host(lib, film2, go2, tc.WHITE, o2, reco, o1, _params(lib, plane_tolerance=tol))
        np.testing.assert_allclose(2.0 * r["rgb"][:, 5, 0].astype(np.float64), want, rtol=1e-4, err_msg=f"orthographic {tol}")
    # a record without history
    empty = rec1.copy()
    empty["length"][:, 6] = 0.0
    hist, length = history(empty, base)
    np.testing.assert_allclose(hist[:, 5], 6.0, rtol=1e-4)
    # all taps rejected: the pixel restarts
    empty["length"][:, 5] = 0.0
    hist, length = history(empty, base)
    assert (length[:, 5] == 1.0).all() and (hist[:, 5] == 0.0).all() and (length[:, 4] == 2.0).all() and (length[:, 6] == 2.0).all()
    both = rec1.copy()
    both["ns"][:, 5:7] = (1.0, 0.0, 0.0)
    _, length = history(both, _params(lib, normal_cos_min=0.5))
    assert (length[:, 5] == 1.0).all() and (length[:, 4] == 2.0).all()
    # nothing rejected whatever the records' guides say
    wild = rec1.copy()
    wild["ns"][...] = (0.0, 0.0, 1.0)
    wild["p"][..., 2] += 100.0
    hist, length = history(wild, _params(lib, normal_cos_min=-1.0, plane_tolerance=INF))
    assert (length == 2.0).all()
    np.testing.assert_allclose(hist[:, 5], 6.5, rtol=1e-4)


def test_degenerate_input(lib):
    """Pixels without a usable guide pass through — c, bit for bit, and a record of length 0 —; a point behind the previous camera, or a motion that is not finite,
    restarts; nothing crashes and no other pixel changes."""
    rng = np.random.default_rng(9)
    w, h = 16, 16
    cam1 = tc.camera(lib)
    k = _params(lib)
    film1, g1 = _plane_frame(cam1, rng)
    rec1, _ = render.temporal_accumulate_host(lib, film1, g1, tc.WHITE, cam1, None, None, k)
    film2, g2 = _plane_frame(cam1, rng)
    clean_rec, clean_out = render.temporal_accumulate_host(lib, film2, g2, tc.WHITE, cam1, rec1, cam1, k)
    g2["p"][2, 3] = (np.nan, 0.0, 4.0)
    g2["p"][2, 4] = (np.inf, 0.0, 4.0)
    g2["p"][2, 5, 2] = -np.inf
    g2["weight_hit"][3, 3] = 0.0
    g2["weight_hit"][3, 4] = -1.0
    film2["weight_sum"][4, 3] = 0.0
    film2["weight_sum"][4, 4] = -2.0
    g2["ns"][5, 3] = 0.0
    film2["rgb_sum"][5, 4, 1] = np.nan
    g2["albedo"][5, 5] = np.nan
    spoiled = np.zeros((h, w), bool)
    for y, x in ((2, 3), (2, 4), (2, 5), (3, 3), (3, 4), (4, 3), (4, 4), (5, 3), (5, 4)):
        spoiled[y, x] = True
    for demodulate in (0, 1):
        kk = _params(lib, demodulate=demodulate)
        rec, out = render.temporal_accumulate_host(lib, film2, g2, tc.WHITE, cam1, rec1, cam1, kk)
        if demodulate:
            spoiled[5, 5] = True  # (the albedo is read only when demodulating)
        c = tc.colour_of(film2)
        assert np.array_equal(tc.bits(tc.result_rgb(out))[spoiled], tc.bits(c)[spoiled])
        assert (rec["length"][spoiled] == 0.0).all() and (rec["rgb"][spoiled] == 0.0).all() and (rec["p"][spoiled] == 0.0).all()
        assert out["weight_sum"][4, 3] == 0.0 and (out["weight_sum"][~spoiled] == 1.0).all()
        if not demodulate:
            assert rec[~spoiled].tobytes() == clean_rec[~spoiled].tobytes() and out[~spoiled].tobytes() == clean_out[~spoiled].tobytes()
    # the previous camera has the plane behind it (it stood beyond the plane, z = 9, looking the same way): no history anywhere
    behind = tc.camera(lib, pos=(0.0, 0.0, 9.0))
    film3, g3 = _plane_frame(cam1, rng)
    rec, out = render.temporal_accumulate_host(lib, film3, g3, tc.WHITE, cam1, rec1, behind, k)
    assert (rec["length"] == 1.0).all() and np.array_equal(tc.bits(tc.result_rgb(out)), tc.bits(tc.colour_of(film3)))
    # ... and on its plane exactly (z = 4: depth 0)
    on = tc.camera(lib, pos=(0.0, 0.0, 4.0))
    rec, _ = render.temporal_accumulate_host(lib, film3, g3, tc.WHITE, cam1, rec1, on, k)
    assert (rec["length"] == 1.0).all()
    # positions so large that the projection overflows: finite P, a motion that is not
    g3["p"][...] = np.float32(3e38)
    rec, out = render.temporal_accumulate_host(lib, film3, g3, tc.WHITE, cam1, rec1, cam1, k)
    assert np.isin(rec["length"], (0.0, 1.0)).all() and np.array_equal(tc.bits(tc.result_rgb(out)), tc.bits(tc.colour_of(film3)))
    # records that hold garbage where their length is 0 are not read into anyone's history
    junk = rec1.copy()
    junk["length"][...] = 0.0
    junk["rgb"][...] = np.nan
    film4, g4 = _plane_frame(cam1, rng)
    rec, out = render.temporal_accumulate_host(lib, film4, g4, tc.WHITE, cam1, junk, cam1, k)
    assert (rec["length"] == 1.0).all() and np.array_equal(tc.bits(tc.result_rgb(out)), tc.bits(tc.colour_of(film4)))


def test_parameter_and_argument_errors(lib):
    rng = np.random.default_rng(10)
    cam = tc.camera(lib)
    film, g = _plane_frame(cam, rng)
    rec, _ = render.temporal_accumulate_host(lib, film, g, tc.WHITE, cam, None, None, _params(lib))
    for bad, word in ((dict(alpha_min=-0.1), "alpha_min"), (dict(alpha_min=1.5), "alpha_min"), (dict(alpha_min=float("nan")), "alpha_min"),
                      (dict(alpha_min_moments=2.0), "alpha_min_moments"), (dict(max_history=0.5), "max_history"), (dict(max_history=float("nan")), "max_history"),
                      (dict(normal_cos_min=1.5), "normal_cos_min"), (dict(normal_cos_min=-1.5), "normal_cos_min"), (dict(plane_tolerance=0.0), "plane_tolerance"),
                      (dict(plane_tolerance=float("nan")), "plane_tolerance"), (dict(albedo_floor=0.0), "albedo_floor"), (dict(albedo_floor=1.5), "albedo_floor")):
        with pytest.raises(abi.ShimmerHipError, match=word):
            render.temporal_accumulate_host(lib, film, g, tc.WHITE, cam, None, None, _params(lib, **bad))
    for ok in (dict(alpha_min=1.0), dict(max_history=1.0), dict(normal_cos_min=1.0), dict(plane_tolerance=INF), dict(albedo_floor=1.0), dict(max_history=INF)):
        render.temporal_accumulate_host(lib, film, g, tc.WHITE, cam, rec, cam, _params(lib, **ok))
    with pytest.raises(abi.ShimmerHipError, match="camera"):  # a history without the camera it was seen through
        render.temporal_accumulate_host(lib, film, g, tc.WHITE, cam, rec, None, _params(lib))
    k = _params(lib)
    w3 = (C.c_double * 3)(*tc.WHITE)
    out, ro = np.zeros(film.shape, render.FILM_DTYPE), np.zeros(film.shape, render.TEMPORAL_DTYPE)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.shm_temporal_accumulate_host(None, ptr(g), None, C.byref(cam), None, 16, 16, w3, C.byref(k), ptr(ro), ptr(out)) == INVALID_ARGUMENT and lib.shm_last_error()
    assert lib.shm_temporal_accumulate_host(ptr(film), ptr(g), None, C.byref(cam), None, 0, 16, w3, C.byref(k), ptr(ro), ptr(out)) == INVALID_ARGUMENT
    sph = abi.ShmCamera()
    ident = np.eye(4, dtype=np.float32)
    abi.check(lib, lib.shm_camera_spherical(ident.ctypes.data_as(abi.c_float_p), 0, (C.c_int32 * 2)(16, 16), abi.SHM_RENDER_SPACE_WORLD, C.byref(sph), None), "shm_camera_spherical")
    assert lib.shm_temporal_accumulate_host(ptr(film), ptr(g), None, C.byref(sph), None, 16, 16, w3, C.byref(k), ptr(ro), ptr(out)) == UNSUPPORTED and b"spherical" in lib.shm_last_error()
    assert lib.shm_temporal_accumulate_host(ptr(film), ptr(g), ptr(rec), C.byref(cam), C.byref(sph), 16, 16, w3, C.byref(k), ptr(ro), ptr(out)) == UNSUPPORTED
    # the filter over the temporal result: spatial variance only, temporal_variance 0 or 1
    res =render.temporal_accumulate_host(lib, film, g, tc.WHITE, cam, None, None, k)[1]
    with pytest.raises(abi.ShimmerHipError, match="variance_source"):
        render.denoise_temporal_host(lib, res, g, rec, tc.WHITE, render.make_denoise_params(lib, variance_source=abi.SHM_DENOISE_VARIANCE_MEASURED))
    with pytest.raises(abi.ShimmerHipError, match="temporal_variance"):
        render.denoise_temporal_host(lib, res, g, rec, tc.WHITE, None, temporal_variance=2)
    with pytest.raises(abi.ShimmerHipError, match="iterations"):
        render.denoise_temporal_host(lib, res, g, rec, tc.WHITE, render.make_denoise_params(lib, iterations=9))


def test_the_filter_over_the_temporal_result(lib):
    """temporal_variance = 0 is shm_denoise_host of the accumulated image; 1 differs from it exactly when some history holds four frames, and then only there does the
    initial variance come from the moments: with records whose m2 = m1^2 (variance 0 everywhere) and a finite sigma_luminance the filter passes nothing across a
    luminance step."""
    rng = np.random.default_rng(11)
    cam = tc.camera(lib)
    k = _params(lib)
    rec = None
    for f in range(5):
        film, g = _plane_frame(cam, rng)
        rec, res = render.temporal_accumulate_host(lib, film, g, tc.WHITE, cam, rec, cam if rec is not None else None, k)
        d = render.make_denoise_params(lib, iterations=2)
        plain = render.denoise_host(lib, res, g, tc.WHITE, d)
        assert render.denoise_temporal_host(lib, res, g, rec, tc.WHITE, d, temporal_variance=0).tobytes() == plain.tobytes()
        with_var = render.denoise_temporal_host(lib, res, g, rec, tc.WHITE, d, temporal_variance=1)
        assert (with_var.tobytes() != plain.tobytes()) == (f + 1 >= 4), f
    # a step image whose records claim no variance at all
    step = np.ones((16, 16, 3)); step[:, 8:] = 3.0
    film, g = tc.make_inputs(step, tc.plane_points(cam, 16, 16, 4.0))
    fake = rec.copy()
    fake["length"][...] = 8.0
    fake["m1"][...] = 2.0
    fake["m2"][...] = 4.0
    _, res = render.temporal_accumulate_host(lib, film, g, tc.WHITE, cam, None, None, k)
    out = render.denoise_temporal_host(lib, res, g, fake, tc.WHITE, render.make_denoise_params(lib, iterations=1, demodulate=0), temporal_variance=1)
    np.testing.assert_allclose(tc.result_rgb(out), step, rtol=1e-5)
    blurred = render.denoise_temporal_host(lib, res, g, fake, tc.WHITE, render.make_denoise_params(lib, iterations=1, demodulate=0), temporal_variance=0)
    assert np.abs(tc.result_rgb(blurred) - step).max() > 0.1


@pytest.mark.parametrize("space", [abi.SHM_RENDER_SPACE_CAMERA_WORLD, abi.SHM_RENDER_SPACE_WORLD])
@pytest.mark.parametrize("orthographic", [False, True])
def test_camera_create_in_reproduces_camera_create(lib, space, orthographic):
    p = tc.camera_params(pos=(0.3, -1.25, 2.5), res=(33, 21), fov=47.0, orthographic=orthographic, render_space=space)
    a, b = np.radians(31.0), np.radians(-17.0)
    m = np.array(p.world_from_camera[:], np.float32).reshape(4, 4)
    m[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    p.world_from_camera[:] = [float(x) for x in m.ravel()]
    p.frame_aspect_ratio = 1.5
    cam, rfw = tc.make_camera(lib, p)
    again = abi.ShmCamera()
    p.render_space = 77  # not read
    assert lib.shm_camera_create_in(C.byref(p), rfw.ctypes.data_as(abi.c_float_p), C.byref(again)) == 0
    assert bytes(again) == bytes(cam)
    # another pose in the same space: render_from_camera = render_from_world world_from_camera
    m[:3, 3] += (0.5, 0.25, -1.0)
    p.world_from_camera[:] = [float(x) for x in m.ravel()]
    assert lib.shm_camera_create_in(C.byref(p), rfw.ctypes.data_as(abi.c_float_p), C.byref(again)) == 0
    np.testing.assert_allclose(np.array(again.render_from_camera[:]).reshape(4, 4), rfw.reshape(4, 4).astype(np.float64) @ m.astype(np.float64), rtol=0, atol=1e-6)
    np.testing.assert_allclose(np.array(again.camera_from_render[:]).reshape(4, 4) @ np.array(again.render_from_camera[:]).reshape(4, 4), np.eye(4), atol=1e-5)
    assert again.camera_from_raster[:] == cam.camera_from_raster[:] and again.kind == cam.kind
    # refusals
    assert lib.shm_camera_create_in(None, rfw.ctypes.data_as(abi.c_float_p), C.byref(again)) == INVALID_ARGUMENT
    assert lib.shm_camera_create_in(C.byref(p), None, C.byref(again)) == INVALID_ARGUMENT
    p.kind = abi.SHM_CAMERA_SPHERICAL
    assert lib.shm_camera_create_in(C.byref(p), rfw.ctypes.data_as(abi.c_float_p), C.byref(again)) == INVALID_ARGUMENT


def test_camera_in_scene_and_the_builder_keep_the_render_space(lib):
    from shimmer_amd import scenes
    sc = scenes.cornell_box(lib, 24, 20)
    rfw = sc.builder.render_from_world
    assert rfw is not None and rfw.shape == (4, 4)
    same = render.camera_in_scene(lib, sc.builder, (0, 1, 3.4), (0, 1, 0), (0, 1, 0), fov=39.0)
    assert bytes(same) == bytes(sc.desc.camera)  # the scene's own pose, in the scene's render space: the scene's own camera
    moved = render.camera_in_scene(lib, rfw, (0.5, 1, 3.4), (0, 1, 0), (0, 1, 0), fov=39.0, full_resolution=(24, 20))
    assert bytes(moved) != bytes(same) and moved.camera_from_raster[:] == same.camera_from_raster[:]
    np.testing.assert_allclose(np.array(moved.render_from_camera[:]).reshape(4, 4)[:3, 3], (0.5, 0.0, 0.0), atol=1e-6)  # CameraWorld: the space is centred on the first camera
    with pytest.raises(ValueError):
        render.camera_in_scene(lib, rfw, (0, 1, 3), (0, 1, 0), (0, 1, 0))
