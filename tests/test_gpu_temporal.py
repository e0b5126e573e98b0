"""The temporal pass on the device (shm_temporal_*, shm_denoise_temporal_device, shm_scene_set_camera) against its CPU twin, bit for bit — the twin
fed with the film, the G-buffer and the previous records read back from the same scene —, against the plain render it must add up to under a still camera, and against a
1024-spp render: does it denoise. Films: 24 x 20 (most taps near a border) and 70 x 45 (a multiple of neither 8 nor 64, several workgroups both ways), 3 spp a frame."""
import ctypes as C

import numpy as np
import pytest

import temporal_cases as tc
from shimmer_amd import abi, render, scenes
from test_gpu_denoise import SCENES, _film

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT, UNSUPPORTED = -1, -2  # SHM_ERR_* (include/shimmer_hip.h)
INF = float("inf")
UP = (0.0, 1.0, 0.0)
SPP = 3  # per frame


def _differing(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    words = a.dtype.itemsize // 8
    return np.flatnonzero((a.view(np.uint64).reshape(-1, words) != b.view(np.uint64).reshape(-1, words)).any(axis=1))


def _frame(r, params, f, spp, cam=None):
    """Frame f of a sequence: the camera, cleared film and G-buffer, samples [f spp, (f + 1) spp) into both."""
    if cam is not None:
        r.set_camera(cam)
    r.clear()
    r.gbuffer_clear()
    r.render_waves(params, waves=[(f * spp, (f + 1) * spp)])
    r.gbuffer_wave(params, f * spp, (f + 1) * spp)


def _cameras(lib, sc, name, motion):
    fov = tc.VIEWS[name][2]
    return [None if v is None else render.camera_in_scene(lib, sc.builder, v[0], v[1], UP, fov=fov) for v in tc.sequence(name, motion)]


@pytest.mark.parametrize("scene,sampler,filt,demodulate,motion,w,h", tc.ROWS, ids=lambda v: str(v))
def test_device_matches_the_host_twin_bit_for_bit(gpu_lib, scene, sampler, filt, demodulate, motion, w, h):
    sc = SCENES[scene](gpu_lib, w, h, _film(filt))
    params = render.make_params(seed=11, spp=3 * SPP, max_depth=5, sampler=sampler)
    k = render.make_temporal_params(gpu_lib, alpha_min=0.2, alpha_min_moments=0.2, max_history=32.0, normal_cos_min=0.9, plane_tolerance=0.02, albedo_floor=0.01,
                                    demodulate=demodulate)
    white = render.gbuffer_white(gpu_lib, sc.desc)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        r.temporal_clear()
        rec, prev_cam, cur_cam = None, None, sc.desc.camera
        grown = restarted = passed = 0
        for f, cam in enumerate(_cameras(gpu_lib, sc, scene, motion)):
            cur_cam = cam if cam is not None else cur_cam
            _frame(r, params, f, SPP, cam)
            r.temporal_accumulate(k)
            film, g = r.read_film(), r.read_gbuffer()
            got, got_rec = r.read_temporal(), r.read_temporal_history()
            want_rec, want = render.temporal_accumulate_host(gpu_lib, film, g, white, cur_cam, rec, prev_cam, k)
            bad, bad_rec = _differing(got, want), _differing(got_rec, want_rec)
            assert bad.size == 0, (f, bad[:8], got.ravel()[bad[:1]], want.ravel()[bad[:1]])
            assert bad_rec.size == 0, (f, bad_rec[:8], got_rec.ravel()[bad_rec[:1]], want_rec.ravel()[bad_rec[:1]])
            valid = got_rec["length"] > 0
            assert valid.any(), "no pixel has a guide: the case checks nothing"
            assert f == 0 or _differing(got[valid], film[valid]).size > 0
            grown += int((got_rec["length"] > 1).sum())
            restarted += int(f > 0) * int((got_rec["length"] == 1).sum())
            passed += int((~valid).sum())
            if (~valid).any():
                c = render.film_to_rgb(film)
                assert np.array_equal(got["rgb_sum"].astype(np.float32)[~valid].view(np.uint32), c[~valid].view(np.uint32))
            rec, prev_cam = got_rec, cur_cam
        assert grown > 0, "no pixel ever had a history"
        assert motion == "still" or restarted > 0, "no pixel restarted under a moving camera"
        assert scene != "escaped" or passed > 0, "no pass-through pixel"
    finally:
        r.close()


@pytest.mark.parametrize("scene", ["cornell", "textured"])
def test_set_camera_renders_what_a_scene_created_with_that_camera_renders(gpu_lib, scene):
    """Scene A, set to camera B, against a scene created from the same description with camera B: film and G-buffer, bit for bit (the textured box reads the
    camera in its ray-differential fallback)."""
    sc = SCENES[scene](gpu_lib, 24, 20, None)
    pos, look = tc.orbit(tc.VIEWS[scene], 7.0, dolly=0.4)
    cam_b = render.camera_in_scene(gpu_lib, sc.builder, pos, look, UP, fov=tc.VIEWS[scene][2])
    params = render.make_params(seed=11, spp=SPP, max_depth=5, sampler="zsobol")
    a = render.Renderer(gpu_lib, sc.desc)
    try:
        film_a, _ = a.render(params)
        a.set_camera(cam_b)
        film_ab, _ = a.render(params)
        g_ab, _ = a.gbuffer(params)
        ortho = abi.ShmCamera.from_buffer_copy(bytes(cam_b))
        ortho.kind = abi.SHM_CAMERA_ORTHOGRAPHIC
        assert gpu_lib.shm_scene_set_camera(a.handle, C.byref(ortho)) == INVALID_ARGUMENT and b"kind" in gpu_lib.shm_last_error()
        assert gpu_lib.shm_scene_set_camera(a.handle, None) == INVALID_ARGUMENT
        assert a.render(params)[0].tobytes() == film_ab.tobytes()  # the refused camera changed nothing
        a.render_sharded(params)  # leaves multi-GPU state behind: the camera is fixed until shm_dist_finalize
        assert gpu_lib.shm_scene_set_camera(a.handle, C.byref(cam_b)) == UNSUPPORTED and b"multi-GPU" in gpu_lib.shm_last_error()
        assert gpu_lib.shm_dist_finalize(a.handle) == 0
        a.set_camera(sc.desc.camera)
        assert a.render(params)[0].tobytes() == film_a.tobytes()  # and back
    finally:
        a.close()
    desc_camera = abi.ShmCamera.from_buffer_copy(bytes(sc.desc.camera))
    sc.desc.camera = cam_b
    b = render.Renderer(gpu_lib, sc.desc)
    try:
        film_b, _ = b.render(params)
        g_b, _ = b.gbuffer(params)
    finally:
        b.close()
        sc.desc.camera = desc_camera
    assert film_ab.tobytes() == film_b.tobytes() and g_ab.tobytes() == g_b.tobytes()
    assert film_a.tobytes() != film_b.tobytes()


@pytest.mark.parametrize("sampler", ["independent", "zsobol"])
def test_accumulating_waves_is_the_plain_render(gpu_lib, sampler):
    """Still camera, alpha_min 0, nothing rejected, box filter, demodulate 0: 8 frames of 3 samples each are a running mean of 8 equal-weight means, the 24-spp render's c
    up to rounding. Per frame one subtraction, one product and one sum — 3 roundings of values no larger than the pixel's largest per-frame value, a few ulp with the
    rounding of a = 1 / length and of c itself —, over 8 frames, doubled: 64 * 2^-24 of that value."""
    sc = SCENES["cornell"](gpu_lib, 24, 20, None)
    params = render.make_params(seed=11, spp=24, max_depth=5, sampler=sampler)
    k = render.make_temporal_params(gpu_lib, alpha_min=0.0, alpha_min_moments=0.0, max_history=8.0, normal_cos_min=-1.0, plane_tolerance=INF, albedo_floor=0.01, demodulate=0)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        plain = render.film_to_rgb(r.render(params)[0]).astype(np.float64)
        r.temporal_clear()
        largest = np.zeros(plain.shape[:2])
        for f in range(8):
            _frame(r, params, f, 3)
            r.temporal_accumulate(k)
            largest = np.maximum(largest, np.abs(render.film_to_rgb(r.read_film()).astype(np.float64)).max(-1))
        rec = r.read_temporal_history()
        # (a pixel whose three samples all missed the box in some frame passed through there and started over: its history is not the eight frames')
        valid = rec["length"] == 8.0
        assert valid.mean() > 0.9 and np.isin(rec["length"], np.arange(9.0)).all()
        got = r.read_temporal()["rgb_sum"]
        err = np.abs(got - plain)[valid]
        bound = (64 * 2.0 ** -24 * largest)[valid][:, None]
        print(f"{sampler}: largest |accumulated - plain| / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    finally:
        r.close()


_TRUTH = {}


def _truth(lib, r, key):
    """The 1024-spp image of the renderer's current view."""
    if key not in _TRUTH:
        film, _ = r.render(render.make_params(seed=3, spp=1024, max_depth=5, sampler="zsobol"))
        _TRUTH[key] = render.film_get_image(lib, film, render.SRGB_FROM_XYZ).astype(np.float64)
    return _TRUTH[key]


ORBIT_DEGREES = 1.0  # per frame: the slow orbit of the measured sequences (profiles/temporal.md)


def denoise_sequence(lib, seed, degrees, tparams, frames=8, spp=4, size=64, textured=False):
    """The 64 x 64 Cornell box, `frames` frames of `spp` disjoint samples each under an orbit of `degrees` a frame. MSEs against a 1024-spp render of the last view, over the
    covered pixels of the output-matrix image: the last noisy frame, the accumulated frame, the accumulated frame filtered (temporal_variance 0 and 1), the last frame
    filtered alone (shm_denoise)."""
    sc = scenes.cornell_box(lib, size, size, textured=textured)
    view = tc.VIEWS["cornell"]
    cams = [None] + [render.camera_in_scene(lib, sc.builder, *tc.orbit(view, degrees * f), UP, fov=view[2]) for f in range(1, frames)]
    params = render.make_params(seed=seed, spp=frames * spp, max_depth=5, sampler="zsobol")
    r = render.Renderer(lib, sc.desc)
    try:
        r.temporal_clear()
        for f, cam in enumerate(cams):
            _frame(r, params, f, spp, cam if degrees else None)
            r.temporal_accumulate(tparams)
        film, g, acc = r.read_film(), r.read_gbuffer(), r.read_temporal()
        tv0, tv1 = r.denoise_temporal(None, 0), r.denoise_temporal(None, 1)
        single = r.denoise()
        truth = _truth(lib, r, (size, textured, degrees * (frames - 1)))
    finally:
        r.close()
    covered = (g["weight_hit"] > 0) & (film["weight_sum"] > 0)
    assert covered.mean() > 0.5
    mse = lambda f: float(((render.film_get_image(lib, f, render.SRGB_FROM_XYZ).astype(np.float64) - truth)[covered] ** 2).mean())
    return {"noisy": mse(film), "accumulated": mse(acc), "filtered_tv0": mse(tv0), "filtered_tv1": mse(tv1), "single_frame_filtered": mse(single)}


def test_it_denoises_under_a_still_camera(gpu_lib):
    """alpha_min 0, demodulate 0: where the history holds, the accumulated frame is the plain mean of 8 frames, its MSE an eighth of one frame's in expectation; below a
    quarter asserted (a factor two for the spread of an MSE over 4 096 pixels). (With demodulate 1 it is no plain mean: a pixel on the emitter's edge is divided by one
    frame's a_eff and multiplied by another's — profiles/temporal.md has that sequence's figures.)"""
    k = render.make_temporal_params(gpu_lib, alpha_min=0.0, alpha_min_moments=0.0, max_history=32.0, normal_cos_min=0.9, plane_tolerance=0.02, albedo_floor=0.01, demodulate=0)
    m = denoise_sequence(gpu_lib, 7, 0.0, k)
    print(f"still camera, 8 x 4 spp: MSE noisy {m['noisy']:.5e}, accumulated {m['accumulated']:.5e} (ratio {m['accumulated'] / m['noisy']:.4f})")
    assert m["accumulated"] < 0.25 * m["noisy"]


ORBIT_SEEDS = (7, 8, 9, 10)
ORBIT_WORST = 0.1746    # the largest accumulated / noisy ratio of the four seeds as measured on an MI355X (0.0745, 0.1746, 0.1341, 0.1116: profiles/temporal.md)


def test_it_denoises_under_a_slow_orbit(gpu_lib):
    """Default parameters, one degree a frame. The bound is the worst ratio measured over the four seeds plus a quarter of the gap between it and 1
    (profiles/temporal.md holds the four values and the filtered ones)."""
    assert ORBIT_WORST is not None and ORBIT_WORST < 1.0
    bound = ORBIT_WORST + 0.25 * (1.0 - ORBIT_WORST)
    k = render.make_temporal_params(gpu_lib)
    for seed in ORBIT_SEEDS:
        m = denoise_sequence(gpu_lib, seed, ORBIT_DEGREES, k)
        ratio = m["accumulated"] / m["noisy"]
        print(f"orbit seed {seed}: MSE noisy {m['noisy']:.5e}, accumulated {m['accumulated']:.5e} (ratio {ratio:.4f}), filtered tv0 {m['filtered_tv0']:.5e} tv1 {m['filtered_tv1']:.5e}, "
              f"the last frame filtered alone {m['single_frame_filtered']:.5e}")
        assert ratio < bound and ratio < 1.0, (seed, ratio, bound)


@pytest.mark.parametrize("scene", ["cornell", "escaped"])
def test_inputs_untouched_and_repeatable(gpu_lib, scene):
    sc = SCENES[scene](gpu_lib, 24, 20, None)
    params = render.make_params(seed=11, spp=3 * SPP, max_depth=5, sampler="independent")
    aparams = render.make_adaptive_params(gpu_lib)
    cams = _cameras(gpu_lib, sc, scene, "orbit")
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        # what the single-frame passes give on a scene that never ran the temporal pass
        _frame(r, params, 0, SPP)
        r.moments_clear()
        r.render_waves(params, waves=[(SPP, 2 * SPP)])
        tiles_before = r.moments_update(aparams)
        moments_before, denoised_before = r.read_moments(), r.denoise()

        def run():
            r.temporal_clear()
            out = []
            for f, cam in enumerate(cams):
                _frame(r, params, f, SPP, cam if cam is not None else sc.desc.camera)
                film, g = r.read_film(), r.read_gbuffer()
                r.temporal_accumulate()
                assert r.read_film().tobytes() == film.tobytes(), "the pass wrote into the film"
                assert r.read_gbuffer().tobytes() == g.tobytes(), "the pass wrote into the G-buffer"
                out.append((r.read_temporal().tobytes(), r.read_temporal_history().tobytes(), r.denoise_temporal(None, 1).tobytes()))
            return out

        first = run()
        assert run() == first
        assert first[0][0] != first[1][0]
        r.set_camera(sc.desc.camera)
        _frame(r, params, 0, SPP)
        r.moments_clear()
        r.render_waves(params, waves=[(SPP, 2 * SPP)])
        assert r.moments_update(aparams).tobytes() == tiles_before.tobytes()
        assert r.read_moments().tobytes() == moments_before.tobytes() and r.denoise().tobytes() == denoised_before.tobytes()
    finally:
        r.close()


def test_the_filter_over_the_temporal_result_matches_its_twin(gpu_lib):
    sc = SCENES["textured"](gpu_lib, 70, 45, None)
    params = render.make_params(seed=11, spp=5 * SPP, max_depth=5, sampler="zsobol")
    white = render.gbuffer_white(gpu_lib, sc.desc)
    k = render.make_temporal_params(gpu_lib, alpha_min=0.2, alpha_min_moments=0.2, max_history=32.0, normal_cos_min=0.9, plane_tolerance=0.02, albedo_floor=0.01, demodulate=1)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        r.temporal_clear()
        for f in range(5):
            _frame(r, params, f, SPP)
            r.temporal_accumulate(k)
        acc, rec, g = r.read_temporal(), r.read_temporal_history(), r.read_gbuffer()
        assert (rec["length"] >= 4).any()
        outs = []
        for tv in (0, 1):
            for d in (render.make_denoise_params(gpu_lib), render.make_denoise_params(gpu_lib, iterations=2, demodulate=0)):
                got = r.denoise_temporal(d, tv)
                want = render.denoise_temporal_host(gpu_lib, acc, g, rec, white, d, tv)
                bad = _differing(got, want)
                assert bad.size == 0, (tv, bad[:8], got.ravel()[bad[:1]], want.ravel()[bad[:1]])
                outs.append(got.tobytes())
        assert outs[0] != outs[2], "the temporal variance changed nothing"
        assert r.read_temporal().tobytes() == acc.tobytes() and r.read_temporal_history().tobytes() == rec.tobytes()
    finally:
        r.close()


def test_rejections(gpu_lib):
    sc = SCENES["cornell"](gpu_lib, 24, 20, None)
    params = render.make_params(seed=11, spp=SPP, max_depth=5)
    k = render.make_temporal_params(gpu_lib)
    d = render.make_denoise_params(gpu_lib)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        r.render(params)
        ms = C.c_double(0.0)
        out = np.zeros((20, 24), render.FILM_DTYPE)
        assert gpu_lib.shm_temporal_read(r.handle, out.ctypes.data_as(C.c_void_p)) == INVALID_ARGUMENT and b"nothing to read" in gpu_lib.shm_last_error()
        assert gpu_lib.shm_denoise_temporal_device(r.handle, C.byref(d), 1, None) == INVALID_ARGUMENT and b"temporal" in gpu_lib.shm_last_error()
        assert gpu_lib.shm_temporal_accumulate_device(r.handle, C.byref(k), C.byref(ms)) == INVALID_ARGUMENT and b"G-buffer" in gpu_lib.shm_last_error()
        r.gbuffer_wave(params, 0, SPP, space=abi.SHM_GBUFFER_SPACE_CAMERA)
        assert gpu_lib.shm_temporal_accumulate_device(r.handle, C.byref(k), C.byref(ms)) == INVALID_ARGUMENT and b"SHM_GBUFFER_SPACE_RENDER" in gpu_lib.shm_last_error()
        r.gbuffer_clear()
        assert gpu_lib.shm_temporal_accumulate_device(r.handle, C.byref(k), C.byref(ms)) == INVALID_ARGUMENT and b"G-buffer" in gpu_lib.shm_last_error()
        r.gbuffer_wave(params, 0, SPP)
        with pytest.raises(abi.ShimmerHipError, match="plane_tolerance"):
            r.temporal_accumulate(render.make_temporal_params(gpu_lib, plane_tolerance=-1.0))
        assert gpu_lib.shm_temporal_accumulate_device(r.handle, None, None) == INVALID_ARGUMENT
        assert gpu_lib.shm_temporal_accumulate_device(r.handle, C.byref(k), C.byref(ms)) == 0 and ms.value > 0.0  # no shm_temporal_clear before: the first call allocates
        assert (r.read_temporal_history()["length"] == 1.0).any()
        measured = render.make_denoise_params(gpu_lib, variance_source=abi.SHM_DENOISE_VARIANCE_MEASURED)
        assert gpu_lib.shm_denoise_temporal_device(r.handle, C.byref(measured), 1, None) == INVALID_ARGUMENT and b"variance_source" in gpu_lib.shm_last_error()
        assert gpu_lib.shm_denoise_temporal_device(r.handle, C.byref(d), 2, None) == INVALID_ARGUMENT and b"temporal_variance" in gpu_lib.shm_last_error()
        assert gpu_lib.shm_denoise_temporal_device(r.handle, C.byref(d), 1, C.byref(ms)) == 0
        r.temporal_clear()
        assert gpu_lib.shm_temporal_read(r.handle, out.ctypes.data_as(C.c_void_p)) == INVALID_ARGUMENT
    finally:
        r.close()
    sph = scenes.cornell_box(gpu_lib, 24, 20, camera={"type": "spherical", "pos": (0.0, 1.0, 0.5)})
    r = render.Renderer(gpu_lib, sph.desc)
    try:
        r.render(params)
        r.gbuffer(params)
        assert gpu_lib.shm_temporal_accumulate_device(r.handle, C.byref(k), None) == UNSUPPORTED and b"spherical" in gpu_lib.shm_last_error()
    finally:
        r.close()


def test_render_frames_is_the_sequence_by_hand(gpu_lib):
    sc = SCENES["cornell"](gpu_lib, 24, 20, None)
    cams = _cameras(gpu_lib, sc, "cornell", "orbit")
    params = render.make_params(seed=11, spp=3 * SPP, max_depth=5, sampler="zsobol")
    d = render.make_denoise_params(gpu_lib, iterations=3)
    frames = render.render_frames(gpu_lib, sc.desc, cams, params, dparams=d, matrix=render.SRGB_FROM_XYZ)
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        r.temporal_clear()
        for f, cam in enumerate(cams):
            _frame(r, params, f, SPP, cam)
            r.temporal_accumulate()
            assert frames[f]["film"].tobytes() == r.read_film().tobytes() and frames[f]["temporal"].tobytes() == r.read_temporal().tobytes()
            den = r.denoise_temporal(d, 1)
            assert frames[f]["denoised"].tobytes() == den.tobytes() and frames[f]["temporal_ms"] > 0.0
            assert np.array_equal(frames[f]["image"], render.film_get_image(gpu_lib, den, render.SRGB_FROM_XYZ))
    finally:
        r.close()
    with pytest.raises(ValueError):
        render.render_frames(gpu_lib, sc.desc, cams, render.make_params(seed=11, spp=4))


def test_the_example_writes_the_frames(gpu_lib, tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "cornell.pfm"
    subprocess.run([sys.executable, os.path.join(root, "examples", "render_scene.py"), "cornell", "--spp", "4", "--res", "48", "--frames", "3", "--orbit", "2", "--temporal", "--denoise",
                    "-o", str(out)], check=True, timeout=120)
    names = [f"cornell.f{f:03d}{ext}" for f in range(3) for ext in (".pfm", ".png")]
    for name in names:
        assert (tmp_path / name).stat().st_size > 0, name
    assert (tmp_path / "cornell.f000.pfm").read_bytes() != (tmp_path / "cornell.f002.pfm").read_bytes()
