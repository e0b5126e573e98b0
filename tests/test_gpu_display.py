"""The display pass on the device (shm_display*) against its CPU twin, bit for bit — the twin fed with the film read back from the same scene.
Films: 24 x 20 (480 pixels: under two workgroups, the last one partial) and 70 x 45 (3150 pixels: 13 workgroups, a multiple of neither 64 nor 256), at 3 spp."""
import ctypes as C
import itertools

import numpy as np
import pytest

import display_cases as dc
import gbuffer_cases as gc
from shimmer_amd import abi, render
from test_gpu_denoise import SCENES

pytestmark = pytest.mark.gpu
INVALID_ARGUMENT = -1  # SHM_ERR_INVALID_ARGUMENT (include/shimmer_hip.h)
SOURCES = {"film": abi.SHM_DISPLAY_SOURCE_FILM, "denoised": abi.SHM_DISPLAY_SOURCE_DENOISED, "temporal": abi.SHM_DISPLAY_SOURCE_TEMPORAL}
ROWS = [("cornell", "film", 24, 20), ("textured", "film", 70, 45), ("escaped", "film", 24, 20), ("cornell", "denoised", 70, 45), ("coated", "denoised", 24, 20),
        ("cornell", "temporal", 24, 20), ("escaped", "temporal", 70, 45)]


def _rendered(lib, scene, w, h):
    """A scene with a film, a G-buffer, a temporal result and a denoised one, and the three read back."""
    sc = SCENES[scene](lib, w, h, None)
    params = gc.params_for("independent")
    r = render.Renderer(lib, sc.desc)
    film, _ = r.render(params)
    r.gbuffer(params)
    r.temporal_clear()
    r.temporal_accumulate()
    temporal = r.read_temporal()
    denoised = r.denoise()
    return sc, r, {"film": film, "denoised": denoised, "temporal": temporal}


def _same(r, lib, film, d, state):
    """One display call on the device and on the twin from `state`; asserts image, counts and state equal and returns (image, the twin's state)."""
    got, got_state = r.display(d, return_state=True)
    counts = r.read_display_histogram()
    want, want_counts, want_state = render.display_host(lib, film, r.width, r.height, d, state)
    bad = np.flatnonzero((got.reshape(-1, 4) != want.reshape(-1, 4)).any(axis=1))
    assert bad.size == 0, (bad[:8], got.reshape(-1, 4)[bad[:2]], want.reshape(-1, 4)[bad[:2]])
    assert dc.state_tuple(got_state) == dc.state_tuple(want_state), (got_state, want_state.as_dict())
    if d.auto_exposure:
        assert np.array_equal(counts, want_counts), np.flatnonzero(counts != want_counts)
    return got, want_state, counts


@pytest.mark.parametrize("scene,source,w,h", ROWS, ids=lambda v: str(v))
def test_device_matches_the_host_twin_bit_for_bit(gpu_lib, scene, source, w, h):
    sc, r, films = _rendered(gpu_lib, scene, w, h)
    try:
        film = films[source]
        for auto in (1, 0):
            for tonemap, transfer, dither in itertools.product(dc.CURVES, dc.TRANSFERS, (0, 1)):
                d = render.make_display_params(gpu_lib, source=SOURCES[source], tonemap=tonemap, transfer=transfer, dither=dither, auto_exposure=auto,
                                               output_rgb_from_sensor_rgb=render.SRGB_FROM_XYZ, exposure=1.0 if auto else 0.7)
                r.display_clear()
                got, state, counts = _same(r, gpu_lib, film, d, None)
                assert np.unique(got.reshape(-1, 4)[:, :3], axis=0).shape[0] > 8, "the image is (nearly) constant: the case checks nothing"
                if auto:
                    assert state.valid == 1 and 0 < state.counted <= w * h and counts.sum() == state.counted and (counts > 0).sum() > 4
                else:
                    assert state.valid == 0 and counts.sum() == 0
    finally:
        r.close()


EDGE_CASES = [(t, x, a) for t in dc.CURVES for x in dc.TRANSFERS for a in (0, 1)]


def _torch_worker(rank, out_path):
    # a fresh process that imports torch FIRST (torch ships its own HIP runtime: it must be the one the process initialises)
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    import torch
    torch.cuda.set_device(0)
    import display_cases as dc_
    from shimmer_amd import abi as abi_, render as render_, scenes as scenes_
    lib = abi_.load_library()
    film, _, _ = dc_.edge_film()
    sc = scenes_.cornell_box(lib, dc_.EDGE_W, dc_.EDGE_H)
    r = render_.Renderer(lib, sc.desc, device=0)
    out = {}
    try:
        r.clear()
        t = render_.film_tensor(r, device="cuda:0")
        assert t.numel() == film.size * 4
        t.copy_(torch.from_numpy(film.view(np.float64).reshape(-1).copy()))
        torch.cuda.synchronize()
        out["film"] = r.read_film().view(np.float64)
        for i, (tonemap, transfer, auto) in enumerate(EDGE_CASES):
            d = dc_.edge_params(lib, tonemap=tonemap, transfer=transfer, auto_exposure=auto, dither=int(tonemap == abi_.SHM_TONEMAP_ACES))
            r.display_clear()
            image, state = r.display(d, return_state=True)
            out[f"image{i}"], out[f"counts{i}"], out[f"state{i}"] = image, r.read_display_histogram(), np.array(dc_.state_tuple(state), np.int64)
        # shm_display_device_ptr: the image where it lies, as a torch view
        ptr, nbytes = r.display_device_ptr()

        class _Holder:
            pass

        holder = _Holder()
        holder.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}
        out["view"] = torch.as_tensor(holder, device="cuda:0").cpu().numpy()
        out["view_bytes"] = np.array([nbytes], np.int64)
    finally:
        r.close()
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def edge_on_the_device(gpu_lib, tmp_path_factory):
    """The edge film written into a scene's device film through render.film_tensor and displayed there, in one child process (torch must initialise the GPU first)."""
    import torch.multiprocessing as mp
    out = tmp_path_factory.mktemp("display") / "edge.npz"
    mp.spawn(_torch_worker, args=(str(out),), nprocs=1, join=True)
    return np.load(out)


def test_the_edge_film_on_the_device(gpu_lib, edge_on_the_device):
    got = edge_on_the_device
    film, bins, at = dc.edge_film()
    assert got["film"].tobytes() == film.tobytes(), "the film the device displayed is not the edge film"
    for i, (tonemap, transfer, auto) in enumerate(EDGE_CASES):
        d = dc.edge_params(gpu_lib, tonemap=tonemap, transfer=transfer, auto_exposure=auto, dither=int(tonemap == abi.SHM_TONEMAP_ACES))
        want, want_counts, want_state = render.display_host(gpu_lib, film, dc.EDGE_W, dc.EDGE_H, d)
        image = got[f"image{i}"]
        bad = np.flatnonzero((image.reshape(-1, 4) != want.reshape(-1, 4)).any(axis=1))
        assert bad.size == 0, (tonemap, transfer, auto, bad[:8], image.reshape(-1, 4)[bad[:2]], want.reshape(-1, 4)[bad[:2]])
        assert tuple(got[f"state{i}"].tolist()) == dc.state_tuple(want_state)
        assert np.array_equal(got[f"counts{i}"], want_counts)
        px = image.reshape(-1, 4)
        assert px[at["plus_inf"]].tolist() == [255, 0, 0, 255]
        for name in ("nan", "all_nan", "negative", "minus_inf", "both_inf", "black", "no_weight_black"):
            assert px[at[name]].tolist() == [0, 0, 0, 255], name
        if auto:
            assert np.array_equal(got[f"counts{i}"], dc.counts_of(bins)) and int(got[f"state{i}"][3]) == int((bins >= 0).sum())


def test_the_device_pointer_is_the_image(gpu_lib, edge_on_the_device):
    got = edge_on_the_device
    last = got[f"image{len(EDGE_CASES) - 1}"]
    assert int(got["view_bytes"][0]) == 4 * dc.EDGE_W * dc.EDGE_H
    assert np.array_equal(got["view"].reshape(dc.EDGE_H, dc.EDGE_W, 4), last) and (last[..., 3] == 255).all() and np.unique(last[..., 0]).size > 8


def test_a_sequence_adapts_as_the_twin_does(gpu_lib):
    sc = SCENES["cornell"](gpu_lib, 70, 45, None)
    r = render.Renderer(gpu_lib, sc.desc)
    params = render.make_params(seed=11, spp=16, max_depth=5)
    try:
        r.clear()
        r.display_clear()
        state, seen = None, []
        # (the key drops by three stops at the third frame: the exposure has somewhere to go)
        for f, (end, compensation, key) in enumerate(((1, 1.0, 0.18), (3, 0.5, 0.18), (7, 2.0, 0.0225), (16, 1.25, 0.0225))):
            r.render_waves(params, waves=[(0 if f == 0 else seen[-1], end)])
            seen.append(end)
            d = render.make_display_params(gpu_lib, auto_exposure=1, dt=1.0 / 30.0, exposure=compensation, key=key, output_rgb_from_sensor_rgb=render.SRGB_FROM_XYZ)
            _, state, _ = _same(r, gpu_lib, r.read_film(), d, state)
            assert f < 2 or abs(state.log2_exposure - state.log2_target) > 1.0, "nothing to adapt to: the frame checks no adaptation"
        r.display_clear()
        _, fresh, _ = _same(r, gpu_lib, r.read_film(), d, None)
        assert fresh.log2_exposure == fresh.log2_target and fresh.log2_exposure != state.log2_exposure
    finally:
        r.close()


def test_the_pass_reads_its_sources_and_writes_none(gpu_lib):
    sc = SCENES["cornell"](gpu_lib, 24, 20, None)
    params = gc.params_for("independent")
    r = render.Renderer(gpu_lib, sc.desc)
    try:
        out = np.zeros((20, 24), np.uint32)
        assert gpu_lib.shm_display_read(r.handle, out.ctypes.data_as(C.c_void_p)) == INVALID_ARGUMENT and b"display" in gpu_lib.shm_last_error()
        assert gpu_lib.shm_display_read_histogram(r.handle, out.ctypes.data_as(C.c_void_p)) == INVALID_ARGUMENT
        p, n = C.c_void_p(), C.c_uint64()
        assert gpu_lib.shm_display_device_ptr(r.handle, C.byref(p), C.byref(n)) == INVALID_ARGUMENT
        film, _ = r.render(params)
        for source, word in (("denoised", b"denoiser"), ("temporal", b"temporal")):
            d = render.make_display_params(gpu_lib, source=SOURCES[source])
            assert gpu_lib.shm_display_device(r.handle, C.byref(d), None, None) == INVALID_ARGUMENT and word in gpu_lib.shm_last_error()
        assert gpu_lib.shm_display_read(r.handle, out.ctypes.data_as(C.c_void_p)) == INVALID_ARGUMENT
        bad = render.make_display_params(gpu_lib, white=0.0)
        assert gpu_lib.shm_display_device(r.handle, C.byref(bad), None, None) == INVALID_ARGUMENT and b"white" in gpu_lib.shm_last_error()
        assert gpu_lib.shm_display_device(r.handle, None, None, None) == INVALID_ARGUMENT and gpu_lib.shm_display_device(None, C.byref(bad), None, None) == INVALID_ARGUMENT
        g, _ = r.gbuffer(params)
        r.temporal_clear()
        r.temporal_accumulate()
        temporal, denoised = r.read_temporal(), r.denoise()
        images = {}
        for source in SOURCES:
            for auto in (0, 1):
                ms = C.c_double(0.0)
                d = render.make_display_params(gpu_lib, source=SOURCES[source], auto_exposure=auto)
                assert gpu_lib.shm_display_device(r.handle, C.byref(d), None, C.byref(ms)) == 0 and ms.value > 0.0
                assert gpu_lib.shm_display_read(r.handle, out.ctypes.data_as(C.c_void_p)) == 0
                images[source, auto] = out.copy()
        assert r.read_film().tobytes() == film.tobytes(), "the display pass wrote into the film"
        assert r.read_temporal().tobytes() == temporal.tobytes(), "the display pass wrote into the temporal result"
        d_again = np.zeros((20, 24), dtype=render.FILM_DTYPE)
        abi.check(gpu_lib, gpu_lib.shm_denoise_read(r.handle, d_again.ctypes.data_as(C.c_void_p)), "shm_denoise_read")
        assert d_again.tobytes() == denoised.tobytes(), "the display pass wrote into the denoiser's result"
        assert r.read_gbuffer().tobytes() == g.tobytes()
        assert not np.array_equal(images["film", 0], images["denoised", 0]) and not np.array_equal(images["film", 0], images["film", 1])
    finally:
        r.close()




def test_the_examples_write_display_pictures(gpu_lib, tmp_path):
    """examples/render_scene.py with the display options (pictures only: no .pfm, and every frame's .png decodes) and examples/render_pbrt.c --png, whose picture is
    the twin's of the same film, bit for bit."""
    import shutil
    import subprocess
    import sys
    from pathlib import Path

    from test_pbrt_loader import S1_TEXT

    root = Path(__file__).resolve().parents[1]
    run = subprocess.run([sys.executable, str(root / "examples" / "render_scene.py"), "cornell", "--spp", "2", "--res", "32", "--frames", "2", "--orbit", "2", "--temporal",
                          "--denoise", "--tonemap", "reinhard", "--auto-exposure", "--dither", "--frame-time", "0.033", "-o", str(tmp_path / "seq.png")],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert not list(tmp_path.glob("*.pfm"))
    for name in ("seq.f000.png", "seq.f001.png", "seq.f000.denoised.png", "seq.f001.denoised.png"):
        picture = dc.decode_png((tmp_path / name).read_bytes())
        assert picture.shape == (32, 32, 3) and np.unique(picture).size > 16, name
    if not shutil.which("gcc"):
        pytest.fail("no host C compiler")
    exe, libdir = tmp_path / "render_pbrt", root / "shimmer_amd" / "csrc"
    subprocess.run(["gcc", "-O2", "-I", str(root / "include"), str(root / "examples" / "render_pbrt.c"), "-L", str(libdir), "-lshimmer_hip", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)], check=True)
    (tmp_path / "s1.pbrt").write_text(S1_TEXT)
    run = subprocess.run([str(exe), str(tmp_path / "s1.pbrt"), str(tmp_path / "s1.pfm"), "--spp", "8", "--png", str(tmp_path / "s1.png")], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    picture = dc.decode_png((tmp_path / "s1.png").read_bytes())
    loaded = C.POINTER(abi.ShmPbrtScene)()
    abi.check(gpu_lib, gpu_lib.shm_scene_parse_pbrt(S1_TEXT.encode(), None, C.byref(loaded)), "shm_scene_parse_pbrt")
    try:
        s = loaded.contents
        s.params.samples_per_pixel = 8
        r = render.Renderer(gpu_lib, s.desc)
        film, _ = r.render(s.params)
        r.close()
        d = render.make_display_params(gpu_lib, output_rgb_from_sensor_rgb=list(s.output_rgb_from_sensor_rgb))
    finally:
        gpu_lib.shm_pbrt_free(loaded)
    want, _, _ = render.display_host(gpu_lib, film, 48, 40, d)
    assert np.array_equal(picture, want[..., :3]) and np.unique(picture).size > 16


def test_render_frames_shows_the_last_stage(gpu_lib):
    sc = SCENES["cornell"](gpu_lib, 24, 20, None)
    params = render.make_params(seed=11, spp=6, max_depth=5)
    d = render.make_display_params(gpu_lib, auto_exposure=1, dt=1.0 / 30.0, key=0.3, output_rgb_from_sensor_rgb=render.SRGB_FROM_XYZ)
    plain = render.render_frames(gpu_lib, sc.desc, [None, None], params)
    assert all("display" not in f for f in plain)
    for dparams, stage in ((None, "temporal"), (render.make_denoise_params(gpu_lib), "denoised")):
        frames = render.render_frames(gpu_lib, sc.desc, [None, None], params, dparams=dparams, display=d)
        state = None
        for f, p in zip(frames, plain):
            assert f["temporal"].tobytes() == p["temporal"].tobytes() and f["image"].shape == p["image"].shape
            want, _, state = render.display_host(gpu_lib, f[stage], 24, 20, d, state)
            assert np.array_equal(f["display"], want) and dc.state_tuple(f["display_state"]) == dc.state_tuple(state)
    assert d.source == abi.SHM_DISPLAY_SOURCE_FILM  # the caller's struct is not written
