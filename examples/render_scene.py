#!/usr/bin/env python3
"""Render one of the repository's scenes on the GPU and write a PFM (and a tone-mapped PNG next to it).

    python examples/render_scene.py cornell --spp 256 --res 512 -o cornell.pfm
    python examples/render_scene.py cornell --filter gaussian        (box | gaussian | mitchell | sinc | triangle)
    python examples/render_scene.py textured | checkerboard | coated | patches | instanced | environment | ganesha | crown | spotlit | fuzz:13
    python examples/render_scene.py diffuse_transmission | translucent   (PBRT-v4's diffuse transmission material: the scene file / the builder)
    python examples/render_scene.py cornell --camera spherical [--mapping equirectangular]   (PBRT-v4's spherical camera in place of the scene's own)
    python examples/render_scene.py disk_and_cylinder | quadrics     (PBRT-v4's disk and cylinder: examples/scenes/disk_and_cylinder.pbrt / the builder)
    python examples/render_scene.py cutout | cutouts                 (PBRT-v4's shape alpha: examples/scenes/cutout.pbrt / the builder, scenes.cutout_scene)
    python examples/render_scene.py cornell_probe                    (examples/scenes/cornell_probe.pbrt: an equal-area probe in the middle of the Cornell box)
    python examples/render_scene.py cornell --spp 256 --adaptive 0.05 [--min-spp 16] [--batch-spp 4]   (adaptive sampling: --spp is the cap)
    python examples/render_scene.py cornell --spp 4 --frames 16 --orbit 1 --temporal [--denoise]        (a turntable accumulated over time: <name>.fNNN.pfm / .png per frame)
    python examples/render_scene.py cornell --integrator ambientocclusion [--ao-distance 0.5] [--spp 4 --frames 16 --orbit 1 --temporal --denoise --tonemap aces]   (PBRT-v4's ambient occlusion: the cheap frame)
    python examples/render_scene.py ambient_occlusion                (examples/scenes/integrators/ambient_occlusion.pbrt: the integrator named by the scene file)
    python examples/render_scene.py cornell --tonemap aces --auto-exposure [--dither] [--frames 16 --orbit 1 --frame-time 0.033]   (the .png from the display pass on the device: DESIGN.md section 4m)

Everything goes through the C ABI of include/shimmer_hip.h (shimmer_amd/abi.py is the ctypes binding): scene description ->
shm_scene_create -> shm_render_device -> shm_film_read -> shm_film_get_image -> shm_write_pfm. Needs an MI355X: there is no CPU path.
"""
import argparse
import ctypes as C
import os
import struct
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shimmer_amd import abi, render, scenes  # noqa: E402


def file_integrator(p, sc, args):
    """The integrator of a render: what the command line names; where it names none, what the scene file names (the ambient occlusion integrator with its two
    parameters: examples/scenes/integrators/ambient_occlusion.pbrt); "path" otherwise. --ao-distance and --ao-sampling, where given, override the file's values."""
    fp = getattr(sc, "file_params", None)
    if args.integrator is None and fp is not None and fp.integrator == abi.SHM_INTEGRATOR_AMBIENT_OCCLUSION:
        p.integrator = fp.integrator
        if args.ao_sampling is None:
            p.ao_uniform_sample = fp.ao_uniform_sample
        if args.ao_distance is None:
            p.ao_max_distance = fp.ao_max_distance
    return p


def make_scene(lib, name, w, h, film=None, camera=None):
    if camera is not None and (name in ("checkerboard", "diffuse_transmission", "cornell_probe", "disk_and_cylinder", "cutout", "ambient_occlusion") or name.startswith(("procedural", "fuzz:"))):
        raise SystemExit(f"--camera does not apply to {name}: a scene file has its own camera, and the procedural and fuzz generators take none")
    if name == "cornell":
        return scenes.cornell_box(lib, w, h, camera=camera, film=film)
    if name == "spotlit":  # the Cornell box under PBRT-v4's spot and distant lights as well (the *_dl kernels; examples/scenes/spot_and_sun.pbrt is the file form of such a scene)
        return scenes.cornell_box(lib, w, h, camera=camera, film=film, extra_lights=scenes.spot_and_distant(spot_from=(0.5, 1.7, 0.8), spot_to=(-0.2, 0.3, -0.2), sun_from=(0.3, 0.4, 3.0),
                                                                                             sun_to=(0.0, 0.8, 0.0)))
    if name == "textured":
        return scenes.cornell_box(lib, w, h, camera=camera, textured=True, film=film)
    if name == "coated":
        return scenes.cornell_box(lib, w, h, camera=camera, coated=True, film=film)
    if name in ("checkerboard", "diffuse_transmission", "cornell_probe", "disk_and_cylinder", "cutout", "ambient_occlusion"):
        # scene FILES through the C++ front end (their own film size; --filter is the file's): PBRT-v4's procedural textures (examples/scenes/checkerboard.pbrt); a back-lit
        # sheet of PBRT-v4's diffuse transmission material in the Cornell box (examples/scenes/diffuse_transmission.pbrt: the extended *_dl kernels); PBRT-v4's
        # spherical camera as an equal-area probe in the middle of the box (examples/scenes/cornell_probe.pbrt; the file's camera: --camera does not apply)
        # ; PBRT-v4's disk and cylinder as a lamp post whose emitter is a disk (examples/scenes/disk_and_cylinder.pbrt: the extended kernels and k_trace_quadrics.hip's)
        # ; PBRT-v4's shape alpha as a fence, a caged ball and a half-transparent veil in front of a wall (examples/scenes/cutout.pbrt: k_trace_alpha.hip's kernels)
        # ; PBRT-v4's ambient occlusion integrator, named by the file (examples/scenes/integrators/ambient_occlusion.pbrt: file_integrator below takes it over unless --integrator is given)
        import ctypes as C
        from types import SimpleNamespace
        out = C.POINTER(abi.ShmPbrtScene)()
        # (the scene that names another integrator than the oracle has lives one folder down: examples/scenes/*.pbrt are the files every integrator of the oracle renders)
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "scenes", *((["integrators"] if name == "ambient_occlusion" else []) + [name + ".pbrt"]))
        abi.check(lib, lib.shm_scene_load_pbrt(path.encode(), C.byref(out)), "shm_scene_load_pbrt")
        res = out.contents.desc.film.full_resolution
        return SimpleNamespace(desc=out.contents.desc, name=name + ".pbrt", res=(res[0], res[1]), keep=out, file_params=out.contents.params)
    if name == "translucent":  # the same material through the Python builder: the sheet and the tall box of scenes.cornell_box
        return scenes.cornell_box(lib, w, h, camera=camera, film=film, diffuse_transmission="sheet tall")
    if name in ("procedural", "procedural-general", "procedural-coated"):  # the same textures through the Python builder (scenes.procedural_cornell)
        return scenes.procedural_cornell(lib, w, h, which={"procedural": "checker", "procedural-general": "general", "procedural-coated": "coated"}[name], film=film)
    if name == "quadrics":  # the same shapes through the Python builder (scenes.quadric_scene)
        return scenes.quadric_scene(lib, "glass", w, h, film=film)
    if name == "cutouts":  # the same feature through the Python builder (scenes.cutout_scene)
        return scenes.cutout_scene(lib, "glass", w, h, film=film, disk=True, n_leaves=24)
    if name == "patches":
        return scenes.cornell_box(lib, w, h, camera=camera, patches=True, film=film)
    if name == "instanced":
        return scenes.instanced_scene(lib, w, h, camera=camera, film=film)
    if name == "environment":
        return scenes.three_spheres(lib, w, h, camera=dict(camera, pos=(0.75, 0.5, 9.0), look_at=(0.75, 0.5, 8.0)) if camera else (0.75, 0.5, 9.0), environment=scenes.environment_image(64), film=film)
    if name == "ganesha":
        return scenes.ganesha_proxy(lib, w, h, camera=camera, film=film)
    if name == "crown":
        return scenes.crown_proxy(lib, w, h, camera=camera, film=film)
    if name.startswith("fuzz:"):
        return scenes.random_scene(lib, int(name.split(":")[1]), w, h, film=film)
    raise SystemExit(f"unknown scene {name}")


# where the builders' cameras stand (shimmer_amd/scenes.py): position, what they look at, fov — what --orbit turns
VIEWS = {name: ((0.0, 1.0, 3.4), (0.0, 1.0, 0.0), 39.0) for name in ("cornell", "spotlit", "textured", "coated", "translucent", "patches")}
VIEWS.update(instanced=((0.0, 2.2, 7.0), (0.0, 0.8, 0.0), 40.0), ganesha=((0.0, 0.6, 4.2), (0.0, 0.0, 0.0), 38.0), crown=((0.0, 2.2, 7.5), (0.0, 1.2, 0.0), 32.0))


def orbit_camera(lib, sc, name, degrees):
    """The scene's camera turned by `degrees` about the vertical through what it looks at, in the scene's render space (render.camera_in_scene)."""
    pos, look, fov = (np.array(v, np.float64) for v in VIEWS[name])
    a = np.radians(degrees)
    rot = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    return render.camera_in_scene(lib, sc.builder, look + rot @ (pos - look), look, (0.0, 1.0, 0.0), fov=float(fov))


def write_png(path, rgb8):
    h, w, _ = rgb8.shape
    raw = b"".join(b"\x00" + rgb8[y].tobytes() for y in range(h))

    def chunk(tag, data):
        c = struct.pack(">I", len(data)) + tag + data
        return c + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def write_ldr_png(path, image, exposure):
    ldr = np.clip(image * exposure, 0.0, 1.0)
    ldr = np.where(ldr <= 0.0031308, 12.92 * ldr, 1.055 * np.power(ldr, 1 / 2.4) - 0.055)
    write_png(path, (ldr * 255 + 0.5).astype(np.uint8))


TONEMAPS = {"none": abi.SHM_TONEMAP_NONE, "reinhard": abi.SHM_TONEMAP_REINHARD, "aces": abi.SHM_TONEMAP_ACES}


class Pictures:
    """The script's .png files. Without a display option: the host arithmetic above on the float image. With one (--tonemap, --auto-exposure, --dither,
    --frame-time): the display pass on the stage's buffer where it lies on the device — 4 bytes per pixel come back — written by
    shm_write_png; --exposure is then the manual exposure or, with --auto-exposure, the compensation."""

    def __init__(self, lib, r, args):
        self.lib, self.r, self.args = lib, r, args
        self.on = args.tonemap is not None or args.auto_exposure or args.dither or args.frame_time is not None
        self.frame_scale = None  # the scale the frame's first picture was given: its other pictures take the same (one adaptation step per frame)
        if self.on and args.auto_exposure:
            r.display_clear()

    def next_frame(self):
        self.frame_scale = None

    def write(self, path, source, image=None):
        """source: abi.SHM_DISPLAY_SOURCE_*, the stage that produced the picture; image: its float image, for the host arithmetic."""
        a = self.args
        if not self.on:
            return write_ldr_png(path, image, a.exposure)
        metered = a.auto_exposure and self.frame_scale is None
        d = render.make_display_params(self.lib, source=source, tonemap=TONEMAPS[a.tonemap or "none"], dither=int(a.dither), auto_exposure=int(metered),
                                       exposure=a.exposure if metered or not a.auto_exposure else self.frame_scale, dt=a.frame_time or 0.0,
                                       output_rgb_from_sensor_rgb=render.SRGB_FROM_XYZ)
        rgba8, state = self.r.display(d, return_state=True)
        if metered:
            self.frame_scale = state["scale"]
        render.write_png(self.lib, path, rgba8)


def render_sequence(lib, args, sc, r, w, h):
    """--frames: one scene, one camera per frame, --spp new samples per frame; with --temporal the frames are accumulated (and, with --denoise, filtered)."""
    if args.adaptive is not None or args.aovs:
        raise SystemExit("--frames renders plain frames: no --adaptive, no --aovs")
    if args.orbit != 0.0 and (args.scene not in VIEWS or args.camera != "scene"):
        raise SystemExit(f"--orbit knows the cameras of {', '.join(VIEWS)} (and not --camera spherical)")
    if args.denoise and not args.temporal:
        raise SystemExit("--frames with --denoise filters the accumulated frame: add --temporal")
    p = render.make_params(seed=args.seed, spp=args.frames * args.spp, max_depth=args.max_depth, integrator=args.integrator or "path", reference_quirks=not args.quirks_off,
                           sampler=args.sampler, ao_max_distance=args.ao_distance or 0.0, ao_uniform_sample=args.ao_sampling == "uniform")
    p = file_integrator(p, sc, args)
    out = args.output or f"{args.scene.replace(':', '_')}.pfm"
    stem = os.path.splitext(out)[0]
    pictures = Pictures(lib, r, args)
    pfm = not (pictures.on and out.endswith(".png"))  # -o <name>.png with a display option: pictures only, and no float image is read back

    def write(path_stem, source, read):
        img = None
        if pfm:
            img = np.ascontiguousarray(render.film_get_image(lib, read(), render.SRGB_FROM_XYZ), np.float32)
            abi.check(lib, lib.shm_write_pfm(f"{path_stem}.pfm".encode(), img.ctypes.data_as(abi.c_float_p), w, h), "shm_write_pfm")
        pictures.write(f"{path_stem}.png", source, img)

    def denoise_temporal():
        """The filter over the accumulated frame, left on the device: (read, its milliseconds)."""
        ms = C.c_double(0.0)
        d = render.make_denoise_params(lib)
        abi.check(lib, lib.shm_denoise_temporal_device(r.handle, C.byref(d), 1, C.byref(ms)), "shm_denoise_temporal_device")

        def read():
            den = np.zeros((h, w), dtype=render.FILM_DTYPE)
            abi.check(lib, lib.shm_denoise_read(r.handle, den.ctypes.data_as(C.c_void_p)), "shm_denoise_read")
            return den
        return read, float(ms.value)

    if args.temporal:
        r.temporal_clear()
    for f in range(args.frames):
        pictures.next_frame()
        if args.orbit != 0.0 and f > 0:
            r.set_camera(orbit_camera(lib, sc, args.scene, args.orbit * f))
        r.clear()
        t0 = time.perf_counter()
        r.render_waves(p, waves=[(f * args.spp, (f + 1) * args.spp)])
        dt = time.perf_counter() - t0
        text = f"frame {f}: {args.spp} spp in {dt * 1e3:.1f} ms"
        if args.temporal:
            r.gbuffer_clear()
            r.gbuffer_wave(p, f * args.spp, (f + 1) * args.spp)
            ms = r.temporal_accumulate(return_ms=True)
            write(f"{stem}.f{f:03d}", abi.SHM_DISPLAY_SOURCE_TEMPORAL, r.read_temporal)
            text += f", accumulated in {ms:.3f} ms"
            if args.denoise:
                read, dms = denoise_temporal()
                write(f"{stem}.f{f:03d}.denoised", abi.SHM_DISPLAY_SOURCE_DENOISED, read)
                text += f", filtered in {dms:.3f} ms"
        else:
            write(f"{stem}.f{f:03d}", abi.SHM_DISPLAY_SOURCE_FILM, r.read_film)
        print(text)
    kinds = (".pfm, .png" if pfm else ".png") + ((", .denoised.pfm, .denoised.png" if pfm else ", .denoised.png") if args.denoise else "")
    print(f"wrote {stem}.f000 .. f{args.frames - 1:03d} ({kinds})")
    r.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--height", type=int, default=0)
    ap.add_argument("--max-depth", type=int, default=5)
    ap.add_argument("--integrator", default=None, choices=["path", "simplepath", "randomwalk", "ambientocclusion"],
                    help="ambientocclusion: PBRT-v4's AO integrator — a clay render, one short occlusion ray per sample (DESIGN.md section 4o); every other option composes with it. Default: the scene file's integrator where it names this one, else path")
    ap.add_argument("--ao-distance", type=float, default=None, metavar="D", help="with the ambient occlusion integrator: the occlusion rays' length (0: unbounded; default: the scene file's, else 0)")
    ap.add_argument("--ao-sampling", default=None, choices=["cosine", "uniform"], help="with the ambient occlusion integrator: the hemisphere sampling (default: the scene file's, else cosine)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--exposure", type=float, default=1.0)
    ap.add_argument("--sampler", default="independent", choices=["independent", "zsobol"], help="ShmRenderParams::sampler (DESIGN.md \"Sampler\")")
    ap.add_argument("--filter", default="box", choices=["box", "gaussian", "mitchell", "sinc", "triangle"],
                    help="the pixel filter, at PBRT-v4's default radius and parameters (DESIGN.md \"Pixel filters\")")
    ap.add_argument("--camera", default="scene", choices=["scene", "spherical"], help="spherical: PBRT-v4's spherical camera where the scene's own camera stands "
                                                                                    "(the generators' camera= argument; DESIGN.md section 4g)")
    ap.add_argument("--mapping", default="equalarea", choices=["equalarea", "equirectangular"], help="with --camera spherical")
    ap.add_argument("--quirks-off", action="store_true",
                    help="ShmRenderParams::disable_reference_quirks: PBRT-v4's forms of the reference's deviations (emitter sampling, instancing, ...: DESIGN.md section 2) "
                         "instead of the reference-exact default")
    ap.add_argument("--aovs", action="store_true", help="also write the G-buffer pass's albedo, normal (shading) and position images beside the beauty, as PFM")
    ap.add_argument("--denoise", action="store_true", help="run the G-buffer pass and the denoiser (DESIGN.md section 4j) on the frame and write <name>.denoised.pfm and .png "
                                                           "beside the beauty")
    ap.add_argument("--adaptive", type=float, default=None, metavar="THRESHOLD",
                    help="adaptive sampling (DESIGN.md section 4k): --spp is the cap, a tile stops once every pixel's relative standard error is below THRESHOLD; also "
                         "writes <name>.spp.pfm (the per-pixel sample count) and <name>.variance.pfm (the variance of the pixel's mean, sensor RGB) beside the beauty")
    ap.add_argument("--min-spp", type=int, default=None, help="with --adaptive: samples every tile receives (a multiple of --batch-spp, at least twice it; default 16)")
    ap.add_argument("--batch-spp", type=int, default=None, help="with --adaptive: samples per batch (default 4)")
    ap.add_argument("--frames", type=int, default=0, metavar="N", help="a sequence of N frames of --spp samples each — frame f draws samples [f spp, (f + 1) spp) — written as "
                                                                       "<name>.fNNN.pfm and .png")
    ap.add_argument("--orbit", type=float, default=0.0, metavar="DEG", help="with --frames: the camera turns DEG degrees a frame about what it looks at (shm_scene_set_camera)")
    ap.add_argument("--temporal", action="store_true", help="with --frames: each frame is accumulated into a history reprojected through the G-buffer (DESIGN.md section 4l); "
                                                            "with --denoise the accumulated frame is filtered as well (<name>.fNNN.denoised.pfm and .png)")
    ap.add_argument("--tonemap", default=None, choices=sorted(TONEMAPS), help="the display pass's tone curve (DESIGN.md section 4m). This and the next three options make "
                                                                              "every .png the script writes come from the display pass on the device (the stage that "
                                                                              "produced the image is its source), written by shm_write_png; with them -o <name>.png "
                                                                              "writes pictures only and reads no float image back")
    ap.add_argument("--auto-exposure", action="store_true", help="meter the exposure from the frame's log-luminance histogram; --exposure is then a compensation, and over "
                                                                 "--frames the exposure adapts by --frame-time a frame")
    ap.add_argument("--dither", action="store_true", help="8x8 ordered dither before the 8-bit quantisation")
    ap.add_argument("--frame-time", type=float, default=None, metavar="SECONDS", help="with --frames and --auto-exposure: the time between two frames (the adaptation's dt; "
                                                                                      "0 or absent: every frame jumps to its own exposure)")
    ap.add_argument("-o", "--output", default="")
    args = ap.parse_args()
    lib = abi.load_library()
    if lib.shm_device_count() < 1:
        raise SystemExit("no HIP device visible (there is no CPU fallback)")
    w, h = args.res, args.height or args.res
    sc = make_scene(lib, args.scene, w, h, film=dict(filter=args.filter), camera=dict(type="spherical", mapping=args.mapping) if args.camera == "spherical" else None)
    w, h = getattr(sc, "res", (w, h))
    r = render.Renderer(lib, sc.desc, 0)
    p = render.make_params(seed=args.seed, spp=args.spp, max_depth=args.max_depth, integrator=args.integrator or "path", reference_quirks=not args.quirks_off,
                           sampler=args.sampler, ao_max_distance=args.ao_distance or 0.0, ao_uniform_sample=args.ao_sampling == "uniform")
    p = file_integrator(p, sc, args)
    if args.frames > 0:
        return render_sequence(lib, args, sc, r, w, h)
    tile_spp = None
    r.clear()
    t0 = time.perf_counter()
    if args.adaptive is None:
        st = r.render_device(p)
    else:
        over = {k: v for k, v in (("min_spp", args.min_spp), ("batch_spp", args.batch_spp)) if v is not None}
        aparams = render.make_adaptive_params(lib, threshold=args.adaptive, **over)
        tile_spp, st = r.render_adaptive(p, aparams)
    dt = time.perf_counter() - t0
    rays = st["rays_closest"] + st["rays_any"]
    spp_text = f"{args.spp} spp" if tile_spp is None else f"{st['paths'] / (w * h):.1f} spp on average (tiles from {tile_spp.min()} to {tile_spp.max()}, cap {args.spp})"
    print(f"{sc.name}: {w}x{h} x {spp_text}, {rays / 1e6:.1f} Mrays in {dt * 1e3:.1f} ms = {rays / dt / 1e6:.0f} Mray/s")
    out = args.output or f"{args.scene.replace(':', '_')}.pfm"
    pictures = Pictures(lib, r, args)
    pfm = not (pictures.on and out.endswith(".png"))  # -o <name>.png with a display option: the picture only, and no float image is read back
    img = None
    if pfm:
        img = render.film_get_image(lib, r.read_film(), render.SRGB_FROM_XYZ)  # RgbFilm::get_image with an sRGB output matrix
        img = np.ascontiguousarray(img, np.float32)
        abi.check(lib, lib.shm_write_pfm(out.encode(), img.ctypes.data_as(abi.c_float_p), w, h), "shm_write_pfm")
    pictures.write(os.path.splitext(out)[0] + ".png", abi.SHM_DISPLAY_SOURCE_FILM, img)
    print(*(("wrote", out, "and", os.path.splitext(out)[0] + ".png") if pfm else ("wrote", out)))
    if tile_spp is not None:  # what the adaptive render measured and where it spent its samples
        stem = os.path.splitext(out)[0]
        count = np.ascontiguousarray(np.repeat(render.tile_spp_image(tile_spp, w, h)[..., None], 3, axis=2), np.float32)
        var = np.ascontiguousarray(render.moments_resolve(lib, r.read_moments(), aparams.floor)["v"], np.float32)
        for name, a in (("spp", count), ("variance", var)):
            abi.check(lib, lib.shm_write_pfm(f"{stem}.{name}.pfm".encode(), a.ctypes.data_as(abi.c_float_p), w, h), "shm_write_pfm")
        print(f"wrote {stem}.spp.pfm and {stem}.variance.pfm")
    if args.aovs:  # the G-buffer pass of the same frame: what a denoiser takes beside the beauty
        aov = render.render_gbuffer(lib, sc.desc, p, matrix=render.SRGB_FROM_XYZ, renderer=r)
        stem = os.path.splitext(out)[0]
        for name, key in (("albedo", "albedo"), ("normal", "ns"), ("position", "p")):
            a = np.ascontiguousarray(aov[key], np.float32)
            abi.check(lib, lib.shm_write_pfm(f"{stem}.{name}.pfm".encode(), a.ctypes.data_as(abi.c_float_p), w, h), "shm_write_pfm")
        print("wrote", ", ".join(f"{stem}.{n}.pfm" for n in ("albedo", "normal", "position")), f"(coverage {float(aov['coverage'].mean()):.3f})")
    if args.denoise:  # the film is still on the device; the pass fills the G-buffer the filter is guided by (a second pass after --aovs's gives the same sums)
        r.gbuffer(p)
        stem = os.path.splitext(out)[0]
        dimg = None
        if pfm:
            den, ms = r.denoise(return_ms=True)
            dimg = np.ascontiguousarray(render.film_get_image(lib, den, render.SRGB_FROM_XYZ), np.float32)
            abi.check(lib, lib.shm_write_pfm(f"{stem}.denoised.pfm".encode(), dimg.ctypes.data_as(abi.c_float_p), w, h), "shm_write_pfm")
        else:  # the result stays on the device: the display pass reads it there
            ms_c, dparams = C.c_double(0.0), render.make_denoise_params(lib)
            abi.check(lib, lib.shm_denoise_device(r.handle, C.byref(dparams), C.byref(ms_c)), "shm_denoise_device")
            ms = float(ms_c.value)
        pictures.write(f"{stem}.denoised.png", abi.SHM_DISPLAY_SOURCE_DENOISED, dimg)
        print((f"wrote {stem}.denoised.pfm and {stem}.denoised.png" if pfm else f"wrote {stem}.denoised.png") + f" (denoiser: {ms:.3f} ms)")
    r.close()


if __name__ == "__main__":
    main()
