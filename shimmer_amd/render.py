"""Python mirror of the reference's render driver for the GPU path (src/render.rs:8-55 ->
ImageTileIntegrator::render, src/integrator.rs:226-322): spp-wave schedule over 8x8 tiles, film read-back,
RgbFilm::get_pixel_rgb (film.rs:720-738).  Multi-GPU: tiles are sharded across ranks (one process per GPU,
no data-path collective while rendering) and the film rows are gathered by RCCL INSIDE libshimmer_hip.so (shm_render_sharded);
the small collectives a host needs around it (barrier, reductions) are the library's too (Renderer.dist_*): no torch.
"""
import contextlib
import ctypes as C
import os

import numpy as np

from . import abi
from .scene import tiles_for, wave_schedule

FILM_DTYPE = np.dtype([("rgb_sum", "<f8", (3,)), ("weight_sum", "<f8")])


def make_params(seed=0, spp=4, max_depth=5, regularize=False, disable_pixel_jitter=False, disable_wavelength_jitter=False,
                integrator="path", sample_lights=True, sample_bsdf=True, force_diffuse=False, disable_texture_filtering=False, reference_quirks=True,
                sampler="independent", randomization="fastowen", ao_max_distance=0.0, ao_uniform_sample=False):
    """sampler: "independent" (the default) or "zsobol"; randomization ("fastowen" or "none") applies to "zsobol" only.
    integrator "ambientocclusion" (PBRT-v4's): ao_max_distance 0 (or inf) is an unbounded occlusion ray, ao_uniform_sample picks uniform over cosine hemisphere sampling;
    the other integrators ignore both."""
    p = abi.ShmRenderParams()
    p.sampler = {"independent": abi.SHM_SAMPLER_INDEPENDENT, "zsobol": abi.SHM_SAMPLER_ZSOBOL}[sampler]
    p.sampler_randomization = {"fastowen": abi.SHM_SAMPLER_FASTOWEN, "none": abi.SHM_SAMPLER_RANDOMIZE_NONE}[randomization]
    p.integrator = {"path": abi.SHM_INTEGRATOR_PATH, "simplepath": abi.SHM_INTEGRATOR_SIMPLE_PATH,
                    "randomwalk": abi.SHM_INTEGRATOR_RANDOM_WALK, "ambientocclusion": abi.SHM_INTEGRATOR_AMBIENT_OCCLUSION}[integrator]
    p.ao_uniform_sample = int(bool(ao_uniform_sample))
    p.ao_max_distance = 0.0 if ao_max_distance == float("inf") else float(ao_max_distance)
    p.sample_lights, p.sample_bsdf = int(sample_lights), int(sample_bsdf)
    p.force_diffuse, p.disable_texture_filtering = int(force_diffuse), int(disable_texture_filtering)
    p.disable_reference_quirks = 0 if reference_quirks else 1  # SHM_REFERENCE_QUIRKS: ON = reference-exact (the default)
    p.seed, p.samples_per_pixel, p.max_depth = seed, spp, max_depth
    p.regularize, p.disable_pixel_jitter, p.disable_wavelength_jitter = int(regularize), int(disable_pixel_jitter), int(disable_wavelength_jitter)
    return p


# XYZ -> linear sRGB (IEC 61966-2-1), the output_rgb_from_sensor_rgb of an sRGB film behind an XYZ sensor (film.rs:524):
# used by the examples and tests; a host that owns an RGBColorSpace passes its own matrix.
SRGB_FROM_XYZ = np.array([[3.2404542, -1.5371385, -0.4985314], [-0.9692660, 1.8760108, 0.0415560], [0.0556434, -0.2040259, 1.0572252]], np.float32)


def film_get_image(lib, film, matrix=None, write_fp16=False):
    """RgbFilm::get_image through the host mirror (shm_film_get_image): (H, W, 3) float32."""
    m = np.ascontiguousarray(np.eye(3, dtype=np.float32) if matrix is None else matrix, dtype=np.float32)
    film = np.ascontiguousarray(film)
    out = np.empty(film.shape + (3,), np.float32)
    abi.check(lib, lib.shm_film_get_image(film.ctypes.data_as(C.c_void_p), film.size, m.ctypes.data_as(abi.c_float_p), int(write_fp16),
                                          out.ctypes.data_as(abi.c_float_p)), "shm_film_get_image")
    return out


def film_to_rgb(film):
    """RgbFilm::get_pixel_rgb without the output colour matrix: rgb_sum / weight_sum as f32 (film.rs:720-731)."""
    rgb = film["rgb_sum"].astype(np.float32)
    w = film["weight_sum"].astype(np.float32)
    out = rgb.copy()
    nz = w != 0
    out[nz] = rgb[nz] / w[nz][..., None]
    return out


def shard_tiles(n_tiles, tiles_per_row, rank, world_size, rows_per_block=None, lib=None):
    """Static interleaved sharding through the C ABI (shm_shard_tiles): blocks of `rows_per_block` tile rows, block b ->
    rank b % world. Default block height: about 16 blocks per rank, so that expensive image regions (the object) and cheap ones
    (walls) are spread over all ranks."""
    lib = lib or abi.load_library()
    idx = (C.c_uint32 * max(1, n_tiles))()
    n = C.c_uint32()
    abi.check(lib, lib.shm_shard_tiles(n_tiles, tiles_per_row, rank, world_size, int(rows_per_block or 0), idx, C.byref(n)), "shm_shard_tiles")
    return np.frombuffer(idx, dtype=np.uint32, count=n.value).astype(np.int64)


class Renderer:
    """Owns a ShmScene on one GPU. Raises if the library or a device is missing: no CPU fallback."""

    def __init__(self, lib, desc, device=0):
        self.lib = lib
        self.desc = desc
        self.handle = C.c_void_p()
        abi.check(lib, lib.shm_scene_create(C.byref(desc), device, C.byref(self.handle)), "shm_scene_create")
        pb = desc.film.pixel_bounds
        self.pixel_bounds = (pb[0], pb[1], pb[2], pb[3])
        self.width, self.height = pb[2] - pb[0], pb[3] - pb[1]
        self.tiles, self.n_tiles = tiles_for(lib, self.pixel_bounds)
        self.tiles_per_row = (self.width + 7) // 8

    def close(self):
        if self.handle:
            self.lib.shm_scene_destroy(self.handle)
            self.handle = C.c_void_p()

    def _tile_subset(self, tile_indices):
        if tile_indices is None:
            return self.tiles, self.n_tiles
        sub = (abi.ShmTile * max(1, len(tile_indices)))()
        for k, i in enumerate(tile_indices):
            sub[k] = self.tiles[int(i)]
        return sub, len(tile_indices)

    def shading_records(self):
        """(records built at scene creation, milliseconds it took): the per-primitive shading records of flat triangles."""
        n, ms = C.c_uint64(0), C.c_double(0.0)
        abi.check(self.lib, self.lib.shm_scene_shading_records(self.handle, C.byref(n), C.byref(ms)), "shm_scene_shading_records")
        return int(n.value), float(ms.value)

    def clear(self):
        abi.check(self.lib, self.lib.shm_film_clear(self.handle), "shm_film_clear")

    def render_waves(self, params, tile_indices=None, waves=None):
        """Enqueue all spp-waves into the device film; returns accumulated stats dict."""
        tiles, n = self._tile_subset(tile_indices)
        stats = abi.ShmStats()
        if n == 0:
            return stats.as_dict()
        for (ws, we) in (waves if waves is not None else wave_schedule(params.samples_per_pixel)):
            abi.check(self.lib, self.lib.shm_render_wave(self.handle, C.byref(params), tiles, n, ws, we, C.byref(stats)), "shm_render_wave")
        return stats.as_dict()

    def render_device(self, params, tile_indices=None):
        """Whole render (all spp-waves, fused into <= 64-spp launches) into the device film; returns the stats dict."""
        tiles, n = self._tile_subset(tile_indices)
        stats = abi.ShmStats()
        if n:
            abi.check(self.lib, self.lib.shm_render_device(self.handle, C.byref(params), tiles, n, C.byref(stats)), "shm_render_device")
        return stats.as_dict()

    # ---- multi-GPU behind the C ABI (one process per GPU; include/shimmer_hip.h "multi-GPU") ----
    def dist_unique_id(self):
        """Rank 0: the 128-byte RCCL unique id the host distributes to every rank (any control channel)."""
        buf = (C.c_uint8 * abi.SHM_DIST_ID_BYTES)()
        abi.check(self.lib, self.lib.shm_dist_unique_id(buf), "shm_dist_unique_id")
        return bytes(buf)

    def dist_init(self, rank, world, unique_id):
        buf = (C.c_uint8 * abi.SHM_DIST_ID_BYTES).from_buffer_copy(bytes(unique_id))
        abi.check(self.lib, self.lib.shm_dist_init(self.handle, rank, world, buf), "shm_dist_init")

    def render_sharded(self, params):
        """Collective: clear, render this rank's tile shard, gather the film rows into rank 0's device film over RCCL."""
        stats = abi.ShmStats()
        abi.check(self.lib, self.lib.shm_render_sharded(self.handle, C.byref(params), C.byref(stats)), "shm_render_sharded")
        return stats.as_dict()

    def dist_barrier(self):
        abi.check(self.lib, self.lib.shm_dist_barrier(self.handle), "shm_dist_barrier")

    def dist_allreduce(self, values, op=abi.SHM_REDUCE_SUM):
        """All-reduce of a short list of host doubles over the scene's communicator (identity without one)."""
        buf = (C.c_double * len(values))(*[float(v) for v in values])
        abi.check(self.lib, self.lib.shm_dist_allreduce_f64(self.handle, buf, len(values), op), "shm_dist_allreduce_f64")
        return list(buf)

    def dist_allgather(self, values):
        """Every rank's short list of host doubles, rank-major: [[rank 0's], [rank 1's], ...]."""
        info = self.dist_info()
        n, world = len(values), max(1, info["world"])
        mine = (C.c_double * n)(*[float(v) for v in values])
        out = (C.c_double * (n * world))()
        abi.check(self.lib, self.lib.shm_dist_allgather_f64(self.handle, mine, n, out), "shm_dist_allgather_f64")
        return [list(out[i * n:(i + 1) * n]) for i in range(world)]

    def dist_info(self):
        info = abi.ShmDistInfo()
        abi.check(self.lib, self.lib.shm_dist_info(self.handle, C.byref(info)), "shm_dist_info")
        return info.as_dict()

    def dist_selftest(self):
        abi.check(self.lib, self.lib.shm_dist_selftest(self.handle), "shm_dist_selftest")

    def read_film(self):
        film = np.zeros((self.height, self.width), dtype=FILM_DTYPE)
        abi.check(self.lib, self.lib.shm_film_read(self.handle, film.ctypes.data_as(C.c_void_p)), "shm_film_read")
        return film

    def film_device_ptr(self):
        p, n = C.c_void_p(), C.c_uint64()
        abi.check(self.lib, self.lib.shm_film_device_ptr(self.handle, C.byref(p), C.byref(n)), "shm_film_device_ptr")
        return p.value, n.value

    def render(self, params, tile_indices=None):
        """ImageTileIntegrator::render: clear, all waves, read back. Returns (film structured array, stats)."""
        self.clear()
        stats = self.render_waves(params, tile_indices)
        return self.read_film(), stats

    # ---- the G-buffer pass (include/shimmer_hip.h "the G-buffer pass") ----
    def gbuffer_clear(self):
        abi.check(self.lib, self.lib.shm_gbuffer_clear(self.handle), "shm_gbuffer_clear")

    def gbuffer_wave(self, params, sample_begin, sample_end, space=abi.SHM_GBUFFER_SPACE_RENDER, tile_indices=None):
        """Samples [sample_begin, sample_end) of the tiles into the device G-buffer (+=); returns the stats dict."""
        tiles, n = self._tile_subset(tile_indices)
        stats = abi.ShmStats()
        abi.check(self.lib, self.lib.shm_gbuffer_render_wave(self.handle, C.byref(params), space, tiles, n, sample_begin, sample_end, C.byref(stats)),
                  "shm_gbuffer_render_wave")
        return stats.as_dict()

    def read_gbuffer(self):
        g = np.zeros((self.height, self.width), dtype=GBUFFER_DTYPE)
        abi.check(self.lib, self.lib.shm_gbuffer_read(self.handle, g.ctypes.data_as(C.c_void_p)), "shm_gbuffer_read")
        return g

    def gbuffer(self, params, space=abi.SHM_GBUFFER_SPACE_RENDER, tile_indices=None):
        """shm_render_gbuffer: clear, every sample, read back. Returns (the sums as a GBUFFER_DTYPE array, stats)."""
        tiles, n = self._tile_subset(tile_indices)
        stats = abi.ShmStats()
        g = np.zeros((self.height, self.width), dtype=GBUFFER_DTYPE)
        abi.check(self.lib, self.lib.shm_render_gbuffer(self.handle, C.byref(params), space, tiles, n, g.ctypes.data_as(C.c_void_p), C.byref(stats)), "shm_render_gbuffer")
        return g, stats.as_dict()

    # ---- the denoiser (include/shimmer_hip.h "the denoiser") ----
    def denoise(self, dparams=None, return_ms=False):
        """shm_denoise: the device film filtered under the device G-buffer's guidance (a G-buffer pass must have run), read back as a FILM_DTYPE array whose
        rgb_sum is the denoised sensor RGB and whose weight_sum is 1 — what film_get_image takes. dparams: an abi.ShmDenoiseParams (None: the defaults)."""
        d = dparams if dparams is not None else make_denoise_params(self.lib)
        out = np.zeros((self.height, self.width), dtype=FILM_DTYPE)
        ms = C.c_double(0.0)
        abi.check(self.lib, self.lib.shm_denoise(self.handle, C.byref(d), out.ctypes.data_as(C.c_void_p), C.byref(ms)), "shm_denoise")
        return (out, float(ms.value)) if return_ms else out

    # ---- a moving camera and temporal accumulation (include/shimmer_hip.h "temporal accumulation") ----
    def set_camera(self, camera):
        """shm_scene_set_camera: the next wave renders from `camera` (an abi.ShmCamera of the scene's kind, in the scene's render space: camera_in_scene builds one).
        Film, G-buffer, moments and history stay as they are."""
        abi.check(self.lib, self.lib.shm_scene_set_camera(self.handle, C.byref(camera)), "shm_scene_set_camera")

    def temporal_clear(self):
        """shm_temporal_clear: forget the history and the camera it was seen through."""
        abi.check(self.lib, self.lib.shm_temporal_clear(self.handle), "shm_temporal_clear")

    def temporal_accumulate(self, tparams=None, return_ms=False):
        """shm_temporal_accumulate_device: the device film and G-buffer of the frame just rendered into the history (a render-space G-buffer wave must have run).
        tparams: an abi.ShmTemporalParams (None: the defaults). Returns the kernel's HIP-event milliseconds when asked; read_temporal gives the result."""
        t = tparams if tparams is not None else make_temporal_params(self.lib)
        ms = C.c_double(0.0)
        abi.check(self.lib, self.lib.shm_temporal_accumulate_device(self.handle, C.byref(t), C.byref(ms)), "shm_temporal_accumulate_device")
        return float(ms.value) if return_ms else None

    def read_temporal(self):
        """The accumulated frame as a FILM_DTYPE array: rgb_sum the sensor RGB, weight_sum 1 — what film_get_image takes."""
        out = np.zeros((self.height, self.width), dtype=FILM_DTYPE)
        abi.check(self.lib, self.lib.shm_temporal_read(self.handle, out.ctypes.data_as(C.c_void_p)), "shm_temporal_read")
        return out

    def read_temporal_history(self):
        """The records the last accumulate wrote, as a TEMPORAL_DTYPE array."""
        out = np.zeros((self.height, self.width), dtype=TEMPORAL_DTYPE)
        abi.check(self.lib, self.lib.shm_temporal_read_history(self.handle, out.ctypes.data_as(C.c_void_p)), "shm_temporal_read_history")
        return out

    def denoise_temporal(self, dparams=None, temporal_variance=1, return_ms=False):
        """shm_denoise_temporal_device + shm_denoise_read: the a-trous filter over the accumulated frame; temporal_variance 1 takes the filter's initial variance
        from the history's luminance moments where the history holds four frames or more."""
        d = dparams if dparams is not None else make_denoise_params(self.lib)
        out = np.zeros((self.height, self.width), dtype=FILM_DTYPE)
        ms = C.c_double(0.0)
        abi.check(self.lib, self.lib.shm_denoise_temporal_device(self.handle, C.byref(d), int(temporal_variance), C.byref(ms)), "shm_denoise_temporal_device")
        abi.check(self.lib, self.lib.shm_denoise_read(self.handle, out.ctypes.data_as(C.c_void_p)), "shm_denoise_read")
        return (out, float(ms.value)) if return_ms else out

    # ---- the display pass (include/shimmer_hip.h "the display pass") ----
    def display_clear(self):
        """shm_display_clear: forget the auto-exposure's adaptation state; the next auto-exposed frame jumps to its target."""
        abi.check(self.lib, self.lib.shm_display_clear(self.handle), "shm_display_clear")

    def display(self, dparams=None, return_state=False, return_ms=False):
        """shm_display: dparams.source (the film, the denoiser's result or the temporal pass's) exposed, tone-mapped, encoded and quantised on the device, read back as an
        (H, W, 4) uint8 array R, G, B, 255. dparams: an abi.ShmDisplayParams (None: the defaults). With return_state / return_ms the result is a tuple that also holds the
        abi.ShmDisplayState as a dict / the launches' HIP-event milliseconds, in that order."""
        d = dparams if dparams is not None else make_display_params(self.lib)
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        state, ms = abi.ShmDisplayState(), C.c_double(0.0)
        abi.check(self.lib, self.lib.shm_display(self.handle, C.byref(d), out.ctypes.data_as(C.c_void_p), C.byref(state), C.byref(ms)), "shm_display")
        image = out.view(np.uint8).reshape(self.height, self.width, 4)
        if not (return_state or return_ms):
            return image
        return (image,) + ((state.as_dict(),) if return_state else ()) + ((float(ms.value),) if return_ms else ())

    def read_display_histogram(self):
        """The 256 counts of the last auto-exposed frame (uint32)."""
        out = np.zeros(256, np.uint32)
        abi.check(self.lib, self.lib.shm_display_read_histogram(self.handle, out.ctypes.data_as(C.c_void_p)), "shm_display_read_histogram")
        return out

    def display_device_ptr(self):
        """(device pointer, bytes) of the RGBA8 image: for interop, as film_device_ptr."""
        p, n = C.c_void_p(), C.c_uint64()
        abi.check(self.lib, self.lib.shm_display_device_ptr(self.handle, C.byref(p), C.byref(n)), "shm_display_device_ptr")
        return p.value, n.value

    # ---- adaptive sampling (include/shimmer_hip.h "adaptive sampling") ----
    def moments_clear(self):
        """shm_moments_clear: zero records that count from the device film as it stands."""
        abi.check(self.lib, self.lib.shm_moments_clear(self.handle), "shm_moments_clear")

    def moments_update(self, aparams, tile_indices=None, tiles=None):
        """shm_moments_update: one batch — the film since the last call — into the records of the tiles' pixels. Returns the tiles' TILE_ERROR_DTYPE array.
        tiles: an abi.ShmTile array of the caller's own instead of indices into the renderer's 8x8 tiling."""
        t, n = (tiles, len(tiles)) if tiles is not None else self._tile_subset(tile_indices)
        out = np.zeros(n, dtype=TILE_ERROR_DTYPE)
        abi.check(self.lib, self.lib.shm_moments_update(self.handle, t, n, C.byref(aparams), out.ctypes.data_as(C.c_void_p)), "shm_moments_update")
        return out

    def read_moments(self):
        m = np.zeros((self.height, self.width), dtype=MOMENTS_DTYPE)
        abi.check(self.lib, self.lib.shm_moments_read(self.handle, m.ctypes.data_as(C.c_void_p)), "shm_moments_read")
        return m

    def render_adaptive(self, params, aparams, tile_indices=None):
        """shm_render_adaptive into the device film: params.samples_per_pixel is the cap. Returns (the samples each tile received as uint32, the stats dict)."""
        tiles, n = self._tile_subset(tile_indices)
        stats = abi.ShmStats()
        spp = np.zeros(n, np.uint32)
        abi.check(self.lib, self.lib.shm_render_adaptive(self.handle, C.byref(params), tiles, n, C.byref(aparams), spp.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(stats)),
                  "shm_render_adaptive")
        return spp, stats.as_dict()

    def trace(self, rays, any_hit=False):
        """Bring-up entry: rays = structured/float32 array (n, 8) [o,d,t_max,pad]. Returns hits (n,8 view) or occluded bytes."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0]
        stats = abi.ShmStats()
        if any_hit:
            out = np.zeros(n, np.uint8)
            abi.check(self.lib, self.lib.shm_trace_any(self.handle, rays.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p), C.byref(stats)), "shm_trace_any")
        else:
            out = np.zeros(n, dtype=HIT_DTYPE)
            abi.check(self.lib, self.lib.shm_trace_closest(self.handle, rays.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p), C.byref(stats)), "shm_trace_closest")
        return out, stats.as_dict()


HIT_DTYPE = np.dtype([("prim", "<i4"), ("t", "<f4"), ("b0", "<f4"), ("b1", "<f4"), ("b2", "<f4"), ("phi", "<f4"), ("instance", "<u4"), ("pad", "<u4")])


GBUFFER_DTYPE = np.dtype([("p", "<f8", (3,)), ("n", "<f8", (3,)), ("ns", "<f8", (3,)), ("uv", "<f8", (2,)), ("albedo", "<f8", (3,)), ("weight_hit", "<f8"),
                          ("weight_sum", "<f8")])
assert GBUFFER_DTYPE.itemsize == C.sizeof(abi.ShmGBufferPixel)


@contextlib.contextmanager
def _renderer_for(lib, desc, device, renderer):
    """`renderer`, left open, or a Renderer created for the with-block and closed behind it."""
    r = renderer or Renderer(lib, desc, device=device)
    try:
        yield r
    finally:
        if renderer is None:
            r.close()


def _with_overrides(who, struct, names, overrides):
    """`struct` with the fields `overrides` names set; a keyword outside `names` is a TypeError in `who`'s name."""
    for k, v in overrides.items():
        if k not in names:
            raise TypeError(f"{who}: no parameter {k!r}")
        setattr(struct, k, v)
    return struct


def gbuffer_white(lib, desc):
    """W_c of the scene's sensor (shm_gbuffer_white): what an albedo sum of a rho = 1 surface averages to, per channel."""
    w = (C.c_double * 3)()
    abi.check(lib, lib.shm_gbuffer_white(C.byref(desc), w), "shm_gbuffer_white")
    return np.array(w[:], np.float64)


def gbuffer_resolve(lib, gbuffer, white, matrix=None):
    """shm_gbuffer_resolve: the G-buffer's sums as a dict of float32 images p, n, ns (.., 3), uv (.., 2), albedo (.., 3) and coverage (..)."""
    g = np.ascontiguousarray(gbuffer, dtype=GBUFFER_DTYPE)
    w = (C.c_double * 3)(*[float(x) for x in white])
    m = None if matrix is None else np.ascontiguousarray(matrix, dtype=np.float32)
    out = np.empty(g.shape + (15,), np.float32)
    abi.check(lib, lib.shm_gbuffer_resolve(g.ctypes.data_as(C.c_void_p), g.size, w, None if m is None else m.ctypes.data_as(abi.c_float_p),
                                           out.ctypes.data_as(abi.c_float_p)), "shm_gbuffer_resolve")
    return {"p": out[..., 0:3], "n": out[..., 3:6], "ns": out[..., 6:9], "uv": out[..., 9:11], "albedo": out[..., 11:14], "coverage": out[..., 14]}


def render_gbuffer(lib, desc, params, device=0, space=abi.SHM_GBUFFER_SPACE_RENDER, matrix=None, renderer=None):
    """The G-buffer pass of a scene as images: first-hit p, n, ns, uv, albedo and coverage (numpy float32), from a scene created for the call or from `renderer`."""
    with _renderer_for(lib, desc, device, renderer) as r:
        g, _ = r.gbuffer(params, space=space)
    return gbuffer_resolve(lib, g, gbuffer_white(lib, desc), matrix)


def make_denoise_params(lib, **overrides):
    """shm_denoise_default_params, with any of iterations, demodulate, sigma_luminance, sigma_normal, sigma_plane, albedo_floor, variance_source set by keyword
    (variance_source: abi.SHM_DENOISE_VARIANCE_SPATIAL, the default, or abi.SHM_DENOISE_VARIANCE_MEASURED: the moments pass's variance)."""
    d = abi.ShmDenoiseParams()
    abi.check(lib, lib.shm_denoise_default_params(C.byref(d)), "shm_denoise_default_params")
    names = ("iterations", "demodulate", "sigma_luminance", "sigma_normal", "sigma_plane", "albedo_floor", "variance_source")
    return _with_overrides("make_denoise_params", d, names, overrides)


def denoise_host(lib, film, gbuffer, white, dparams=None, moments=None):
    """shm_denoise_host, the denoiser's CPU twin: (H, W) FILM_DTYPE and GBUFFER_DTYPE arrays (Renderer.read_film / read_gbuffer, or made in numpy) and gbuffer_white's
    W into the FILM_DTYPE result Renderer.denoise gives for the same inputs, bit for bit. No GPU needed. moments: a (H, W) MOMENTS_DTYPE array (Renderer.read_moments)
    for variance_source = measured — shm_denoise_host_moments."""
    f = np.ascontiguousarray(film, dtype=FILM_DTYPE)
    g = np.ascontiguousarray(gbuffer, dtype=GBUFFER_DTYPE)
    if f.ndim != 2 or g.shape != f.shape:
        raise ValueError("denoise_host: film and gbuffer must be (height, width) arrays of one shape")
    d = dparams if dparams is not None else make_denoise_params(lib)
    w = (C.c_double * 3)(*[float(x) for x in white])
    out = np.zeros(f.shape, dtype=FILM_DTYPE)
    if moments is not None:
        m = np.ascontiguousarray(moments, dtype=MOMENTS_DTYPE)
        if m.shape != f.shape:
            raise ValueError("denoise_host: moments must have the film's shape")
        abi.check(lib, lib.shm_denoise_host_moments(f.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), f.shape[1], f.shape[0], w,
                                                    C.byref(d), out.ctypes.data_as(C.c_void_p)), "shm_denoise_host_moments")
        return out
    abi.check(lib, lib.shm_denoise_host(f.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), f.shape[1], f.shape[0], w, C.byref(d), out.ctypes.data_as(C.c_void_p)),
              "shm_denoise_host")
    return out


def render_denoised(lib, desc, params, dparams=None, device=0, matrix=None, renderer=None):
    """Render, G-buffer pass and denoiser in one call, from a scene created for it or from `renderer`. Returns a dict: "film" and "denoised" (FILM_DTYPE), "noisy" and
    "image" (their film_get_image under `matrix`: float32 (H, W, 3)), "gbuffer" (GBUFFER_DTYPE), "stats" (the render's) and "denoise_ms" (the filter's HIP-event time)."""
    with _renderer_for(lib, desc, device, renderer) as r:
        film, stats = r.render(params)
        g, _ = r.gbuffer(params)
        den, ms = r.denoise(dparams, return_ms=True)
    return {"film": film, "denoised": den, "noisy": film_get_image(lib, film, matrix), "image": film_get_image(lib, den, matrix), "gbuffer": g, "stats": stats,
            "denoise_ms": ms}


TEMPORAL_DTYPE = np.dtype([("rgb", "<f4", (3,)), ("m1", "<f4"), ("m2", "<f4"), ("length", "<f4"), ("p", "<f4", (3,)), ("ns", "<f4", (3,)), ("pad", "<u4", (4,))])
assert TEMPORAL_DTYPE.itemsize == C.sizeof(abi.ShmTemporalPixel)


def make_temporal_params(lib, **overrides):
    """shm_temporal_default_params, with any of alpha_min, alpha_min_moments, max_history, normal_cos_min, plane_tolerance, albedo_floor, demodulate set by keyword."""
    t = abi.ShmTemporalParams()
    abi.check(lib, lib.shm_temporal_default_params(C.byref(t)), "shm_temporal_default_params")
    names = ("alpha_min", "alpha_min_moments", "max_history", "normal_cos_min", "plane_tolerance", "albedo_floor", "demodulate")
    return _with_overrides("make_temporal_params", t, names, overrides)


def temporal_accumulate_host(lib, film, gbuffer, white, camera, history=None, previous_camera=None, tparams=None):
    """shm_temporal_accumulate_host, the temporal pass's CPU twin: one frame from (H, W) FILM_DTYPE and GBUFFER_DTYPE arrays, gbuffer_white's W, the frame's
    abi.ShmCamera and — where there is a previous frame — its TEMPORAL_DTYPE records and camera. Returns (the new records, the FILM_DTYPE result): what
    Renderer.read_temporal_history / read_temporal give for the same inputs, bit for bit. No GPU needed."""
    f = np.ascontiguousarray(film, dtype=FILM_DTYPE)
    g = np.ascontiguousarray(gbuffer, dtype=GBUFFER_DTYPE)
    if f.ndim != 2 or g.shape != f.shape:
        raise ValueError("temporal_accumulate_host: film and gbuffer must be (height, width) arrays of one shape")
    h = None
    if history is not None:
        h = np.ascontiguousarray(history, dtype=TEMPORAL_DTYPE)
        if h.shape != f.shape:
            raise ValueError("temporal_accumulate_host: history must have the film's shape")
    t = tparams if tparams is not None else make_temporal_params(lib)
    w = (C.c_double * 3)(*[float(x) for x in white])
    records = np.zeros(f.shape, dtype=TEMPORAL_DTYPE)
    out = np.zeros(f.shape, dtype=FILM_DTYPE)
    abi.check(lib, lib.shm_temporal_accumulate_host(f.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), None if h is None else h.ctypes.data_as(C.c_void_p),
                                                    C.byref(camera), None if previous_camera is None else C.byref(previous_camera), f.shape[1], f.shape[0], w,
                                                    C.byref(t), records.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)), "shm_temporal_accumulate_host")
    return records, out


def denoise_temporal_host(lib, temporal, gbuffer, history, white, dparams=None, temporal_variance=1):
    """shm_denoise_temporal_host: Renderer.denoise_temporal's CPU twin, from read_temporal's, read_gbuffer's and read_temporal_history's arrays."""
    f = np.ascontiguousarray(temporal, dtype=FILM_DTYPE)
    g = np.ascontiguousarray(gbuffer, dtype=GBUFFER_DTYPE)
    h = np.ascontiguousarray(history, dtype=TEMPORAL_DTYPE)
    if f.ndim != 2 or g.shape != f.shape or h.shape != f.shape:
        raise ValueError("denoise_temporal_host: temporal, gbuffer and history must be (height, width) arrays of one shape")
    d = dparams if dparams is not None else make_denoise_params(lib)
    w = (C.c_double * 3)(*[float(x) for x in white])
    out = np.zeros(f.shape, dtype=FILM_DTYPE)
    abi.check(lib, lib.shm_denoise_temporal_host(f.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), f.shape[1], f.shape[0], w,
                                                 C.byref(d), int(temporal_variance), out.ctypes.data_as(C.c_void_p)), "shm_denoise_temporal_host")
    return out


def camera_in_scene(lib, builder_or_rfw, pos, look_at, up, fov=90.0, full_resolution=None, lens_radius=0.0, focal_distance=1e6, orthographic=False,
                    frame_aspect_ratio=0.0, screen_window=None):
    """A second camera for a scene that exists: shm_look_at + shm_camera_create_in, in the render space the scene's geometry was baked in. builder_or_rfw: the
    SceneBuilder the scene was made from (its render_from_world and film resolution are taken) or a (4, 4) render_from_world with `full_resolution` given.
    Returns the abi.ShmCamera Renderer.set_camera takes."""
    rfw = getattr(builder_or_rfw, "render_from_world", builder_or_rfw)
    if rfw is None:
        raise ValueError("camera_in_scene: the builder has no camera yet (set_camera_look_at returns and keeps render_from_world)")
    if full_resolution is None:
        film = getattr(builder_or_rfw, "film", None)
        if film is None:
            raise ValueError("camera_in_scene: full_resolution is needed with a bare render_from_world")
        full_resolution = tuple(film.full_resolution)
    rfw32 = np.ascontiguousarray(rfw, dtype=np.float32).reshape(16)
    wfc32 = np.zeros(16, np.float32)
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32)
    pos32, look32, up32 = f32(pos), f32(look_at), f32(up)
    abi.check(lib, lib.shm_look_at(pos32.ctypes.data_as(abi.c_float_p), look32.ctypes.data_as(abi.c_float_p), up32.ctypes.data_as(abi.c_float_p),
                                   wfc32.ctypes.data_as(abi.c_float_p)), "shm_look_at")
    p = abi.ShmCameraParams()
    p.kind = abi.SHM_CAMERA_ORTHOGRAPHIC if orthographic else abi.SHM_CAMERA_PERSPECTIVE
    p.world_from_camera[:] = [float(x) for x in wfc32]
    p.fov_deg = float(fov)
    p.full_resolution[:] = [int(full_resolution[0]), int(full_resolution[1])]
    p.lens_radius, p.focal_distance, p.frame_aspect_ratio = float(lens_radius), float(focal_distance), float(frame_aspect_ratio)
    if screen_window is not None:
        p.has_screen_window = 1
        p.screen_window[:] = [float(x) for x in screen_window]
    cam = abi.ShmCamera()
    abi.check(lib, lib.shm_camera_create_in(C.byref(p), rfw32.ctypes.data_as(abi.c_float_p), C.byref(cam)), "shm_camera_create_in")
    return cam


DISPLAY_PARAM_NAMES = ("source", "tonemap", "transfer", "auto_exposure", "dither", "exposure", "key", "white", "log2_min", "log2_max", "percentile_low", "percentile_high",
                       "adaptation_rate", "dt", "output_rgb_from_sensor_rgb")


def make_display_params(lib, **overrides):
    """shm_display_default_params (the film through ACES and sRGB at exposure 1, no auto-exposure, no dither), with any of DISPLAY_PARAM_NAMES set by keyword.
    output_rgb_from_sensor_rgb: anything numpy turns into nine floats, row-major (SRGB_FROM_XYZ)."""
    d = abi.ShmDisplayParams()
    abi.check(lib, lib.shm_display_default_params(C.byref(d)), "shm_display_default_params")
    if overrides.get("output_rgb_from_sensor_rgb") is not None:
        m = np.asarray(overrides["output_rgb_from_sensor_rgb"], np.float32).reshape(9)
        overrides = dict(overrides, output_rgb_from_sensor_rgb=(C.c_float * 9)(*[float(x) for x in m]))
    return _with_overrides("make_display_params", d, DISPLAY_PARAM_NAMES, overrides)


def display_host(lib, film, width, height, dparams=None, state=None):
    """shm_display_host, the display pass's CPU twin: a FILM_DTYPE array of width * height pixels into (rgba8 as (height, width, 4) uint8, the 256 counts as uint32, the
    abi.ShmDisplayState after the frame) — what Renderer.display and read_display_histogram give for the same film and state, bit for bit. state: the
    abi.ShmDisplayState before the frame (None: a fresh one); it is not modified. Without auto_exposure the counts are zeros and the state comes back as it went in.
    No GPU needed."""
    f = np.ascontiguousarray(film, dtype=FILM_DTYPE)
    if f.size != int(width) * int(height):
        raise ValueError("display_host: the film does not hold width * height pixels")
    d = dparams if dparams is not None else make_display_params(lib)
    st = abi.ShmDisplayState.from_buffer_copy(state) if state is not None else abi.ShmDisplayState()
    counts = np.zeros(256, np.uint32)
    out = np.zeros((int(height), int(width)), np.uint32)
    abi.check(lib, lib.shm_display_host(f.ctypes.data_as(C.c_void_p), int(width), int(height), C.byref(d), C.byref(st), counts.ctypes.data_as(C.c_void_p),
                                        out.ctypes.data_as(C.c_void_p)), "shm_display_host")
    return out.view(np.uint8).reshape(int(height), int(width), 4), counts, st


def write_png(lib, path, rgba8):
    """shm_write_png: an (H, W, 4) uint8 (or (H, W) uint32) image as Renderer.display gives it into an 8-bit RGB PNG; the alpha byte is dropped."""
    a = np.ascontiguousarray(rgba8)
    if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 4:
        a = a.view(np.uint32).reshape(a.shape[0], a.shape[1])
    if a.dtype != np.uint32 or a.ndim != 2:
        raise ValueError("write_png: an (H, W, 4) uint8 or (H, W) uint32 image")
    abi.check(lib, lib.shm_write_png(os.fsencode(path), a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0]), "shm_write_png")


def render_frames(lib, desc, cameras, params, tparams=None, dparams=None, temporal_variance=1, device=0, matrix=None, renderer=None, display=None):
    """A sequence of frames of one static scene under a moving camera, accumulated over time. cameras: one abi.ShmCamera per frame (camera_in_scene; None keeps the
    camera as it is). params.samples_per_pixel is the TOTAL over the sequence and a multiple of the frame count: frame f renders samples [f spp, (f + 1) spp) of it,
    so that no two frames share a sample. Per frame: set_camera, clear film and G-buffer, one render wave and one G-buffer wave over those samples,
    temporal_accumulate, and — with dparams — denoise_temporal. Returns a list of dicts: "film", "temporal" and, where filtered, "denoised" (FILM_DTYPE), "image"
    (film_get_image of the last of them under `matrix`) and "temporal_ms". display: an abi.ShmDisplayParams (make_display_params) — every frame's dict then also
    holds "display", the (H, W, 4) uint8 picture the display pass makes of the last of those stages on the device (display.source is not read: the stage decides),
    and "display_state"; the auto-exposure's state is cleared before the first frame and adapts from frame to frame by display.dt."""
    n = len(cameras)
    if n < 1 or params.samples_per_pixel % n:
        raise ValueError("render_frames: params.samples_per_pixel is the total over the frames and must be a multiple of their count")
    spp = params.samples_per_pixel // n
    frames = []
    with _renderer_for(lib, desc, device, renderer) as r:
        r.temporal_clear()
        if display is not None:
            r.display_clear()
            shown = abi.ShmDisplayParams.from_buffer_copy(display)
            shown.source = abi.SHM_DISPLAY_SOURCE_TEMPORAL if dparams is None else abi.SHM_DISPLAY_SOURCE_DENOISED
        for f, cam in enumerate(cameras):
            if cam is not None:
                r.set_camera(cam)
            r.clear()
            r.gbuffer_clear()
            r.render_waves(params, waves=[(f * spp, (f + 1) * spp)])
            r.gbuffer_wave(params, f * spp, (f + 1) * spp)
            ms = r.temporal_accumulate(tparams, return_ms=True)
            out = {"film": r.read_film(), "temporal": r.read_temporal(), "temporal_ms": ms}
            last = out["temporal"]
            if dparams is not None:
                last = out["denoised"] = r.denoise_temporal(dparams, temporal_variance)
            out["image"] = film_get_image(lib, last, matrix)
            if display is not None:
                out["display"], out["display_state"] = r.display(shown, return_state=True)
            frames.append(out)
    return frames


MOMENTS_DTYPE = np.dtype([("prev", "<f8", (4,)), ("mean", "<f8", (3,)), ("m2", "<f8", (3,)), ("weight", "<f8"), ("batches", "<f8")])
TILE_ERROR_DTYPE = np.dtype([("unconverged", "<u4"), ("max_e2", "<f4")])
assert MOMENTS_DTYPE.itemsize == C.sizeof(abi.ShmMomentsPixel) and TILE_ERROR_DTYPE.itemsize == C.sizeof(abi.ShmTileError)


def make_adaptive_params(lib, **overrides):
    """shm_adaptive_default_params (min_spp 16, batch_spp 4, threshold 0.05, floor 0.01), with any of the four set by keyword."""
    a = abi.ShmAdaptiveParams()
    abi.check(lib, lib.shm_adaptive_default_params(C.byref(a)), "shm_adaptive_default_params")
    return _with_overrides("make_adaptive_params", a, ("min_spp", "batch_spp", "threshold", "floor"), overrides)


def make_tiles(boxes):
    """An abi.ShmTile array from (x0, y0, x1, y1) boxes: a tiling of the caller's own for Renderer.moments_update / moments_update_host."""
    t = (abi.ShmTile * max(1, len(boxes)))()
    for i, b in enumerate(boxes):
        t[i] = abi.ShmTile(*[int(v) for v in b])
    return t


def moments_update_host(lib, film, moments, tiles, aparams, n_tiles=None):
    """shm_moments_update_host, the moments pass's CPU twin: one batch from a (H, W) FILM_DTYPE array into a (H, W) MOMENTS_DTYPE array, IN PLACE (it must be
    C-contiguous), over an abi.ShmTile array in film coordinates. Returns the tiles' TILE_ERROR_DTYPE array — what Renderer.moments_update gives, bit for bit."""
    f = np.ascontiguousarray(film, dtype=FILM_DTYPE)
    if moments.dtype != MOMENTS_DTYPE or not moments.flags.c_contiguous or f.ndim != 2 or moments.shape != f.shape:
        raise ValueError("moments_update_host: film and moments must be C-contiguous (height, width) arrays of one shape")
    n = len(tiles) if n_tiles is None else n_tiles
    out = np.zeros(n, dtype=TILE_ERROR_DTYPE)
    abi.check(lib, lib.shm_moments_update_host(f.ctypes.data_as(C.c_void_p), moments.ctypes.data_as(C.c_void_p), f.shape[1], f.shape[0], tiles, n, C.byref(aparams),
                                               out.ctypes.data_as(C.c_void_p)), "shm_moments_update_host")
    return out


def moments_resolve(lib, moments, floor=0.01):
    """shm_moments_resolve: the records as a dict of float32 images — "v" (variance of the pixel's mean) and "s2" (per-sample variance), (.., 3) in SENSOR RGB (an
    output matrix cannot be applied to variances without covariances), "batches" and "e2" (the squared relative error the adaptive render stops by)."""
    m = np.ascontiguousarray(moments, dtype=MOMENTS_DTYPE)
    out = np.empty(m.shape + (8,), np.float32)
    abi.check(lib, lib.shm_moments_resolve(m.ctypes.data_as(C.c_void_p), m.size, float(floor), out.ctypes.data_as(abi.c_float_p)), "shm_moments_resolve")
    return {"v": out[..., 0:3], "s2": out[..., 3:6], "batches": out[..., 6], "e2": out[..., 7]}


def render_adaptive(lib, desc, params, aparams=None, device=0, renderer=None):
    """An adaptive render (shm_render_adaptive; params.samples_per_pixel is the cap) of a scene created for the call or of `renderer`. Returns
    (film as FILM_DTYPE, tile_spp as uint32 per 8x8 tile in row-major tile order, moments as MOMENTS_DTYPE, stats)."""
    with _renderer_for(lib, desc, device, renderer) as r:
        tile_spp, stats = r.render_adaptive(params, aparams if aparams is not None else make_adaptive_params(lib))
        film, moments = r.read_film(), r.read_moments()
    return film, tile_spp, moments, stats


def tile_spp_image(tile_spp, width, height, tile=8):
    """The per-pixel sample count of an adaptive render: tile_spp (row-major over the renderer's `tile` x `tile` tiling) spread over its pixels, float32 (H, W)."""
    tw, th = (width + tile - 1) // tile, (height + tile - 1) // tile
    grid = np.asarray(tile_spp, np.float32).reshape(th, tw)
    return np.repeat(np.repeat(grid, tile, axis=0), tile, axis=1)[:height, :width]


def film_tensor(renderer, device=None):
    """The renderer's film as a flat float64 torch tensor: zero-copy view of the HBM buffer when `device` is given."""
    import torch

    if device is not None:
        ptr, nbytes = renderer.film_device_ptr()

        class _Holder:
            pass

        h = _Holder()
        h.__cuda_array_interface__ = {"shape": (nbytes // 8,), "typestr": "<f8", "data": (ptr, False), "version": 2}
        return torch.as_tensor(h, device=device)
    return torch.from_numpy(renderer.read_film().view(np.float64).reshape(-1).copy())


def render_multi(lib, desc, devices, params):
    """One process, n devices: shm_render_multi (one host thread + scene replica per device, film rows gathered over xGMI peer copies).
    Returns (film, [stats per device])."""
    pb = desc.film.pixel_bounds
    film = np.zeros((pb[3] - pb[1], pb[2] - pb[0]), dtype=FILM_DTYPE)
    devs = (C.c_int32 * len(devices))(*devices)
    stats = (abi.ShmStats * len(devices))()
    abi.check(lib, lib.shm_render_multi(C.byref(desc), devs, len(devices), C.byref(params), film.ctypes.data_as(C.c_void_p), stats), "shm_render_multi")
    return film, [st.as_dict() for st in stats]


def gather_film(local, rank, world_size, height, width, to_host=True):
    """TEST HARNESS (the product's gather is shm_render_sharded / shm_render_multi behind the C ABI): gather the per-rank films
    (flat float64 tensors) to rank 0 through torch.distributed ('gloo' in the CPU tests, 'nccl' = RCCL on a GPU).  Pixel ownership is exclusive (tiles are disjoint) and untouched
    pixels are exactly 0.0, so adding the slabs reproduces the single-process film bit for bit.
    to_host=False leaves the summed film on rank 0's device (a flat float64 tensor): the read-back is the caller's business
    (the reference writes its image once at the end, integrator.rs:311-321) and stays out of a timed region."""
    import torch
    import torch.distributed as dist

    gathered = [torch.empty_like(local) for _ in range(world_size)] if rank == 0 else None
    dist.gather(local, gathered, dst=0)
    if rank != 0:
        return None
    total = gathered[0].clone()
    for g in gathered[1:]:
        total += g
    if not to_host:
        return total
    return total.cpu().numpy().view(FILM_DTYPE).reshape(height, width)
