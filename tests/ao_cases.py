"""The ambient occlusion integrator's CPU chain, shared by tests/test_ambient_occlusion.py and tests/test_gpu_ambient_occlusion.py: host-twin camera rays
(shm_gbuffer_camera_rays) -> the oracle's closest-hit trace -> shm_ao_samples_host (shm/ao.h on the host) -> the oracle's any-hit trace over the queued occlusion rays
-> the film's own rule, a pixel's samples added in increasing sample index in float64 (include/shimmer_hip.h, at shm_ao_samples_host)."""
import ctypes as C

import numpy as np

import gbuffer_cases as gc
import oracle_py
from shimmer_amd import abi, render

RAY_DTYPE = np.dtype([("o", np.float32, 3), ("d", np.float32, 3), ("t_max", np.float32), ("pad", np.float32)])


def params_for(sampler="independent", seed=11, spp=4, uniform=False, max_distance=0.0, **kw):
    return render.make_params(seed=seed, spp=spp, max_depth=5, sampler=sampler, integrator="ambientocclusion", ao_uniform_sample=uniform, ao_max_distance=max_distance, **kw)


def twin(lib, desc, params, pix, idx, hits):
    """shm_ao_samples_host: (occlusion rays as an (n, 8) float32 array, queued flags (n,) uint8, (n, 5) float32: rgb if unoccluded, the filter weight, the direction's pdf)."""
    hits = np.ascontiguousarray(hits)
    n = len(idx)
    rays, queued, sample = np.zeros((n, 8), np.float32), np.zeros(n, np.uint8), np.zeros((n, 5), np.float32)
    abi.check(lib, lib.shm_ao_samples_host(C.byref(desc), C.byref(params), gc._i32(pix), gc._i32(idx), hits.ctypes.data_as(C.c_void_p), n, rays.ctypes.data_as(C.c_void_p),
                                           queued.ctypes.data_as(C.c_void_p), sample.ctypes.data_as(abi.c_float_p)), "shm_ao_samples_host")
    return rays, queued, sample


def open_oracle(desc, params):
    """An oracle whose two traversals enter instances as a render with these parameters does (ShmRenderParams::disable_reference_quirks)."""
    orc = oracle_py.Oracle(desc)
    orc.lib.orc_set_quirks_off.restype, orc.lib.orc_set_quirks_off.argtypes = None, [C.c_void_p, C.c_int]
    orc.lib.orc_set_quirks_off(orc.handle, int(params.disable_reference_quirks))
    return orc


class Chain:
    """One scene through the CPU chain, samples [begin, end) of every pixel of the film (or of `pixels`, an (n, 2) list)."""

    def __init__(self, lib, desc, params, orc=None, begin=0, end=None, pixels=None):
        self.lib, self.desc, self.params = lib, desc, params
        pb = tuple(desc.film.pixel_bounds)
        self.pb, self.width, self.height = pb, pb[2] - pb[0], pb[3] - pb[1]
        end = params.samples_per_pixel if end is None else end
        pix, idx = gc.all_samples(pb, end - begin)
        idx = np.ascontiguousarray(idx + begin, dtype=np.int32)
        if pixels is not None:
            keep = np.zeros((self.height, self.width), bool)
            for x, y in pixels:
                keep[y - pb[1], x - pb[0]] = True
            sel = keep[pix[:, 1] - pb[1], pix[:, 0] - pb[0]]
            pix, idx = np.ascontiguousarray(pix[sel]), np.ascontiguousarray(idx[sel])
        self.pix, self.idx, self.n_per_pixel = pix, idx, end - begin
        own = orc is None
        orc = open_oracle(desc, params) if own else orc
        self.rays = gc.twin_rays(lib, desc, params, pix, idx)
        self.hits, s_closest = orc.trace(self.rays)
        self.occ_rays, self.queued, self.sample = twin(lib, desc, params, pix, idx, self.hits)
        q = self.queued != 0
        self.occluded = np.zeros(len(idx), bool)
        s_any = dict(rays_any=0, nodes_any=0, tris_any=0)
        if q.any():
            occ, s_any = orc.trace(self.occ_rays[q], any_hit=True)
            self.occluded[q] = occ != 0
        self.unoccluded = q & ~self.occluded
        self.stats = dict(paths=len(idx), rays_closest=s_closest["rays_closest"], rays_any=s_any["rays_any"], nodes_closest=s_closest["nodes_closest"],
                          tris_closest=s_closest["tris_closest"], nodes_any=s_any["nodes_any"], tris_any=s_any["tris_any"])
        if own:
            orc.close()

    def film(self, into=None):
        """The film pixels these samples make: rgb_sum[c] += (double)(w * rgb[c]) and weight_sum += (double)w, per pixel in sample order."""
        film = np.zeros((self.height, self.width), dtype=render.FILM_DTYPE) if into is None else into.copy()
        w = self.sample[:, 3]
        rgb = np.where(self.unoccluded[:, None], self.sample[:, :3], np.float32(0.0))
        contrib = (w[:, None] * rgb).astype(np.float32).astype(np.float64)  # the float product, widened
        y, x = self.pix[:, 1] - self.pb[1], self.pix[:, 0] - self.pb[0]
        # all_samples is pixel-major with a pixel's samples adjacent and increasing: add sample k of every pixel, k ascending
        n = self.n_per_pixel
        for k in range(n):
            s = slice(k, None, n)
            film["rgb_sum"][y[s], x[s]] += contrib[s]
            film["weight_sum"][y[s], x[s]] += w[s].astype(np.float64)
        return film


def stats_equal(gpu, cpu):
    return {k: (gpu[k], cpu[k]) for k in cpu if gpu[k] != cpu[k]}
