"""The G-buffer pass's test scenes and the chain both suites share: host-twin camera rays -> a closest-hit trace (the CPU oracle's in tests/test_gbuffer.py, the GPU's own
in tests/test_gpu_gbuffer.py) -> shm_gbuffer_samples_host -> a pixel's sums, the samples added in increasing sample index in float64."""
import ctypes as C

import numpy as np

from shimmer_amd import abi, render, scenes

W, H, SPP = 24, 20, 3  # not a multiple of the 8x8 tile; not a power of two

# one row per scene class: name -> generator(lib, width, height, film)
SCENES = {
    "cornell": lambda lib, w, h, film: scenes.cornell_box(lib, w, h, film=film),                                       # the lean class
    "materials": lambda lib, w, h, film: scenes.cornell_box(lib, w, h, glass=True, mix=True, film=film),                # conductor, thin dielectric, coated diffuse, mix
    "coated": lambda lib, w, h, film: scenes.cornell_box(lib, w, h, coated=True, glass_too=True, film=film),            # both coated BxDFs, smooth and rough dielectric
    "textured": lambda lib, w, h, film: scenes.cornell_box(lib, w, h, textured=True, film=film),                        # HAS_TEX: ray differentials, bump and normal maps
    "quadrics": lambda lib, w, h, film: scenes.quadric_scene(lib, width=w, height=h, film=film),
    "patches": lambda lib, w, h, film: scenes.cornell_box(lib, w, h, patches=True, patch_skew=0.1, film=film),
    "instanced": lambda lib, w, h, film: scenes.instanced_scene(lib, w, h, film=film),
    "diffuse_transmission": lambda lib, w, h, film: scenes.cornell_box(lib, w, h, diffuse_transmission="sheet tall sphere", film=film),
    "spherical": lambda lib, w, h, film: scenes.cornell_box(lib, w, h, camera={"type": "spherical", "pos": (0.0, 1.0, 0.5)}, film=film),
    # (the orthographic camera's rays stay in camera space, as the reference leaves them: a camera whose axes are the world's sees the room, through its back wall)
    "orthographic": lambda lib, w, h, film: scenes.cornell_box(lib, w, h, camera={"type": "orthographic", "pos": (0.0, 1.0, -5.0), "look_at": (0.0, 1.0, 0.0)}, film=film),
    "tilted": lambda lib, w, h, film: scenes.cornell_box(lib, w, h, camera={"type": "perspective", "pos": (0.8, 1.6, 3.2)}, film=film),  # camera space is a general rotation away
    "fuzz1": lambda lib, w, h, film: scenes.random_scene(lib, 1, w, h, film=film),
    "fuzz2": lambda lib, w, h, film: scenes.random_scene(lib, 2, w, h, film=film),
}
FILTERS = ("box", "gaussian", "mitchell")  # weight 1 / one constant / signed per sample
SAMPLERS = ("independent", "zsobol")
SPACES = (abi.SHM_GBUFFER_SPACE_RENDER, abi.SHM_GBUFFER_SPACE_CAMERA)


def gpu_rows():
    """(scene, sampler, filter, space): every variation on the Cornell box, and one per other scene — walking through the variations so that each is met off the box too."""
    rows = [("cornell", s, f, sp) for s in SAMPLERS for f in FILTERS for sp in SPACES]
    k = 0
    for name in SCENES:
        if name == "cornell":
            continue
        rows.append((name, SAMPLERS[k % 2], FILTERS[k % 3], SPACES[(k // 2) % 2]))
        k += 1
    return rows


def make_scene(lib, name, filt="box", size=(W, H)):
    return SCENES[name](lib, size[0], size[1], None if filt == "box" else {"filter": filt})


def all_samples(pixel_bounds, spp):
    """Every (pixel, sample) of the film, pixel-major in row order, a pixel's samples in increasing index: (n, 2) int32 pixels and (n,) int32 indices."""
    x0, y0, x1, y1 = pixel_bounds
    ys, xs, ss = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), np.arange(spp), indexing="ij")
    pix = np.ascontiguousarray(np.stack([xs.ravel(), ys.ravel()], axis=1), dtype=np.int32)
    return pix, np.ascontiguousarray(ss.ravel(), dtype=np.int32)


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def twin_rays(lib, desc, params, pix, idx):
    out = np.zeros((len(idx), 8), np.float32)
    abi.check(lib, lib.shm_gbuffer_camera_rays(C.byref(desc), C.byref(params), _i32(pix), _i32(idx), len(idx), out.ctypes.data_as(C.c_void_p)), "shm_gbuffer_camera_rays")
    return out


def twin_samples(lib, desc, params, space, pix, idx, hits):
    hits = np.ascontiguousarray(hits)
    out = np.zeros((len(idx), 16), np.float64)
    abi.check(lib, lib.shm_gbuffer_samples_host(C.byref(desc), C.byref(params), space, _i32(pix), _i32(idx), hits.ctypes.data_as(C.c_void_p), len(idx),
                                                out.ctypes.data_as(C.POINTER(C.c_double))), "shm_gbuffer_samples_host")
    return out


def twin_rho(lib, desc, params, pix, idx, hits):
    """(n, 12) float32: rho[4], lambda[4], pdf[4]."""
    hits = np.ascontiguousarray(hits)
    out = np.zeros((len(idx), 12), np.float32)
    abi.check(lib, lib.shm_gbuffer_rho_host(C.byref(desc), C.byref(params), _i32(pix), _i32(idx), hits.ctypes.data_as(C.c_void_p), len(idx),
                                            out.ctypes.data_as(abi.c_float_p)), "shm_gbuffer_rho_host")
    return out


def pixel_sums(samples, n_pixels, spp, begin=0, end=None):
    """(n_pixels, 16) float64: samples [begin, end) of every pixel added in increasing index, as the accumulation kernel adds them."""
    s = samples.reshape(n_pixels, spp, 16)
    out = np.zeros((n_pixels, 16), np.float64)
    for k in range(begin, spp if end is None else end):
        out = out + s[:, k]
    return out


def gbuffer_as_rows(g):
    """A GBUFFER_DTYPE array as (n_pixels, 16) float64, in ShmGBufferPixel's order."""
    return np.ascontiguousarray(g).view(np.float64).reshape(-1, 16)


def triangle_of(desc, prim):
    """The three float32 vertices (3, 3), the mesh's uv rows or None, and the mesh of a triangle hit's leaf-order primitive slot."""
    p = desc.primitives[prim]
    assert p.shape_kind == abi.SHM_SHAPE_TRIANGLE
    t = p.shape_index
    for m in range(desc.n_meshes):
        mesh = desc.meshes[m]
        if t < mesh.n_triangles:
            vi = [mesh.vertex_indices[3 * t + k] for k in range(3)]
            pts = np.array([[mesh.p[3 * v + c] for c in range(3)] for v in vi], np.float32)
            uv = np.array([[mesh.uv[2 * v + c] for c in range(2)] for v in vi], np.float32) if mesh.uv else None
            return pts, uv, mesh
        t -= mesh.n_triangles
    raise AssertionError("triangle index outside the scene's meshes")


def params_for(sampler="independent", seed=11, spp=SPP, **kw):
    return render.make_params(seed=seed, spp=spp, max_depth=5, sampler=sampler, **kw)
