"""What both temporal suites share: cameras through the library's own constructors, synthetic film / G-buffer builders whose positions a camera sees at the pixel centres,
the GPU suite's case table, and a float32 numpy restatement of the blend that shares no code with shm/temporal.h: whole-image arrays, numpy's
own float32 operations — one rounding each, no contraction, as the header's."""
import ctypes as C

import numpy as np

from shimmer_amd import abi, render

WHITE = np.array([106.0, 107.0, 105.0])  # what shm_gbuffer_white would give: any positive triple serves the twin
F1 = np.float32(1.0)


# ---- cameras ----
def camera_params(pos=(0.0, 0.0, 0.0), res=(16, 16), fov=90.0, orthographic=False, render_space=abi.SHM_RENDER_SPACE_WORLD):
    """A camera at `pos` looking down +z with +y up (world_from_camera is a translation), for shm_camera_create / shm_camera_create_in."""
    p = abi.ShmCameraParams()
    p.kind = abi.SHM_CAMERA_ORTHOGRAPHIC if orthographic else abi.SHM_CAMERA_PERSPECTIVE
    p.render_space = render_space
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = pos
    p.world_from_camera[:] = [float(x) for x in m.ravel()]
    p.fov_deg = fov
    p.full_resolution[:] = list(res)
    p.focal_distance = 1e6
    return p


def make_camera(lib, params):
    """(abi.ShmCamera, render_from_world (16,) float32) of shm_camera_create."""
    cam, rfw = abi.ShmCamera(), np.zeros(16, np.float32)
    abi.check(lib, lib.shm_camera_create(C.byref(params), C.byref(cam), rfw.ctypes.data_as(abi.c_float_p)), "shm_camera_create")
    return cam, rfw


def camera(lib, **kw):
    return make_camera(lib, camera_params(**kw))[0]


def plane_points(cam, width, height, depth, offset=None):
    """(H, W, 3) float64 render-space points: where the camera's ray through each pixel's centre (plus `offset`, (H, W, 2) raster units) meets the plane at `depth` along
    the camera's axis. From the ShmCamera's own matrices, in float64."""
    cfr = np.array(cam.camera_from_raster[:], np.float64).reshape(4, 4)
    rfc = np.array(cam.render_from_camera[:], np.float64).reshape(4, 4)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    r = np.stack([xx + 0.5, yy + 0.5, np.zeros_like(xx), np.ones_like(xx)], axis=-1)
    if offset is not None:
        r[..., :2] += offset
    pc = r @ cfr.T
    pc = pc[..., :3] / pc[..., 3:4]
    if cam.kind == abi.SHM_CAMERA_PERSPECTIVE:
        pc = pc * (depth / pc[..., 2:3])
    else:
        pc[..., 2] = depth
    return (np.concatenate([pc, np.ones_like(pc[..., :1])], axis=-1) @ rfc.T)[..., :3]


# ---- inputs ----
def make_inputs(colour, position, normal=None, albedo=None, weight=1.0):
    """FILM_DTYPE and GBUFFER_DTYPE arrays (H, W) whose every double is a float32 value. colour, position: (H, W, 3); normal: (H, W, 3), default -z (facing a camera
    that looks down +z); albedo: (H, W, 3), default 1 (a_eff = 1 exactly: white / white); weight: weight_sum = weight_hit of every pixel (1: c is rgb_sum itself)."""
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    h, w = colour.shape[:2]
    film = np.zeros((h, w), render.FILM_DTYPE)
    g = np.zeros((h, w), render.GBUFFER_DTYPE)
    ws = f32(np.full((h, w), weight))
    if normal is None:
        normal = np.zeros((h, w, 3)); normal[..., 2] = -1.0
    if albedo is None:
        albedo = np.ones((h, w, 3))
    film["weight_sum"] = ws
    film["rgb_sum"] = f32(f32(colour) * ws[..., None])
    g["weight_sum"] = ws
    g["weight_hit"] = ws
    g["p"] = f32(f32(position) * ws[..., None])
    g["ns"] = f32(f32(normal) * ws[..., None])
    g["n"] = g["ns"]
    g["albedo"] = f32(f32(albedo) * ws[..., None] * WHITE)
    return film, g


def colour_of(film):
    """c as the twin defines it: float32(rgb_sum) / float32(weight_sum), 0 where weight_sum is 0."""
    rgb, w = film["rgb_sum"].astype(np.float32), film["weight_sum"].astype(np.float32)
    out = np.zeros_like(rgb)
    nz = w != 0
    out[nz] = rgb[nz] / w[nz][..., None]
    return out


def result_rgb(out):
    return out["rgb_sum"].astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the blend, restated ----
def luminance(c):
    c = np.asarray(c, np.float32)
    return ((c[..., 0] + c[..., 1]) + c[..., 2]) / np.float32(3.0)


def start(c1):
    """The record of a pixel without history: (rgb, m1, m2, length), float32."""
    c1 = np.asarray(c1, np.float32)
    l = luminance(c1)
    return c1.copy(), l, l * l, np.ones(l.shape, np.float32)


def blend(h, c1, alpha_min, alpha_min_moments, max_history):
    """Step 4 with history h = (rgb, m1, m2, length): the new (rgb, m1, m2, length), float32 throughout."""
    h_rgb, h_m1, h_m2, h_len = (np.asarray(a, np.float32) for a in h)
    c1 = np.asarray(c1, np.float32)
    l = luminance(c1)
    length = np.minimum(h_len + F1, np.float32(max_history))
    inv = F1 / length
    a = np.maximum(inv, np.float32(alpha_min))
    am = np.maximum(inv, np.float32(alpha_min_moments))
    rgb = h_rgb + a[..., None] * (c1 - h_rgb)
    m1 = h_m1 + am * (l - h_m1)
    m2 = h_m2 + am * (l * l - h_m2)
    return rgb, m1, m2, length


def record_fields(rec):
    return rec["rgb"], rec["m1"], rec["m2"], rec["length"]


def assert_record_is(rec, want, where=None, what=""):
    """rec's (rgb, m1, m2, length) equal `want`'s, bit for bit (over the mask `where`)."""
    for name, got, exp in zip(("rgb", "m1", "m2", "length"), record_fields(rec), want):
        g, e = bits(got), bits(exp)
        if where is not None:
            g, e = g[where], e[where]
        assert np.array_equal(g, e), (what, name, np.argwhere(g != e)[:4])


# ---- the GPU suite's cases ----
# name -> (the camera's position, what it looks at, fov): the generators' own cameras (shimmer_amd/scenes.py), which frame 0 keeps
VIEWS = {"cornell": ((0.0, 1.0, 3.4), (0.0, 1.0, 0.0), 39.0), "textured": ((0.0, 1.0, 3.4), (0.0, 1.0, 0.0), 39.0), "escaped": ((0.0, 0.0, 8.0), (0.0, 0.0, 0.0), 60.0)}  # (the escaped camera looks down -z: towards the middle sphere)


def orbit(view, degrees, dolly=0.0, centre=None):
    """The view turned by `degrees` about the vertical through `centre` (default: what it looks at) and moved `dolly` towards it: (pos, look_at)."""
    pos, look, _ = view
    pos, look = np.array(pos, np.float64), np.array(look, np.float64)
    c = look if centre is None else np.array(centre, np.float64)
    a = np.radians(degrees)
    rot = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    p = c + rot @ (pos - c)
    p = p + dolly * (look - p) / np.linalg.norm(look - p)
    return tuple(p), tuple(look)


def sequence(name, motion):
    """Three frames' (pos, look_at) or None (frame 0: the scene's own camera). motion: "still" | "orbit" | "dolly"."""
    v = VIEWS[name]
    centre = None
    if motion == "still":
        return [None, None, None]
    step = 8.0 if name == "escaped" else 3.0  # (degrees a frame; the spheres' silhouettes move a pixel per three degrees at 24 x 20: eight uncover sky-backed pixels)
    if motion == "orbit":
        return [None, orbit(v, step, centre=centre), orbit(v, 2.0 * step, centre=centre)]
    return [None, orbit(v, 0.0, dolly=0.3 if name != "escaped" else 1.0), orbit(v, step, dolly=0.6 if name != "escaped" else 2.0, centre=centre)]


# (scene, sampler, filter, demodulate, motion, width, height)
ROWS = [(sc, sa, f, dm, mo, 24, 20) for sc in VIEWS for sa in ("independent", "zsobol") for f in ("box", "mitchell") for dm in (0, 1)
        for mo in (("orbit",) if (sa, f) != ("independent", "box") else ("orbit", "dolly"))]
ROWS += [("cornell", "zsobol", "box", 1, "still", 24, 20), ("cornell", "independent", "box", 1, "orbit", 70, 45), ("escaped", "zsobol", "mitchell", 1, "dolly", 70, 45)]
