"""What both denoiser suites share: synthetic film / G-buffer builders and a float64 numpy restatement of the filter, written from DESIGN.md section 4j alone (it shares no
code with shm/denoise.h: whole-image shifted arrays instead of per-pixel loops, numpy's exp and power instead of fp.h's)."""
import numpy as np

from shimmer_amd import render

SIZES = ((24, 20), (37, 70))  # (width, height): one smaller than the last iterations' reach, one that is a multiple of nothing
WHITE = np.array([106.0, 107.0, 105.0])  # what shm_gbuffer_white would give: any positive triple serves the twin
TINY = 1e-10
U = 2.0 ** -24  # float32's unit roundoff


def unity_bound(iterations):
    """The relative error a constant (or, times the input range, a linearly filtered) signal may pick up in `iterations` iterations of float32 arithmetic: per iteration the
    25 products w e of the numerator — the sums run in step over the same w, so their rounding is shared with the denominator's to first order — and the division, 26
    roundings; once, the division by a_eff, the multiplication by a_eff, and the two roundings that made c = rgb_sum / weight_sum a float32: 4."""
    return (26 * iterations + 4) * U


def make_inputs(width, height, rng, colour=None, normal=None, position=None, albedo=None, coverage=None):
    """FILM_DTYPE and GBUFFER_DTYPE arrays (height, width) whose every double is a float32 value (so float32(a / b) in double and float32(a) / float32(b) agree: double
    rounding is innocuous for a quotient of 24-bit operands at 53 bits). colour / normal / position / albedo: (H, W, 3) or None for defaults; coverage: (H, W) in (0, 1]."""
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    film = np.zeros((height, width), render.FILM_DTYPE)
    g = np.zeros((height, width), render.GBUFFER_DTYPE)
    ws = f32(rng.uniform(2.0, 4.0, (height, width)))
    cov = f32(np.ones((height, width)) if coverage is None else coverage)
    wh = f32(ws * cov)
    yy, xx = np.mgrid[0:height, 0:width]
    if colour is None:
        colour = rng.uniform(0.2, 1.5, (height, width, 3))
    if normal is None:
        normal = np.zeros((height, width, 3)); normal[..., 2] = 1.0
    if position is None:  # the plane z = 0, one unit per pixel
        position = np.stack([xx, yy, np.zeros_like(xx)], axis=-1).astype(np.float64)
    if albedo is None:
        albedo = np.full((height, width, 3), 0.5)
    film["weight_sum"] = ws
    film["rgb_sum"] = f32(f32(colour) * ws[..., None])
    g["weight_sum"] = ws
    g["weight_hit"] = wh
    g["p"] = f32(f32(position) * wh[..., None])
    g["ns"] = f32(f32(normal) * wh[..., None])
    g["n"] = g["ns"]
    g["albedo"] = f32(f32(albedo) * wh[..., None] * WHITE)
    return film, g


def bumpy_guides(width, height, rng):
    """Arbitrary valid guides: a heightfield's normals and positions, varying albedo and coverage."""
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    z = 0.8 * np.sin(xx * 0.37) * np.cos(yy * 0.23) + 0.05 * rng.normal(size=(height, width))
    n = np.stack([-0.3 * np.cos(xx * 0.37), 0.2 * np.sin(yy * 0.23), np.ones_like(xx)], axis=-1) + 0.05 * rng.normal(size=(height, width, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    p = np.stack([xx * 0.1, yy * 0.1, z * 0.1], axis=-1)
    albedo = rng.uniform(0.05, 0.9, (height, width, 3))
    coverage = rng.uniform(0.5, 1.0, (height, width))
    return n, p, albedo, coverage


def colour_of(film):
    """c as the twin defines it: float32(rgb_sum) / float32(weight_sum), 0 where weight_sum is 0."""
    rgb, w = film["rgb_sum"].astype(np.float32), film["weight_sum"].astype(np.float32)
    out = np.zeros_like(rgb)
    nz = w != 0
    out[nz] = rgb[nz] / w[nz][..., None]
    return out


def result_rgb(out):
    assert np.array_equal(out["weight_sum"] != 0, out["weight_sum"] == 1.0)
    return out["rgb_sum"].astype(np.float32)


def _shift(a, dx, dy):
    """b[y, x] = a[y + dy, x + dx] where that lies inside the image, 0 elsewhere."""
    h, w = a.shape[:2]
    b = np.zeros_like(a)
    ys, yd = slice(max(0, dy), min(h, h + dy)), slice(max(0, -dy), min(h, h - dy))
    xs, xd = slice(max(0, dx), min(w, w + dx)), slice(max(0, -dx), min(w, w - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        b[yd, xd] = a[ys, xs]
    return b


def _geometry_weight(n, p, nq, pq, k):
    d = (n * nq).sum(-1)
    w_n = np.where(d > 0, np.power(np.maximum(d, 1e-300), k["sigma_normal"]), 0.0)
    dp = pq - p
    w_z = np.exp(-np.abs((n * dp).sum(-1)) / (k["sigma_plane"] * np.linalg.norm(dp, axis=-1) + TINY))
    return w_n * w_z


def params_dict(d):
    return {f: getattr(d, f) for f in ("iterations", "demodulate", "sigma_luminance", "sigma_normal", "sigma_plane", "albedo_floor")}


def reference(film, g, white, k, return_parts=False):
    """The filter of DESIGN.md section 4j in float64: (H, W, 3) sensor RGB. k: params_dict(ShmDenoiseParams)."""
    ws, wh = film["weight_sum"], g["weight_hit"]
    with np.errstate(all="ignore"):
        c = np.where((ws != 0)[..., None], film["rgb_sum"] / ws[..., None], 0.0)
        if k["iterations"] == 0:
            return c
        valid = (ws > 0) & (wh > 0)
        cov = np.clip(wh / g["weight_sum"], 0.0, 1.0)[..., None]  # the G-buffer's own ratio
        a = g["albedo"] / wh[..., None] / np.asarray(white, np.float64)
        ns = g["ns"] / wh[..., None]
        p = g["p"] / wh[..., None]
        a_eff = cov * a + (1.0 - cov)
        a_eff = np.where(a_eff < k["albedo_floor"], 1.0, a_eff) if k["demodulate"] else np.ones_like(c)
        e = c / a_eff
        length = np.linalg.norm(ns, axis=-1)
        n = ns / length[..., None]
        valid &= length > 0
        for arr in (c, n, p, a_eff, e):
            valid &= np.isfinite(arr).all(-1)
    vf = valid.astype(np.float64)
    e, n, p = (np.where(valid[..., None], arr, 0.0) for arr in (e, n, p))
    var = np.zeros_like(vf)
    use_l = np.isfinite(k["sigma_luminance"])
    if use_l:  # the 7x7 moments of l
        l = e.mean(-1)
        sw, s1, s2 = (np.zeros_like(vf) for _ in range(3))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                vq, lq = _shift(vf, dx, dy), _shift(l, dx, dy)
                w = vq * (1.0 if dx == 0 and dy == 0 else _geometry_weight(n, p, _shift(n, dx, dy), _shift(p, dx, dy), k))
                sw += w; s1 += w * lq; s2 += w * lq * lq
        with np.errstate(all="ignore"):
            var = np.where(valid, np.maximum(0.0, s2 / sw - (s1 / sw) ** 2), 0.0)
    h1 = {0: 6 / 16, 1: 4 / 16, -1: 4 / 16, 2: 1 / 16, -2: 1 / 16}
    g1 = {0: 0.5, 1: 0.25, -1: 0.25}
    for it in range(k["iterations"]):
        s = 1 << it
        l = e.mean(-1)
        if use_l:
            gs, gw = np.zeros_like(vf), np.zeros_like(vf)
            for j in (-1, 0, 1):
                for i in (-1, 0, 1):
                    kq = g1[j] * g1[i] * _shift(vf, i * s, j * s)
                    if i or j:
                        kq = kq * _geometry_weight(n, p, _shift(n, i * s, j * s), _shift(p, i * s, j * s), k)
                    gs += kq * _shift(var, i * s, j * s)
                    gw += kq
            with np.errstate(all="ignore"):
                denom = k["sigma_luminance"] * np.sqrt(np.where(valid, gs / gw, 0.0)) + TINY
        sw, sv = np.zeros_like(vf), np.zeros_like(vf)
        se = np.zeros_like(e)
        for j in range(-2, 3):
            for i in range(-2, 3):
                dx, dy = i * s, j * s
                w = h1[j] * h1[i] * _shift(vf, dx, dy)
                if i or j:
                    w = w * _geometry_weight(n, p, _shift(n, dx, dy), _shift(p, dx, dy), k)
                    if use_l:
                        w = w * np.exp(-np.abs(l - _shift(l, dx, dy)) / denom)
                sw += w
                se += w[..., None] * _shift(e, dx, dy)
                sv += w * w * _shift(var, dx, dy)
        with np.errstate(all="ignore"):
            e = np.where(valid[..., None], se / sw[..., None], 0.0)
            var = np.where(valid, sv / (sw * sw), 0.0)
    out = np.where(valid[..., None], e * a_eff, c)
    return (out, e, a_eff, valid) if return_parts else out
