"""What both moments suites share: synthetic film sequences and a float64 numpy restatement of the moments pass, written from DESIGN.md section 4k alone (it shares no
code with shm/moments.h: whole-image arrays instead of per-pixel loops). numpy's float64 + - * / are the correctly rounded operations the section names, taken in
the order it gives, so the restatement is held to the library bit for bit."""
import numpy as np

from shimmer_amd import render

EPS = 2.0 ** -53  # double's unit roundoff


def tile_boxes(width, height, tile=8):
    """(x0, y0, x1, y1) of the row-major tile x tile tiling of a width x height film, edge tiles clipped: what shm_tile_bounds gives for bounds (0, 0, w, h)."""
    return [(x, y, min(x + tile, width), min(y + tile, height)) for y in range(0, height, tile) for x in range(0, width, tile)]


def clear(film):
    """Records that count from `film`: zeros, prev = the film."""
    m = np.zeros(film.shape, render.MOMENTS_DTYPE)
    m["prev"][..., 0:3] = film["rgb_sum"]
    m["prev"][..., 3] = film["weight_sum"]
    return m


def e2_of(m, floor):
    """(v, s2, e2) of records in float64: s2 = m2 / (B - 1), v = s2 / W (0 while B < 2), e2 = (((v_r + v_g) + v_b) / 3) / max(((mean_r + mean_g) + mean_b) / 3, floor)^2."""
    with np.errstate(all="ignore"):
        two = (m["batches"] >= 2.0)[..., None]
        s2 = np.where(two, m["m2"] / (m["batches"] - 1.0)[..., None], 0.0)
        v = np.where(two, s2 / m["weight"][..., None], 0.0)
        mu = ((m["mean"][..., 0] + m["mean"][..., 1]) + m["mean"][..., 2]) / 3.0
        fl = np.float64(np.float32(floor))
        den = np.where(mu > fl, mu, fl)
        e2 = (((v[..., 0] + v[..., 1]) + v[..., 2]) / 3.0) / (den * den)
    return v, s2, e2


def converged(m, floor, threshold, min_batches):
    _, _, e2 = e2_of(m, floor)
    t = np.float64(np.float32(threshold))
    with np.errstate(all="ignore"):
        return (m["batches"] >= float(min_batches)) & (e2 < t * t)


def _total_order_max(e):
    """The maximum of float32 values (no NaN among them) under the total order in which -0 is below +0."""
    top = e.max()
    if top == 0.0:
        return np.float32(0.0) if (~np.signbit(e[e == 0.0])).any() else np.float32(-0.0)
    return top


def update(film, m, boxes, min_batches, threshold, floor):
    """One batch, in place, over the pixels of `boxes`; returns the TILE_ERROR_DTYPE array. The section's update, verbatim:
        dw = F.w - prev.w;  x_c = (F.c - prev.c) / dw
        not counted (prev = F, nothing else) unless dw > 0 and every x_c finite
        W' = W + dw;  d_c = x_c - mean_c;  mean_c' = mean_c + d_c * (dw / W');  m2_c' = m2_c + (dw * d_c) * (x_c - mean_c');  B' = B + 1"""
    mask = np.zeros(film.shape, bool)
    for (x0, y0, x1, y1) in boxes:
        mask[y0:y1, x0:x1] = True
    F = np.concatenate([film["rgb_sum"], film["weight_sum"][..., None]], axis=-1)
    with np.errstate(all="ignore"):
        dw = F[..., 3] - m["prev"][..., 3]
        x = (F[..., 0:3] - m["prev"][..., 0:3]) / dw[..., None]
        counted = mask & (dw > 0.0) & np.isfinite(x).all(axis=-1)
        w1 = m["weight"] + dw
        r = dw / w1
        d = x - m["mean"]
        mean1 = m["mean"] + d * r[..., None]
        m2 = m["m2"] + (dw[..., None] * d) * (x - mean1)
    c3 = counted[..., None]
    m["prev"] = np.where(mask[..., None], F, m["prev"])
    m["mean"] = np.where(c3, mean1, m["mean"])
    m["m2"] = np.where(c3, m2, m["m2"])
    m["weight"] = np.where(counted, w1, m["weight"])
    m["batches"] = np.where(counted, m["batches"] + 1.0, m["batches"])
    _, _, e2 = e2_of(m, floor)
    conv = converged(m, floor, threshold, min_batches)
    with np.errstate(all="ignore"):
        e2f = e2.astype(np.float32)
    e2f = np.where(np.isnan(e2f), np.float32(np.inf), e2f)
    out = np.zeros(len(boxes), render.TILE_ERROR_DTYPE)
    for i, (x0, y0, x1, y1) in enumerate(boxes):
        out["unconverged"][i] = int((~conv[y0:y1, x0:x1]).sum())
        out["max_e2"][i] = _total_order_max(e2f[y0:y1, x0:x1].ravel())
    return out


def resolve(m, floor):
    """shm_moments_resolve's 8 floats per record: v[3], s2[3], B, e2, each rounded from float64 once."""
    v, s2, e2 = e2_of(m, floor)
    with np.errstate(all="ignore"):
        return np.concatenate([v, s2, m["batches"][..., None], e2[..., None]], axis=-1).astype(np.float32)


def film_sequence(width, height, weights, rng, mean=1.0, sigma=0.5, per_pixel_weights=False):
    """Films after each batch of a synthetic render: batch b adds weight w_b (or, per_pixel_weights, a signed per-pixel weight around it, as a Mitchell filter's) and
    w_b times a batch mean drawn around `mean`. Returns (the list of FILM_DTYPE arrays, the batch means (B, H, W, 3), the batch weights (B, H, W))."""
    film = np.zeros((height, width), render.FILM_DTYPE)
    films, xs, ws = [], [], []
    for w in weights:
        wb = np.full((height, width), float(w)) if not per_pixel_weights else float(w) * rng.uniform(-0.3, 1.3, (height, width))
        x = mean + sigma * rng.normal(size=(height, width, 3))
        film = film.copy()
        film["rgb_sum"] += x * wb[..., None]
        film["weight_sum"] += wb
        films.append(film)
        xs.append(x)
        ws.append(wb)
    return films, np.array(xs), np.array(ws)


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
