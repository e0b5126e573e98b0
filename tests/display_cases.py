"""Shared inputs of the display pass's tests (tests/test_display.py on the CPU twin, tests/test_gpu_display.py on the device): numpy-built films,
the edge film both suites bin and map, and a float64 restatement of the per-pixel pipeline of include/shimmer_hip.h's "the display pass"."""
import struct
import zlib

import numpy as np

from shimmer_amd import abi, render

CURVES = (abi.SHM_TONEMAP_NONE, abi.SHM_TONEMAP_REINHARD, abi.SHM_TONEMAP_ACES)
TRANSFERS = (abi.SHM_TRANSFER_LINEAR, abi.SHM_TRANSFER_SRGB)
LOG2_MIN = -16.0
LOG2_MAX_EIGHTHS = LOG2_MIN + 254 / 8  # 15.75: with it a bin is exactly an eighth of a stop, and 2^(log2_min + (b - 0.5) / 8) is bin b's centre
EDGE_W, EDGE_H = 24, 20  # the GPU suite's small film: the edge film is written into a scene of this size


def film_of(rgb, weight=1.0):
    """A FILM_DTYPE array (rgb's leading shape) whose pixels resolve to `rgb`: rgb_sum = rgb weight, weight_sum = weight (a power of two keeps the quotient exact)."""
    rgb = np.asarray(rgb, np.float64)
    film = np.zeros(rgb.shape[:-1], dtype=render.FILM_DTYPE)
    w = np.broadcast_to(np.asarray(weight, np.float64), rgb.shape[:-1])
    film["rgb_sum"] = rgb * w[..., None]
    film["weight_sum"] = w
    return film


def grey_film(values, shape):
    v = np.asarray(values, np.float64).reshape(shape)
    return film_of(np.repeat(v[..., None], 3, axis=-1))


def centre(b, log2_min=LOG2_MIN, log2_max=LOG2_MAX_EIGHTHS):
    """The luminance at the centre of bin b (1 .. 254)."""
    return 2.0 ** (log2_min + (b - 0.5) * (log2_max - log2_min) / 254)


def edge_film():
    """(film of EDGE_H x EDGE_W, the bin each pixel is counted in or -1, the indices of the named special pixels). Bins are those of log2_min = LOG2_MIN and
    log2_max = LOG2_MAX_EIGHTHS. Every bin's centre once; pixels without weight; Y = 0, negative, NaN, +inf and -inf; luminances below, above and on the range's ends; a
    weight that is not 1; the rest greys at the centres of random bins."""
    inf, nan = np.inf, np.nan
    rows = [((centre(b),) * 3, 1.0, b) for b in range(1, 255)]
    at = {}

    def add(name, rgb, weight, b):
        at[name] = len(rows)
        rows.append((rgb, weight, b))

    add("no_weight", (0.5, 0.25, 0.125), 0.0, -1)
    add("no_weight_black", (0.0, 0.0, 0.0), 0.0, -1)
    add("black", (0.0, 0.0, 0.0), 1.0, -1)
    add("negative", (-1.0, -2.0, -0.5), 1.0, -1)
    add("nan", (nan, 0.5, 0.5), 1.0, -1)
    add("all_nan", (nan, nan, nan), 1.0, -1)
    add("plus_inf", (inf, 0.0, 0.0), 1.0, -1)
    add("minus_inf", (0.5, -inf, 0.5), 1.0, -1)
    add("both_inf", (inf, -inf, 0.0), 1.0, -1)
    add("below", (2.0 ** -20,) * 3, 1.0, 0)
    add("far_below", (1e-30,) * 3, 1.0, 0)
    add("above", (2.0 ** 17,) * 3, 1.0, 255)
    add("far_above", (1e30,) * 3, 1.0, 255)
    add("red", (1.0, 0.0, 0.0), 1.0, 1 + int(np.floor((np.log2(0.2126) - LOG2_MIN) * 8)))
    add("weight_4", (centre(100),) * 3, 4.0, 100)
    add("mixed_negative", (2.0, -0.25, 0.5), 1.0, 1 + int(np.floor((np.log2(0.2126 * 2.0 + 0.7152 * -0.25 + 0.0722 * 0.5) - LOG2_MIN) * 8)))
    rng = np.random.default_rng(5)
    while len(rows) < EDGE_W * EDGE_H:
        b = int(rng.integers(1, 255))
        rows.append(((centre(b),) * 3, 1.0, b))
    rgb = np.array([r[0] for r in rows], np.float64).reshape(EDGE_H, EDGE_W, 3)
    weight = np.array([r[1] for r in rows], np.float64).reshape(EDGE_H, EDGE_W)
    film = np.zeros((EDGE_H, EDGE_W), dtype=render.FILM_DTYPE)
    with np.errstate(invalid="ignore"):
        film["rgb_sum"] = rgb * np.where(weight == 0.0, 1.0, weight)[..., None]
    film["weight_sum"] = weight
    return film, np.array([r[2] for r in rows]), at


def edge_params(lib, **overrides):
    return render.make_display_params(lib, log2_min=LOG2_MIN, log2_max=LOG2_MAX_EIGHTHS, **overrides)


def counts_of(bins):
    return np.bincount(bins[bins >= 0], minlength=256).astype(np.uint32)


def restate(rgb, scale, tonemap, transfer, white=4.0):
    """Steps 6 to 9 of the header's pipeline in float64 numpy, without dither: linear output RGB (.., 3) and the scale into the three codes (.., 3) as int64."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = np.asarray(rgb, np.float64) * np.float64(scale)
        c = np.where(s > 0, np.minimum(s, 65504.0), 0.0)
        if tonemap == abi.SHM_TONEMAP_REINHARD:
            Y = 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]
            Yd = Y * (1 + Y / (white * white)) / (1 + Y)
            c = c * np.where(Y > 0, Yd / np.where(Y > 0, Y, 1.0), 1.0)[..., None]
        elif tonemap == abi.SHM_TONEMAP_ACES:
            c = c * (2.51 * c + 0.03) / (c * (2.43 * c + 0.59) + 0.14)
        v = np.clip(c, 0.0, 1.0)
        if transfer == abi.SHM_TRANSFER_SRGB:
            v = np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(np.maximum(v, 1e-300), 1 / 2.4) - 0.055)
        return np.clip(np.floor(v * 255 + 0.5), 0, 255).astype(np.int64)


def state_tuple(st):
    """The named fields of an abi.ShmDisplayState (or of Renderer.display's dict) with the floats as bit patterns: what "the same state" compares."""
    get = (lambda n: st[n]) if isinstance(st, dict) else (lambda n: getattr(st, n))
    return tuple(int(np.float32(get(n)).view(np.uint32)) for n in ("log2_target", "log2_exposure", "scale")) + (int(get("counted")), int(get("valid")))


def decode_png(data):
    """An 8-bit RGB PNG decoded with zlib and struct, every chunk's CRC checked: (H, W, 3) uint8."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        (n,), tag = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        at += 12 + n
    assert [t for t, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3)
