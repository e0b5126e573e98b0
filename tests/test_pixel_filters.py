"""The pixel filters (shm/filter.h; DESIGN.md "Pixel filters") on the CPU: the sampler against a float64 restatement of PBRT-v4's 2-D FilterSampler, the rendered image
against the scene convolved with the filter (a step edge under an orthographic camera, rendered by the oracle), the film's weight sums, the loader, the ABI."""
import ctypes as C
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import oracle_py
from shimmer_amd import abi, render, scenes
from shimmer_amd.scene import SceneBuilder, blackbody_dense

ROOT = Path(__file__).resolve().parents[1]
KIND = {"box": 0, "gaussian": 1, "mitchell": 2, "sinc": 3, "triangle": 4}
# name -> (default radius, default parameters), PBRT-v4's
DEFAULTS = {"box": (0.5, ()), "gaussian": (1.5, (0.5,)), "mitchell": (2.0, (1.0 / 3.0, 1.0 / 3.0)), "sinc": (4.0, (3.0,)), "triangle": (2.0, ())}
TABULATED = ("gaussian", "mitchell", "sinc")
ANISOTROPIC = {"gaussian": (1.5, 2.25), "mitchell": (2.0, 3.0), "sinc": (4.0, 2.5)}
N_DRAWS = 4096


def f32(x):
    return float(np.float32(x))


def bits(x):
    return int(np.float32(x).view(np.uint32))


# ---- the restatement: PBRT-v4's filters and its 2-D FilterSampler, in float64 ----
def g1(name, x, r, params):
    """One axis of the separable filter, f(x, y) = g(x; rx) g(y; ry)."""
    x = np.asarray(x, np.float64)
    if name == "box":
        return (np.abs(x) <= r).astype(np.float64)
    if name == "triangle":
        return np.maximum(0.0, r - np.abs(x))
    if name == "gaussian":
        sigma = params[0]
        gauss = lambda v: np.exp(-v * v / (2 * sigma * sigma)) / np.sqrt(2 * np.pi * sigma * sigma)  # noqa: E731
        return np.maximum(0.0, gauss(x) - gauss(r))
    if name == "mitchell":
        b, c = params
        t = np.abs(2 * x / r)
        near = ((12 - 9 * b - 6 * c) * t**3 + (-18 + 12 * b + 6 * c) * t**2 + (6 - 2 * b)) / 6
        far = ((-b - 6 * c) * t**3 + (6 * b + 30 * c) * t**2 + (-12 * b - 48 * c) * t + (8 * b + 24 * c)) / 6
        return np.where(t <= 1, near, np.where(t <= 2, far, 0.0))
    if name == "sinc":
        return np.where(np.abs(x) > r, 0.0, np.sinc(x) * np.sinc(x / params[0]))  # np.sinc(x) = sin(pi x) / (pi x)
    raise KeyError(name)


def n_cells(r):
    return int(np.float32(32) * np.float32(r))


def cell_centres(r, n):
    return -r + 2 * r * (np.arange(n) + 0.5) / n


def find_interval(cdf, u):
    return np.clip(np.searchsorted(cdf, u, side="right") - 1, 0, len(cdf) - 2)


class FilterSampler2D:
    """FilterSampler: the filter at the cell centres of an int(32 rx) x int(32 ry) grid over [-r, r]^2, PiecewiseConstant2D over its absolute values."""

    def __init__(self, name, rx, ry, params):
        self.rx, self.ry, self.nx, self.ny = rx, ry, n_cells(rx), n_cells(ry)
        self.table = np.outer(g1(name, cell_centres(ry, self.ny), ry, params), g1(name, cell_centres(rx, self.nx), rx, params))  # [y, x]
        a = np.abs(self.table)
        self.cond_cdf = np.concatenate([np.zeros((self.ny, 1)), np.cumsum(a * (2 * rx / self.nx), axis=1)], axis=1)
        self.row_int = self.cond_cdf[:, -1].copy()
        for y in range(self.ny):
            self.cond_cdf[y] = self.cond_cdf[y] / self.row_int[y] if self.row_int[y] > 0 else np.arange(self.nx + 1) / self.nx
        self.marg_cdf = np.concatenate([[0.0], np.cumsum(self.row_int * (2 * ry / self.ny))])
        self.integral = self.marg_cdf[-1]
        self.marg_cdf = self.marg_cdf / self.integral
        self.k = float(a.sum() * (2 * rx / self.nx) * (2 * ry / self.ny))

    def sample(self, u):
        """u: [n, 2] -> p [n, 2], weight [n] = table[cell] / pdf(cell)."""
        ux, uy = u[:, 0].astype(np.float64), u[:, 1].astype(np.float64)
        iy = find_interval(self.marg_cdf, uy)
        dy = (uy - self.marg_cdf[iy]) / (self.marg_cdf[iy + 1] - self.marg_cdf[iy])
        ty = (iy + dy) / self.ny
        pdf_y = self.row_int[iy] / self.integral
        ix = np.array([find_interval(self.cond_cdf[y], x) for y, x in zip(iy, ux)])
        c0, c1 = self.cond_cdf[iy, ix], self.cond_cdf[iy, ix + 1]
        tx = (ix + (ux - c0) / (c1 - c0)) / self.nx
        pdf_x = np.abs(self.table[iy, ix]) / self.row_int[iy]
        p = np.stack([(1 - tx) * -self.rx + tx * self.rx, (1 - ty) * -self.ry + ty * self.ry], axis=1)
        return p, self.table[iy, ix] / (pdf_x * pdf_y)


def tent_inverse_cdf(u, r):
    u = u.astype(np.float64)
    return np.where(u < 0.5, -r + r * np.sqrt(2 * u), r - r * np.sqrt(np.maximum(2 * (1 - u), 0.0)))


# ---- the host build of shm/filter.h ----
DRIVER = r"""
#include <stdio.h>
#include <string.h>
#include <vector>
#include "shm/filter.h"
using namespace shm;
static float fl(unsigned b) { float f; memcpy(&f, &b, 4); return f; }
static unsigned bi(float f) { unsigned b; memcpy(&b, &f, 4); return b; }
int main() {
    unsigned kind, rx, ry, a, b, n;
    while (scanf("%u %u %u %u %u %u", &kind, &rx, &ry, &a, &b, &n) == 6) {
        std::vector<float> table(FILTER_TABLE_MAX_FLOATS, 0.0f);
        if (filter_class_of(kind) == FILTER_CLASS_TABULATED && filter_build_table(kind, fl(rx), fl(ry), fl(a), fl(b), table.data()) == 0) return 2;
        printf("%u", bi(table[0]));
        for (unsigned i = 0; i < n; ++i) {
            unsigned ux, uy; if (scanf("%u %u", &ux, &uy) != 2) return 1;
            V2 p; float w;
            filter_sample(kind, fl(rx), fl(ry), table.data(), v2(fl(ux), fl(uy)), p, w);
            printf(" %u %u %u", bi(p.x), bi(p.y), bi(w));
        }
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_filter(tmp_path_factory):
    """run(name, rx, ry, params, u) -> (K, p [n, 2], weight [n]) as float32, from a g++ build of shm/filter.h."""
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("filter")
    (d / "drv.cpp").write_text(DRIVER)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", str(ROOT / "shimmer_amd" / "csrc"), "-I", str(ROOT / "include"),
                    str(d / "drv.cpp"), "-o", str(d / "drv")], check=True)

    def run(name, rx, ry, params, u):
        words = filter_words(name, rx, ry, params, u)
        out = subprocess.run([str(d / "drv")], input=" ".join(map(str, words)) + "\n", check=True, capture_output=True, text=True).stdout.split()
        w = np.array(list(map(int, out)), np.uint32).view(np.float32)
        rest = w[1:].reshape(-1, 3)
        return float(w[0]), rest[:, :2].copy(), rest[:, 2].copy()
    return run


def filter_words(name, rx, ry, params, u):
    """The argument words of the driver and of the device probe (PROBE_FILTER_SAMPLE): kind, radius, two parameters, n, then n pairs of u, floats by their bits."""
    pr = (tuple(params) + (0.0, 0.0))[:2]
    return [KIND[name], bits(rx), bits(ry), bits(pr[0]), bits(pr[1]), len(u)] + [int(v) for v in np.ascontiguousarray(u, np.float32).view(np.uint32).ravel()]


def draws(seed=20240607):
    return np.random.default_rng(seed).random((N_DRAWS, 2), dtype=np.float32)


def sampler_cases():
    for name in TABULATED:
        r, params = DEFAULTS[name]
        yield name, r, r, params
        yield (name,) + ANISOTROPIC[name] + (params,)


@pytest.mark.parametrize("name, rx, ry, params", list(sampler_cases()))
def test_tabulated_sampler_equals_the_2d_filter_sampler(host_filter, name, rx, ry, params):
    """4 096 draws: p within 1e-5 r per axis of the float64 2-D FilterSampler's, |weight| its constant K within 1e-5, sign(weight) the sign of the table cell that holds p
    (draws within 2e-5 of a cell edge left out of the sign check only; at most 1 % of the draws)."""
    u = draws()
    ref = FilterSampler2D(name, f32(rx), f32(ry), tuple(f32(v) for v in params))
    p_ref, w_ref = ref.sample(u)
    assert np.allclose(np.abs(w_ref), ref.k, rtol=1e-7, atol=0.0)  # (the weight IS +-K)
    k, p, w = host_filter(name, rx, ry, params, u)
    err = np.abs(p.astype(np.float64) - p_ref) / np.array([rx, ry])
    print(f"[filter] {name} r = ({rx}, {ry}): max |p - p_ref| / r = {err.max():.3e}, K = {k:.9g} (restatement {ref.k:.9g})")
    assert (err <= 1e-5).all(), err.max()
    assert abs(k / ref.k - 1.0) <= 1e-5 and (np.abs(w) == np.float32(k)).all()
    # the sign: of the restatement's table at the cell that contains the driver's p
    fx, fy = (p[:, 0].astype(np.float64) + rx) / (2 * rx) * ref.nx, (p[:, 1].astype(np.float64) + ry) / (2 * ry) * ref.ny
    near_edge = (np.abs(fx - np.round(fx)) * (2 * rx / ref.nx) < 2e-5) | (np.abs(fy - np.round(fy)) * (2 * ry / ref.ny) < 2e-5)
    assert near_edge.mean() <= 0.01, near_edge.mean()
    ix, iy = np.clip(np.floor(fx).astype(int), 0, ref.nx - 1), np.clip(np.floor(fy).astype(int), 0, ref.ny - 1)
    keep = ~near_edge
    assert (np.sign(w[keep]) == np.sign(ref.table[iy[keep], ix[keep]])).all()
    if name != "gaussian":
        assert (w < 0).any() and (w > 0).any()  # (negative lobes are drawn)


def test_triangle_and_box_samplers(host_filter):
    u = draws()
    for rx, ry in ((2.0, 2.0), (1.25, 3.0)):
        k, p, w = host_filter("triangle", rx, ry, (), u)
        want = np.stack([tent_inverse_cdf(u[:, 0], rx), tent_inverse_cdf(u[:, 1], ry)], axis=1)
        assert (np.abs(p - want) <= 1e-5 * np.array([rx, ry])).all() and (w == 1.0).all()
    for rx, ry in ((0.5, 0.5), (0.75, 1.5)):
        k, p, w = host_filter("box", rx, ry, (), u)
        one, r = np.float32(1.0), np.array([rx, ry], np.float32)
        want = (-r) * (one - u) + r * u  # lerp(u, -r, r) in float32 (shm/fp.h)
        assert want.dtype == np.float32 and np.array_equal(p.view(np.uint32), want.view(np.uint32)) and (w == 1.0).all()


# ---- the image is the scene convolved with the filter ----
EDGE_W, EDGE_H, EDGE_AT, EDGE_SPP = 32, 64, 15.7, 1024


def step_edge_scene(lib, name, **film):
    """An orthographic camera at (0, 0, -5) looking down +z — its axes are the world's, so camera space and render space agree whichever of the two the camera ray is
    expressed in — at one emissive quad that covers every film point at raster x >= EDGE_AT (and goes on far beyond the image on its other three sides); nothing else.
    The film is higher than wide: the screen window is [-1, 1] in x, one pixel is 2 / EDGE_W world units, raster x grows with world x."""
    b = SceneBuilder()
    b.set_film(EDGE_W, EDGE_H, filter=name, **film)
    rfw = b.set_camera_look_at(lib, (0, 0, -5), (0, 0, 0), (0, 1, 0), 40.0, orthographic=True)
    x_edge = -1.0 + 2.0 * EDGE_AT / EDGE_W
    p = np.array([(x_edge, -10, 0), (10, -10, 0), (10, 10, 0), (x_edge, 10, 0)], np.float32)
    vi = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    b.add_mesh(scenes._to_render(p, rfw), vi, b.material_diffuse(0.0), emission=blackbody_dense(6500.0), emission_scale=1.0, two_sided=True)
    desc, info = b.build(lib)
    return desc, b


def edge_params():
    return render.make_params(seed=11, spp=EDGE_SPP, max_depth=1, disable_wavelength_jitter=True)


def edge_expectation(name, r, params, column):
    """(expected pooled pixel / a covered pixel, its standard error at n samples = 1) for the pixel column `column`: the filter's cells weighted by the fraction of each that
    lies at raster x >= EDGE_AT. Delta method for the ratio estimator sum(w I) / sum(w), w = K s with s = +-1 the cell's sign and I the coverage indicator:
    var = E[(I - R)^2] / (E[s_x] E[s_y])^2 per sample, the expectations under the sampling density |f| / K."""
    d = EDGE_AT - (column + 0.5)  # the edge's offset from the pixel centre
    if name == "box":
        ratio = float(np.clip((r - d) / (2 * r), 0.0, 1.0))
        return ratio, np.sqrt(ratio * (1 - ratio))
    if name == "triangle":
        cdf = 0.0 if d <= -r else (1.0 if d >= r else ((d + r) ** 2 / (2 * r * r) if d < 0 else 1 - (r - d) ** 2 / (2 * r * r)))
        ratio = 1.0 - cdf
        return ratio, np.sqrt(max(ratio * (1 - ratio), 0.0))
    n = n_cells(r)
    g = g1(name, cell_centres(r, n), r, params)
    lo = -r + 2 * r * np.arange(n) / n
    covered = np.clip((lo + 2 * r / n - d) / (2 * r / n), 0.0, 1.0)
    ratio = float((g * covered).sum() / g.sum())
    q, s = np.abs(g) / np.abs(g).sum(), np.sign(g)
    e_i, e_s = float((q * covered).sum()), float((q * s).sum())
    return ratio, np.sqrt(max(e_i - 2 * ratio * e_i + ratio * ratio, 0.0)) / (e_s * e_s)  # (y: the same filter at the same radius, E[s_y] = E[s_x])


def pooled_columns(film):
    """Per column: one channel's rgb_sum over all rows / weight_sum over all rows — one ratio of N samples."""
    return film["rgb_sum"][:, :, 1].sum(axis=0) / film["weight_sum"].sum(axis=0)


@pytest.mark.parametrize("name", list(KIND))
def test_step_edge_is_the_scene_convolved_with_the_filter(lib, name):
    r, params = DEFAULTS[name]
    desc, keep = step_edge_scene(lib, name)
    orc = oracle_py.Oracle(desc)
    film, _ = orc.render(edge_params(), n_threads=os.cpu_count() or 1)
    orc.close()
    col = pooled_columns(film)
    covered = col[EDGE_W - 1]  # (4.5 pixels or more inside the quad for every filter: radius <= 4, the quad goes on far beyond the image)
    assert covered > 0 and np.isfinite(col).all()
    n_samples = EDGE_H * EDGE_SPP
    negative = []
    for c in range(EDGE_W):
        if abs(c + 0.5 - EDGE_AT) > r + 1:
            continue
        want, se1 = edge_expectation(name, r, params, c)
        got, se = col[c] / covered, se1 / np.sqrt(n_samples)
        print(f"[filter] {name} column {c}: rendered {got:+.6f} expected {want:+.6f} se {se:.2e} ({(got - want) / se if se > 0 else 0.0:+.2f} se)")
        assert abs(got - want) <= 5 * se + 1e-9, (name, c, got, want, se)  # (1e-9: the f64 sums of float32 products where the expectation is exactly 0 or 1)
        if want < 0:
            negative.append((c, got, want))
    if name in ("mitchell", "sinc"):  # signed weights reach the film: a pixel centred 1.2 px outside the edge is NEGATIVE (sinc -0.051, mitchell -0.017)
        c, got, want = min(negative, key=lambda t: t[2])
        assert c == 14 and got < 0 and want < (-0.04 if name == "sinc" else -0.012), (c, got, want)
    else:
        assert not negative


# ---- film invariants ----
def small_scene(lib, name=None, **film):
    return scenes.cornell_box(lib, 12, 10, film=dict(filter=name, **film) if name else None)


@pytest.mark.parametrize("name", list(KIND))
def test_weight_sums(lib, host_filter, name):
    sc = small_scene(lib, name)
    spp = 6
    orc = oracle_py.Oracle(sc.desc)
    film, _ = orc.render(render.make_params(seed=3, spp=spp, max_depth=3), n_threads=2)
    orc.close()
    if name in ("box", "triangle"):
        assert (film["weight_sum"] == spp).all()
    elif name == "gaussian":  # one float32 constant summed in f64: exact
        k, _, _ = host_filter(name, 1.5, 1.5, (0.5,), draws()[:1])
        assert (film["weight_sum"] == spp * float(np.float32(k))).all()
    else:  # every weight is +-K: the sum is K times an integer of spp's parity between -spp and spp
        k, _, _ = host_filter(name, DEFAULTS[name][0], DEFAULTS[name][0], DEFAULTS[name][1], draws()[:1])
        m = film["weight_sum"] / float(np.float32(k))
        assert (m == np.round(m)).all() and (np.abs(m) <= spp).all() and ((m.astype(int) - spp) % 2 == 0).all()
        assert (m < spp).any()  # (some sample drew a negative lobe)


def test_without_pixel_jitter_every_filter_is_the_box_film(lib):
    p = render.make_params(seed=3, spp=4, max_depth=3, disable_pixel_jitter=True)
    films = {}
    for name in KIND:
        sc = small_scene(lib, name)  # (the description points into the builder's arrays: keep it)
        orc = oracle_py.Oracle(sc.desc)
        films[name], _ = orc.render(p, n_threads=2)
        orc.close()
        assert (films[name]["weight_sum"] == 4).all()
        assert np.array_equal(films[name], films["box"]), name


def test_filtered_film_differs_from_the_box_film_and_image_divides_by_the_weight(lib):
    p = render.make_params(seed=3, spp=4, max_depth=3)
    films = {}
    for name in KIND:
        sc = small_scene(lib, name)
        orc = oracle_py.Oracle(sc.desc)
        films[name], _ = orc.render(p, n_threads=2)
        orc.close()
    for name in KIND:
        if name != "box":
            assert not np.array_equal(films[name]["rgb_sum"], films["box"]["rgb_sum"]), name
    # shm_film_get_image divides where weight_sum != 0 (as PBRT-v4's RGBFilm::GetPixelRGB does) — also by a negative sum, and leaves a zero sum's pixel as it is
    film = films["sinc"].copy()
    film["weight_sum"][0, 0], film["weight_sum"][0, 1] = 0.0, -abs(film["weight_sum"][0, 1]) - 1.0
    img = render.film_get_image(lib, film, render.SRGB_FROM_XYZ)
    assert np.isfinite(img).all()
    ident = np.eye(3, dtype=np.float32)
    raw = render.film_get_image(lib, film, ident)
    assert np.allclose(raw[0, 1], film["rgb_sum"][0, 1] / film["weight_sum"][0, 1], rtol=1e-6)
    assert np.allclose(raw[0, 0], film["rgb_sum"][0, 0], rtol=1e-6)


# ---- the loader ----
SCENE = 'WorldBegin\nLightSource "point" "rgb I" [1 1 1]\nShape "sphere" "float radius" 1\n'


def parse(lib, text):
    out = C.POINTER(abi.ShmPbrtScene)()
    return lib.shm_scene_parse_pbrt(text.encode(), None, C.byref(out)), out


@pytest.mark.parametrize("line, kind, radius, params", [
    ("", "box", (0.5, 0.5), (0.0, 0.0)),
    ('PixelFilter "box"', "box", (0.5, 0.5), (0.0, 0.0)),
    ('PixelFilter "box" "float xradius" 1 "float yradius" 0.75', "box", (1.0, 0.75), (0.0, 0.0)),
    ('PixelFilter "gaussian"', "gaussian", (1.5, 1.5), (0.5, 0.0)),
    ('PixelFilter "gaussian" "float sigma" 0.75 "float xradius" 2 "float yradius" 1.25', "gaussian", (2.0, 1.25), (0.75, 0.0)),
    ('PixelFilter "mitchell"', "mitchell", (2.0, 2.0), (1.0 / 3.0, 1.0 / 3.0)),
    ('PixelFilter "mitchell" "float B" 0.5 "float C" 0.25 "float xradius" 3 "float yradius" 2.5', "mitchell", (3.0, 2.5), (0.5, 0.25)),
    ('PixelFilter "sinc"', "sinc", (4.0, 4.0), (3.0, 0.0)),
    ('PixelFilter "sinc" "float tau" 2 "float xradius" 3 "float yradius" 5', "sinc", (3.0, 5.0), (2.0, 0.0)),
    ('PixelFilter "triangle"', "triangle", (2.0, 2.0), (0.0, 0.0)),
    ('PixelFilter "triangle" "float xradius" 1.5 "float yradius" 3', "triangle", (1.5, 3.0), (0.0, 0.0)),
])
def test_loader_fills_the_filter(lib, line, kind, radius, params):
    rc, out = parse(lib, line + "\n" + SCENE)
    assert rc == 0, lib.shm_last_error()
    f = out.contents.desc.film
    assert f.filter == KIND[kind] and tuple(f.filter_radius) == tuple(map(f32, radius)) and tuple(f.filter_params) == tuple(map(f32, params))
    orc = oracle_py.Oracle(out.contents.desc)  # (the scene is created: the table is built)
    orc.close()
    lib.shm_pbrt_free(out)


def test_loader_rejects_unknown_filters(lib):
    rc, out = parse(lib, '\nPixelFilter "bogus"\n' + SCENE)
    assert rc == -2 and not out  # SHM_ERR_UNSUPPORTED
    msg = lib.shm_last_error().decode()
    assert all(n in msg for n in KIND) and '"bogus"' in msg, msg


@pytest.mark.parametrize("line, needle", [
    ('PixelFilter "gaussian" "float sigma" 0', "sigma"), ('PixelFilter "gaussian" "float sigma" -1', "sigma"), ('PixelFilter "sinc" "float tau" 0', "tau"),
    ('PixelFilter "mitchell" "float xradius" 0', "radius"), ('PixelFilter "triangle" "float yradius" -2', "radius"), ('PixelFilter "box" "float xradius" 0', "radius"),
    ('PixelFilter "gaussian" "float xradius" 0.02', "cells"), ('PixelFilter "sinc" "float yradius" 9', "cells"), ('PixelFilter "mitchell" "float xradius" 1e30', "cells"),
])
def test_bad_filter_values_fail_at_scene_creation(lib, line, needle):
    rc, out = parse(lib, line + "\n" + SCENE)
    assert rc == 0, lib.shm_last_error()
    with pytest.raises(RuntimeError, match=needle):
        oracle_py.Oracle(out.contents.desc)
    lib.shm_pbrt_free(out)


def test_example_scene_with_a_gaussian_filter_loads(lib):
    out = C.POINTER(abi.ShmPbrtScene)()
    path = ROOT / "examples" / "scenes" / "gaussian_filter.pbrt"
    abi.check(lib, lib.shm_scene_load_pbrt(str(path).encode(), C.byref(out)), "shm_scene_load_pbrt")
    f = out.contents.desc.film
    assert f.filter == abi.SHM_FILTER_GAUSSIAN and tuple(f.filter_radius) == (1.5, 1.5) and f.filter_params[0] == 0.5
    orc = oracle_py.Oracle(out.contents.desc)
    film, _ = orc.render(out.contents.params, n_threads=os.cpu_count() or 1)
    orc.close()
    lib.shm_pbrt_free(out)
    assert (film["weight_sum"] > 0).all() and (film["rgb_sum"] > 0).any()


# ---- the ABI ----
def test_set_film_arguments(lib):
    b = SceneBuilder()
    b.set_film(8, 8)
    assert b.film.filter == abi.SHM_FILTER_BOX == 0 and tuple(b.film.filter_radius) == (0.5, 0.5)
    b.set_film(8, 8, filter="mitchell", filter_params=(0.5, 0.25), filter_radius=(2.0, 1.0))
    assert b.film.filter == abi.SHM_FILTER_MITCHELL and tuple(b.film.filter_params) == (0.5, 0.25) and tuple(b.film.filter_radius) == (2.0, 1.0)
    b.set_film(8, 8, filter="sinc")
    assert b.film.filter == abi.SHM_FILTER_SINC and tuple(b.film.filter_radius) == (4.0, 4.0) and b.film.filter_params[0] == 3.0
    with pytest.raises(ValueError):
        b.set_film(8, 8, filter="lanczos")
    with pytest.raises(ValueError):
        b.set_film(8, 8, filter="gaussian", filter_params=(0.5, 0.5))


def test_header_agrees_with_abi_py_on_the_filter_fields(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "shimmer_hip.h"\nint main(void) {\n'
           '  printf("%d %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", SHM_ABI_VERSION, sizeof(ShmFilm), offsetof(ShmFilm, filter_radius), offsetof(ShmFilm, filter),'
           ' offsetof(ShmFilm, filter_params), offsetof(ShmFilm, sensor_r_bar), offsetof(ShmSceneDesc, film),'
           ' SHM_FILTER_BOX, SHM_FILTER_GAUSSIAN, SHM_FILTER_MITCHELL, SHM_FILTER_SINC, SHM_FILTER_TRIANGLE);\n  return 0;\n}\n')
    (tmp_path / "p.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "p.c"), "-o", str(tmp_path / "p")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "p")], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [abi.SHM_ABI_VERSION, C.sizeof(abi.ShmFilm), abi.ShmFilm.filter_radius.offset, abi.ShmFilm.filter.offset, abi.ShmFilm.filter_params.offset,
                   abi.ShmFilm.sensor_r_bar.offset, abi.ShmSceneDesc.film.offset,
                   abi.SHM_FILTER_BOX, abi.SHM_FILTER_GAUSSIAN, abi.SHM_FILTER_MITCHELL, abi.SHM_FILTER_SINC, abi.SHM_FILTER_TRIANGLE]
    assert got[7:] == [0, 1, 2, 3, 4]


def test_a_zeroed_filter_field_is_the_box_filter(lib):
    sc = scenes.cornell_box(lib, 10, 8)
    assert sc.desc.film.filter == 0 and tuple(sc.desc.film.filter_params) == (0.0, 0.0)
    p = render.make_params(seed=5, spp=3, max_depth=3)
    films = []
    for s in (sc, scenes.cornell_box(lib, 10, 8, film=dict(filter="box"))):
        orc = oracle_py.Oracle(s.desc)
        films.append(orc.render(p, n_threads=2)[0])
        orc.close()
    assert np.array_equal(films[0], films[1]) and (films[0]["weight_sum"] == 3).all()
    sc.desc.film.filter = 5
    with pytest.raises(RuntimeError, match="pixel filter"):
        oracle_py.Oracle(sc.desc)
