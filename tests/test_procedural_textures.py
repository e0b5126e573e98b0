"""PBRT-v4's procedural float textures (shm/texture.h: Perlin noise, FBm, turbulence, the filtered checkerboard in two and three dimensions, dots, bilerp) on the CPU, through the
oracle's existing entry points (orc_fn_float_texture_evaluate, orc_fn_spectrum_texture_evaluate) and the PBRT front end: against an independent float64 numpy restatement
of PBRT-v4's published formulas, exact properties of the construction, one rendered check, the loader against the builder, flatten_scene's rejections, the ABI, and the
films of two existing textured scenes, which must not have moved.

U = 2^-24 is float32's unit roundoff: one rounded operation on a value of magnitude m errs by at most U m. Every tolerance below is a count of such operations times the
magnitude of what they act on, worked out where it is used; the float64 side is taken as exact.

One class is absent from the loader cases: `Texture .. "float" "wrinkled"`. tests/test_pbrt_loader.py pins that directive to the answer "Texture wrinkled unknown", so the
front end keeps giving it; SHM_FLOATTEX_WRINKLED is covered here through the ABI and the builder."""
import ctypes as C
import hashlib
import json
import math
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_py
from oracle_py import fa
from shimmer_amd import abi, render, scene as scn, scenes

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests" / "golden"))
f32 = np.float32
U = 2.0 ** -24
PERM_SHA256 = "3682c3d0020436c45462995a4f64438c144bbfeba725b00de5906ab322b6b915"

# ---- the compiled probe: the table, the version, the struct sizes and the enum values as the C++ headers have them -------------------------------------------
PROBE_SRC = r'''
#include <stdio.h>
#include "shm/path.h"
int main() {
    for (int i = 0; i < 256; ++i) printf("%d ", (int)shm::NOISE_PERM[i]);
    printf("\n%d %zu %zu %zu\n", SHM_ABI_VERSION, sizeof(ShmFloatTexture), sizeof(ShmImageTexture), sizeof(ShmSceneDesc));
    printf("%d %d %d %d %d %d %d\n", SHM_TEXMAP_POINT3D, SHM_FLOATTEX_CHECKERBOARD, SHM_FLOATTEX_DOTS, SHM_FLOATTEX_FBM, SHM_FLOATTEX_WRINKLED, SHM_FLOATTEX_WINDY, SHM_FLOATTEX_BILERP);
    return 0;
}
'''


@pytest.fixture(scope="module")
def header_probe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("proctex")
    (d / "p.cpp").write_text(PROBE_SRC)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", str(ROOT / "shimmer_amd" / "csrc"), "-I", str(ROOT / "include"), str(d / "p.cpp"), "-o", str(d / "p")], check=True)
    lines = subprocess.run([str(d / "p")], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    return [list(map(int, l.split())) for l in lines]


def test_the_permutation_table(header_probe):
    perm = header_probe[0]
    assert sorted(perm) == list(range(256))
    assert hashlib.sha256(bytes(perm)).hexdigest() == PERM_SHA256
    assert perm[:16] == [151, 160, 137, 91, 90, 15, 131, 13, 201, 95, 96, 53, 194, 233, 7, 225] and perm[-6:] == [78, 66, 215, 61, 156, 180]


def test_abi_version_sizes_and_enum_values(header_probe):
    """The version stays 10 and no struct changes size (48, 136 and 640 bytes are what the parent's header gives); the new enum values agree with abi.py."""
    assert header_probe[1] == [10, 48, 136, 640]
    assert abi.SHM_ABI_VERSION == 10 and (C.sizeof(abi.ShmFloatTexture), C.sizeof(abi.ShmImageTexture), C.sizeof(abi.ShmSceneDesc)) == (48, 136, 640)
    assert header_probe[2] == [abi.SHM_TEXMAP_POINT3D, abi.SHM_FLOATTEX_CHECKERBOARD, abi.SHM_FLOATTEX_DOTS, abi.SHM_FLOATTEX_FBM, abi.SHM_FLOATTEX_WRINKLED,
                               abi.SHM_FLOATTEX_WINDY, abi.SHM_FLOATTEX_BILERP] == [4, 5, 6, 7, 8, 9, 10]
    assert abi.ShmSceneDesc._fields_[-1][0] == "spot_lights"


# ---- the float64 restatement of PBRT-v4's formulas ---------------------------------------------------------------------------------------------------------
def perm_table(header_probe_rows=None):
    """Ken Perlin's permutation from its published construction is not derivable; the restatement reads the table the way a reader of PBRT-v4 would: as data. It is pinned
    by its sha256 in test_the_permutation_table; here it is parsed out of the header text (not through the code under test)."""
    text = (ROOT / "shimmer_amd" / "csrc" / "shm" / "texture.h").read_text()
    body = text[text.index("NOISE_PERM[256] = {") + len("NOISE_PERM[256] = {"):]
    body = body[:body.index("}")]
    p = [int(v) for v in body.replace("\n", " ").split(",")]
    assert len(p) == 256 and hashlib.sha256(bytes(p)).hexdigest() == PERM_SHA256
    return p


PERM = perm_table()


def grad64(x, y, z, dx, dy, dz):
    h = PERM[(PERM[(PERM[x & 255] + y) & 255] + z) & 255] & 15
    u = dx if (h < 8 or h == 12 or h == 13) else dy
    v = dy if (h < 4 or h == 12 or h == 13) else dz
    return (-u if h & 1 else u) + (-v if h & 2 else v)


def noise_weight64(t):
    return 6 * t ** 5 - 15 * t ** 4 + 10 * t ** 3


def lerp64(t, a, b):
    return (1 - t) * a + t * b


def noise64(x, y, z):
    """Noise at a point whose coordinates are float32 values (held in float64)."""
    ix, iy, iz = math.floor(x), math.floor(y), math.floor(z)
    dx, dy, dz = x - ix, y - iy, z - iz
    ix, iy, iz = ix & 255, iy & 255, iz & 255
    w = {(a, b, c): grad64(ix + a, iy + b, iz + c, dx - a, dy - b, dz - c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    wx, wy, wz = noise_weight64(dx), noise_weight64(dy), noise_weight64(dz)
    x00, x10, x01, x11 = lerp64(wx, w[0, 0, 0], w[1, 0, 0]), lerp64(wx, w[0, 1, 0], w[1, 1, 0]), lerp64(wx, w[0, 0, 1], w[1, 0, 1]), lerp64(wx, w[0, 1, 1], w[1, 1, 1])
    return lerp64(wz, lerp64(wy, x00, x10), lerp64(wy, x01, x11))


# One float32 Noise against noise64 at the same float32 point. The offsets d are exact (x - floor x), d - 1 rounds once; a corner's Grad is a sum of two such values, each at
# most 1 in magnitude: error <= 4 U. NoiseWeight: the terms 6 t^5, 15 t^4 and 10 t^3 take 5, 4 and 3 rounded operations and reach 6, 15 and 10: <= (30 + 60 + 30) U, and the two
# sums of magnitudes <= 9 and <= 1 add 10 U: 130 U. Lerp(w, a, b) with |a|, |b| <= 2: the weight's error moves it by |b - a| 130 U <= 520 U, its own five operations by 8 U, and
# it passes its inputs' error on: 4 U -> 532 U -> 1060 U -> 1588 U over the three levels.
NOISE_TOL = 1600 * U


def smooth_step64(x, a, b):
    t = min(max((x - a) / (b - a), 0.0), 1.0)
    return t * t * (3 - 2 * t)


def octaves64(dpdx, dpdy, max_octaves):
    len2 = max(float(np.dot(dpdx, dpdx)), float(np.dot(dpdy, dpdy)))
    n = math.inf if len2 == 0 else -1 - math.log2(len2) / 2
    return min(max(n, 0.0), float(max_octaves))


def scaled32(lam, p):
    """lambda * p as the statement prescribes it: one float32 product per component (the ARGUMENT of Noise is a float32 point on both sides; Noise, the weights and the sums are float64 here)."""
    return [float(f32(lam) * f32(c)) for c in p]


def fbm64(p, dpdx, dpdy, omega, max_octaves, turbulence=False):
    """Returns the value and S, the sum of the octave weights |o| it added up (the magnitude of the quantities summed)."""
    n = octaves64(dpdx, dpdy, max_octaves)
    n_int = int(math.floor(n))
    total, lam, o, S = 0.0, f32(1.0), 1.0, 0.0
    for _ in range(n_int):
        v = noise64(*scaled32(lam, p))
        total += o * (abs(v) if turbulence else v)
        S += abs(o)
        lam = f32(lam * f32(1.99))
        o *= omega
    v = noise64(*scaled32(lam, p))
    ss = smooth_step64(n - n_int, 0.3, 0.7)
    total += o * lerp64(ss, 0.2, abs(v)) if turbulence else o * ss * v
    S += abs(o)
    if turbulence:
        for _ in range(n_int, max_octaves):
            total += o * 0.2
            S += abs(o)
            o *= omega
    return total, S, n


def checker_d64(x):
    y = x / 2 - math.floor(x / 2) - 0.5
    return x / 2 + y * (1 - 2 * abs(y))


def checker_bf64(x, r):
    if math.floor(x - r) == math.floor(x + r):
        return 1 - 2 * (int(math.floor(x)) & 1)
    return (checker_d64(x + r) - 2 * checker_d64(x) + checker_d64(x - r)) / (r * r)


def tent_integral64(x, r):
    """The mean of the +-1 square wave c(x) = 1 - 2 (floor(x) & 1) over the footprint [x - r, x + r] under the weight the closed form implements: d'' = c, so its second
    difference over r is c convolved with the box of width r TWICE, i.e. with the tent (r - |u|) / r^2. A quadrature that is exact for a piecewise constant integrand:
    the window is split at the integers and at x, and the tent is integrated in closed form on every piece."""
    F = lambda u: r * u - u * abs(u) / 2  # noqa: E731 (an antiderivative of r - |u|)
    cuts = sorted({x - r, x + r, x, *[float(k) for k in range(math.ceil(x - r), math.floor(x + r) + 1)]})
    acc = 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        acc += (1 - 2 * (int(math.floor((a + b) / 2)) & 1)) * (F(b - x) - F(a - x))
    return acc / (r * r)


def bf_tol(x, r):
    """checker_bf in float32 against float64. d(x) = x/2 + y (1 - 2|y|): the argument x +- r rounds once (U (|x| + r), passed on with |d'| <= 1), d's own operations add about
    U (|x|/2 + 1): each of the four d values (2 d(x) counts twice) errs by <= U (1.5 (|x| + r) + 1), the two subtractions of values near |x|/2 by U |x| each; all of it divided by r^2."""
    return U * ((8 * (abs(x) + r) + 4) / (r * r) + 4)


def near_integer(v, bound):
    return abs(v - round(v)) <= bound


# ---- the leaf scene: one node per kind, evaluated through the oracle at explicit contexts -------------------------------------------------------------------
SU, SV, DU, DV = 3.0, 2.0, 0.25, -0.5
M3 = np.array([[1.5, 0.25, 0.0, 0.25], [0.0, 2.0, -0.5, -0.125], [0.25, 0.0, 1.25, 0.5], [0, 0, 0, 1]], np.float32)  # texture_from_render of the 3-D mapping: exact in float32


def leaf_scene(lib):
    """One node per kind and form (also what tests/test_gpu_procedural_textures.py hands to the device probe): name -> node index, plus the builder and the description."""
    b = scenes.cornell_box(lib, 8, 8).builder
    uv = b.add_texture_mapping("uv", su=SU, sv=SV, du=DU, dv=DV)
    p3 = b.add_texture_mapping("point3d", texture_from_render=M3)
    ident = b.add_texture_mapping("point3d")
    n = dict(uv=uv, p3=p3, ident=ident)
    n["noise"] = b.ftex_fbm(1, 0.5, ident)  # with zero differentials: n = 1, one full octave, and the partial one is o * SmoothStep(0) * Noise = 0: Noise(p) itself
    n["fbm"] = b.ftex_fbm(8, 0.5, p3)
    n["fbm7"] = b.ftex_fbm(5, 0.7, ident)
    n["wrinkled"] = b.ftex_wrinkled(8, 0.5, p3)
    n["wrinkled6"] = b.ftex_wrinkled(6, 0.6, ident)
    n["windy"] = b.ftex_windy(p3)
    n["checker2"] = b.ftex_checkerboard(None, None, uv)
    n["checker3"] = b.ftex_checkerboard(None, None, p3)
    n["checker2_children"] = b.ftex_checkerboard(0.0, 1.0, uv)
    n["checker_values"] = b.ftex_checkerboard(0.25, b.ftex_scaled(0.5, 3.0), uv)
    n["dots"] = b.ftex_dots(None, None, uv)
    n["dots_values"] = b.ftex_dots(0.125, 0.75, uv)
    n["bilerp"] = b.ftex_bilerp(0.1, 0.9, -0.4, 2.0, uv)
    tex1, tex2 = b.spectrum_piecewise([400.0, 700.0], [0.2, 0.8]), b.spectrum_constant(0.35)
    n["stex_checker"], n["tex1"], n["tex2"] = b.stex_checkerboard(tex1, tex2, uv), tex1, tex2
    desc, _ = b.build(lib)
    n["builder"], n["desc"] = b, desc
    return n


LEAF_NODES = ("noise", "fbm", "fbm7", "wrinkled", "wrinkled6", "windy", "checker2", "checker3", "checker2_children", "checker_values", "dots", "dots_values", "bilerp")


def leaf_contexts(seed=31, n=240):
    """Contexts of every family the tests below use: lattice points, zero differentials, footprints from a thousandth of a cell to many cells."""
    rng = np.random.default_rng(seed)
    out = [ctx_of(p=(ix, iy, iz)) for ix in (-1, 0, 3) for iy in (0, 255, 256) for iz in (-2, 7)]
    for k in range(n):
        size = 2.0 ** rng.uniform(-11, 5)
        zero = k % 6 == 0
        out.append(ctx_of(p=rng.uniform(-6, 6, 3), dpdx=(0, 0, 0) if zero else rng.normal(size=3) * size, dpdy=(0, 0, 0) if zero else rng.normal(size=3) * size,
                          uv=rng.uniform(-4, 4, 2), duv=(0, 0, 0, 0) if zero else rng.normal(size=4) * size))
    return out


@pytest.fixture(scope="module")
def leaves(lib):
    n = leaf_scene(lib)
    o = oracle_py.Oracle(n["desc"])
    n["ev"] = lambda node, ctx: float(o.lib.orc_fn_float_texture_evaluate(o.handle, node, fa(*ctx)))
    n["oracle"] = o
    yield n
    o.close()


def test_every_leaf_is_finite_over_the_shared_contexts(leaves):
    """The contexts the device probe replays (tests/test_gpu_procedural_textures.py): every node gives a finite value at each, the noise kinds within their octave sums."""
    for name in LEAF_NODES:
        vals = np.array([leaves["ev"](leaves[name], c) for c in leaf_contexts()])
        assert np.isfinite(vals).all(), name
        if name in ("checker2", "checker3", "checker2_children", "dots"):
            assert vals.min() >= -1e-3 and vals.max() <= 1 + 1e-3 and len(set(vals.tolist())) > 2 - (name == "dots"), name


def ctx_of(p=(0, 0, 0), dpdx=(0, 0, 0), dpdy=(0, 0, 0), uv=(0, 0), duv=(0, 0, 0, 0)):
    """18 float32 values: p, dpdx, dpdy, n, uv, dudx, dudy, dvdx, dvdy"""
    return [float(f32(v)) for v in (*p, *dpdx, *dpdy, 0.0, 0.0, 1.0, *uv, *duv)]


def map3(ctx):
    """The 3-D mapping in float64 from the float32 context. The float32 side rounds each of the <= 7 operations of a row: the mapped point errs by <= 4 U (|row| . |p| + |t|)."""
    m = M3.astype(np.float64)
    return m[:3, :3] @ np.array(ctx[0:3]) + m[:3, 3], m[:3, :3] @ np.array(ctx[3:6]), m[:3, :3] @ np.array(ctx[6:9])


def test_noise_is_zero_on_the_lattice_and_matches_float64(leaves):
    ev, node = leaves["ev"], leaves["noise"]
    for ix in range(-3, 4):
        for iy in (-2, 0, 1, 255, 256):
            for iz in (-1, 0, 7):
                assert ev(node, ctx_of(p=(ix, iy, iz))) == 0.0
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(400):
        ctx = ctx_of(p=rng.uniform(-20, 20, 3))
        got, want = ev(node, ctx), noise64(*ctx[0:3])
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= NOISE_TOL, (ctx[0:3], got, want)
    assert abs(ev(node, ctx_of(p=(0.5, 0.5, 0.5)))) <= 1.0 and worst > 0.0  # (float32 and float64 are not the same arithmetic: the comparison is not vacuous)


@pytest.mark.parametrize("name, omega, octaves, turb, mapped", [("fbm", 0.5, 8, False, True), ("fbm7", 0.7, 5, False, False), ("wrinkled", 0.5, 8, True, True),
                                                                ("wrinkled6", 0.6, 6, True, False)])
def test_fbm_and_turbulence_match_float64(leaves, name, omega, octaves, turb, mapped):
    """The octave count n = clamp(-1 - log2(len2) / 2, 0, octaves) comes from a float32 log2 of a float32 len2 (5 operations: 3 U relative, i.e. 3 U / ln 2 < 5 U in log2, plus
    log2's own error, a few U of |log2| <= 24: 48 U), halved: n errs by <= 32 U. A point whose n lies within that of an integer (the floor) or of the clamp's ends is excluded.
    The sum: every octave is o times a Noise (1600 U), the partial one besides times a SmoothStep whose slope is <= 1.5 / 0.4, i.e. 120 U more for n's error; the running sum's
    own roundings are <= 2 U S. Under the 3-D mapping the point itself errs by <= 4 U (|row| . |p| + |t|) <= 40 U for |p| <= 4, scaled by lambda <= 1.99^8 = 246 in the last
    octave, where Noise's slope is <= 4 per axis over three axes: 40 U * 12 * sum(o lambda) — so the mapped nodes are probed with zero rotation error instead: at points p whose
    mapped image is exact in float32 (p on a grid of 1/64 with |p| <= 4: every product and sum of M3's rows is exact)."""
    ev, node = leaves["ev"], leaves[name]
    rng = np.random.default_rng(5 if turb else 3)
    n_cases, n_excluded = 300, 0
    for k in range(n_cases):
        p = np.round(rng.uniform(-4, 4, 3) * 64) / 64
        size = 2.0 ** rng.uniform(-11, 1)
        dpdx, dpdy = np.round(rng.normal(size=3) * size * 4096) / 4096, np.round(rng.normal(size=3) * size * 4096) / 4096
        if k % 10 == 0:
            dpdx, dpdy = np.zeros(3), np.zeros(3)  # zero differentials: log2(0), n = octaves
        ctx = ctx_of(p=p, dpdx=dpdx, dpdy=dpdy)
        tp, tdx, tdy = map3(ctx) if mapped else (np.array(ctx[0:3]), np.array(ctx[3:6]), np.array(ctx[6:9]))
        assert all(float(f32(v)) == v for v in tp)  # (the mapped point is exact in float32)
        want, S, n = fbm64(tp, [float(f32(v)) for v in tdx], [float(f32(v)) for v in tdy], omega, octaves, turb)
        if 0.0 < n < octaves and near_integer(n, 32 * U):
            n_excluded += 1
            continue
        got = ev(node, ctx)
        assert abs(got - want) <= (1600 + 120 + 2) * U * S, (k, got, want, n)
    assert n_excluded <= 0.02 * n_cases


def test_fbm_vanishes_and_turbulence_is_its_constant_for_a_wide_footprint(leaves):
    """len2 >= 0.25: n = 0, SmoothStep(0) = 0: FBm is exactly 0; Turbulence is Lerp(0, 0.2, |Noise|) = 0.2 and then 0.2 o for every octave: 0.2 (1 + omega + ...) in float32 order."""
    ev = leaves["ev"]
    rng = np.random.default_rng(2)
    for _ in range(50):
        p = rng.uniform(-5, 5, 3)
        ctx = ctx_of(p=p, dpdx=(0.5, 0, 0), dpdy=(0, 0.75, 0))
        assert ev(leaves["fbm7"], ctx) == 0.0
        # the partial octave: sum = 1 * Lerp(0, 0.2, |Noise|) = (1 - 0) * 0.2 + 0 * |Noise| = 0.2 exactly; then for i in 0 .. 5: sum += o * 0.2, o *= omega, from o = 1
        total, o = f32(f32(1.0) * f32(0.2)), f32(1.0)
        for i in range(6):
            total = f32(total + f32(o * f32(0.2)))
            o = f32(o * f32(0.6))
        got = ev(leaves["wrinkled6"], ctx)
        assert f32(got) == total, (got, total)


def test_windy_matches_float64(leaves):
    """|FBm(0.1 p, .., 0.5, 3)| * FBm(p, .., 0.5, 6): each factor within its own bound (previous test), the factors at most S1 and S2 in magnitude: the product errs by
    <= S1 tol2 + S2 tol1 (+ U S1 S2 for the product and the scaling by 0.1, which the restatement does in float32 as the statement has it)."""
    ev, node = leaves["ev"], leaves["windy"]
    rng = np.random.default_rng(9)
    n_excluded = 0
    for k in range(200):
        p = np.round(rng.uniform(-4, 4, 3) * 64) / 64
        size = 2.0 ** rng.uniform(-10, 0)
        dpdx, dpdy = np.round(rng.normal(size=3) * size * 4096) / 4096, np.round(rng.normal(size=3) * size * 4096) / 4096
        ctx = ctx_of(p=p, dpdx=dpdx, dpdy=dpdy)
        tp, tdx, tdy = map3(ctx)
        s32 = lambda v: [float(f32(0.1) * f32(c)) for c in v]  # noqa: E731
        w1, S1, n1 = fbm64(s32(tp), s32(tdx), s32(tdy), 0.5, 3)
        w2, S2, n2 = fbm64(tp, [float(f32(v)) for v in tdx], [float(f32(v)) for v in tdy], 0.5, 6)
        if (0.0 < n1 < 3 and near_integer(n1, 32 * U)) or (0.0 < n2 < 6 and near_integer(n2, 32 * U)):
            n_excluded += 1
            continue
        tol = 1722 * U * (S1 * S2 + S2 * S1) + U * S1 * S2
        assert abs(ev(node, ctx) - abs(w1) * w2) <= tol, k
    assert n_excluded <= 4


def st_of(ctx):
    """The uv mapping in float64 from the float32 context; s = su u + du takes two float32 operations: s errs by <= 2 U (|su u| + |du|)."""
    s, t = SU * ctx[12] + DU, SV * ctx[13] + DV
    return s, t, 1.5 * max(abs(SU * ctx[14]), abs(SU * ctx[15])), 1.5 * max(abs(SV * ctx[16]), abs(SV * ctx[17]))


def test_checkerboard_weight_point_sampled_is_exact(leaves):
    ev = leaves["ev"]
    rng = np.random.default_rng(21)
    for _ in range(300):
        uv = rng.uniform(-4, 4, 2)
        ctx = ctx_of(uv=uv)
        s, t, _, _ = st_of(ctx)
        if near_integer(s, 8 * U * 16) or near_integer(t, 8 * U * 16):
            continue
        assert ev(leaves["checker2"], ctx) == float((math.floor(s) + math.floor(t)) & 1)
        p = rng.uniform(-3, 3, 3)
        ctx3 = ctx_of(p=p)
        tp, _, _ = map3(ctx3)
        if any(near_integer(v, 64 * U) for v in tp):
            continue
        assert ev(leaves["checker3"], ctx3) == float((math.floor(tp[0]) + math.floor(tp[1]) + math.floor(tp[2])) & 1)


def test_checkerboard_weight_filtered_matches_float64_and_the_box_integral(leaves):
    """w = 0.5 - bf(s) bf(t) / 2 with |bf| <= 1: w errs by <= (tol_s + tol_t) / 2 + 2 U, where tol is bf_tol plus the mapping's share: s errs by 2 U (|s| + |du|) and
    bf's slope in s is <= 2 / r (the wave's mean over a window of width 2 r moves by at most 2 per 2 r... per unit 1 / r, doubled for safety); r's own 2 U r moves bf by <= 4 U.
    Points where the float32 and the float64 side may choose different branches of bf (x +- r within its rounding of an integer) are excluded.
    The same bound holds against a numerical integral of the square wave over the footprint [x - r, x + r] (tent_integral64). NOTE: the weight under that integral is the box of
    width r applied twice (a tent), not one box of width 2 r: the closed form that PBRT-v4 uses is a SECOND difference of the wave's second antiderivative. Against a single box
    of width 2 r the closed form differs by up to a few 1e-3 (measured: 2.4e-3 at s = -2.864, r = 3.926, where the single box gives bf = 0.01879), far outside any rounding bound."""
    ev = leaves["ev"]
    rng = np.random.default_rng(8)
    n_cases, n_excluded = 400, 0
    for k in range(n_cases):
        uv = rng.uniform(-3, 3, 2)
        duv = rng.choice([-1.0, 1.0], 4) * rng.uniform(0.02, 1.0, 4)  # half-widths from 0.06 cells (1 / r^2 <= 280) to 4.5 cells
        ctx = ctx_of(uv=uv, duv=duv)
        s, t, rs, rt = st_of(ctx)
        assert rs >= 0.05 and rt >= 0.05
        if any(near_integer(v, 4 * U * (abs(v) + 1)) for v in (s - rs, s + rs, t - rt, t + rt)):
            n_excluded += 1
            continue
        tol = sum(bf_tol(x, r) + 2 * U * (abs(x) + 1) * 2 / r + 4 * U for x, r in ((s, rs), (t, rt))) / 2 + 2 * U
        got = ev(leaves["checker2"], ctx)
        assert abs(got - (0.5 - checker_bf64(s, rs) * checker_bf64(t, rt) / 2)) <= tol, k
        assert abs(got - (0.5 - tent_integral64(s, rs) * tent_integral64(t, rt) / 2)) <= tol, k
    # three dimensions, through the 3-D mapping (points and differentials on grids that the mapping keeps exact)
    n_checked = 0
    for k in range(250):
        p = np.round(rng.uniform(-3, 3, 3) * 64) / 64
        dpdx, dpdy = np.round(rng.normal(size=3) * 0.3 * 256) / 256, np.round(rng.normal(size=3) * 0.3 * 256) / 256
        ctx = ctx_of(p=p, dpdx=dpdx, dpdy=dpdy)
        tp, tdx, tdy = map3(ctx)
        r = [1.5 * max(abs(tdx[i]), abs(tdy[i])) for i in range(3)]
        if min(r) < 0.05:  # (outside the range of half-widths probed: 1 / r^2 grows without bound)
            continue
        if any(near_integer(v, 4 * U * (abs(v) + 1)) for i in range(3) for v in (tp[i] - r[i], tp[i] + r[i])):
            n_excluded += 1
            continue
        n_checked += 1
        tol = sum(bf_tol(tp[i], r[i]) for i in range(3)) / 2 + 4 * U
        want = 0.5 - checker_bf64(tp[0], r[0]) * checker_bf64(tp[1], r[1]) * checker_bf64(tp[2], r[2]) / 2
        assert abs(ev(leaves["checker3"], ctx) - want) <= tol, k
    assert n_checked >= 150 and n_excluded <= 0.02 * (n_cases + 250)


def test_checkerboard_weight_is_a_half_under_a_wide_footprint(leaves):
    """Over a window of half-width r the cells cancel in pairs; what is left is at most one cell: |bf| <= 1 / (2 r), so |w - 0.5| <= 1 / (8 rs rt), plus bf's bound."""
    ev = leaves["ev"]
    rng = np.random.default_rng(4)
    for _ in range(100):
        uv = rng.uniform(-3, 3, 2)
        ctx = ctx_of(uv=uv, duv=(20.0, 3.0, -1.0, 25.0))
        s, t, rs, rt = st_of(ctx)
        assert rs > 50 and rt > 50
        assert abs(ev(leaves["checker2"], ctx) - 0.5) <= 1 / (8 * rs * rt) + (bf_tol(s, rs) + bf_tol(t, rt)) / 2 + 2 * U


def test_weight_form_equals_the_child_form_bit_for_bit(leaves):
    ev = leaves["ev"]
    rng = np.random.default_rng(6)
    for k in range(300):
        ctx = ctx_of(uv=rng.uniform(-3, 3, 2), duv=(rng.normal(size=4) * 0.2 if k % 2 else (0, 0, 0, 0)))
        w = ev(leaves["checker2"], ctx)
        assert f32(ev(leaves["checker2_children"], ctx)).tobytes() == f32(w).tobytes()
        # the child form on other operands: (1 - w) * t1 + w * t2 with the lazy selects, in float32
        w32, t1, t2 = f32(w), f32(0.25), f32(f32(0.5) * f32(3.0))
        want = f32(f32(f32(1.0) - w32) * (t1 if w32 != 1 else f32(0.0))) + f32(w32 * (t2 if w32 != 0 else f32(0.0)))
        assert f32(ev(leaves["checker_values"], ctx)).tobytes() == f32(want).tobytes()


def test_spectrum_checkerboard_is_the_mix_over_the_weight_form_bit_for_bit(leaves):
    o, lams = leaves["oracle"], (452.0, 533.0, 601.5, 688.25)
    out = (C.c_float * 4)()

    def sev(sp, ctx):
        o.lib.orc_fn_spectrum_texture_evaluate(o.handle, C.byref(sp), fa(*ctx), fa(*lams), out)
        return np.array(out[:], np.float32)
    assert leaves["builder"].spectrum_textures[leaves["stex_checker"].offset].kind == abi.SHM_SPECTEX_MIX
    rng = np.random.default_rng(12)
    for k in range(200):
        ctx = ctx_of(uv=rng.uniform(-3, 3, 2), duv=(rng.normal(size=4) * 0.2 if k % 2 else (0, 0, 0, 0)))
        w = f32(leaves["ev"](leaves["checker2"], ctx))
        t1 = sev(leaves["tex1"], ctx) if w != 1 else np.zeros(4, np.float32)
        t2 = sev(leaves["tex2"], ctx) if w != 0 else np.zeros(4, np.float32)
        want = (t1 * f32(f32(1.0) - w)).astype(np.float32) + (t2 * w).astype(np.float32)
        assert sev(leaves["stex_checker"], ctx).tobytes() == want.astype(np.float32).tobytes(), k


def dots64(s, t):
    """-> (inside, margin): margin is how far the nearest of the three decisions (floor, Noise > 0, the rim) is from flipping, each in units of its own float32 bound"""
    sc, tc = math.floor(s + 0.5), math.floor(t + 0.5)
    margin = min(abs(s + 0.5 - round(s + 0.5)), abs(t + 0.5 - round(t + 0.5))) / (8 * U * (abs(s) + abs(t) + 1))
    # at a cell's centre every offset is 1/2, every NoiseWeight(1/2) = 1/2 and every gradient product a multiple of 1/2: each float32 operation is exact, the value is a multiple
    # of 1/8 (often 0) and `Noise > 0` is decided alike on both sides: no margin
    n0 = noise64(float(f32(sc + 0.5)), float(f32(tc + 0.5)), 0.5)
    assert n0 * 8 == round(n0 * 8)
    if n0 <= 0:
        return False, margin
    radius, max_shift = float(f32(0.35)), float(f32(0.5) - f32(0.35))
    cs = sc + max_shift * noise64(float(f32(sc) + f32(1.5)), float(f32(tc) + f32(2.8)), 0.5)  # (the float32 sums of the statement: 2.8f and 9.8f are not exact)
    ct = tc + max_shift * noise64(float(f32(sc) + f32(4.5)), float(f32(tc) + f32(9.8)), 0.5)
    d2 = (s - cs) ** 2 + (t - ct) ** 2
    # the centre errs by 0.15 * 1600 U + 4 U (|cell| + 1), s and t by 2 U (|s| + 1): d2, of slope <= 2 * 0.7, by about 1.4 times their sum, plus its own 4 operations
    rim = 1.4 * (2 * 0.15 * 1600 * U + 8 * U * (abs(s) + abs(t) + 2)) + 4 * U
    return d2 < radius * radius, min(margin, abs(d2 - radius * radius) / rim)


def test_dots_and_bilerp_match_float64(leaves):
    ev = leaves["ev"]
    rng = np.random.default_rng(17)
    n_cases, n_excluded, n_inside = 400, 0, 0
    for k in range(n_cases):
        ctx = ctx_of(uv=rng.uniform(-4, 4, 2))
        s, t, _, _ = st_of(ctx)
        inside, margin = dots64(s, t)
        if margin <= 1.0:
            n_excluded += 1
        else:
            n_inside += inside
            assert ev(leaves["dots"], ctx) == (0.0 if inside else 1.0), k
            assert ev(leaves["dots_values"], ctx) == (0.125 if inside else 0.75), k
        # bilerp: four terms of three operations each on |v| <= 2 and weights <= (|s| + 1)(|t| + 1) =: W, three sums; s and t err by 2 U (|s| + 1): 8 U W sum|v| covers it
        v00, v01, v10, v11 = (float(f32(v)) for v in (0.1, 0.9, -0.4, 2.0))
        want = (1 - s) * (1 - t) * v00 + s * (1 - t) * v10 + (1 - s) * t * v01 + s * t * v11
        W = (abs(s) + 1) * (abs(t) + 1)
        assert abs(ev(leaves["bilerp"], ctx) - want) <= 8 * U * W * (0.1 + 0.9 + 0.4 + 2.0), k
    assert n_excluded <= 0.02 * n_cases and 20 < n_inside < 300


# ---- one rendered check -------------------------------------------------------------------------------------------------------------------------------------
def test_rendered_checkerboard_reflects_in_the_ratio_of_its_albedos(lib):
    """An orthographic camera straight at one diffuse quad under a uniform infinite light: the quad sees no other surface, so the radiance it sends back is albedo * L in the
    mean, whatever the path length. Its reflectance is a spectrum checkerboard of two constant albedos over s = 4 x + 0.5, t = 4 y + 0.5 (cells centred on the multiples of 1/4:
    the partition is the same whichever way the camera's axes point); a 16 x 16 film over the window [-1, 1]^2 puts the pixel centres, the odd multiples of 1/16, a quarter cell
    from the cell borders, and without pixel jitter every sample sits there. The texture is point-sampled (disable_texture_filtering): a pixel is half a cell wide, so the
    filtered weight of PBRT-v4's footprint of 1.5 pixels blends the two albedos at every pixel centre and the populations would stand in another ratio. Eight independent seeds give eight ratios of the two populations' mean radiance; their mean must
    lie within four of its own standard errors of the albedos' ratio."""
    a1, a2 = 0.2, 0.6
    b = scn.SceneBuilder()
    b.set_film(16, 16)
    rfw = b.set_camera_look_at(lib, (0, 0, -5), (0, 0, 0), (0, 1, 0), 0.0, orthographic=True)  # (down +z: the camera's axes are the world's)
    m = b.add_texture_mapping("planar", vs=(4.0, 0.0, 0.0), vt=(0.0, 4.0, 0.0), du=0.5, dv=0.5, texture_from_render=np.linalg.inv(np.asarray(rfw, np.float64).reshape(4, 4)))
    mat = b.material_diffuse(b.stex_checkerboard(a1, a2, m))
    p, vi = scenes._quad((-2, -2, 0), (-2, 2, 0), (2, 2, 0), (2, -2, 0))  # (its normal faces the camera, -z)
    b.add_mesh(scenes._to_render(p, rfw), vi, mat)
    b.light_uniform_infinite(scenes.blackbody_dense(6500.0), scale=1.0)
    desc, _ = b.build(lib)
    centres = (np.arange(16) + 0.5) / 8 - 1
    parity = (np.round(4 * centres)[None, :].astype(int) + np.round(4 * centres)[:, None].astype(int)) & 1  # w = 1: tex2 = a2
    assert parity.sum() == 128
    o = oracle_py.Oracle(desc)
    ratios = []
    try:
        for seed in range(8):
            film, _ = o.render(render.make_params(seed=100 + seed, spp=16, max_depth=5, disable_pixel_jitter=True, disable_texture_filtering=True), n_threads=8)
            y = film["rgb_sum"][..., 1] / film["weight_sum"]
            ratios.append(y[parity == 0].mean() / y[parity == 1].mean())
    finally:
        o.close()
    mean, se = float(np.mean(ratios)), float(np.std(ratios, ddof=1) / math.sqrt(len(ratios)))
    print("ratios", ratios, "mean", mean, "standard error", se)
    assert se > 0 and abs(mean - a1 / a2) <= 4 * se, (mean, se, a1 / a2)


# ---- the loader ---------------------------------------------------------------------------------------------------------------------------------------------
HEAD = 'LookAt 0 1 5  0 0 0  0 1 0\nCamera "perspective" "float fov" [ 40 ]\nFilm "rgb" "integer xresolution" [ 8 ] "integer yresolution" [ 8 ] "string filename" "x.pfm"\nWorldBegin\n'
TEXTURES = '''Texture "cb" "float" "checkerboard"
Texture "cb3" "float" "checkerboard" "integer dimension" 3 "float tex1" 0.25 "texture tex2" "cb"
Texture "d0" "float" "dots"
Texture "d" "float" "dots" "float uscale" 3 "float vscale" 5 "float udelta" 0.5 "float inside" 0.125 "texture outside" "cb"
Texture "f0" "float" "fbm"
Texture "f" "float" "fbm" "integer octaves" 5 "float roughness" 0.75
Texture "wi" "float" "windy"
Texture "bl0" "float" "bilerp"
Texture "bl" "float" "bilerp" "float v00" 0.125 "float v01" 0.25 "float v10" 0.375 "float v11" 0.5 "string mapping" "planar" "vector3 v1" [ 0 1 0 ] "vector3 v2" [ 0 0 1 ] "float udelta" 0.25
Texture "scb0" "spectrum" "checkerboard"
Texture "scb" "spectrum" "checkerboard" "spectrum tex1" [ 359 0.125 831 0.625 ] "float tex2" 0.75 "string mapping" "spherical"
Texture "sd" "spectrum" "dots" "float inside" 0.25
Material "diffuse" "texture reflectance" "scb"
Shape "sphere"
'''


def parse(lib, text):
    out = C.POINTER(abi.ShmPbrtScene)()
    rc = lib.shm_scene_parse_pbrt(text.encode(), None, C.byref(out))
    return rc, out, lib.shm_last_error().decode()


def table_bytes(desc):
    """The texture tables of a description, byte for byte; a spectrum node's leaf by what it evaluates (pool offsets are layout)."""
    ft = C.string_at(desc.float_textures, C.sizeof(abi.ShmFloatTexture) * desc.n_float_textures) if desc.n_float_textures else b""
    it = C.string_at(desc.image_textures, C.sizeof(abi.ShmImageTexture) * desc.n_image_textures) if desc.n_image_textures else b""
    data = np.ctypeslib.as_array(desc.spectrum_data, shape=(max(1, desc.n_spectrum_floats),))
    st = []
    for i in range(desc.n_spectrum_textures):
        t = desc.spectrum_textures[i]
        lf = t.leaf
        n = {abi.SHM_SPECTRUM_DENSE: lf.n, abi.SHM_SPECTRUM_PIECEWISE_LINEAR: 2 * lf.n}.get(lf.kind, 0)
        st.append((t.kind, t.a, t.b, t.f, list(t.dir), lf.kind, f32(lf.c).tobytes(), data[lf.offset:lf.offset + n].tobytes() if t.kind == abi.SHM_SPECTEX_LEAF else b""))
    return ft, it, st


def test_every_class_loads_and_equals_the_builder(lib):
    rc, out, err = parse(lib, HEAD + TEXTURES)
    assert rc == 0, err
    try:
        got = table_bytes(out.contents.desc)
        b = scn.SceneBuilder()
        b.set_film(8, 8)
        rfw = b.set_camera_look_at(lib, (0, 1, 5), (0, 0, 0), (0, 1, 0), 40.0)
        tfr = np.linalg.inv(np.asarray(rfw, np.float64).reshape(4, 4))
        cb = b.ftex_checkerboard()
        b.ftex_checkerboard(0.25, cb, b.add_texture_mapping("point3d", texture_from_render=tfr))
        b.ftex_dots()
        b.ftex_dots(0.125, cb, b.add_texture_mapping("uv", su=3.0, sv=5.0, du=0.5))
        b.ftex_fbm(mapping=b.add_texture_mapping("point3d", texture_from_render=tfr))  # (the front end's 3-D mapping is the CTM's)
        b.ftex_fbm(5, 0.75, b.add_texture_mapping("point3d", texture_from_render=tfr))
        b.ftex_windy(b.add_texture_mapping("point3d", texture_from_render=tfr))
        b.ftex_bilerp()
        b.ftex_bilerp(0.125, 0.25, 0.375, 0.5, b.add_texture_mapping("planar", vs=(0, 1, 0), vt=(0, 0, 1), du=0.25, texture_from_render=tfr))
        b.stex_checkerboard()
        b.stex_checkerboard(b.spectrum_piecewise([359.0, 831.0], [0.125, 0.625]), 0.75, b.add_texture_mapping("spherical", texture_from_render=tfr))
        b.stex_dots(0.25, 0.0)
        b.add_sphere(1.0, b.material_diffuse(0.5))
        desc, _ = b.build(lib)
        want = table_bytes(desc)
        assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
        ft = out.contents.desc.float_textures
        kinds = [ft[i].kind for i in range(out.contents.desc.n_float_textures)]
        for k in (abi.SHM_FLOATTEX_CHECKERBOARD, abi.SHM_FLOATTEX_DOTS, abi.SHM_FLOATTEX_FBM, abi.SHM_FLOATTEX_WINDY, abi.SHM_FLOATTEX_BILERP):
            assert k in kinds
        # the defaults: fbm has 8 octaves and roughness 0.5, bilerp (0, 1, 0, 1)
        f0 = next(ft[i] for i in range(len(kinds)) if kinds[i] == abi.SHM_FLOATTEX_FBM)
        assert (f0.pad[0], f0.value) == (8, 0.5)
        bl0 = next(ft[i] for i in range(len(kinds)) if kinds[i] == abi.SHM_FLOATTEX_BILERP)
        assert (bl0.value, list(bl0.dir)) == (0.0, [1.0, 0.0, 1.0])
        # ... and the scene is a valid one
        o = oracle_py.Oracle(out.contents.desc)
        film, _ = o.render(render.make_params(seed=1, spp=1, max_depth=3), n_threads=4)
        o.close()
        assert np.isfinite(film["rgb_sum"]).all()
    finally:
        lib.shm_pbrt_free(out)


@pytest.mark.parametrize("line, needle", [('Texture "m" "spectrum" "marble"', "marble"), ('Texture "m" "float" "marble"', "marble"), ('Texture "p" "spectrum" "ptex"', "ptex"),
                                          ('Texture "p" "float" "ptex"', "ptex"), ('Texture "b" "spectrum" "bilerp"', "bilerp"),
                                          ('Texture "c" "float" "checkerboard" "integer dimension" 4', "4 dimensional checkerboard"),
                                          ('Texture "c" "spectrum" "checkerboard" "integer dimension" 4', "4 dimensional checkerboard")])
def test_out_of_scope_classes_are_unsupported_with_file_and_line(lib, line, needle):
    rc, out, err = parse(lib, HEAD + line + '\nMaterial "diffuse" "texture reflectance" "c"\nShape "sphere"\n')
    assert rc == -2 and not out
    assert "<string>:5: " in err and needle in err and "unknown" not in err, err


def test_example_scene_loads_as_a_procedural_textured_scene(lib):
    out = C.POINTER(abi.ShmPbrtScene)()
    abi.check(lib, lib.shm_scene_load_pbrt(str(ROOT / "examples" / "scenes" / "checkerboard.pbrt").encode(), C.byref(out)), "checkerboard.pbrt")
    d = out.contents.desc
    kinds = {d.float_textures[i].kind for i in range(d.n_float_textures)}
    assert abi.SHM_FLOATTEX_CHECKERBOARD in kinds and d.n_image_levels == 0 and all(d.image_textures[i].n_levels == 0 for i in range(d.n_image_textures))
    lib.shm_pbrt_free(out)


# ---- flatten_scene's rejections -----------------------------------------------------------------------------------------------------------------------------
def rejected(lib, edit, match):
    b = scenes.cornell_box(lib, 8, 8).builder
    edit(b)
    with pytest.raises(RuntimeError, match=match):
        oracle_py.Oracle(b.build(lib)[0])


def test_flatten_scene_rejections(lib):
    def image_node_on_a_mapping_record(b):
        b._ftex(abi.SHM_FLOATTEX_IMAGE, image=b.add_texture_mapping("uv"))
    rejected(lib, image_node_on_a_mapping_record, "mapping-only record")

    def spectrum_leaf_on_a_mapping_record(b):
        sp = abi.ShmSpectrum()
        sp.kind, sp.offset = abi.SHM_SPECTRUM_IMAGE_TEXTURE, b.add_texture_mapping("uv")
        b.materials[0].a = sp
    rejected(lib, spectrum_leaf_on_a_mapping_record, "mapping-only record")

    def normal_map_on_a_mapping_record(b):
        b.materials[0].normal_map = b.add_texture_mapping("uv") + 1
    rejected(lib, normal_map_on_a_mapping_record, "normal map")
    rejected(lib, lambda b: b.ftex_dots(None, None, b.add_texture_mapping("point3d")), "dots / bilerp float texture: needs")
    rejected(lib, lambda b: b.ftex_bilerp(mapping=b.add_texture_mapping("point3d")), "dots / bilerp float texture: needs")
    for make in ("ftex_fbm", "ftex_wrinkled"):
        rejected(lib, lambda b, make=make: getattr(b, make)(8, 0.5, b.add_texture_mapping("uv")), "needs the 3-D point mapping")
    rejected(lib, lambda b: b.ftex_windy(b.add_texture_mapping("planar")), "needs the 3-D point mapping")
    rejected(lib, lambda b: b._ftex(abi.SHM_FLOATTEX_CHECKERBOARD, a=7, b=0, image=b.add_texture_mapping("uv")), "child index out of range")
    rejected(lib, lambda b: b._ftex(abi.SHM_FLOATTEX_DOTS, a=abi.SHM_FLOATTEX_WEIGHT_FORM, b=0, image=b.add_texture_mapping("uv")), "child index out of range")
    rejected(lib, lambda b: b._ftex(abi.SHM_FLOATTEX_FBM, image=99), "texture mapping index out of range")
    rejected(lib, lambda b: b.ftex_fbm(33, 0.5), "more than 32 octaves")
    rejected(lib, lambda b: b.ftex_checkerboard(mapping=b.add_image_texture(scenes.test_image(8, 1), color_space=False).offset), "must be a mapping-only record")
    rejected(lib, lambda b: b._ftex(11), "unknown float texture kind")

    def image_texture_with_the_point_mapping(b):
        b.add_image_texture(scenes.test_image(8, 1), color_space=False)
        b.textures[-1].mapping = abi.SHM_TEXMAP_POINT3D
    rejected(lib, image_texture_with_the_point_mapping, r"no \(s, t\)")


def test_a_scene_with_procedural_textures_alone_is_valid_and_textured(lib):
    """No image, no level, no texel: the description carries mapping-only records alone, and the render differs from the untextured scene's."""
    sc = scenes.procedural_cornell(lib, 24, 24)
    assert sc.desc.n_image_textures > 0 and sc.desc.n_image_levels == 0 and sc.desc.n_texel_floats == 0
    p = render.make_params(seed=3, spp=2, max_depth=4)
    films = []
    for s in (sc, scenes.procedural_cornell(lib, 24, 24, which="general"), scenes.procedural_cornell(lib, 24, 24, which="coated")):
        o = oracle_py.Oracle(s.desc)
        film, _ = o.render(p, n_threads=8)
        o.close()
        assert np.isfinite(film["rgb_sum"]).all() and film["rgb_sum"].sum() > 0
        films.append(film)
    rgb = render.film_to_rgb(films[0])
    floor = rgb[19:23, 4:20, 1]
    assert floor.std() > 0.02  # the checkerboard on the floor


# ---- unchanged behaviour ------------------------------------------------------------------------------------------------------------------------------------
def test_existing_textured_scenes_render_what_they_rendered(lib):
    import gen_procedural_textures_before as before
    golden = json.loads((ROOT / "tests" / "golden" / "procedural_textures_before.json").read_text())
    assert [c["scene"] for c in golden["films"]] == [c["scene"] for c in before.CASES]
    for case in golden["films"]:
        film, st = before.film_of(lib, case)
        assert hashlib.sha256(np.ascontiguousarray(film).tobytes()).hexdigest() == case["sha256"], case["scene"]
        assert [int(st[k]) for k in before.STATS] == case["stats"], case["scene"]
