"""PBRT-v4's ambient occlusion integrator (SHM_INTEGRATOR_AMBIENT_OCCLUSION; shm/ao.h) without a GPU: the CPU twin shm_ao_samples_host through the
chain of tests/ao_cases.py — twin camera rays, the oracle's closest hits, the twin, the oracle's any-hit trace, the film's rule —, its leaf values against a float64
re-evaluation, cases whose film is known exactly, its expectation against the oracle's path integrator, the ABI, the loader and the host mirror."""
import ctypes as C
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ao_cases as ao
import gbuffer_cases as gc
import oracle_py
from shimmer_amd import abi, render, scenes
from shimmer_amd.scene import SceneBuilder, tables

ROOT = Path(__file__).resolve().parents[1]
U = 2.0 ** -24  # the unit roundoff of float32
F32 = np.float32
INVALID_ARGUMENT = -1  # SHM_ERR_INVALID_ARGUMENT


def illum_scale_of(desc):
    """1 / CIE Y of the scene's illuminant: in double, rounded to float once (host_illuminant_scale)."""
    illum = np.ctypeslib.as_array(desc.color_space.illuminant, shape=(471,)).astype(np.float64)
    t = tables()
    return F32(float(F32(t["CIE_Y_INTEGRAL"])) / float((t["CIE_Y"].astype(F32).astype(np.float64) * illum).sum()))


# ---- the ABI ----
def test_header_against_abi_py(tmp_path):
    P = abi.ShmRenderParams
    assert C.sizeof(P) == 32 and P.ao_uniform_sample.offset == 27 and P.ao_max_distance.offset == 28 and P.pad.offset == 27 and P.pad.size == 5
    assert abi.SHM_INTEGRATOR_AMBIENT_OCCLUSION == 3
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "shimmer_hip.h"\nint main(void) {\n'
           '  ShmRenderParams p; printf("%zu %zu %zu %zu %zu %d\\n", sizeof(ShmRenderParams), offsetof(ShmRenderParams, ao_uniform_sample), offsetof(ShmRenderParams, ao_max_distance),'
           ' offsetof(ShmRenderParams, pad), sizeof(p.pad), SHM_INTEGRATOR_AMBIENT_OCCLUSION);\n  return 0;\n}\n')
    (tmp_path / "p.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "p.c"), "-o", str(tmp_path / "p")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "p")], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [32, P.ao_uniform_sample.offset, P.ao_max_distance.offset, P.pad.offset, P.pad.size, abi.SHM_INTEGRATOR_AMBIENT_OCCLUSION]


def test_zeroed_pad_gives_the_defaults():
    p = render.make_params(integrator="ambientocclusion")
    assert p.integrator == 3 and bytes(p.pad) == bytes(5) and p.ao_uniform_sample == 0 and p.ao_max_distance == 0.0
    assert bytes(render.make_params().pad) == bytes(5)  # every other caller's pad stays zero
    p = render.make_params(integrator="ambientocclusion", ao_uniform_sample=True, ao_max_distance=2.5)
    assert p.ao_uniform_sample == 1 and p.ao_max_distance == 2.5
    assert bytes(p.pad) == bytes([1]) + np.float32(2.5).tobytes()  # the same five bytes
    p.pad[:] = [0] * 5
    assert p.ao_uniform_sample == 0 and p.ao_max_distance == 0.0
    assert render.make_params(integrator="ambientocclusion", ao_max_distance=math.inf).ao_max_distance == 0.0  # infinite is the zero


def _twin_rc(lib, desc, params):
    pix, idx = np.zeros((1, 2), np.int32), np.zeros(1, np.int32)
    hits = np.zeros(1, dtype=render.HIT_DTYPE)
    hits["prim"] = -1
    rays, queued, sample = np.zeros((1, 8), F32), np.zeros(1, np.uint8), np.zeros((1, 5), F32)
    rc = lib.shm_ao_samples_host(C.byref(desc), C.byref(params), gc._i32(pix), gc._i32(idx), hits.ctypes.data_as(C.c_void_p), 1, rays.ctypes.data_as(C.c_void_p),
                                 queued.ctypes.data_as(C.c_void_p), sample.ctypes.data_as(abi.c_float_p))
    return rc, lib.shm_last_error().decode()


def test_validation(lib):
    sc = scenes.cornell_box(lib, 8, 8)
    assert _twin_rc(lib, sc.desc, ao.params_for())[0] == 0
    for bad in (-1.0, -0.0001, math.nan, -math.inf):
        rc, msg = _twin_rc(lib, sc.desc, ao.params_for(max_distance=bad))
        assert rc == INVALID_ARGUMENT and "ao_max_distance" in msg, (bad, rc, msg)
    keep = sc.desc.color_space.illuminant
    assert keep  # the builder attaches it to every scene
    sc.desc.color_space.illuminant = None
    rc, msg = _twin_rc(lib, sc.desc, ao.params_for())
    sc.desc.color_space.illuminant = keep
    assert rc == INVALID_ARGUMENT and "illuminant" in msg


def test_the_other_integrators_ignore_the_new_bytes(lib):
    """The two fields set to valid garbage under the path integrator. On the CPU the library reads ShmRenderParams in the G-buffer pass's twin: its camera rays and
    per-sample records are byte for byte those of zeroed fields. The oracle's path render is compared too, but the oracle never reads the bytes: that half only pins
    make_params. The device's kernels are held to it in tests/test_gpu_ambient_occlusion.py::test_the_other_integrators_after_an_ao_render."""
    sc = scenes.cornell_box(lib, 16, 12)
    pix, idx = gc.all_samples(tuple(sc.desc.film.pixel_bounds), 2)
    twins = []
    for kw in (dict(), dict(ao_uniform_sample=True, ao_max_distance=0.37)):
        p = render.make_params(seed=3, spp=2, max_depth=3, sampler="zsobol", **kw)
        rays = gc.twin_rays(lib, sc.desc, p, pix, idx)
        o = oracle_py.Oracle(sc.desc)
        hits, _ = o.trace(rays)
        o.close()
        twins.append(rays.tobytes() + gc.twin_samples(lib, sc.desc, p, abi.SHM_GBUFFER_SPACE_RENDER, pix, idx, hits).tobytes())
    assert twins[0] == twins[1]
    o = oracle_py.Oracle(sc.desc)
    films = []
    for kw in (dict(), dict(ao_uniform_sample=True, ao_max_distance=0.37)):
        films.append(o.render(render.make_params(seed=3, spp=2, max_depth=3, **kw), n_threads=4)[0])
    o.close()
    assert films[0].tobytes() == films[1].tobytes() and films[0]["rgb_sum"].sum() > 0


# ---- leaf values ----
def _stream(orc, px, py, index, seed, n):
    out = (C.c_float * n)()
    orc.lib.orc_fn_sampler_stream(px, py, index, seed, n, out)
    return np.array(out[:], F32)


def _coordinate_system64(v):
    """Frame::from_z's two tangents (Duff et al., vec.h coordinate_system) in float64."""
    sign = math.copysign(1.0, v[2])
    a = -1.0 / (sign + v[2])
    b = v[0] * v[1] * a
    return np.array([1.0 + sign * v[0] * v[0] * a, sign * b, -sign * v[0]]), np.array([b, sign + v[1] * v[1] * a, -v[1]])


def _direction64(u, uniform):
    """steps 5: (wl, pdf) of the 2-D draw u in float64."""
    if uniform:
        z = float(u[0])
        r = math.sqrt(max(0.0, 1.0 - z * z))
        phi = 2.0 * math.pi * float(u[1])
        return np.array([r * math.cos(phi), r * math.sin(phi), z]), 1.0 / (2.0 * math.pi)
    ox, oy = 2.0 * float(u[0]) - 1.0, 2.0 * float(u[1]) - 1.0  # sample_uniform_disk_concentric
    if ox == 0.0 and oy == 0.0:
        d = (0.0, 0.0)
    elif abs(ox) > abs(oy):
        d = (ox * math.cos(math.pi / 4 * (oy / ox)), ox * math.sin(math.pi / 4 * (oy / ox)))
    else:
        t = math.pi / 2 - math.pi / 4 * (ox / oy)
        d = (oy * math.cos(t), oy * math.sin(t))
    z = math.sqrt(max(0.0, 1.0 - d[0] * d[0] - d[1] * d[1]))
    return np.array([d[0], d[1], z]), z / math.pi


def _kind_of(desc, hit):
    p = desc.primitives[int(hit["prim"])]
    inst = "instanced " if int(hit["instance"]) else ""
    if p.shape_kind == abi.SHM_SHAPE_TRIANGLE:
        return inst + "triangle"
    if p.shape_kind == abi.SHM_SHAPE_SPHERE:
        return inst + {abi.SHM_QUADRIC_SPHERE: "sphere", abi.SHM_QUADRIC_DISK: "disk", abi.SHM_QUADRIC_CYLINDER: "cylinder"}[desc.spheres[p.shape_index].quadric]
    return inst + "patch"


LEAF_SCENES = {
    "quadrics": lambda lib: scenes.quadric_scene(lib, width=24, height=20),
    "instanced": lambda lib: scenes.instanced_scene(lib, 24, 20),
    "patches": lambda lib: scenes.cornell_box(lib, 24, 20, patches=True, patch_skew=0.1),
    "spheres": lambda lib: scenes.three_spheres(lib, 24, 20, camera=(0.0, 0.0, 8.0)),
}


@pytest.mark.parametrize("uniform", [False, True], ids=["cosine", "uniform"])
def test_leaf_values_against_float64(lib, uniform):
    """Steps 3-7 of the definition, re-evaluated in float64 from the oracle's interaction (p, n) at the camera ray's hit and the oracle's sampler stream.
    Tolerances, in units of U = 2^-24:
      wi   the local direction is two products of a radius and a sine / cosine (a few U each) and a square root for z, whose error grows like 1 / z towards the horizon;
           the frame and from_local add three products and two sums per component: 32 U tangentially, (32 / z) U along n
      pdf  cosine: z / pi, so the same (32 / z) U relative to 1 / pi; uniform: the literal, exact
      L    rgb = average over four wavelengths of sensor * (illum_scale * illuminant * dot / (pi pdf)) / pdf_lambda: a dozen roundings, and dot / pdf carries wi's error
           in z twice in the cosine mode: 64 U + (64 / z) U relative
      o    the point moved along n by the error bounds: within 1e-3 of p (the bounds are a few U of the coordinates), on wi's side of the plane through p."""
    seen = set()
    worst = dict(wi=0.0, L=0.0)
    for name, make in LEAF_SCENES.items():
        sc = make(lib)
        desc = sc.desc
        params = ao.params_for(seed=5, spp=2, uniform=uniform)
        orc = ao.open_oracle(desc, params)
        ch = ao.Chain(lib, desc, params, orc=orc)
        scale = float(illum_scale_of(desc))
        illum = np.ctypeslib.as_array(desc.color_space.illuminant, shape=(471,)).astype(np.float64)
        sensor = [np.ctypeslib.as_array(t, shape=(471,)).astype(np.float64) for t in (desc.film.sensor_r_bar, desc.film.sensor_g_bar, desc.film.sensor_b_bar)]
        out12, out14 = (C.c_float * 12)(), (C.c_float * 14)()
        step = max(1, len(ch.idx) // 160)
        for k in range(0, len(ch.idx), step):
            if ch.hits["prim"][k] < 0:
                assert not ch.queued[k] and not ch.sample[k, :3].any()
                continue
            px, py, index = int(ch.pix[k, 0]), int(ch.pix[k, 1]), int(ch.idx[k])
            ray = (C.c_float * 8)(*ch.rays[k])
            assert orc.lib.orc_fn_hit_interaction(orc.handle, ray, out12, None) == 1
            p, n = np.array(out12[0:3], np.float64), np.array(out12[3:6], np.float64)
            d = ch.rays[k, 3:6].astype(np.float64)
            if n @ -d < 0:
                n = -n
            u = _stream(orc, px, py, index, params.seed, 8)[6:8]  # behind lambda (1), the filter (2), the lens (2) and time (1)
            wl, pdf = _direction64(u, uniform)
            if pdf == 0.0:
                assert not ch.queued[k]
                continue
            assert ch.queued[k]
            z = max(wl[2], 1e-12)
            tx, ty = _coordinate_system64(n)
            wi = wl[0] * tx + wl[1] * ty + wl[2] * n
            got_wi = ch.occ_rays[k, 3:6].astype(np.float64)
            err = got_wi - wi
            along = abs(err @ n)
            tang = np.linalg.norm(err - (err @ n) * n)
            assert tang <= 32 * U and along <= 32 * U / z + 32 * U, (name, k, tang, along, z)
            worst["wi"] = max(worst["wi"], tang / U)
            assert abs(float(ch.sample[k, 4]) - pdf) <= (32 * U / z + 4 * U) / math.pi, (name, k)
            assert np.isinf(ch.occ_rays[k, 6]) and ch.occ_rays[k, 7] == 0.0
            # the origin: near p, displaced along n only, on wi's side
            o = ch.occ_rays[k, 0:3].astype(np.float64)
            off = o - p
            assert np.linalg.norm(off) <= 1e-3 * max(1.0, np.linalg.norm(p)) and (off @ n) * (wi @ n) > 0.0, (name, k, off, n, wi)
            assert np.linalg.norm(off - (off @ n) * n) <= 8 * U * max(1.0, np.abs(p).max()), (name, k)
            # the contribution as the film sees it
            orc.lib.orc_fn_camera_ray(orc.handle, px, py, index, params.seed, out14)
            lam, lpdf = np.array(out14[6:10], np.float64), np.array(out14[10:14], np.float64)
            idxs = np.floor(lam + 0.5).astype(int) - 360
            L = scale * illum[idxs] * ((wi @ n) / (math.pi * pdf))
            want = np.array([np.mean(s[idxs] * np.where(lpdf != 0, L / np.where(lpdf != 0, lpdf, 1.0), 0.0)) for s in sensor]) * float(desc.film.imaging_ratio)
            tol = (64 * U + 64 * U / z) * np.abs(want).max()
            assert np.all(np.abs(ch.sample[k, :3].astype(np.float64) - want) <= tol), (name, k, ch.sample[k, :3], want, z)
            worst["L"] = max(worst["L"], float(np.abs(ch.sample[k, :3] - want).max() / (U * np.abs(want).max())))
            seen.add(_kind_of(desc, ch.hits[k]))
        orc.close()
    print(f"worst tangential |wi - wi64| = {worst['wi']:.2f} U, worst |rgb - rgb64| / max rgb = {worst['L']:.2f} U; kinds {sorted(seen)}")
    assert {"triangle", "patch", "sphere", "disk", "instanced triangle"} <= seen, seen


# ---- exact cases, through the CPU chain ----
def _closed_box(lib, n=12, half=1.0):
    b = SceneBuilder()
    b.set_film(n, n - 2)
    rfw = b.set_camera_look_at(lib, (0.1, 0.2, 0.5), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 70.0)
    p, vi = scenes._box((-half, -half, -half), (half, half, half))
    b.add_mesh(scenes._to_render(p, rfw), vi, b.material_diffuse(0.5))
    return scenes._finish(b, lib)


def _lone_quad(lib, n=12, quad=True):
    b = SceneBuilder()
    b.set_film(n, n - 2)
    rfw = b.set_camera_look_at(lib, (0.0, 0.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0)
    s = 5.0 if quad else 0.4  # the small one leaves the outer pixels' rays nothing to hit
    p, vi = scenes._quad((-s, -s, 0), (s, -s, 0), (s, s, 0), (-s, s, 0))
    b.add_mesh(scenes._to_render(p, rfw), vi, b.material_diffuse(0.5))
    return scenes._finish(b, lib)


@pytest.mark.parametrize("sampler", ["independent", "zsobol"])
@pytest.mark.parametrize("uniform", [False, True], ids=["cosine", "uniform"])
def test_exact_cases(lib, sampler, uniform):
    spp = 4
    # a camera inside a closed box, infinite distance: every occlusion ray ends on a wall
    sc = _closed_box(lib)
    ch = ao.Chain(lib, sc.desc, ao.params_for(sampler, spp=spp, uniform=uniform))
    film = ch.film()
    assert (ch.hits["prim"] >= 0).all() and ch.queued.all() and ch.occluded.all()
    assert not film["rgb_sum"].any() and np.all(film["weight_sum"] == spp)
    # ... and with a distance far below the box's size, every hit sample is unoccluded
    # (a cosine sample grazes the wall it starts on no closer than its error offset: 1e-4 of a 2-unit box cannot reach another wall except from within 1e-4 of an edge)
    ch = ao.Chain(lib, sc.desc, ao.params_for(sampler, spp=spp, uniform=uniform, max_distance=1e-4))
    assert ch.queued.all() and ch.unoccluded.all() and np.all(ch.occ_rays[:, 6] == F32(1e-4))
    film = ch.film()
    assert np.all(film["rgb_sum"][..., 1] > 0) and np.all(film["weight_sum"] == spp)
    # a lone quad facing the camera with nothing around it: unoccluded at every sample
    sc = _lone_quad(lib)
    ch = ao.Chain(lib, sc.desc, ao.params_for(sampler, spp=spp, uniform=uniform))
    assert (ch.hits["prim"] >= 0).all() and ch.queued.all() and ch.unoccluded.all()
    # ... and around a small one the camera rays escape: those pixels are exactly 0 and keep their weight
    sc = _lone_quad(lib, quad=False)
    ch = ao.Chain(lib, sc.desc, ao.params_for(sampler, spp=spp, uniform=uniform))
    film = ch.film()
    escaped = (ch.hits["prim"] < 0).reshape(film.shape + (spp,)).all(axis=2)
    assert escaped.any() and not escaped.all()
    assert not film["rgb_sum"][escaped].any() and np.all(film["weight_sum"] == spp) and not ch.queued[ch.hits["prim"] < 0].any()
    assert np.all(film["rgb_sum"][~escaped][:, 1] > 0)


# ---- physics: the expectation against the oracle's path integrator ----
# 48 seeds, not the minimum of 8: the standard error is itself estimated from the seeds, so z is Student-t distributed with about 2 (N - 1) degrees of freedom, and the
# 4-standard-error rule only has the normal tail it is argued with (P(|z| > 4) ~ 6e-5 per block) once N is large: at 16 seeds P(|t_30| > 4) ~ 4e-4 per block, 2.4 % over
# 64 blocks — and seeds 101..116 are such a draw (block 37 at |z| = 4.13, which 48 fresh seeds put at 0.2: profiles/ambient_occlusion.md) —, at 48 it is 1.2e-4, 0.8 %.
# The seed count was raised AFTER that failure was seen, so the control stays on record: 48 fresh seeds (1000..1047) gave a largest |z| of 2.44, block 37 at 0.0 / -0.2 / 0.8,
# a mean z of 0.14 with standard deviation 1.00 and whole-image means 0.8 standard errors apart — no bias. Should this test fail after a change to the arithmetic, that is
# to be read as a possible real bias and investigated as one; adding seeds again is not a fix.
N_SEEDS, STAT_SPP, STAT_RES = 48, 64, 32


def _clay_box(lib, light):
    """A Cornell-like box with two blocks, every surface a flat-shaded DiffuseMaterial of reflectance 1, open towards the camera; `light`: a uniform infinite light
    whose spectrum is the scene's illuminant at illum_scale — what the AO integrator integrates against."""
    b = SceneBuilder()
    b.set_film(STAT_RES, STAT_RES)
    rfw = b.set_camera_look_at(lib, (0.0, 1.0, 2.4), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), 40.0)
    white = b.material_diffuse(1.0)
    parts = [scenes._box((-1.0, 0.0, -1.0), (1.0, 2.0, 1.0), faces="xXyYz")]  # the room: five walls seen from inside (the +z face is the opening)
    room_p, room_vi = parts[0]
    room_vi = room_vi[:, ::-1].copy()
    b.add_mesh(scenes._to_render(room_p, rfw), room_vi, white)
    for lo, hi in (((-0.7, 0.0, -0.6), (-0.1, 1.2, 0.0)), ((0.15, 0.0, -0.1), (0.75, 0.6, 0.5))):
        p, vi = scenes._box(lo, hi)
        b.add_mesh(scenes._to_render(p, rfw), vi, white)
    if light:
        illum = scenes_illuminant()
        b.light_uniform_infinite(illum, scale=1.0)
    sc = scenes._finish(b, lib)
    if light:
        sc.desc.lights[0].scale = float(illum_scale_of(sc.desc))
    return sc


def scenes_illuminant():
    from shimmer_amd.scene import piecewise_from_interleaved, piecewise_to_dense
    return piecewise_to_dense(*piecewise_from_interleaved(tables()["CIE_ILLUM_D6500"], True))


def _block_means(rgb, mask):
    """4 x 4 block means of an (H, W, 3) image over the pixels of `mask`; blocks without one are dropped. (n_blocks, 3)."""
    h, w = mask.shape
    out = []
    for y in range(0, h, 4):
        for x in range(0, w, 4):
            m = mask[y:y + 4, x:x + 4]
            if m.any():
                out.append(rgb[y:y + 4, x:x + 4][m].mean(axis=0))
    return np.array(out)


@pytest.fixture(scope="module")
def stat_renders(lib):
    """Per seed: the AO film (cosine and uniform) through the CPU chain and the oracle's path render of the lit twin of the scene, as rgb_sum / weight_sum."""
    sc_ao, sc_path = _clay_box(lib, False), _clay_box(lib, True)
    orc_ao, orc_path = oracle_py.Oracle(sc_ao.desc), oracle_py.Oracle(sc_path.desc)
    cos, uni, path = [], [], []
    covered = np.ones((STAT_RES, STAT_RES), bool)
    for seed in range(101, 101 + N_SEEDS):
        for uniform, dst in ((False, cos), (True, uni)):
            ch = ao.Chain(lib, sc_ao.desc, ao.params_for(seed=seed, spp=STAT_SPP, uniform=uniform), orc=orc_ao)
            dst.append(render.film_to_rgb(ch.film()).astype(np.float64))
            covered &= (ch.hits["prim"] >= 0).reshape(STAT_RES, STAT_RES, STAT_SPP).all(axis=2)  # G-buffer coverage 1: the infinite light is not seen directly
        film, _ = orc_path.render(render.make_params(seed=seed, spp=STAT_SPP, max_depth=1), n_threads=8)
        path.append(render.film_to_rgb(film).astype(np.float64))
    orc_ao.close()
    orc_path.close()
    return dict(cos=np.array(cos), uni=np.array(uni), path=np.array(path), covered=covered)


def _max_z(a, b, covered):
    """The largest |z| over the 4 x 4 blocks and the three channels: the difference of the seed means over its standard error, estimated from both renders' spread."""
    ba = np.array([_block_means(x, covered) for x in a])  # (seeds, blocks, 3)
    bb = np.array([_block_means(x, covered) for x in b])
    n = ba.shape[0]
    diff = ba.mean(axis=0) - bb.mean(axis=0)
    se = np.sqrt((ba.var(axis=0, ddof=1) + bb.var(axis=0, ddof=1)) / n)
    assert np.all(se > 0)
    return float(np.abs(diff / se).max()), ba.shape[1], float(np.abs(diff).max() / bb.mean())


def test_expectation_equals_the_path_integrators_direct_lighting(stat_renders):
    """Cosine sampling, infinite distance, against the oracle's path integrator at max_depth 1 (reference-exact quirks: its uniform infinite light is sampled over the
    sphere with density 1 / (4 pi), which is right there) on the same geometry with reflectance 1 under the illuminant as a uniform infinite light: both estimate
    illum_scale * illuminant * (1 / pi) * the cosine-weighted visibility of the sky. Every block mean within 4 standard errors: P(|z| > 4) ~ 6e-5 per block."""
    r = stat_renders
    assert r["covered"].sum() >= 0.75 * r["covered"].size
    z, n_blocks, rel = _max_z(r["cos"], r["path"], r["covered"])
    print(f"AO cosine vs path integrator: {n_blocks} blocks, {N_SEEDS} seeds x {STAT_SPP} spp, largest |z| = {z:.3f}, largest |difference| / mean = {rel:.4f}")
    assert r["path"][:, r["covered"]].mean() > 0.01
    assert z <= 4.0


def test_uniform_sampling_agrees_with_cosine_sampling(stat_renders):
    r = stat_renders
    z, n_blocks, rel = _max_z(r["uni"], r["cos"], r["covered"])
    print(f"AO uniform vs cosine: {n_blocks} blocks, largest |z| = {z:.3f}, largest |difference| / mean = {rel:.4f}")
    assert z <= 4.0


# ---- the loader and the host mirror ----
PBRT = """
LookAt 0 1 3  0 1 0  0 1 0
Camera "perspective" "float fov" 40
Film "rgb" "integer xresolution" 8 "integer yresolution" 8
Sampler "independent" "integer pixelsamples" 4
{integrator}
WorldBegin
Shape "sphere"
"""


def _parse(lib, integrator):
    out = C.POINTER(abi.ShmPbrtScene)()
    rc = lib.shm_scene_parse_pbrt(PBRT.format(integrator=integrator).encode(), None, C.byref(out))
    return rc, out


def test_loader(lib):
    rc, out = _parse(lib, 'Integrator "ambientocclusion"')
    assert rc == 0
    s = out.contents
    assert s.integrator == b"ambientocclusion" and s.params.integrator == 3 and s.params.ao_uniform_sample == 0 and s.params.ao_max_distance == 0.0
    assert s.desc.color_space.illuminant  # the loader hands the illuminant over with every scene
    want = ao.params_for(seed=0, spp=4)
    assert bytes(s.params) == bytes(want)  # the round trip against make_params
    lib.shm_pbrt_free(out)
    rc, out = _parse(lib, 'Integrator "ambientocclusion" "float maxdistance" 1.5 "bool cossample" false')
    assert rc == 0
    s = out.contents
    want = ao.params_for(seed=0, spp=4, uniform=True, max_distance=1.5)
    assert s.params.ao_uniform_sample == 1 and s.params.ao_max_distance == 1.5 and bytes(s.params) == bytes(want)
    lib.shm_pbrt_free(out)
    for bad in ("-1", "0"):
        rc, out = _parse(lib, f'Integrator "ambientocclusion" "float maxdistance" {bad}')
        assert rc == INVALID_ARGUMENT and not out and "<string>:6" in lib.shm_last_error().decode() and "maxdistance" in lib.shm_last_error().decode()
    rc, out = _parse(lib, 'Integrator "bdpt"')
    assert rc == INVALID_ARGUMENT and not out and "<string>:6: Unknown integrator bdpt" in lib.shm_last_error().decode()
    # the other integrators leave the two fields zero
    rc, out = _parse(lib, 'Integrator "path"')
    assert rc == 0 and bytes(out.contents.params.pad) == bytes(5)
    lib.shm_pbrt_free(out)


def test_host_mirror_knows_the_name(lib):
    sc = scenes.cornell_box(lib, 16, 16)
    film = np.zeros((16, 16), dtype=render.FILM_DTYPE)
    args = (C.byref(sc.desc), 0, 5, 0, 1, 1, 2, 0, 0, 0, film.ctypes.data_as(C.c_void_p), None, None)
    assert lib.shm_integrator_render(b"bdpt", *args) == -2 and b"Unknown integrator bdpt" in lib.shm_last_error()
    rc = lib.shm_integrator_render(b"ambientocclusion", *args)
    if lib.shm_device_count() == 0:
        assert rc == -2 and b"no CPU fallback" in lib.shm_last_error()  # a known name: it gets as far as the device
    else:
        assert rc == 0 and film["weight_sum"].min() == 2.0


def test_the_example_scene_names_the_integrator(lib):
    out = C.POINTER(abi.ShmPbrtScene)()
    abi.check(lib, lib.shm_scene_load_pbrt(str(ROOT / "examples" / "scenes" / "integrators" / "ambient_occlusion.pbrt").encode(), C.byref(out)), "ambient_occlusion.pbrt")
    s = out.contents
    assert s.integrator == b"ambientocclusion" and s.params.integrator == 3 and s.params.ao_max_distance > 0.0
    params = abi.ShmRenderParams.from_buffer_copy(bytes(s.params))
    params.samples_per_pixel = 2
    ch = ao.Chain(lib, s.desc, params)
    film = ch.film()
    assert ch.occluded.any() and ch.unoccluded.any() and film["rgb_sum"].sum() > 0 and np.all(film["weight_sum"] == 2.0)
    lib.shm_pbrt_free(out)
