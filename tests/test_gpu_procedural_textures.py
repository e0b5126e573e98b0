"""PBRT-v4's procedural float textures on the device: every kernel class that evaluates textures renders the film, the hit records and the seven counters of the CPU oracle bit
for bit; ZSobol against the oracle too and by decomposition invariance; the leaf probe (PROBE_FLOAT_TEXTURE) on the CPU test's leaf scene and contexts, bit-equal to the
oracle; and the films of two existing textured scenes, which must be what the library before this change rendered (tests/golden/procedural_textures_before.json).
The film is 33 x 31 at 3 samples: 3069 paths, no multiple of 256 — a partial last wave, and queues that compact."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_py
import test_procedural_textures as pt
import zsobol_cases as zc
from oracle_py import fa
from shimmer_amd import abi, render, scene as scn, scenes
from test_gpu_zsobol import probe_op

pytestmark = pytest.mark.gpu
STATS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")
W, H, SPP, DEPTH = 33, 31, 3, 5
SPOT = dict(spot_from=(0.5, 1.7, 0.8), spot_to=(-0.2, 0.3, -0.2), sun_from=(0.3, 0.4, 3.0), sun_to=(0.0, 0.8, 0.0))


def rays_through(sc, n=300, seed=5):
    rng = np.random.default_rng(seed)
    b = sc.info["bounds"]
    lo, hi = b[:, :3].min(0), b[:, 3:].max(0)
    c, r = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    o = c + (rng.random((n, 3)) * 2 - 1) * r
    d = (c + (rng.random((n, 3)) - 0.5) * r) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3], rays[:, 3:6], rays[:, 6] = o, d, np.inf
    return rays


def assert_equals_oracle(lib, sc, p, what):
    g = render.Renderer(lib, sc.desc, 0)
    f_gpu, s_gpu = g.render(p)
    rays = rays_through(sc)
    h_gpu, _ = g.trace(rays)
    g.close()
    orc = oracle_py.Oracle(sc.desc)
    f_cpu, s_cpu = orc.render(p, n_threads=min(16, os.cpu_count() or 1))
    h_cpu, _ = orc.trace(rays)
    orc.close()
    for field in ("rgb_sum", "weight_sum"):
        assert np.array_equal(f_gpu[field], f_cpu[field]), (what, field)
    for k in STATS:
        assert s_gpu[k] == s_cpu[k], (what, k)
    hit = h_cpu["prim"] >= 0  # (the record of a miss is only defined up to prim = -1)
    assert np.array_equal(h_gpu["prim"], h_cpu["prim"]) and hit.sum() > 100, what
    for k in ("t", "b0", "b1", "b2", "phi", "instance"):
        assert np.array_equal(h_gpu[k].view(np.uint32)[hit], h_cpu[k].view(np.uint32)[hit]), (what, k)
    assert np.isfinite(f_gpu["rgb_sum"]).all() and f_gpu["rgb_sum"].sum() > 0 and (f_gpu["weight_sum"] == p.samples_per_pixel).all()
    return f_gpu


CASES = {
    # the split pass (plain diffuse walls beside textured ones) + k_vertex_tex / the fused textured kernel
    "cornell_checker": ("checker", dict(), dict()),
    # a sphere with a 3-D checkerboard, a bilinear patch with dots: the general-geometry textured units (gen_tex)
    "sphere_and_patch": ("general", dict(), dict()),
    # a coated material with a wrinkled bump map, fbm roughness and windy thickness: the staged layered textured units
    "coated_wrinkled_fbm": ("coated", dict(), dict()),
    # a spot and a distant light: the *_dl builds
    "cornell_checker_spot": ("checker", dict(extra_lights=scenes.spot_and_distant(**SPOT)), dict()),
    # PBRT-v4's forms: the strict spherical mapping under the dots of the back wall
    "cornell_checker_quirks_off": ("checker", dict(), dict(reference_quirks=False)),
    # the other integrators: k_shade_other
    "cornell_checker_simplepath": ("checker", dict(), dict(integrator="simplepath")),
    "cornell_checker_randomwalk": ("checker", dict(), dict(integrator="randomwalk")),
    "sphere_and_patch_simplepath": ("general", dict(), dict(integrator="simplepath")),
    # zero differentials: the point-sampled branch of the checkerboard and the log2(0) clamp of the octave count
    "cornell_checker_unfiltered": ("checker", dict(), dict(disable_texture_filtering=True)),
    "coated_unfiltered": ("coated", dict(), dict(disable_texture_filtering=True)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_film_hits_and_counters_equal_the_oracle(gpu_lib, name):
    which, scene_kw, param_kw = CASES[name]
    sc = scenes.procedural_cornell(gpu_lib, W, H, which=which, **scene_kw)
    assert (W * H * SPP) % 256 != 0 and sc.desc.n_image_levels == 0
    assert_equals_oracle(gpu_lib, sc, render.make_params(seed=13, spp=SPP, max_depth=DEPTH, **param_kw), name)


def test_the_textures_are_used(gpu_lib):
    """The floor's checkerboard shows; filtering changes the film; PBRT-v4's spherical mapping changes the dots of the back wall."""
    sc = scenes.procedural_cornell(gpu_lib, W, H)
    g = render.Renderer(gpu_lib, sc.desc, 0)
    a, _ = g.render(render.make_params(seed=13, spp=16, max_depth=DEPTH))
    b, _ = g.render(render.make_params(seed=13, spp=16, max_depth=DEPTH, disable_texture_filtering=True))
    c, _ = g.render(render.make_params(seed=13, spp=16, max_depth=DEPTH, reference_quirks=False))
    g.close()
    assert not np.array_equal(a["rgb_sum"], b["rgb_sum"]) and not np.array_equal(a["rgb_sum"], c["rgb_sum"])
    rgb = render.film_to_rgb(b)
    assert rgb[H - 6:H - 2, 6:W - 6, 1].std() > 0.03


@pytest.mark.parametrize("which", ["checker", "coated"])
def test_zsobol_decomposition_invariance(gpu_lib, which):
    """The *_zs textured kernels are held to the oracle's film and counters, and to a film that is repeatable, does not depend on how the work is cut up, and agrees with
    independent sampling in the mean."""
    sc = scenes.procedural_cornell(gpu_lib, W, H, which=which)
    p = render.make_params(seed=21, spp=8, max_depth=DEPTH, sampler="zsobol")
    g = render.Renderer(gpu_lib, sc.desc, 0)
    f1, s1 = g.render(p)
    f2, _ = g.render(p)
    assert np.array_equal(f1, f2) and (f1["weight_sum"] == 8.0).all() and np.isfinite(f1["rgb_sum"]).all()
    zc.assert_equals_oracle(sc.desc, p, f1, s1, which)
    f_ind, _ = g.render(render.make_params(seed=21, spp=8, max_depth=DEPTH))
    assert not np.array_equal(f1, f_ind)
    g.clear()
    idx = np.arange(g.n_tiles)
    for ws, we in scn.wave_schedule(8):
        g.render_waves(p, tile_indices=idx[idx % 3 != 0], waves=[(ws, we)])
        g.render_waves(p, tile_indices=idx[idx % 3 == 0], waves=[(ws, we)])
    assert np.array_equal(g.read_film(), f1)
    g.clear()
    g.render_device(p)
    assert np.array_equal(g.read_film(), f1)
    a = render.film_to_rgb(g.render(render.make_params(seed=2, spp=64, max_depth=DEPTH, sampler="zsobol"))[0]).mean()
    c = render.film_to_rgb(g.render(render.make_params(seed=2, spp=64, max_depth=DEPTH))[0]).mean()
    g.close()
    assert abs(a / c - 1.0) < 0.05, (a, c)  # (margin of tests/test_gpu_delta_lights.py's check of the same kind)


def test_the_probe_replays_the_leaf_vectors(gpu_lib):
    """PROBE_FLOAT_TEXTURE: the device's float_texture_evaluate_v on the CPU test's leaf scene at its shared contexts, bit-equal to the oracle's, with the reference quirks on
    and (the 2-D mappings are UV here, so the switch must change nothing) off."""
    plib = abi.load_probe_library()
    op = probe_op("FLOAT_TEXTURE")
    n = pt.leaf_scene(gpu_lib)
    b = n["builder"]
    ctxs = pt.leaf_contexts()
    fb = lambda v: int(np.float32(v).view(np.uint32))  # noqa: E731
    records = b"".join(bytes(t) for t in b.float_textures) + b"".join(bytes(t) for t in b.textures)
    tail = [fb(v) for c in ctxs for v in c] + list(np.frombuffer(records, np.uint32))
    o = oracle_py.Oracle(n["desc"])
    try:
        for name in pt.LEAF_NODES:
            want = np.array([o.lib.orc_fn_float_texture_evaluate(o.handle, n[name], fa(*c)) for c in ctxs], np.float32)
            for quirks_off in (0, 1):
                words = [n[name], len(b.float_textures), len(b.textures), quirks_off, len(ctxs)] + tail
                a = (C.c_uint32 * len(words))(*[int(w) for w in words])
                out = (C.c_uint32 * len(ctxs))()
                res = C.c_int()
                abi.check(plib, plib.shm_debug_eval_leaf(0, op, a, len(words), out, len(ctxs), C.byref(res)), "shm_debug_eval_leaf")
                assert res.value == len(ctxs)
                got = np.frombuffer(bytes(out), np.float32)
                assert got.tobytes() == want.tobytes(), (name, quirks_off, int(np.argmax(got != want)))
    finally:
        o.close()


def test_existing_textured_scenes_render_what_they_rendered(gpu_lib):
    """Before / after on the device: the two films of tests/golden/procedural_textures_before.json, rendered by the library before this change."""
    import gen_procedural_textures_before as before
    golden = json.loads((pt.ROOT / "tests" / "golden" / "procedural_textures_before.json").read_text())
    for case in golden["films"]:
        desc, keep = before.scene(gpu_lib, case["scene"])
        g = render.Renderer(gpu_lib, desc, 0)
        film, st = g.render(render.make_params(seed=case["seed"], spp=case["spp"], max_depth=case["max_depth"]))
        g.close()
        assert hashlib.sha256(np.ascontiguousarray(film).tobytes()).hexdigest() == case["sha256"], case["scene"]
        assert [int(st[k]) for k in STATS] == case["stats"], case["scene"]
