"""PBRT-v4's shape alpha on the device: the six traversal kernels of k_trace_alpha.hip against the CPU oracle, bit for bit — the film and the seven counters of
scenes.cutout_scene in every scene class, on both general rows of the traversal table, under both samplers and both settings of disable_reference_quirks (the STRICT
any-hit pair); shm_trace_closest / shm_trace_any against orc_trace_closest / orc_trace_any for a cut triangle mesh, patch, sphere, disk and instanced mesh; the G-buffer
pass against its CPU twin; and the films of scenes without a cutout as the parent commit rendered them. Films are 32 x 32 at 4 spp or fewer, ray batches 4096 rays.
Which test launches which kernel: profiles/shape_alpha.md."""
import json
import os
import sys

import numpy as np
import pytest

import gbuffer_cases as gc
import oracle_py
import zsobol_cases as zc
from shimmer_amd import abi, render, scenes
from test_shape_alpha import ROOT, SHAPES, STATS, build, on_cut_shape, rays_at, uniform_targets

sys.path.insert(0, str(ROOT / "tests" / "golden"))
pytestmark = pytest.mark.gpu
VARIANTS = ["lean", "glass", "coated", "textured", "environment", "instances"]
TRACE_GEN, TRACE_GEN_HEAVY = 1, 2  # (host/render_plan.hpp)


def gpu_render(lib, desc, p):
    g = render.Renderer(lib, desc, 0)
    try:
        return g.render(p)
    finally:
        g.close()


_ORACLE = {}


def oracle_render(sc, key, p):
    """The oracle's film of a scene and parameter set, computed once and shared (a test never writes to it)."""
    if key not in _ORACLE:
        o = oracle_py.Oracle(sc.desc)
        try:
            _ORACLE[key] = o.render(p, n_threads=min(16, os.cpu_count() or 1))
        finally:
            o.close()
    return _ORACLE[key]


def assert_equals(f_gpu, s_gpu, f_cpu, s_cpu, what):
    for field in ("rgb_sum", "weight_sum"):
        assert np.array_equal(f_gpu[field], f_cpu[field]), (what, field)
    for k in STATS:
        assert s_gpu[k] == s_cpu[k], (what, k)
    assert np.isfinite(f_gpu["rgb_sum"]).all(), what


def set_row(monkeypatch, gen_heavy):
    monkeypatch.delenv("SHM_GEN_HEAVY", raising=False)
    if gen_heavy is not None:
        monkeypatch.setenv("SHM_GEN_HEAVY", gen_heavy)


def row_of(desc, gen_heavy):
    o = oracle_py.Oracle(desc)
    plan = o.trace_plan(gen_heavy_knob=-1 if gen_heavy is None else int(gen_heavy))
    o.close()
    return plan["variant"]


@pytest.mark.parametrize("gen_heavy", [None, "0"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_film_and_counters_equal_the_oracle(gpu_lib, monkeypatch, variant, gen_heavy):
    """Every scene class on both general rows: the cut records of these small scenes are a twelfth of all records or more, so they take the five-wave row by themselves
    (k_trace5_alpha<., true>); SHM_GEN_HEAVY=0 puts the same scenes on the seven-wave row (k_trace5_alpha<., false>). The scene holds a cut disk as well in the lean
    class (the K_QUADRICS half of the build)."""
    sc = scenes.cutout_scene(gpu_lib, variant, disk=(variant == "lean"))
    assert row_of(sc.desc, gen_heavy) == (TRACE_GEN_HEAVY if gen_heavy is None else TRACE_GEN)
    set_row(monkeypatch, gen_heavy)
    p = render.make_params(seed=13, spp=4, max_depth=5)
    f_gpu, s_gpu = gpu_render(gpu_lib, sc.desc, p)
    f_cpu, s_cpu = oracle_render(sc, (variant, "path", 13), p)
    assert_equals(f_gpu, s_gpu, f_cpu, s_cpu, (variant, gen_heavy))
    assert f_gpu["rgb_sum"].max() > 0 and s_gpu["rays_any"] > 0
    # the field is read: the same shapes uncut render another film
    solid = scenes.cutout_scene(gpu_lib, variant, disk=(variant == "lean"), cut=False)  # (held: the builder owns the arrays the description points at)
    f_solid, _ = gpu_render(gpu_lib, solid.desc, p)
    assert not np.array_equal(f_solid["rgb_sum"], f_gpu["rgb_sum"])


@pytest.mark.parametrize("variant", ["lean", "coated", "instances"])
def test_zsobol_equals_the_oracle(gpu_lib, variant):
    sc = scenes.cutout_scene(gpu_lib, variant)
    p = render.make_params(seed=21, spp=4, max_depth=5, sampler="zsobol")
    f, s = gpu_render(gpu_lib, sc.desc, p)
    zc.assert_equals_oracle(sc.desc, p, f, s, variant)
    assert f["rgb_sum"].max() > 0


@pytest.mark.parametrize("gen_heavy", [None, "0"])
@pytest.mark.parametrize("quirks", [True, False])
def test_an_instanced_cutout_under_both_quirk_settings(gpu_lib, monkeypatch, gen_heavy, quirks):
    """disable_reference_quirks = 1 in a scene with instances: the shadow rays take k_trace5_alpha_any_strict (five and seven waves); = 0: k_trace5_alpha<true, .>."""
    set_row(monkeypatch, gen_heavy)
    sc = scenes.cutout_scene(gpu_lib, "instances")
    p = render.make_params(seed=17, spp=4, max_depth=5, reference_quirks=quirks)
    f_gpu, s_gpu = gpu_render(gpu_lib, sc.desc, p)
    f_cpu, s_cpu = oracle_render(sc, ("instances", "quirks", quirks, 17), p)
    assert_equals(f_gpu, s_gpu, f_cpu, s_cpu, ("instances", gen_heavy, quirks))
    assert f_gpu["rgb_sum"].max() > 0


# ---- the trace API ------------------------------------------------------------------------------------------------------------------------
def cut_alpha(b):
    """Holes, coin and solid: a 4 x 4 checkerboard over the shape's (u, v) between 0 and a 2 x 2 checkerboard between one half and 1 (a program of five ops)."""
    inner = b.ftex_checkerboard(0.5, 1.0, mapping=b.add_texture_mapping("uv", su=2.0, sv=2.0))
    return b.ftex_checkerboard(0.0, inner, mapping=b.add_texture_mapping("uv", su=4.0, sv=4.0))


@pytest.mark.parametrize("gen_heavy", [None, "0"])
@pytest.mark.parametrize("shape", SHAPES)
def test_trace_api_equals_the_oracle(gpu_lib, monkeypatch, shape, gen_heavy):
    """shm_trace_closest against orc_trace_closest — the hit records byte for byte — and shm_trace_any against orc_trace_any, with the counters, for a cut triangle
    mesh, bilinear patch, sphere, disk and a triangle mesh inside an instance: accepted, rejected and coin-tossed candidates all occur. The cut records are a twelfth or
    more of these scenes' records: the five-wave row by count; SHM_GEN_HEAVY=0: the seven-wave row."""
    _, desc = build(gpu_lib, shape, make_alpha=cut_alpha)
    assert row_of(desc, gen_heavy) == (TRACE_GEN_HEAVY if gen_heavy is None else TRACE_GEN)
    set_row(monkeypatch, gen_heavy)
    rays = rays_at(uniform_targets(half=1.5))
    short = rays.copy()
    short[:, 6] = 1.2
    o = oracle_py.Oracle(desc)
    g = render.Renderer(gpu_lib, desc, 0)
    try:
        want, s_want = o.trace(rays)
        got, s_got = g.trace(rays)
        assert got.tobytes() == want.tobytes(), (shape, np.flatnonzero(got["prim"] != want["prim"])[:8])
        for k in ("rays_closest", "nodes_closest", "tris_closest"):
            assert s_got[k] == s_want[k], (shape, k)
        on = on_cut_shape(desc, want, shape).sum()
        _, uncut = build(gpu_lib, shape)
        o_uncut = oracle_py.Oracle(uncut)
        solid, _ = o_uncut.trace(rays)
        o_uncut.close()
        candidates = on_cut_shape(uncut, solid, shape).sum()
        assert 0 < on < candidates, (on, candidates)
        for r in (rays, short):
            want_any, s_want = o.trace(r, any_hit=True)
            got_any, s_got = g.trace(r, any_hit=True)
            assert np.array_equal(got_any, want_any), shape
            for k in ("rays_any", "nodes_any", "tris_any"):
                assert s_got[k] == s_want[k], (shape, k)
    finally:
        g.close()
        o.close()


def test_many_cut_triangles_in_shared_leaves(gpu_lib):
    """Forty small cut triangles among the scene's shapes (scenes.cutout_scene, n_leaves): leaves that hold several cut records, one ray after the other."""
    sc = scenes.cutout_scene(gpu_lib, "lean", n_leaves=40)
    p = render.make_params(seed=5, spp=2, max_depth=4)
    f_gpu, s_gpu = gpu_render(gpu_lib, sc.desc, p)
    f_cpu, s_cpu = oracle_render(sc, ("leaves", 5), p)
    assert_equals(f_gpu, s_gpu, f_cpu, s_cpu, "leaves")


# ---- the G-buffer -------------------------------------------------------------------------------------------------------------------------
def test_gbuffer_shows_the_wall_through_the_holes(gpu_lib):
    """The G-buffer pass of a cutout scene against its CPU twin: the twin's camera rays, traced by the ORACLE, through shm_gbuffer_samples_host, summed in sample order —
    bit for bit; and there are samples whose first hit is the cut quad in the uncut scene and something behind it here."""
    sc = scenes.cutout_scene(gpu_lib, "textured", 24, 20)
    solid = scenes.cutout_scene(gpu_lib, "textured", 24, 20, cut=False)
    params = gc.params_for("independent")
    r = render.Renderer(gpu_lib, sc.desc)
    o, o_solid = oracle_py.Oracle(sc.desc), oracle_py.Oracle(solid.desc)
    try:
        pix, idx = gc.all_samples(r.pixel_bounds, params.samples_per_pixel)
        rays = gc.twin_rays(gpu_lib, sc.desc, params, pix, idx)
        hits, _ = o.trace(rays)
        hits_solid, _ = o_solid.trace(rays)
        dev_hits, _ = r.trace(rays)
        assert dev_hits.tobytes() == hits.tobytes()
        through = (hits["t"] > hits_solid["t"]) | ((hits["prim"] < 0) & (hits_solid["prim"] >= 0))
        assert through.sum() > 50
        want = gc.pixel_sums(gc.twin_samples(gpu_lib, sc.desc, params, abi.SHM_GBUFFER_SPACE_RENDER, pix, idx, hits), r.width * r.height, gc.SPP)
        g, stats = r.gbuffer(params)
        got = gc.gbuffer_as_rows(g)
        assert np.isfinite(got).all() and stats["rays_closest"] == r.width * r.height * gc.SPP
        bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
        assert bad.size == 0, (bad[:8], got[bad[:1]], want[bad[:1]])
        want_solid = gc.pixel_sums(gc.twin_samples(gpu_lib, solid.desc, params, abi.SHM_GBUFFER_SPACE_RENDER, pix, idx, hits_solid), r.width * r.height, gc.SPP)
        changed = (got != want_solid).any(axis=1)
        pixels_through = through.reshape(-1, gc.SPP).any(axis=1)
        assert changed[pixels_through].all() and not changed[~pixels_through].any()  # position, albedo and coverage differ exactly where a sample went through a hole
    finally:
        r.close()
        o.close()
        o_solid.close()


# ---- before and after ---------------------------------------------------------------------------------------------------------------------
def test_scenes_without_a_cutout_render_what_the_parent_commit_rendered(gpu_lib):
    """tests/golden/shape_alpha_before.json on the device: three_spheres, instanced_scene, the Cornell box as patches and the lean disk-and-cylinder scene take the kernels
    they took — those of k_trace.hip and k_trace_quadrics.hip, instruction-identical to the parent's (tools/kernel_isa_diff.py, profiles/shape_alpha.md) — and render
    the parent's films."""
    import gen_shape_alpha_before as gen
    before = json.loads((ROOT / "tests" / "golden" / "shape_alpha_before.json").read_text())
    assert len(before["films"]) == 8
    for rec in before["films"]:
        sc = gen.scene(gpu_lib, rec["scene"])
        assert all(s.alpha == 0 for s in sc.builder.spheres) and all(m["alpha"] == 0 for m in sc.builder.meshes + sc.builder.patch_meshes)
        f, st = gpu_render(gpu_lib, sc.desc, gen.params_of(rec))
        assert gen.film_sha256(f) == rec["sha256"], rec["scene"]
        assert [int(st[k]) for k in STATS] == rec["stats"], rec["scene"]
