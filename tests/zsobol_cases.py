"""The ZSobol edge cases, as data: one table that tests/test_zsobol_oracle.py checks on the CPU for WHERE each row lands (host/render_plan.hpp's coordinates of the
kernel table, through the oracle library's orc_fn_scene_facts / orc_fn_render_plan) and that tests/test_gpu_zsobol_oracle.py renders on the device and holds to the CPU
oracle bit for bit. No GPU is needed to import this module.

A row: name, the scene builder call (builder, keywords), make_params keywords (the sampler is ZSobol in every row), the environment knobs of the render, the CELL the
row is meant to exercise, and how the render is cut up (`cut`): None (one render), "waves" (wave by wave with sample_begin > 0, the accumulated film), "tiles" (a
third of the tiles), "crop" (the tiles of CROP in a 1024 x 768 film). A cell is a point in the plan's coordinates (COORDS); CELLS names them. The cells are pairwise
distinct, every cell has a row, and every row lands on its cell: a change to render_plan.hpp that moves a case onto other kernels fails the CPU test. The rows of the
stream, Morton, depth and sample-index edges share the cell of a class row on purpose (they vary the sampler's inputs, not the kernels)."""
from collections import namedtuple

COORDS = ("route", "geo", "img", "img_lean", "img_generate", "flt", "dl", "lean_first", "fused_from_0", "split", "divert_vertex", "layered_onepass")
ROUTE_LEAN, ROUTE_STAGED, ROUTE_SIMPLE, ROUTE_RANDOM_WALK = 0, 1, 2, 3   # host/render_plan.hpp
GEO_TRI, GEO_GEN = 0, 1
IMG_NONE, IMG_TEX, IMG_ENV = 0, 1, 2
FLT_BOX, FLT_TRIANGLE, FLT_TABULATED, FLT_TABULATED_SIGNED = 0, 1, 2, 3
ENV = "environment_image(32)"  # (a scene keyword with this value gets scenes.environment_image(32))
CROP = (600, 496, 616, 512)    # 16 x 16 pixels, every coordinate above 255, tile-aligned


def cell(route, geo=GEO_TRI, img=IMG_NONE, img_lean=IMG_NONE, img_generate=IMG_NONE, flt=FLT_BOX, dl=0, lean_first=0, fused_from_0=0, split=0, divert_vertex=0,
         layered_onepass=0):
    return dict(zip(COORDS, (route, geo, img, img_lean, img_generate, flt, dl, lean_first, fused_from_0, split, divert_vertex, layered_onepass)))


CELLS = {
    # ---- the lean route: all-diffuse scenes, bounce 0 on known constants
    "lean": cell(ROUTE_LEAN, lean_first=1),
    "lean_env": cell(ROUTE_LEAN, img=IMG_ENV, img_lean=IMG_ENV, lean_first=1),
    "lean_general_env": cell(ROUTE_LEAN, geo=GEO_GEN, img=IMG_ENV, img_lean=IMG_ENV, lean_first=1),
    # ---- several BxDF classes, none coated: the material-sorted fused kernel from the camera ray on (plain-diffuse hits diverted to the lean kernel) ...
    "sorted_fused": cell(ROUTE_STAGED, lean_first=1, fused_from_0=1, divert_vertex=1),
    "staged": cell(ROUTE_STAGED, divert_vertex=1),            # ... from a later bounce or never (SHM_TAIL_FUSED_BOUNCE), and the coated scenes: k_vertex -> k_scatter<class>
    "fused_textured": cell(ROUTE_STAGED, img=IMG_TEX, img_generate=IMG_TEX, fused_from_0=1),
    "staged_textured": cell(ROUTE_STAGED, img=IMG_TEX, img_generate=IMG_TEX),
    "staged_textured_split": cell(ROUTE_STAGED, img=IMG_TEX, img_generate=IMG_TEX, split=1),
    "staged_env": cell(ROUTE_STAGED, img=IMG_ENV, img_lean=IMG_ENV, divert_vertex=1),
    "general": cell(ROUTE_STAGED, geo=GEO_GEN, lean_first=1, fused_from_0=1, divert_vertex=1),
    "general_staged": cell(ROUTE_STAGED, geo=GEO_GEN, divert_vertex=1),
    "general_env": cell(ROUTE_STAGED, geo=GEO_GEN, img=IMG_ENV, img_lean=IMG_ENV, lean_first=1, fused_from_0=1, divert_vertex=1),
    "general_textured": cell(ROUTE_STAGED, geo=GEO_GEN, img=IMG_TEX, img_generate=IMG_TEX, fused_from_0=1),
    # ---- the extended (*_dl) builds
    "lean_dl": cell(ROUTE_LEAN, dl=1, lean_first=1),
    "sorted_fused_dl": cell(ROUTE_STAGED, dl=1, lean_first=1, fused_from_0=1, divert_vertex=1),
    "staged_dl": cell(ROUTE_STAGED, dl=1, divert_vertex=1),
    "general_dl": cell(ROUTE_STAGED, geo=GEO_GEN, dl=1, lean_first=1, fused_from_0=1, divert_vertex=1),
    # ---- the other integrators
    "simple": cell(ROUTE_SIMPLE),
    "random_walk": cell(ROUTE_RANDOM_WALK),
    # ---- options.force_diffuse: the staged route whatever the scene, the LayeredBxDF class in one pass, no diversion and no fused kernel
    "force_diffuse": cell(ROUTE_STAGED, layered_onepass=1),
    # ---- pixel filters
    "lean_triangle": cell(ROUTE_LEAN, flt=FLT_TRIANGLE, lean_first=1),
    "lean_gaussian": cell(ROUTE_LEAN, flt=FLT_TABULATED, lean_first=1),
    "lean_mitchell": cell(ROUTE_LEAN, flt=FLT_TABULATED_SIGNED, lean_first=1),
    "staged_gaussian": cell(ROUTE_STAGED, flt=FLT_TABULATED, divert_vertex=1),
    "textured_mitchell": cell(ROUTE_STAGED, img=IMG_TEX, img_generate=IMG_TEX, flt=FLT_TABULATED_SIGNED),
}

Case = namedtuple("Case", "name scene scene_kw params env cell cut")


def case(name, scene, scene_kw, cell, cut=None, env=None, **params):
    params = dict(dict(seed=5, spp=4, max_depth=5), **params)
    return Case(name, scene, scene_kw, params, env or {}, cell, cut)


CORNELL = dict(width=24, height=24)
CROWN = dict(width=30, height=42, level=1, n_glass=6, n_gold=2)
COATED = dict(width=32, height=32, coated=True)

CASES = [
    # ---- scene classes under the default filter and sampler options
    case("lean", "cornell_box", CORNELL, "lean"),
    case("lean_env", "cornell_box", dict(CORNELL, environment=ENV), "lean_env"),
    case("sorted_fused", "crown_proxy", CROWN, "sorted_fused", max_depth=6),
    case("sorted_fused_from_bounce_3", "crown_proxy", CROWN, "staged", env={"SHM_TAIL_FUSED_BOUNCE": "3"}, max_depth=6),
    case("fused_textured", "cornell_box", dict(width=32, height=32, textured=True, textured_coated_ceiling=False), "fused_textured", max_depth=6),
    case("sorted_fused_never", "crown_proxy", CROWN, "staged", env={"SHM_TAIL_FUSED_BOUNCE": "-1"}, max_depth=6),  # the staged class kernels throughout
    case("staged_coated_divert", "cornell_box", COATED, "staged"),
    case("staged_coated_env", "cornell_box", dict(COATED, environment=ENV), "staged_env"),
    case("staged_textured", "cornell_box", dict(width=32, height=32, textured=True), "staged_textured", max_depth=6),
    case("staged_textured_split", "ganesha_proxy", dict(width=48, height=48, n=24, variant="textured_floor"), "staged_textured_split"),
    case("staged_textured_split_coated", "cornell_box", dict(width=32, height=32, textured=True), "staged_textured_split", env={"SHM_SPLIT_PASS": "1"}, max_depth=6),
    case("general_glass_patches", "cornell_box", dict(width=32, height=32, glass=True, patches=True), "general"),
    case("general_glass_patches_env", "cornell_box", dict(width=32, height=32, glass=True, patches=True, environment=ENV), "general_env"),
    case("general_textured", "cornell_box", dict(width=32, height=32, textured=True, textured_coated_ceiling=False, patches=True), "general_textured", max_depth=6),
    case("instances", "instanced_scene", dict(width=40, height=30), "general_staged"),
    case("spheres_env", "three_spheres", dict(width=40, height=30, camera=(0.75, 0.5, 9.0), environment=ENV), "lean_general_env"),
    case("random_scene_3", "random_scene", dict(seed=3), "general_staged", max_depth=6),
    # ---- the extended kernels and the other integrators
    case("dl_lean", "delta_lights:lean", {}, "lean_dl"),
    case("dl_sorted_fused", "delta_lights:sorted_fused", {}, "sorted_fused_dl", max_depth=6),
    case("dl_staged_coated", "delta_lights:staged_coated", {}, "staged_dl"),
    case("dl_general", "delta_lights:general", {}, "general_dl"),
    case("diffuse_transmission", "diffuse_transmission:beside_diffuse", {}, "sorted_fused_dl"),
    case("simplepath", "cornell_box", CORNELL, "simple", integrator="simplepath", max_depth=4),
    case("simplepath_no_lights", "cornell_box", CORNELL, "simple", integrator="simplepath", sample_lights=False, max_depth=4),
    case("simplepath_no_bsdf", "cornell_box", CORNELL, "simple", integrator="simplepath", sample_bsdf=False, max_depth=4),
    case("simplepath_neither", "cornell_box", CORNELL, "simple", integrator="simplepath", sample_lights=False, sample_bsdf=False, max_depth=4),
    case("randomwalk", "cornell_box", CORNELL, "random_walk", integrator="randomwalk", max_depth=4),
    case("lean_force_diffuse", "cornell_box", CORNELL, "force_diffuse", force_diffuse=True),
    case("staged_force_diffuse", "cornell_box", COATED, "force_diffuse", force_diffuse=True),
    case("lean_regularize", "cornell_box", CORNELL, "lean", regularize=True),
    case("staged_regularize", "cornell_box", COATED, "staged", regularize=True),
    # ---- pixel filters
    case("filter_triangle", "cornell_box", dict(CORNELL, film=dict(filter="triangle")), "lean_triangle"),
    case("filter_gaussian", "cornell_box", dict(CORNELL, film=dict(filter="gaussian")), "lean_gaussian"),
    case("filter_mitchell", "cornell_box", dict(CORNELL, film=dict(filter="mitchell")), "lean_mitchell"),
    case("filter_gaussian_staged", "cornell_box", dict(COATED, film=dict(filter="gaussian")), "staged_gaussian"),
    case("filter_mitchell_textured", "cornell_box", dict(width=32, height=32, textured=True, film=dict(filter="mitchell")), "textured_mitchell"),
    case("filter_gaussian_no_jitter", "cornell_box", dict(CORNELL, film=dict(filter="gaussian")), "lean", disable_pixel_jitter=True),  # falls back to FLT_BOX
    # ---- stream edges on the lean Cornell box (one pipeline: nothing else to agree with)
    case("spp_1", "cornell_box", CORNELL, "lean", spp=1),
    case("spp_2", "cornell_box", CORNELL, "lean", spp=2),
    case("spp_6", "cornell_box", CORNELL, "lean", spp=6),
    case("spp_8", "cornell_box", CORNELL, "lean", spp=8),
    case("spp_16", "cornell_box", CORNELL, "lean", spp=16),
    case("randomization_none", "cornell_box", CORNELL, "lean", randomization="none"),
    case("seed_high_bits", "cornell_box", CORNELL, "lean", seed=(0xa5 << 56) | (1 << 47) | (1 << 41) | 0x1234567),
    case("max_depth_0", "cornell_box", CORNELL, "lean", max_depth=0),
    case("no_wavelength_jitter", "cornell_box", CORNELL, "lean", disable_wavelength_jitter=True),
    case("quirks_off", "cornell_box", CORNELL, "lean", reference_quirks=False),
    # ---- Morton and digit-count edges
    case("crop_above_255", "cornell_box", dict(width=1024, height=768), "lean", cut="crop"),
    case("smaller_than_a_tile", "cornell_box", dict(width=5, height=3), "lean"),
    # ---- dimension depth: well over a hundred dimensions, a save / resume at every kernel boundary
    case("glass_depth_32", "cornell_box", dict(width=24, height=24, glass=True), "sorted_fused", max_depth=32),
    case("coated_depth_8", "cornell_box", dict(width=24, height=24, coated=True), "staged", max_depth=8),
    # ---- sample-index offsets
    case("waves_from_an_offset", "cornell_box", CORNELL, "lean", cut="waves", spp=8),
    case("waves_from_an_offset_staged", "cornell_box", COATED, "staged", cut="waves", spp=8),
    case("tile_subset", "cornell_box", CORNELL, "lean", cut="tiles"),
]
WAVES = [(0, 3), (3, 4), (4, 8)]  # of the "waves" rows (spp 8): no wave of the default schedule but the first starts where these do


def build_scene(lib, c):
    """The row's scene: a builder of shimmer_amd.scenes, or "<module>:<which>" for the class scenes of tests/test_gpu_delta_lights.py and
    tests/test_gpu_diffuse_transmission.py."""
    from shimmer_amd import scenes
    kw = {k: (scenes.environment_image(32) if isinstance(v, str) and v == ENV else v) for k, v in c.scene_kw.items()}
    if c.scene.startswith("delta_lights:"):
        import test_gpu_delta_lights
        return test_gpu_delta_lights.class_scene(lib, c.scene.split(":")[1])[0]
    if c.scene.startswith("diffuse_transmission:"):
        import test_gpu_diffuse_transmission
        return test_gpu_diffuse_transmission.class_scene(lib, c.scene.split(":")[1])
    if c.scene == "random_scene":
        return scenes.random_scene(lib, kw.pop("seed"), **kw)
    return getattr(scenes, c.scene)(lib, **kw)


def make_params(c):
    from shimmer_amd import render
    return render.make_params(sampler="zsobol", **c.params)


def knobs(c):
    """(SHM_SPLIT_PASS, SHM_TAIL_FUSED_BOUNCE) as orc_fn_render_plan's input columns read them: -1 for an unset split knob, a negative bounce for "never"."""
    return int(c.env.get("SHM_SPLIT_PASS", -1)), int(c.env.get("SHM_TAIL_FUSED_BOUNCE", 0))


def waves(c):
    return WAVES if c.cut == "waves" else None


def tile_rects(lib, c, pixel_bounds):
    """The tiles the row renders as (x0, y0, x1, y1) tuples, or None for all of them."""
    from shimmer_amd import scene as scn
    if c.cut == "crop":
        tiles, n = scn.tiles_for(lib, CROP)
    elif c.cut == "tiles":
        tiles, n = scn.tiles_for(lib, pixel_bounds)
    else:
        return None
    rects = [(tiles[i].x0, tiles[i].y0, tiles[i].x1, tiles[i].y1) for i in range(n)]
    return rects if c.cut == "crop" else rects[::3]


# ---- holding a device render to the oracle (the GPU tests) ----
STATS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")


def oracle_threads():
    import os
    return min(16, os.cpu_count() or 1)


def assert_equals_oracle(desc, p, f_gpu, s_gpu, what, **oracle_render_kw):
    """A device film (rgb_sum, weight_sum) and its seven counters against the CPU oracle's render of the same description and params, bit for bit.
    `oracle_render_kw`: Oracle.render's tiles / n_tiles / waves where the device render was cut up."""
    import numpy as np
    import oracle_py
    orc = oracle_py.Oracle(desc)
    try:
        f_cpu, s_cpu = orc.render(p, n_threads=oracle_threads(), **oracle_render_kw)
    finally:
        orc.close()
    for field in ("rgb_sum", "weight_sum"):
        assert np.array_equal(f_gpu[field], f_cpu[field]), (what, field)
    for k in STATS:
        assert s_gpu[k] == s_cpu[k], (what, k)
    assert np.isfinite(f_gpu["rgb_sum"]).all(), what
