"""host/render_plan.hpp — WHICH pipeline a scene and a render run, and the path workspace that needs — over the whole domain flatten_scene and ShmRenderParams can
produce, through the oracle library's orc_fn_render_plan (pure host code: no GPU). 2 654 208 (scene, knobs, render) combinations of integer logic.

What is asserted, per combination:
  * the workspace budget's bytes per path equal the sum over the allocation walk;
  * every array a planned stage touches is in the layout, and no array the plan's launchers would index is missing;
  * q_lean is drained exactly where something fills it, by exactly one filler;
  * no launcher coordinate names a null cell of the kernel table (the table's null pattern is exported as data), and the plan's own validation agrees;
  * the extended (*_dl) build runs for exactly the scenes with a distant / spot light or a diffuse transmission material.
"Present exactly when": the layout is the SCENE's, kept from render to render, so exactness is held over the renders of a scene — an array is present if and only if
some render of that scene touches it — for the auxiliary rays, rng0 / pixel0 and filter_weight. The staging arrays (bx, the class queues, q_lean, q_split) and the
lean kernel's e_* / q_emit are allocated by scene CLASS, as before the plan existed: every non-lean scene keeps them, also a scene whose every bounce the fused
all-materials kernel shades (SHM_TAIL_FUSED_BOUNCE=0 without coated materials). There the assertion is the safety half — touched implies present — and
test_staging_arrays_follow_the_scene_class pins the rule itself.

The traversal part of the plan — which row of the kernel table a scene's rays take, and the stack that row and the scene's tree need — is walked separately, through
orc_fn_trace_plan: the variant and strictness rules, the stack bound against the deepest leaf, and every row's LDS against the compute unit's.

The shading launchers' serving rule — which build of a launcher family serves which cell of render.hip's table (serving_build; the table is computed from it) — is
walked through orc_fn_shade_serving: its shape, its 44 builds, and that every launcher a plan of the domain above would call is served.

K1's and K6's rule — which camera-ray kernel builds exist, the filter class a plan's FLT_* runs, and where the film kernel takes a sample's weight from — is walked
through orc_fn_generate_rule (the tests at the end): its fixed points, its 36 builds, and that every plan of the domain lands on a build that exists."""
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
import oracle_py  # noqa: E402

ROUTE_LEAN, ROUTE_STAGED, ROUTE_SIMPLE, ROUTE_RANDOM_WALK = 0, 1, 2, 3
IMG_NONE, IMG_TEX, IMG_ENV = 0, 1, 2
NEVER = 1 << 30


def _filter_constants():
    import re
    text = (Path(__file__).resolve().parent.parent / "include" / "shimmer_hip.h").read_text()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"SHM_FILTER_(\w+)\s*=\s*(\d+)", text)}


def scene_rows():
    """Every class combination flatten_scene can produce x the two knobs: BxDF classes (every non-empty subset; diffuse_only only with the diffuse class alone) x
    material textures x image light x spheres x instances x extended build x plain-diffuse share (none / below a quarter / a quarter or more) x SHM_SPLIT_PASS
    (unset / 0 / 1) x SHM_TAIL_FUSED_BOUNCE (0 / 2 / never)."""
    classes = [(m, d) for m in range(1, 16) for d in (0, 1) if not (d and m != 1)]
    rows = []
    for (mask, donly), mt, il, sph, inst, ext, plain, split, tail in itertools.product(classes, (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2), (-1, 0, 1), (0, 2, -1)):
        rows.append((mask, donly, mt, il, sph, inst, ext, 1 if plain else 0, 1 if plain == 2 else 0, split, tail))
    return np.array(rows, np.int32)


def render_rows():
    """integrator x force_diffuse x sampler x disable_pixel_jitter x max_depth 0 / 5"""
    return np.array(list(itertools.product((0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 5))), np.int32)


@pytest.fixture(scope="module", params=["BOX", "TRIANGLE", "GAUSSIAN", "MITCHELL"])
def plans(request):
    """One pixel-filter class at a time (box / triangle / gaussian / Mitchell; a quarter of the domain each, 190 MB of columns): {class: the inputs and
    orc_fn_render_plan's outputs}, rows ordered scene-major."""
    fc = _filter_constants()
    sc, rr = scene_rows(), render_rows()
    S, R = len(sc), len(rr)
    out = {}
    for name in (request.param,):
        rows = np.empty((S * R, len(oracle_py.PLAN_IN)), np.int32)
        rows[:, 0:9] = np.repeat(sc[:, 0:9], R, axis=0)
        rows[:, 9] = fc[name]
        rows[:, 10:12] = np.repeat(sc[:, 9:11], R, axis=0)
        rows[:, 12:17] = np.tile(rr, (S, 1))
        res = oracle_py.render_plans(rows)
        res["in"] = {n: rows[:, i] for i, n in enumerate(oracle_py.PLAN_IN)}
        res["S"], res["R"] = S, R
        out[name] = res
    return out


def _present(p, name):
    return p["ws"][:, p["ws_names"].index(name)] != 0


def test_the_domain_is_whole(plans):
    (p,) = plans.values()
    assert p["S"] == 16 * 2 * 2 * 2 * 2 * 2 * 3 * 3 * 3 and p["R"] == 3 * 2 * 2 * 2 * 2
    assert len(p["route"]) * 4 == 2654208  # (x the four filter classes of the fixture)
    for q in plans.values():
        assert set(np.unique(q["route"])) == {ROUTE_LEAN, ROUTE_STAGED, ROUTE_SIMPLE, ROUTE_RANDOM_WALK}
        assert q["ws"].shape[1] == q["n_arrays"][0] == len(q["ws_names"]) == 35


def test_budget_is_the_sum_of_the_allocation_walk(plans):
    for q in plans.values():
        assert np.array_equal(q["budget"], q["ws"].sum(axis=1))
        assert q["budget"].min() >= 288 + 12  # the path state and the three queues every render has


def test_every_array_a_planned_stage_touches_is_in_the_layout(plans):
    for name, q in plans.items():
        i = q["in"]
        S, R = q["S"], q["R"]
        staged_bounce = (q["route"] == ROUTE_STAGED) & (q["fused_from"] > 0)   # bounce 0 exists in every render
        over_scene = lambda a: a.reshape(S, R)
        # auxiliary rays: exactly where the generate kernel is a HAS_TEX one
        for a in ("AUX0", "AUX1", "AUX2"):
            assert np.array_equal(_present(q, a), q["img_generate"] == IMG_TEX)
        # rng0 / pixel0: a lean_first render reads them; the scene holds them exactly when some render of it does
        for a in ("RNG0", "PIXEL0"):
            pr = _present(q, a)
            assert not np.any((q["lean_first"] != 0) & ~pr)
            assert np.array_equal(over_scene(pr).all(axis=1), over_scene(q["lean_first"] != 0).any(axis=1))
            assert np.array_equal(over_scene(pr).any(axis=1), over_scene(pr).all(axis=1))
        # q_lean: drained exactly where filled, by one filler; present wherever it is used
        fills = q["split"] + q["divert_vertex"]
        assert np.array_equal(fills, q["drain_lean"]) and fills.max() == 1
        assert not np.any((q["drain_lean"] != 0) & staged_bounce & ~_present(q, "Q_LEAN"))
        assert not np.any((q["drain_lean"] != 0) & (q["route"] != ROUTE_STAGED))
        # q_split: the split pass
        assert not np.any((q["split"] != 0) & ~_present(q, "Q_SPLIT"))
        assert not np.any((q["split"] != 0) & ~((q["split_pass"] != 0) & (i["force_diffuse"] == 0) & (q["route"] == ROUTE_STAGED)))
        # e_* and q_emit: a lean kernel, direct or diverted
        lean_kernel_runs = (q["route"] == ROUTE_LEAN) | ((q["drain_lean"] != 0) & staged_bounce)
        for a in ("E_RAY", "E_BETA", "E_CTX0", "E_CTX1", "E_CTX2", "E_FLAGS", "Q_EMIT"):
            assert not np.any(lean_kernel_runs & ~_present(q, a))
        # bx and the class queues: a staged bounce (the hit half writes the parameter block and pushes to the queue of every class the scene holds)
        assert not np.any(staged_bounce & ~_present(q, "BX"))
        for c in range(4):
            assert not np.any(staged_bounce & ((i["classes"] >> c) & 1 != 0) & ~_present(q, f"Q_SCATTER{c}"))
        # the staged kernels of a scene with textures carry ray differentials
        tex = (i["has_material_textures"] != 0) | (i["has_image_light"] != 0)
        for a in ("DD0", "DD1", "DD2"):
            assert not np.any((q["route"] == ROUTE_STAGED) & tex & ~_present(q, a))
        # filter_weight: the film kernel that reads per-sample weights; the scene holds it exactly when some render of it does
        pr = _present(q, "FILTER_WEIGHT")
        assert not np.any((q["film_per_sample"] != 0) & ~pr)
        assert np.array_equal(over_scene(pr).all(axis=1), over_scene(q["film_per_sample"] != 0).any(axis=1))
        assert pr.any() == (name == "MITCHELL")
        # what every render has
        for a in ("RAY", "HIT", "SHADOW_RAY", "SHADOW_CONTRIB", "L", "REC", "LAMBDA", "LAMBDA_PDF", "CTX", "Q_ACTIVE0", "Q_ACTIVE1", "Q_SHADOW"):
            assert _present(q, a).all()


def test_staging_arrays_follow_the_scene_class(plans):
    """Every non-lean scene keeps the staging arrays whether or not the render uses them; a lean scene has them exactly in a staged render (force_diffuse)."""
    for q in plans.values():
        i = q["in"]
        bx = _present(q, "BX")
        assert np.array_equal(bx, (q["lean"] == 0) | (q["route"] == ROUTE_STAGED))
        assert np.array_equal(_present(q, "Q_LEAN"), bx & (q["lean_divert"] != 0))
        assert np.array_equal(_present(q, "Q_SPLIT"), bx & (q["split_pass"] != 0))
        for c in range(4):
            assert np.array_equal(_present(q, f"Q_SCATTER{c}"), bx & ((i["classes"] >> c) & 1 != 0))
        assert np.array_equal(_present(q, "E_RAY"), (q["lean"] != 0) | (q["lean_divert"] != 0))


def test_no_launcher_coordinate_names_a_null_cell(plans):
    for q in plans.values():
        # the table's null pattern, as data: the textured image class has no lean kernels and no k_generate<., LEAN>
        has_lean = np.stack([q["has_lean_none"], q["has_lean_tex"], q["has_lean_env"]], axis=1)
        assert np.array_equal(has_lean[0], [1, 0, 1]) and (has_lean == has_lean[0]).all()
        rows = np.arange(len(q["route"]))
        calls_lean = (q["route"] == ROUTE_LEAN) | (q["drain_lean"] != 0)
        assert not np.any(calls_lean & (has_lean[rows, q["img_lean"]] == 0))
        assert not np.any((q["lean_first"] != 0) & (has_lean[rows, q["img_generate"]] == 0))
        assert not q["error"].any()
        for col, n in (("geo", 2), ("img", 3), ("img_lean", 3), ("img_generate", 3), ("flt", 4)):
            assert q[col].min() >= 0 and q[col].max() < n
        # the one-pass LayeredBxDF launcher has no K_ENV_LIGHT build: it runs under force_diffuse, where the image class is never env
        assert not np.any((q["layered_onepass"] != 0) & (q["img"] == IMG_ENV))


def test_extended_build_and_sampler_coordinates(plans):
    for name, q in plans.items():
        i = q["in"]
        assert np.array_equal(q["dl"], i["extended"])
        assert np.array_equal(q["zs"], i["sampler"])
        assert np.array_equal(q["geo"], i["has_spheres"])
        assert np.array_equal(q["flt"] != 0, (i["disable_pixel_jitter"] == 0) & (name != "BOX"))
        assert np.array_equal(q["layered_onepass"], i["force_diffuse"])


def test_routes_and_hit_record_forms(plans):
    (q,) = plans.values()
    i = q["in"]
    path = i["integrator"] == 0
    assert np.array_equal(q["route"] == ROUTE_STAGED, path & ((q["lean"] == 0) | (i["force_diffuse"] != 0)))
    assert np.array_equal(q["route"] == ROUTE_LEAN, path & (q["lean"] != 0) & (i["force_diffuse"] == 0))
    assert np.array_equal(q["route"] == ROUTE_RANDOM_WALK, i["integrator"] == 2)
    assert np.array_equal(q["hit16"] != 0, path & ~((i["has_spheres"] != 0) & (i["has_instances"] != 0)))
    assert np.array_equal(q["hit_split"] != 0, (q["hit16"] != 0) & (i["has_spheres"] != 0))
    assert np.array_equal(q["hit_kept"] != 0, (q["route"] == ROUTE_LEAN) & (q["hit16"] != 0) & (i["has_spheres"] == 0))
    # the fused all-materials kernel: never with coated materials, never under force_diffuse, from the knob's bounce on
    fused = q["fused_from"] != NEVER
    assert not np.any(fused & (((i["classes"] >> 3) & 1 != 0) | (i["force_diffuse"] != 0) | (q["route"] != ROUTE_STAGED)))
    assert np.array_equal(q["fused_from"][fused], np.where(i["tail_fused_bounce"][fused] < 0, NEVER, i["tail_fused_bounce"][fused]))


# ---- the traversal part of the plan (TRACE_SHAPES, ScenePlan::trace_variant / trace_spill_levels, RenderPlan::trace_any_strict) through orc_fn_trace_plan ----
TRACE_TRI, TRACE_GEN, TRACE_GEN_HEAVY = 0, 1, 2
CU_LDS_BYTES = 160 << 10  # MI355X: the LDS of one compute unit
STACK_LEVEL_BYTES = 256 * 8  # one stack level of a four-wave workgroup: 256 lanes x an 8-byte entry


@pytest.fixture(scope="module")
def trace_plans():
    """Every scene the traversal plan can see: spheres x instances x patch-heavy x quadric / patch x the deepest leaf 0 .. 63 (flatten_scene refuses deeper trees) x
    SHM_GEN_HEAVY (unset / 0 / 1) x disable_reference_quirks. 6 144 rows."""
    rows = np.array(list(itertools.product((0, 1), (0, 1), (0, 1), (0, 1), range(64), (-1, 0, 1), (0, 1))), np.int32)
    q = oracle_py.trace_plans(rows)
    q["in"] = {n: rows[:, i] for i, n in enumerate(oracle_py.TRACE_IN)}
    return q


def test_trace_variant_and_strictness_follow_their_rules(trace_plans):
    q, i = trace_plans, trace_plans["in"]
    assert len(q["variant"]) == 2 * 2 * 2 * 2 * 64 * 3 * 2
    heavy = (i["has_spheres"] != 0) & np.where(i["gen_heavy_knob"] >= 0, i["gen_heavy_knob"] != 0, i["patch_heavy"] != 0)
    assert np.array_equal(q["variant"], np.where(i["has_spheres"] == 0, TRACE_TRI, np.where(heavy, TRACE_GEN_HEAVY, TRACE_GEN)))
    assert set(np.unique(q["variant"])) == {TRACE_TRI, TRACE_GEN, TRACE_GEN_HEAVY}
    assert np.array_equal(q["strict"] != 0, (i["has_instances"] != 0) & (i["disable_reference_quirks"] != 0))


def test_trace_stack_holds_the_deepest_leaf(trace_plans):
    """The stack a kernel gets — its LDS levels and the HBM spill sized at scene creation — against the tree: a ray's stack holds at most one entry per level it
    descended, and the spill keeps one level beyond that. The STRICT any-hit kernels run on the any-hit side's spill: held to the same bound with their own LDS levels."""
    q, i = trace_plans, trace_plans["in"]
    depth = i["max_leaf_depth"]
    for kind in ("closest", "any"):
        lds, spill = q[f"lds_levels_{kind}"], q[f"spill_levels_{kind}"]
        assert np.array_equal(spill, np.maximum(0, depth + 1 - lds) + 1)
        assert np.all(lds + spill >= depth + 2) and spill.min() >= 1
    assert np.all(q["strict_lds_levels"] + q["spill_levels_any"] >= depth + 2)


def test_trace_rows_fit_the_lds_of_a_compute_unit(trace_plans):
    """Per variant and ray kind: waves per SIMD — one four-wave workgroup each — x (stack levels + save area) within the CU's 160 KiB."""
    q = trace_plans
    seen = set()
    for kind in ("closest", "any", "strict"):
        waves, levels, lds = (q[f"strict_{c}"] for c in ("waves", "lds_levels", "lds_bytes")) if kind == "strict" else (q[f"{c}_{kind}"] for c in ("waves", "lds_levels", "lds_bytes"))
        save = lds - levels * STACK_LEVEL_BYTES
        assert set(np.unique(save)) <= {0, 12 << 10}
        assert np.array_equal(save != 0, q["variant"] == TRACE_GEN_HEAVY)
        assert np.all(waves * lds <= CU_LDS_BYTES) and waves.min() >= 1 and levels.min() >= 1
        seen |= set(zip(q["variant"].tolist(), [kind] * len(waves), waves.tolist(), levels.tolist()))
    # the table itself, as data: every (variant, ray kind) has ONE row, whatever the scene's depth, flags and knobs
    rows = {(v, k): (w, l) for v, k, w, l in seen}
    assert len(rows) == len(seen) == 9
    assert rows[TRACE_TRI, "closest"] == (8, 9) and rows[TRACE_TRI, "any"] == (7, 11)
    assert rows[TRACE_GEN, "closest"] == rows[TRACE_GEN, "any"] == (7, 11)
    assert rows[TRACE_GEN_HEAVY, "closest"] == rows[TRACE_GEN_HEAVY, "any"] == (5, 9)


def test_strict_kernels_take_the_general_any_hit_row(trace_plans):
    """k_trace5_any_strict<heavy> is compiled from the GEN / GEN_HEAVY any-hit row, and launched on the grid and spill of the scene's own any-hit row: wherever a
    render can be strict, the two rows are one."""
    q = trace_plans
    gen_any = {v: (int(q["waves_any"][q["variant"] == v][0]), int(q["lds_levels_any"][q["variant"] == v][0]), int(q["lds_bytes_any"][q["variant"] == v][0]))
               for v in (TRACE_GEN, TRACE_GEN_HEAVY)}
    want = np.array([gen_any[TRACE_GEN_HEAVY if v == TRACE_GEN_HEAVY else TRACE_GEN] for v in q["variant"]], np.int32)
    assert np.array_equal(np.stack([q["strict_waves"], q["strict_lds_levels"], q["strict_lds_bytes"]], axis=1), want)
    s = q["strict"] != 0
    assert s.any()
    assert np.array_equal(q["strict_waves"][s], q["waves_any"][s]) and np.array_equal(q["strict_lds_levels"][s], q["lds_levels_any"][s])


# ---- the shading launchers' serving rule (serving_build: family x geo x img -> the build that serves the cell) through orc_fn_shade_serving ----
GEO_TRI, GEO_GEN = 0, 1
FAMILY_BUILDS = {"LEAN": 4, "LEAN_DIVERTED": 4, "FUSED_ALL": 6, "VERTEX": 5, "SCATTER_DIFFUSE": 5, "SCATTER_CONDUCTOR": 5, "SCATTER_DIELECTRIC": 5, "SCATTER_LAYERED": 5,
                 "SCATTER_LAYERED_ONEPASS": 3, "SIMPLE": 1, "RANDOMWALK": 1}


@pytest.fixture(scope="module")
def serving():
    names, table = oracle_py.shade_serving()
    return {name: table[f] for f, name in enumerate(names)}  # [geo][img] -> (geo', img')


def test_serving_rule_names_builds_that_serve_themselves(serving):
    assert list(serving) == list(FAMILY_BUILDS)
    for name, t in serving.items():
        assert t.shape == (2, 3, 2)
        for g, i in itertools.product(range(2), range(3)):
            bg, bi = (int(v) for v in t[g, i])
            if (bg, bi) == (-1, -1):
                continue
            assert 0 <= bg < 2 and 0 <= bi < 3, (name, g, i)
            assert tuple(t[bg, bi]) == (bg, bi), (name, g, i)  # a build serves the cell it is named after


def test_serving_rule_has_the_44_builds(serving):
    builds = {name: {tuple(int(v) for v in t[g, i]) for g, i in itertools.product(range(2), range(3))} - {(-1, -1)} for name, t in serving.items()}
    assert {name: len(b) for name, b in builds.items()} == FAMILY_BUILDS
    assert sum(len(b) for b in builds.values()) == 44


def test_serving_rule_is_null_exactly_where_there_is_no_lean_kernel(serving, plans):
    (q,) = plans.values()
    has_lean = [int(q["has_lean_none"][0]), int(q["has_lean_tex"][0]), int(q["has_lean_env"][0])]
    assert has_lean == [1, 0, 1]
    for name, t in serving.items():
        for g, i in itertools.product(range(2), range(3)):
            null = tuple(t[g, i]) == (-1, -1)
            assert null == (name in ("LEAN", "LEAN_DIVERTED") and not has_lean[i]), (name, g, i)
            if name in ("LEAN", "LEAN_DIVERTED") and not null:
                assert tuple(t[g, i]) == (g, i)  # its own build


def test_one_pass_layered_family_has_no_env_build(serving):
    t = serving["SCATTER_LAYERED_ONEPASS"]
    assert not np.any(t[:, :, 1] == IMG_ENV)
    for g in range(2):
        assert tuple(t[g, IMG_ENV]) == (g, IMG_NONE)  # the env cells: the build without the light, of the same geometry
        assert tuple(t[g, IMG_TEX]) == (GEO_GEN, IMG_TEX)


def test_every_launcher_a_plan_calls_has_a_serving_build(serving, plans):
    """render.hip's kernels_complete on the plan's columns: select_kernels takes the lean launchers at (geo, img_lean), everything else at (geo, img), and puts the
    one-pass LayeredBxDF launcher in the class's place where the plan says so."""
    served = {name: t[:, :, 0] >= 0 for name, t in serving.items()}  # [geo][img]
    for q in plans.values():
        i = q["in"]
        geo, img, img_lean = q["geo"], q["img"], q["img_lean"]
        at = lambda name, im: served[name][geo, im]
        staged0 = (q["route"] == ROUTE_STAGED) & (q["fused_from"] > 0)  # RenderPlan::staged_bounce(0)
        missing = (q["route"] == ROUTE_LEAN) & ~at("LEAN", img_lean)
        missing |= (q["route"] == ROUTE_SIMPLE) & ~at("SIMPLE", img)
        missing |= (q["route"] == ROUTE_RANDOM_WALK) & ~at("RANDOMWALK", img)
        missing |= (q["route"] == ROUTE_STAGED) & (q["fused_from"] != NEVER) & ~at("FUSED_ALL", img)
        missing |= staged0 & ~at("VERTEX", img)
        missing |= staged0 & (q["drain_lean"] != 0) & ~at("LEAN_DIVERTED", img_lean)
        for c, name in enumerate(("SCATTER_DIFFUSE", "SCATTER_CONDUCTOR", "SCATTER_DIELECTRIC")):
            missing |= staged0 & ((i["classes"] >> c) & 1 != 0) & ~at(name, img)
        layered = np.where(q["layered_onepass"] != 0, at("SCATTER_LAYERED_ONEPASS", img), at("SCATTER_LAYERED", img))
        missing |= staged0 & ((i["classes"] >> 3) & 1 != 0) & ~layered
        assert not missing.any()
        assert staged0.any() and (q["route"] == ROUTE_LEAN).any() and (q["drain_lean"] != 0).any()


# ---- K1's and K6's rule (has_generate_build, generate_filter_class, film_weight: the plan's coordinates -> the camera-ray kernel and the film kernel) through orc_fn_generate_rule ----
FLT_BOX, FLT_TRIANGLE, FLT_TABULATED, FLT_TABULATED_SIGNED = (oracle_py.FLT.index(n) for n in ("BOX", "TRIANGLE", "TABULATED", "TABULATED_SIGNED"))


@pytest.fixture(scope="module")
def generate_rule():
    t = oracle_py.generate_rule()  # [tex][lean][flt] -> (exists, filter class, film weight)
    assert t.shape == (2, 2, 4, 3) and t.min() >= 0
    return t


def test_generate_rule_fixed_points(generate_rule):
    t = generate_rule
    for tex, lean in itertools.product(range(2), range(2)):  # the filter class and the film weight go by the plan's filter class alone
        assert [oracle_py.FILTER_CLASS[c] for c in t[tex, lean, :, 1]] == ["BOX", "TRIANGLE", "TABULATED", "TABULATED"]
        assert [oracle_py.FILM_WEIGHT[w] for w in t[tex, lean, :, 2]] == ["ONE", "ONE", "CONSTANT", "PER_SAMPLE"]
        assert len(set(t[tex, lean, :, 0])) == 1  # ... and whether a build exists by (tex, lean) alone


def test_generate_rule_has_the_36_builds(generate_rule, plans):
    t = generate_rule
    builds = {(tex, lean, int(t[tex, lean, flt, 1])) for tex, lean, flt in itertools.product(range(2), range(2), range(4)) if t[tex, lean, flt, 0]}
    assert len(builds) == 9 and len(builds) * 2 * 2 == 36  # x camera (perspective / orthographic, spherical) x sampler
    empty = {(tex, lean) for tex, lean in itertools.product(range(2), range(2)) if not t[tex, lean, :, 0].any()}
    assert empty == {(1, 1)}  # lean with image textures, and nothing else: the textured class has no lean kernels
    (q,) = plans.values()
    assert bool(t[1, 1, 0, 0]) == bool(q["has_lean_tex"][0]) and bool(t[0, 1, 0, 0]) == bool(q["has_lean_none"][0])  # read from HAS_LEAN_KERNELS


def test_every_plan_lands_on_a_generate_build_and_its_film_kernel(generate_rule, plans):
    t = generate_rule
    for name, q in plans.items():
        i = q["in"]
        assert not np.any(q["img_generate"] == IMG_ENV)
        tex, lean, flt = (q["img_generate"] == IMG_TEX).astype(int), (q["lean_first"] != 0).astype(int), q["flt"]
        assert t[tex, lean, flt, 0].all()
        assert np.array_equal(q["film_per_sample"] != 0, t[tex, lean, flt, 2] == oracle_py.FILM_WEIGHT.index("PER_SAMPLE"))
        assert not np.any((flt != FLT_BOX) & ((i["disable_pixel_jitter"] != 0) | (name == "BOX")))
        assert set(np.unique(flt)) == {"BOX": {FLT_BOX}, "TRIANGLE": {FLT_BOX, FLT_TRIANGLE}, "GAUSSIAN": {FLT_BOX, FLT_TABULATED}, "MITCHELL": {FLT_BOX, FLT_TABULATED_SIGNED}}[name]
