"""Every camera-ray kernel (K1) and every film kernel (K6) on the device, cell by cell: the grid camera x scene class x sampler x pixel filter — 48 small renders, which
between them launch each of the 36 k_generate / k_generate_filtered builds (wf_generate, k_generate.inl) and the three film kernels (launch_film, render.hip) — each
held to the CPU oracle bit for bit: film sums, weight sums and the seven counters. A launcher table with a wrong cell cannot pass: another camera, sampler or filter
class changes the film; a lean K1 in front of a consumer that is not (or the reverse) reads arrays nobody wrote; the box film kernel behind a tabulated K1 leaves
weight_sum = spp where the oracle has spp * K.

The CPU test of this module (no GPU: the plan through the oracle library) holds the grid to the rule of host/render_plan.hpp: every case lands on the cell its place
in the grid says, and together the cases cover every build the rule names.

The film is 33 x 17: ragged, so that the last workgroup is partial and tiles are cut."""
import itertools

import pytest

import oracle_py
import zsobol_cases as zc
from shimmer_amd import abi, render, scenes

WIDTH, HEIGHT, SPP, DEPTH = 33, 17, 4, 2
CAMERAS = ["perspective", "spherical"]
# class -> (cornell_box keywords, K1's HAS_TEX, K1's LEAN)
CLASSES = {"lean": (dict(), 0, 1), "plain": (dict(coated=True), 0, 0), "textured": (dict(textured=True), 1, 0)}
SAMPLERS = ["independent", "zsobol"]
# filter -> (the plan's FLT_*, K1's filter class, K6's weight)
FILTERS = {None: ("BOX", "BOX", "ONE"), "triangle": ("TRIANGLE", "TRIANGLE", "ONE"), "gaussian": ("TABULATED", "TABULATED", "CONSTANT"),
           "mitchell": ("TABULATED_SIGNED", "TABULATED", "PER_SAMPLE")}


def case_scene(lib, camera, which, filter_name):
    """The Cornell box of the class under its own perspective camera, or under an equal-area spherical one that stands inside it (camera and positions as
    tests/test_gpu_spherical_camera.py's class_scene)."""
    cam = dict(type="spherical", mapping="equalarea", pos=(0.1, 1.1, 0.4), look_at=(0, 1, -1)) if camera == "spherical" else None
    film = dict(film=dict(filter=filter_name)) if filter_name else {}
    return scenes.cornell_box(lib, WIDTH, HEIGHT, camera=cam, **CLASSES[which][0], **film)


def case_params(sampler):
    return render.make_params(seed=17, spp=SPP, max_depth=DEPTH, sampler=sampler)


def test_the_grid_covers_every_generate_build_and_film_kernel(lib):
    """Each of the 48 cases through scene_facts and render_plan (host/render_plan.hpp, the code shm_render_wave runs) and the K1 / K6 rule: it lands on the build its
    place in the grid declares; two cases share a K1 build only where they differ in gaussian / Mitchell; and the cases cover every build the rule says exists, for
    both cameras and samplers, and the three film kernels."""
    rule = oracle_py.generate_rule()  # [tex][lean][flt] -> (exists, filter class, film weight)
    landed = {}
    for camera, which, filter_name in itertools.product(CAMERAS, CLASSES, FILTERS):
        sc = case_scene(lib, camera, which, filter_name)  # (kept: the description points into the builder's arrays)
        assert (sc.desc.camera.kind == abi.SHM_CAMERA_SPHERICAL) == (camera == "spherical")  # (the plan rows carry no camera column: RenderPlan::spherical is this)
        o = oracle_py.Oracle(sc.desc)
        facts = o.scene_facts()
        assert (o.width, o.height) == (WIDTH, HEIGHT)
        o.close()
        for sampler in SAMPLERS:
            p = case_params(sampler)
            row = dict(facts, split_knob=-1, tail_fused_bounce=0, integrator=p.integrator, force_diffuse=p.force_diffuse, sampler=p.sampler,
                       disable_pixel_jitter=p.disable_pixel_jitter, max_depth=p.max_depth)
            plan = oracle_py.render_plans([[row[k] for k in oracle_py.PLAN_IN]])
            got = {k: int(plan[k][0]) for k in oracle_py.PLAN_OUT}
            assert got["error"] == 0
            tex, lean, flt = int(got["img_generate"] == 1), got["lean_first"], got["flt"]
            exists, fc, weight = (int(v) for v in rule[tex, lean, flt])
            what = (camera, which, sampler, filter_name)
            assert exists, what
            _, want_tex, want_lean = CLASSES[which]
            want_flt, want_fc, want_weight = FILTERS[filter_name]
            assert (tex, lean, got["zs"]) == (want_tex, want_lean, SAMPLERS.index(sampler)), what
            assert (oracle_py.FLT[flt], oracle_py.FILTER_CLASS[fc], oracle_py.FILM_WEIGHT[weight]) == (want_flt, want_fc, want_weight), what
            landed[what] = ((camera, got["zs"], tex, lean, fc), weight)
    assert len(landed) == 48
    for a, b in itertools.combinations(landed, 2):  # pairwise: the same K1 build only for the two tabulated filters of one (camera, class, sampler)
        assert (landed[a][0] == landed[b][0]) == (a[:3] == b[:3] and {a[3], b[3]} == {"gaussian", "mitchell"}), (a, b)
    builds = {(camera, zs, tex, lean, int(rule[tex, lean, flt, 1])) for camera, zs, tex, lean, flt in itertools.product(CAMERAS, range(2), range(2), range(2), range(4))
              if rule[tex, lean, flt, 0]}
    assert len(builds) == 36 and {k1 for k1, _ in landed.values()} == builds
    assert {w for _, w in landed.values()} == set(range(len(oracle_py.FILM_WEIGHT)))


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(CLASSES))
@pytest.mark.parametrize("camera", CAMERAS)
def test_every_cell_equals_the_oracle(gpu_lib, camera, which):
    for filter_name in FILTERS:
        sc = case_scene(gpu_lib, camera, which, filter_name)
        g = render.Renderer(gpu_lib, sc.desc, 0)
        try:
            for sampler in SAMPLERS:
                p = case_params(sampler)
                f, s = g.render(p)
                zc.assert_equals_oracle(sc.desc, p, f, s, (camera, which, sampler, filter_name))
                assert f["rgb_sum"].max() > 0
        finally:
            g.close()
