"""PBRT-v4's diffuse transmission material on the device: every shading pipeline that can meet it — the material-sorted fused kernels, the staged k_vertex ->
k_scatter_diffuse pair beside a coated material, the lean diversion beside it (and with nothing to divert), the general-geometry, textured and environment builds,
the other integrators — against the CPU oracle bit for bit (film, weight_sum, the seven counters); ZSobol against the oracle too, by decomposition invariance and by
the pipelines agreeing with each other; the leaf probe on tests/test_diffuse_transmission.py's vectors; and a scene without the material, which renders the film
the parent commit rendered. A scene with the material runs the extended (*_dl) kernel set (wavefront.h)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_py
import test_diffuse_transmission as dt
import zsobol_cases as zc
from shimmer_amd import abi, render, scene as scn, scenes

pytestmark = pytest.mark.gpu
STATS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")
CORNELL_LIGHTS = dict(spot_from=(0.5, 1.7, 0.8), spot_to=(-0.2, 0.3, -0.2), sun_from=(0.3, 0.4, 3.0), sun_to=(0.0, 0.8, 0.0))
N = 32
leaf = dt.leaf  # (the fixture: shm/probe.h's leaf_probe compiled for the host)


def class_scene(lib, which, width=N, height=N):
    c = lambda words, **kw: scenes.cornell_box(lib, width, height, diffuse_transmission=words, **kw)  # noqa: E731
    if which == "sorted_fused":   # triangles only: the material beside a gold conductor and a rough glass wall, no plain diffuse material, no coated one
        return c("all gold", glass_too=True)
    if which == "only":           # the material alone: the lean diversion is on and diverts nothing
        return c("all")
    if which == "beside_diffuse":  # ... beside plain DiffuseMaterials: their hits are diverted to the lean kernel, the sheet's and the tall box's are not
        return c("sheet tall")
    if which == "gen":            # a sphere and bilinear patches: the general-geometry builds
        return c("sheet sphere", patches=True)
    if which == "tex":            # an image texture on the transmittance, a checkerboard on the reflectance, a scale on both: the textured builds, auxiliary rays
        return c("sheet textured")
    if which == "env":            # under an environment map: the *_env builds
        return c("sheet tall", environment=scenes.environment_image(32))
    if which == "staged_coated":  # beside coated boxes: k_vertex -> k_scatter_diffuse for the sheet, the lean diversion for the walls
        return c("sheet", coated=True)
    if which == "staged_coated_only":  # ... and with no plain diffuse material beside them
        return c("sheet all", coated=True)
    if which == "delta_lights":
        return c("sheet tall", extra_lights=scenes.spot_and_distant(**CORNELL_LIGHTS))
    if which == "instanced":
        return scenes.instanced_scene(lib, 40, 30, diffuse_transmission=True)
    assert which == "mix"         # both children of a MixMaterial
    return c("sheet mixed")


CLASSES = ["sorted_fused", "only", "beside_diffuse", "gen", "tex", "env", "staged_coated", "staged_coated_only", "delta_lights", "instanced", "mix"]


def gpu_render(lib, desc, p):
    g = render.Renderer(lib, desc, 0)
    out = g.render(p)
    g.close()
    return out


def assert_equals_oracle(lib, sc, p, what):
    assert any(m.kind == abi.SHM_MATERIAL_DIFFUSE_TRANSMISSION for m in sc.builder.materials), what
    f_gpu, s_gpu = gpu_render(lib, sc.desc, p)
    orc = oracle_py.Oracle(sc.desc)
    f_cpu, s_cpu = orc.render(p, n_threads=min(16, os.cpu_count() or 1))
    orc.close()
    for field in ("rgb_sum", "weight_sum"):
        assert np.array_equal(f_gpu[field], f_cpu[field]), (what, field)
    for k in STATS:
        assert s_gpu[k] == s_cpu[k], (what, k)
    assert np.isfinite(f_gpu["rgb_sum"]).all() and f_gpu["rgb_sum"].max() > 0
    return f_gpu, s_gpu


@pytest.mark.parametrize("which", CLASSES)
def test_film_and_counters_equal_the_oracle(gpu_lib, which):
    sc = class_scene(gpu_lib, which)
    assert_equals_oracle(gpu_lib, sc, render.make_params(seed=13, spp=4, max_depth=5), which)


def test_the_material_is_what_is_rendered(gpu_lib):
    """The sheet transmits: the film with it differs from the film of the same scene whose sheet only reflects, in the pixels that see the sheet."""
    p = render.make_params(seed=13, spp=4, max_depth=5)
    sc = class_scene(gpu_lib, "beside_diffuse")
    f, _ = gpu_render(gpu_lib, sc.desc, p)
    sheet = max(i for i, m in enumerate(sc.builder.materials) if m.kind == abi.SHM_MATERIAL_DIFFUSE_TRANSMISSION)
    sc.builder.materials[sheet].b = sc.builder.spectrum_constant(0.0)
    desc, _ = sc.builder.build(gpu_lib)
    g, _ = gpu_render(gpu_lib, desc, p)
    assert not np.array_equal(f["rgb_sum"], g["rgb_sum"])


@pytest.mark.parametrize("integrator, lights, bsdf", [("simplepath", True, True), ("simplepath", True, False), ("simplepath", False, True), ("simplepath", False, False),
                                                      ("randomwalk", True, True)])
def test_the_other_integrators_equal_the_oracle(gpu_lib, integrator, lights, bsdf):
    for which in ("beside_diffuse", "tex"):
        p = render.make_params(seed=3, spp=4, max_depth=4, integrator=integrator, sample_lights=lights, sample_bsdf=bsdf)
        assert_equals_oracle(gpu_lib, class_scene(gpu_lib, which), p, (which, integrator, lights, bsdf))


@pytest.mark.parametrize("kw", [dict(reference_quirks=False), dict(force_diffuse=True), dict(regularize=True)], ids=["quirks_off", "force_diffuse", "regularize"])
def test_render_options(gpu_lib, kw):
    for which in ("sorted_fused", "staged_coated"):
        assert_equals_oracle(gpu_lib, class_scene(gpu_lib, which), render.make_params(seed=17, spp=4, max_depth=5, **kw), (which, kw))


def test_a_film_smaller_than_a_tile(gpu_lib):
    """5 x 3 pixels: one partial tile, a partial wave."""
    for which in ("beside_diffuse", "staged_coated"):
        assert_equals_oracle(gpu_lib, class_scene(gpu_lib, which, 5, 3), render.make_params(seed=5, spp=4, max_depth=5), which)


@pytest.mark.parametrize("which", ["beside_diffuse", "staged_coated"])
def test_zsobol_decomposition_invariance_and_the_pipelines_agree(gpu_lib, which, monkeypatch):
    """As tests/test_gpu_zsobol.py does, the *_zs_dl kernels are held to the oracle's film and counters, to a film that does not depend on how the work is cut up, and the
    staged pipeline from the camera ray on (SHM_TAIL_FUSED_BOUNCE=-1) to the same bits and counters as the default."""
    sc = class_scene(gpu_lib, which)
    p = render.make_params(seed=21, spp=8, max_depth=5, sampler="zsobol")
    gpu = render.Renderer(gpu_lib, sc.desc, 0)
    f1, s1 = gpu.render(p)
    f2, _ = gpu.render(p)
    assert np.array_equal(f1, f2) and (f1["weight_sum"] == 8.0).all() and np.isfinite(f1["rgb_sum"]).all()
    zc.assert_equals_oracle(sc.desc, p, f1, s1, which)
    f_ind, _ = gpu.render(render.make_params(seed=21, spp=8, max_depth=5))
    assert not np.array_equal(f1, f_ind)
    gpu.clear()
    idx = np.arange(gpu.n_tiles)
    for ws, we in scn.wave_schedule(8):
        gpu.render_waves(p, tile_indices=idx[idx % 3 != 0], waves=[(ws, we)])
        gpu.render_waves(p, tile_indices=idx[idx % 3 == 0], waves=[(ws, we)])
    assert np.array_equal(gpu.read_film(), f1)
    gpu.clear()
    gpu.render_device(p)
    assert np.array_equal(gpu.read_film(), f1)
    gpu.close()
    monkeypatch.setenv("SHM_TAIL_FUSED_BOUNCE", "-1")
    f3, s3 = gpu_render(gpu_lib, sc.desc, p)
    monkeypatch.delenv("SHM_TAIL_FUSED_BOUNCE")
    assert np.array_equal(f3, f1)
    for k in STATS:
        assert s3[k] == s1[k], k
    # ... and the image is the independent sampler's in the mean (margin and sample counts of tests/test_gpu_delta_lights.py's check of the same kind)
    a = render.film_to_rgb(gpu_render(gpu_lib, sc.desc, render.make_params(seed=2, spp=64, max_depth=5, sampler="zsobol"))[0]).mean()
    c = render.film_to_rgb(gpu_render(gpu_lib, sc.desc, render.make_params(seed=2, spp=64, max_depth=5))[0]).mean()
    assert abs(a / c - 1.0) < 0.05, (a, c)


def test_the_pipelines_agree_with_the_independent_sampler_too(gpu_lib, monkeypatch):
    p = render.make_params(seed=9, spp=4, max_depth=5)
    for which in ("sorted_fused", "only", "gen", "tex", "env"):
        sc = class_scene(gpu_lib, which)
        f0, s0 = gpu_render(gpu_lib, sc.desc, p)
        monkeypatch.setenv("SHM_TAIL_FUSED_BOUNCE", "-1")  # k_vertex -> k_scatter_diffuse from the camera ray on, instead of the fused all-materials kernel
        f1, s1 = gpu_render(gpu_lib, sc.desc, p)
        monkeypatch.delenv("SHM_TAIL_FUSED_BOUNCE")
        assert np.array_equal(f0, f1), which
        for k in STATS:
            assert s0[k] == s1[k], (which, k)


def test_the_probe_replays_the_leaf_vectors(gpu_lib, leaf):
    """The grid of tests/test_diffuse_transmission.py's float64 comparison through the device's own bxdf_f / bxdf_pdf / bxdf_sample_f: bit-equal to the host's."""
    plib = abi.load_probe_library()
    vec = dt.leaf_vectors()
    jobs = dt.leaf_jobs((leaf.op_sample, leaf.op_f_pdf), vec)
    host = leaf.run(jobs)
    for (op, words), (ok_h, out_h) in zip(jobs, host):
        a = (C.c_uint32 * len(words))(*words)
        out = (C.c_uint32 * 10)()
        res = C.c_int()
        abi.check(plib, plib.shm_debug_eval_leaf(0, op, a, len(words), out, 10, C.byref(res)), "shm_debug_eval_leaf")
        assert res.value == ok_h
        n = (10 if ok_h else 0) if op == leaf.op_sample else 6
        assert np.array_equal(np.frombuffer(bytes(out), np.uint32)[:n], out_h.view(np.uint32)[:n]), words


def test_a_scene_without_the_material_renders_what_it_rendered(gpu_lib):
    """Before / after: the Cornell box and the S3 proxy render the films that the parent commit rendered (tests/golden/diffuse_transmission_before.json: its CPU oracle,
    which its device path equals bit for bit) — through the kernels built without the material, which are instruction-identical to that library's."""
    import sys
    sys.path.insert(0, str(dt.ROOT / "tests" / "golden"))
    import gen_diffuse_transmission_before as gen
    before = json.loads((dt.ROOT / "tests" / "golden" / "diffuse_transmission_before.json").read_text())
    for case in before["films"]:
        sc = gen.scene(gpu_lib, case["scene"])
        f, st = gpu_render(gpu_lib, sc.desc, render.make_params(seed=case["seed"], spp=case["spp"], max_depth=case["max_depth"]))
        assert hashlib.sha256(np.ascontiguousarray(f).tobytes()).hexdigest() == case["sha256"], case["scene"]
        assert [st[k] for k in STATS] == case["stats"], case["scene"]
