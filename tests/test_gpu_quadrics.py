"""PBRT-v4's disk and cylinder (ShmSphere.quadric) on the device: the six traversal kernels of k_trace_quadrics.hip and the extended (*_dl) shading kernels of every scene
class the general kernels serve, against the CPU oracle bit for bit — film and the seven counters —; the STRICT any-hit pair, both samplers, the other integrators and
the pipeline knobs; the leaf probes on the records of tests/quadric_cases.py; and the films of scenes without such a shape as the parent commit rendered them.
Films are at most 48 x 48 at 8 spp or fewer. (Which kernels a run of this file launches is what tools/kernel_coverage.py shows of a kernel trace: profiles/quadrics.md.)"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import oracle_py
import quadric_cases as qc
import zsobol_cases as zc
from device_leaves import DeviceLeaves, _fl, _f, _struct_words
from shimmer_amd import abi, render, scene as scn, scenes
from test_quadrics import ROOT, fa, one_shape_scene

sys.path.insert(0, str(ROOT / "tests" / "golden"))
pytestmark = pytest.mark.gpu
STATS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")
VARIANTS = ["lean", "glass", "coated", "textured", "environment", "instances", "many_disks"]
TRACE_GEN, TRACE_GEN_HEAVY = 1, 2  # (host/render_plan.hpp)
F = C.c_float


def gpu_render(lib, desc, p):
    g = render.Renderer(lib, desc, 0)
    out = g.render(p)
    g.close()
    return out


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


def scene_of(lib, variant, **kw):
    return scenes.quadric_scene(lib, variant, 40, 32, **kw)


def leaf_holds_a_quadric_with_triangles(desc):
    for i in range(desc.n_nodes):
        nd = desc.nodes[i]
        if nd.n_prims > 1:
            kinds = {desc.primitives[nd.offset + k].shape_kind for k in range(nd.n_prims)}
            if abi.SHM_SHAPE_SPHERE in kinds and abi.SHM_SHAPE_TRIANGLE in kinds:
                return True
    return False


@pytest.mark.parametrize("gen_heavy", [None, "0"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_film_and_counters_equal_the_oracle(gpu_lib, monkeypatch, variant, gen_heavy):
    """Every scene class, on both general rows of the traversal table: these small scenes are quadrics by a twelfth of their records or more, so they take the five-wave
    row by themselves (asserted for the many-disks scene); SHM_GEN_HEAVY=0 puts the same scenes on the seven-wave row."""
    sc = scene_of(gpu_lib, variant)
    assert leaf_holds_a_quadric_with_triangles(sc.desc)
    kinds = {s.quadric for s in sc.builder.spheres}
    assert kinds == {abi.SHM_QUADRIC_DISK, abi.SHM_QUADRIC_CYLINDER} and any(l.kind == abi.SHM_LIGHT_DIFFUSE_AREA for l in sc.builder.lights)
    o = oracle_py.Oracle(sc.desc)
    plan, facts = o.trace_plan(gen_heavy_knob=-1 if gen_heavy is None else int(gen_heavy)), o.scene_facts()
    o.close()
    assert facts["extended"] == 1 and facts["has_spheres"] == 1 and facts["has_instances"] == (variant == "instances")
    assert plan["variant"] == (TRACE_GEN_HEAVY if gen_heavy is None else TRACE_GEN)
    monkeypatch.delenv("SHM_GEN_HEAVY", raising=False)
    if gen_heavy is not None:
        monkeypatch.setenv("SHM_GEN_HEAVY", gen_heavy)
    p = render.make_params(seed=13, spp=4, max_depth=5)
    f_gpu, s_gpu = gpu_render(gpu_lib, sc.desc, p)
    f_cpu, s_cpu = oracle_render(sc, (variant, "path", 13), p)
    assert_equals(f_gpu, s_gpu, f_cpu, s_cpu, (variant, gen_heavy))
    assert f_gpu["rgb_sum"].max() > 0 and s_gpu["rays_any"] > 0
    # the byte is read: the same records as spheres render another film
    f_sph, _ = gpu_render(gpu_lib, scene_of(gpu_lib, variant, as_spheres=True).desc, p)
    assert not np.array_equal(f_sph["rgb_sum"], f_gpu["rgb_sum"])


@pytest.mark.parametrize("gen_heavy", [None, "0"])
def test_the_strict_any_hit_pair(gpu_lib, monkeypatch, gen_heavy):
    """Instances under disable_reference_quirks: the shadow rays take k_trace5_quadrics_any_strict (five and seven waves)."""
    monkeypatch.delenv("SHM_GEN_HEAVY", raising=False)
    if gen_heavy is not None:
        monkeypatch.setenv("SHM_GEN_HEAVY", gen_heavy)
    sc = scene_of(gpu_lib, "instances")
    p = render.make_params(seed=17, spp=4, max_depth=5, reference_quirks=False)
    f_gpu, s_gpu = gpu_render(gpu_lib, sc.desc, p)
    f_cpu, s_cpu = oracle_render(sc, ("instances", "strict", 17), p)
    assert_equals(f_gpu, s_gpu, f_cpu, s_cpu, ("strict", gen_heavy))
    f_ref, _ = oracle_render(sc, ("instances", "path", 13), render.make_params(seed=13, spp=4, max_depth=5))
    assert f_gpu["rgb_sum"].max() > 0 and f_ref is not None


def test_the_quirks_switch_changes_nothing_for_these_shapes(gpu_lib):
    sc = scene_of(gpu_lib, "lean")
    a, sa = gpu_render(gpu_lib, sc.desc, render.make_params(seed=9, spp=4, max_depth=4, reference_quirks=True))
    b, sb = gpu_render(gpu_lib, sc.desc, render.make_params(seed=9, spp=4, max_depth=4, reference_quirks=False))
    assert_equals(a, sa, b, sb, "quirks")


@pytest.mark.parametrize("integrator, lights, bsdf", [("simplepath", True, True), ("simplepath", False, True), ("randomwalk", True, True)])
def test_the_other_integrators_equal_the_oracle(gpu_lib, integrator, lights, bsdf):
    for variant in ("lean", "instances"):
        sc = scene_of(gpu_lib, variant)
        p = render.make_params(seed=3, spp=4, max_depth=4, integrator=integrator, sample_lights=lights, sample_bsdf=bsdf)
        f_gpu, s_gpu = gpu_render(gpu_lib, sc.desc, p)
        f_cpu, s_cpu = oracle_render(sc, (variant, integrator, lights, bsdf), p)
        assert_equals(f_gpu, s_gpu, f_cpu, s_cpu, (variant, integrator, lights, bsdf))
        assert f_gpu["rgb_sum"].max() > 0


@pytest.mark.parametrize("variant", ["lean", "glass", "coated"])
def test_zsobol_decomposition_invariance(gpu_lib, variant):
    """The *_zs_dl kernels (as tests/test_gpu_delta_lights.py has it): the oracle's film and counters, and a film that does not depend on how the work is cut up."""
    sc = scene_of(gpu_lib, variant)
    p = render.make_params(seed=21, spp=8, max_depth=5, sampler="zsobol")
    gpu = render.Renderer(gpu_lib, sc.desc, 0)
    f1, s1 = gpu.render(p)
    f2, _ = gpu.render(p)
    assert np.array_equal(f1, f2) and (f1["weight_sum"] == 8.0).all() and np.isfinite(f1["rgb_sum"]).all()
    zc.assert_equals_oracle(sc.desc, p, f1, s1, variant)
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


def test_the_pipelines_agree(gpu_lib, monkeypatch):
    """Staged from the camera ray on (SHM_TAIL_FUSED_BOUNCE=-1) against the default, and the split pass on against off: the same bits and counters, in every scene
    class, under both samplers and under force_diffuse / regularize (the general scatter kernels)."""
    variants = ((None, None), ("SHM_TAIL_FUSED_BOUNCE", "-1"), ("SHM_SPLIT_PASS", "0"), ("SHM_SPLIT_PASS", "1"))
    for variant in VARIANTS:
        sc = scene_of(gpu_lib, variant)
        for sampler in ("independent", "zsobol"):
            for kw in (dict(), dict(force_diffuse=True), dict(regularize=True)):
                p = render.make_params(seed=9, spp=2, max_depth=5, sampler=sampler, **kw)
                out = []
                for var, val in variants if not kw else variants[:2]:
                    for v in ("SHM_TAIL_FUSED_BOUNCE", "SHM_SPLIT_PASS"):
                        monkeypatch.delenv(v, raising=False)
                    if var:
                        monkeypatch.setenv(var, val)
                    out.append(gpu_render(gpu_lib, sc.desc, p))
                for v in ("SHM_TAIL_FUSED_BOUNCE", "SHM_SPLIT_PASS"):
                    monkeypatch.delenv(v, raising=False)
                if sampler == "zsobol" or kw:
                    f_cpu, s_cpu = oracle_render(sc, (variant, sampler, tuple(kw)), p)
                    assert_equals(out[0][0], out[0][1], f_cpu, s_cpu, (variant, sampler, kw))
                for f, s in out[1:]:
                    assert_equals(f, s, out[0][0], out[0][1], (variant, sampler, kw))


# ---- leaf probes -------------------------------------------------------------------------------------------------------------------------
def test_the_probes_equal_the_oracle_bit_for_bit(gpu_lib):
    """PROBE_SPHERE_INTERSECT, PROBE_SPHERE_SAMPLE_WITH_CONTEXT and PROBE_SPHERE_PDF_WITH_CONTEXT on the CPU tests' records: the device's own quadric code
    (the probe library is built with SHM_QUADRICS on) against the oracle's."""
    dev = DeviceLeaves(gpu_lib)
    orc = oracle_py.load()
    FP = C.POINTER(F)
    orc.orc_fn_sphere_sample_with_context.restype = C.c_int
    orc.orc_fn_sphere_sample_with_context.argtypes = [C.POINTER(abi.ShmSphere), FP, FP, FP, FP, FP]
    orc.orc_fn_sphere_pdf_with_context.restype, orc.orc_fn_sphere_pdf_with_context.argtypes = F, [C.POINTER(abi.ShmSphere), FP, FP, FP, FP]
    n_hits = 0
    for name, (rec, ro, rd, t_max, expect_hit) in qc.HIT_CASES.items():
        r, w = dev._run("sphere_intersect", _fl(ro) + _fl(rd) + [_f(t_max)] + _struct_words(rec), 5)
        assert bool(r) == expect_hit, name
        b, desc = one_shape_scene(gpu_lib, rec)
        o = oracle_py.Oracle(desc)
        ray = abi.ShmRay()
        ray.o[:], ray.d[:], ray.t_max = [float(x) for x in ro], [float(x) for x in rd], t_max
        out, hit = (F * 12)(), abi.ShmHit()
        ok = o.lib.orc_fn_hit_interaction(o.handle, C.byref(ray), out, C.byref(hit))
        o.close()
        assert bool(ok) == expect_hit, name
        if expect_hit:
            want = np.array([hit.t, hit.b0, hit.b1, hit.b2, hit.phi], np.float32)
            assert np.array_equal(w.view(np.float32), want), (name, w.view(np.float32), want)
            n_hits += 1
    assert n_hits >= 12
    rng = np.random.Generator(np.random.PCG64(31))
    zero = fa([0.0, 0.0, 0.0])
    for name, (rec, ctx_p) in qc.SAMPLE_CASES.items():
        for u in rng.random((6, 2)):
            a, b = (F * 7)(), (F * 7)()
            ra = orc.orc_fn_sphere_sample_with_context(C.byref(rec), fa(ctx_p), zero, zero, fa(u), a)
            rb = dev.orc_fn_sphere_sample_with_context(C.byref(rec), fa(ctx_p), zero, zero, fa(u), b)
            assert ra == rb == 1 and np.array_equal(np.array(a[:], np.float32), np.array(b[:], np.float32)), (name, u, list(a), list(b))
            wi = np.array(a[0:3], np.float64) - np.asarray(ctx_p, np.float64)
            wi = (wi / np.linalg.norm(wi)).astype(np.float32)
            pa = orc.orc_fn_sphere_pdf_with_context(C.byref(rec), fa(ctx_p), zero, zero, fa(wi))
            pb = dev.orc_fn_sphere_pdf_with_context(C.byref(rec), fa(ctx_p), zero, zero, fa(wi))
            assert np.float32(pa) == np.float32(pb) and pa > 0.0, (name, u, pa, pb)


# ---- before and after --------------------------------------------------------------------------------------------------------------------
def test_scenes_without_the_shapes_render_what_the_parent_commit_rendered(gpu_lib):
    """tests/golden/quadrics_before.json on the device: three_spheres, instanced_scene and the Cornell box as patches take the kernels they took — those of k_trace.hip
    and the builds without the shapes, instruction-identical to the parent's (tools/kernel_isa_diff.py, profiles/quadrics.md) — and render the parent's films."""
    import gen_quadrics_before as gen
    before = json.loads((ROOT / "tests" / "golden" / "quadrics_before.json").read_text())
    assert len(before["films"]) == 6
    for rec in before["films"]:
        sc = gen.scene(gpu_lib, rec["scene"])
        assert all(s.quadric == 0 for s in sc.builder.spheres)
        f, st = gpu_render(gpu_lib, sc.desc, gen.params_of(rec))
        assert gen.film_sha256(f) == rec["sha256"], rec["scene"]
        assert [int(st[k]) for k in STATS] == rec["stats"], rec["scene"]
