"""The ZSobol sampler on the device: the probe's stream against the Python restatement (tests/test_zsobol_sampler.py), films equal to the CPU oracle's bit for bit
(the oracle honours ShmRenderParams::sampler; tests/test_zsobol_oracle.py holds it to the restatement) and invariant under every decomposition of the work, every
kernel class drawing the same dimensions, unbiased against independent sampling, and a lower error at equal spp. tests/test_gpu_zsobol_oracle.py walks the table
of edge cases."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import test_zsobol_sampler as ref
import zsobol_cases as zc
from shimmer_amd import abi, render, scene as scn, scenes

pytestmark = pytest.mark.gpu
STATS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")


def probe_op(name):
    """The value of shm/probe.h's PROBE_<name>, read from the header's enum (numbered from 1 in order)."""
    text = (ref.ROOT / "shimmer_amd" / "csrc" / "shm" / "probe.h").read_text()
    body = re.search(r"enum\s*:\s*int\s*\{(.*?)\};", text, re.S).group(1)
    ops = [w.split("=")[0].strip() for w in body.split(",") if w.strip()]
    return ops.index("PROBE_" + name) + 1


def probe_stream(plib, px, py, index, spp, rx, ry, seed, none, kinds):
    op = probe_op("ZSOBOL_STREAM")
    words = [px, py, index, spp, rx, ry, seed & 0xffffffff, seed >> 32, int(none), len(kinds)] + list(kinds)
    n_out = 4 * len(kinds)
    a = (C.c_uint32 * len(words))(*words)
    out = (C.c_uint32 * n_out)()
    res = C.c_int()
    abi.check(plib, plib.shm_debug_eval_leaf(0, op, a, len(words), out, n_out, C.byref(res)), "shm_debug_eval_leaf")
    w, u, f, o = list(out), [], [], 0
    for k in kinds:
        u += w[o:o + k]
        f += w[o + k:o + 2 * k]
        o += 2 * k
    assert res.value == o
    return u, f


def test_device_stream_equals_the_restatement(gpu_lib):
    plib = abi.load_probe_library()
    for c in ref.random_cases(400, random.Random(77)):
        u, f = probe_stream(plib, *c)
        want = ref.stream(*c)
        assert u == want, c
        assert f == [int(np.float32(ref.to_float(v)).view(np.uint32)) for v in want], c


def test_zsobol_film_decomposition_invariance(gpu_lib, monkeypatch):
    """As test_render_decomposition_invariance, with ZSobol: two runs, tile subsets wave by wave, shm_render_device, small batches, no overlap and
    shm_render_sharded at world 1 all give the same bits, and those are the oracle's."""
    sc = scenes.ganesha_proxy(gpu_lib, 160, 120, n=64)
    p = render.make_params(seed=21, spp=12, max_depth=5, sampler="zsobol")
    gpu = render.Renderer(gpu_lib, sc.desc, 0)
    f1, s1 = gpu.render(p)
    f2, _ = gpu.render(p)
    assert np.array_equal(f1, f2) and (f1["weight_sum"] == 12.0).all()
    zc.assert_equals_oracle(sc.desc, p, f1, s1, sc.name)
    f_ind, _ = gpu.render(render.make_params(seed=21, spp=12, max_depth=5))
    assert not np.array_equal(f1, f_ind)  # (the sampler is used)
    gpu.clear()
    idx = np.arange(gpu.n_tiles)
    for ws, we in scn.wave_schedule(12):
        gpu.render_waves(p, tile_indices=idx[idx % 3 != 0], waves=[(ws, we)])
        gpu.render_waves(p, tile_indices=idx[idx % 3 == 0], waves=[(ws, we)])
    assert np.array_equal(gpu.read_film(), f1)
    gpu.clear()
    gpu.render_device(p)
    assert np.array_equal(gpu.read_film(), f1)
    gpu.clear()
    uid = gpu.dist_unique_id()
    gpu.dist_init(0, 1, uid)
    gpu.render_sharded(p)
    assert np.array_equal(gpu.read_film(), f1)
    abi.check(gpu_lib, gpu_lib.shm_dist_finalize(gpu.handle), "shm_dist_finalize")
    gpu.close()
    for var, val in (("SHM_BATCH_PATHS", "8192"), ("SHM_OVERLAP_PATHS", "0")):
        monkeypatch.setenv(var, val)
        g = render.Renderer(gpu_lib, sc.desc, 0)
        f3, s3 = g.render(p)
        g.close()
        monkeypatch.delenv(var)
        assert np.array_equal(f3, f1), var
        assert s3["rays_any"] == s1["rays_any"], var


def test_zsobol_sample_index_range_is_checked(gpu_lib):
    sc = scenes.cornell_box(gpu_lib, 16, 16)
    g = render.Renderer(gpu_lib, sc.desc, 0)
    p = render.make_params(seed=1, spp=6, sampler="zsobol")  # log2spp = 3: indices 0..7
    g.render_waves(p, waves=[(6, 8)])
    with pytest.raises(abi.ShimmerHipError):
        g.render_waves(p, waves=[(7, 9)])
    p.sampler = 2
    with pytest.raises(abi.ShimmerHipError):
        g.render(p)
    g.close()


def class_scenes(lib):
    return [(scenes.cornell_box(lib, 48, 48, glass=True), 6, 14), (scenes.crown_proxy(lib, 40, 56, level=1, n_glass=6, n_gold=3), 4, 12),
            (scenes.cornell_box(lib, 40, 40, textured=True, textured_coated_ceiling=False), 4, 6), (scenes.instanced_scene(lib, 48, 36), 4, 6),
            (scenes.three_spheres(lib, 48, 36, camera=(0.75, 0.5, 9.0), environment=scenes.environment_image(32)), 4, 5),
            (scenes.ganesha_proxy(lib, 64, 64, n=24, variant="textured_floor"), 6, 5), (scenes.cornell_box(lib, 40, 40, textured=True), 4, 6),
            (scenes.ganesha_proxy(lib, 64, 64, n=24, coated=True), 4, 5), (scenes.cornell_box(lib, 40, 40, coated=True, patches=True), 4, 5),
            (scenes.cornell_box(lib, 40, 40, coated=True, mix=True, environment=scenes.environment_image(32)), 4, 5)]


def test_zsobol_kernel_classes_agree(gpu_lib, monkeypatch):
    """Every kernel class of the path integrator draws the same dimensions: the film and the seven counters stay the same bits whichever kernels run — the fused
    kernel from bounce -1 / 0 / 3 on, the split pass on and off —, and the default pipeline's are the oracle's, whose li draws in the reference's order without a
    save / resume. SimplePath and RandomWalk have one kernel each: equal to the oracle, deterministic, finite, image mean within 3 % of independent sampling."""
    for sc, spp, depth in class_scenes(gpu_lib):
        p = render.make_params(seed=5, spp=spp, max_depth=depth, sampler="zsobol")
        runs = []
        for var, val in ((None, None), ("SHM_TAIL_FUSED_BOUNCE", "-1"), ("SHM_TAIL_FUSED_BOUNCE", "0"), ("SHM_TAIL_FUSED_BOUNCE", "3"),
                         ("SHM_SPLIT_PASS", "0"), ("SHM_SPLIT_PASS", "1")):
            monkeypatch.delenv("SHM_TAIL_FUSED_BOUNCE", raising=False)
            monkeypatch.delenv("SHM_SPLIT_PASS", raising=False)
            if var:
                monkeypatch.setenv(var, val)
            g = render.Renderer(gpu_lib, sc.desc, 0)
            runs.append((var, val) + g.render(p))
            g.close()
        monkeypatch.delenv("SHM_TAIL_FUSED_BOUNCE", raising=False)
        monkeypatch.delenv("SHM_SPLIT_PASS", raising=False)
        zc.assert_equals_oracle(sc.desc, p, runs[0][2], runs[0][3], sc.name)
        for var, val, f, s in runs[1:]:
            assert np.array_equal(f, runs[0][2]), (sc.name, var, val)
            for k in STATS:
                assert s[k] == runs[0][3][k], (sc.name, var, val, k)
    # simplepath / randomwalk: the oracle's film, deterministic, finite, image mean close to independent sampling's
    sc = scenes.cornell_box(gpu_lib, 32, 32)
    g = render.Renderer(gpu_lib, sc.desc, 0)
    for integ in ("simplepath", "randomwalk"):
        fz, sz = g.render(render.make_params(seed=3, spp=256, max_depth=4, integrator=integ, sampler="zsobol"))
        zc.assert_equals_oracle(sc.desc, render.make_params(seed=3, spp=256, max_depth=4, integrator=integ, sampler="zsobol"), fz, sz, integ)
        fz2, _ = g.render(render.make_params(seed=3, spp=256, max_depth=4, integrator=integ, sampler="zsobol"))
        fi, _ = g.render(render.make_params(seed=3, spp=1024, max_depth=4, integrator=integ))
        a, b = render.film_to_rgb(fz), render.film_to_rgb(fi)
        assert np.array_equal(fz, fz2) and np.isfinite(a).all()
        assert abs(a.mean() / b.mean() - 1.0) < 0.03, integ
    g.close()


def mean_and_mse(lib, sc, spp_ref, spp, depth, seeds):
    g = render.Renderer(lib, sc.desc, 0)
    ref_img = render.film_to_rgb(g.render(render.make_params(seed=1000, spp=spp_ref, max_depth=depth))[0]).astype(np.float64)
    out = {}
    for sampler in ("independent", "zsobol"):
        imgs = [render.film_to_rgb(g.render(render.make_params(seed=s, spp=spp, max_depth=depth, sampler=sampler))[0]).astype(np.float64) for s in seeds]
        out[sampler] = (imgs, float(np.mean([np.mean((im - ref_img) ** 2) for im in imgs])))
    g.close()
    return ref_img, out


@pytest.mark.parametrize("name", ["C2", "S1"])
def test_zsobol_is_unbiased(gpu_lib, name):
    """Against independent sampling at 4 096 spp (itself held to the oracle; here the mean of 64 images at 64 spp, whose spread gives each pixel's
    standard error): ZSobol at 1 024 spp has the same image mean within 0.5 % and no pixel beyond 5 standard errors (the error of the reference
    plus that of a 1 024-spp independent estimate: ZSobol's own is smaller)."""
    sc = scenes.cornell_box(gpu_lib, 48, 48) if name == "C2" else scenes.sphere_light(gpu_lib, 48, 48)
    g = render.Renderer(gpu_lib, sc.desc, 0)
    ind = np.stack([render.film_to_rgb(g.render(render.make_params(seed=1000 + s, spp=64, max_depth=5))[0]).astype(np.float64) for s in range(64)])
    z = render.film_to_rgb(g.render(render.make_params(seed=7, spp=1024, max_depth=5, sampler="zsobol"))[0]).astype(np.float64)
    g.close()
    ref_img = ind.mean(axis=0)
    assert abs(z.mean() / ref_img.mean() - 1.0) < 0.005, (z.mean(), ref_img.mean())
    var64 = ind.var(axis=0, ddof=1)
    se = np.sqrt(var64 / 64.0 + var64 / 16.0)
    dev = np.abs(z - ref_img) / (se + 1e-12)
    print(f"[zsobol] {name}: mean ratio {z.mean() / ref_img.mean():.5f}, max |z - ref| / se {dev[se > 0].max():.2f}")
    assert (np.abs(z - ref_img) <= 5.0 * se + 1e-6).all(), float(dev.max())


@pytest.mark.parametrize("depth, bound", [(1, 0.6), (5, 1.0)])
def test_zsobol_has_lower_error(gpu_lib, depth, bound):
    """MSE against 4 096-spp independent sampling, averaged over 4 seeds at 64 spp, on the C2 Cornell box at 48^2: ZSobol / independent at most
    `bound`. Measured on an MI355X: 0.085 at max_depth 1 (2.41e-3 against 2.84e-2), 0.101 at max_depth 5 (2.96e-3 against 2.94e-2)."""
    sc = scenes.cornell_box(gpu_lib, 48, 48)
    _, out = mean_and_mse(gpu_lib, sc, 4096, 64, depth, range(4))
    ratio = out["zsobol"][1] / out["independent"][1]
    print(f"[zsobol] C2 48^2 depth {depth}: MSE independent {out['independent'][1]:.4e} zsobol {out['zsobol'][1]:.4e} ratio {ratio:.3f}")
    assert ratio <= bound, ratio


def test_pbrt_zsobol_file_renders_as_make_params(gpu_lib, tmp_path):
    text = (ref.ROOT / "examples" / "scenes" / "cornell_box.pbrt").read_text()
    text = text.replace('Sampler "independent" "integer pixelsamples" 64', 'Sampler "zsobol" "integer pixelsamples" 8 "integer seed" 3')
    assert 'Sampler "zsobol"' in text
    (tmp_path / "z.pbrt").write_text(text)
    out = C.POINTER(abi.ShmPbrtScene)()
    abi.check(gpu_lib, gpu_lib.shm_scene_load_pbrt(str(tmp_path / "z.pbrt").encode(), C.byref(out)), "shm_scene_load_pbrt")
    ps = out.contents
    assert ps.params.sampler == abi.SHM_SAMPLER_ZSOBOL
    g = render.Renderer(gpu_lib, ps.desc, 0)
    f_file, _ = g.render(ps.params)
    mp = render.make_params(seed=3, spp=8, max_depth=ps.params.max_depth, sampler="zsobol")
    mp.disable_reference_quirks = ps.params.disable_reference_quirks
    f_mp, _ = g.render(mp)
    g.close()
    gpu_lib.shm_pbrt_free(out)
    assert np.array_equal(f_file, f_mp)


def test_zsobol_kernel_classes_agree_under_every_option(gpu_lib, monkeypatch):
    """The same agreement with force_diffuse and regularize (the general scatter kernels of every class), under environment maps (the *_env kernels)
    and on the random fuzzing scenes (every shape and material kind, rough dielectrics): the staged kernels from the camera ray on
    (SHM_TAIL_FUSED_BOUNCE=-1) against the default, the same bits and counters, and the default's against the oracle. Between them, the ZSobol tests launch every
    ZSobol kernel."""
    env = scenes.environment_image(32)
    cases = [scenes.crown_proxy(lib := gpu_lib, 30, 42, level=1, n_glass=6, n_gold=2), scenes.crown_proxy(lib, 30, 42, level=1, n_glass=6, n_gold=2, environment=env),
             scenes.cornell_box(lib, 32, 32, textured=True), scenes.cornell_box(lib, 32, 32, glass=True, environment=env),
             scenes.cornell_box(lib, 32, 32, coated=True, environment=env), scenes.three_spheres(lib, 40, 30, camera=(0.75, 0.5, 9.0), environment=env),
             scenes.instanced_scene(lib, 40, 30, environment=env), scenes.cornell_box(lib, 32, 32, coated=True),
             scenes.cornell_box(lib, 32, 32, glass=True, patches=True), scenes.cornell_box(lib, 32, 32, glass=True, patches=True, environment=env),
             scenes.cornell_box(lib, 32, 32, textured=True, textured_coated_ceiling=False, patches=True)] + [scenes.random_scene(lib, k) for k in (1, 3, 11, 13)]
    for sc in cases:
        for kw in (dict(), dict(force_diffuse=True), dict(regularize=True)):
            p = render.make_params(seed=9, spp=4, max_depth=6, sampler="zsobol", **kw)
            out = []
            for first in (None, "-1"):
                if first is None:
                    monkeypatch.delenv("SHM_TAIL_FUSED_BOUNCE", raising=False)
                else:
                    monkeypatch.setenv("SHM_TAIL_FUSED_BOUNCE", first)
                g = render.Renderer(lib, sc.desc, 0)
                out.append(g.render(p))
                g.close()
            monkeypatch.delenv("SHM_TAIL_FUSED_BOUNCE", raising=False)
            assert np.array_equal(out[0][0], out[1][0]), (sc.name, kw)
            zc.assert_equals_oracle(sc.desc, p, out[0][0], out[0][1], (sc.name, kw))
            assert np.isfinite(render.film_to_rgb(out[0][0])).all(), (sc.name, kw)
            for k in STATS:
                assert out[0][1][k] == out[1][1][k], (sc.name, kw, k)
