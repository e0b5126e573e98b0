"""The traversal kernels' control flow (k_trace.inl: the node step with its one regularity branch, the triangle kernels' refill threshold and loop exit, push / pop
with the spill behind a wave-level test; the leaf gate's thresholds, which that change left as they were) against the CPU oracle, as tests/test_gpu_parity.py compares them: hit records byte for byte, occlusion flags, and rays_* / nodes_* / tris_* of both ray kinds —
on inputs chosen by the arms of that control flow: waves that hold irregular rays in every arrangement, every refill / leaf threshold that takes another path,
queue sizes around the 64-ray chunk, a deep tree that spills its stack, and the general kernels' parked round and marker pop."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")


@pytest.fixture(scope="module")
def env(gpu_lib):
    import oracle_py
    from shimmer_amd import render, scenes
    return gpu_lib, oracle_py, render, scenes


def _box(sc):
    b = sc.info["bounds"]
    return b[:, :3].min(0).astype(np.float32), b[:, 3:].max(0).astype(np.float32)


def _rays(sc, n, seed, t_max=np.inf, toward_centre=0.5):
    """Seeded rays around the scene's box, `toward_centre` of them aimed into it."""
    rng = np.random.default_rng(seed)
    lo, hi = _box(sc)
    c, r = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    o = c + (rng.random((n, 3)) * 2 - 1) * r * 1.5
    d = rng.normal(size=(n, 3))
    aim = rng.random(n) < toward_centre
    d[aim] = (c + (rng.random((int(aim.sum()), 3)) - 0.5) * r * 0.5) - o[aim]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3], rays[:, 3:6], rays[:, 6] = o, d, t_max
    return rays


N_IRREGULAR_KINDS = 9


def _make_irregular(rays, idx, sc):
    """Turns rays[idx] into irregular rays (k_trace.inl, set_ray: a direction component that is 0 makes the reciprocal infinite), the kinds in turn: a zero component
    on each axis, two zero components, and an origin ON a plane of the scene's box with that component zero — (plane - o) * (1 / d) = 0 * inf, a NaN slab distance."""
    lo, hi = _box(sc)
    for k, i in enumerate(idx):
        kind = k % N_IRREGULAR_KINDS
        d = rays[i, 3:6].astype(np.float64)
        if kind < 3:
            d[kind] = 0.0
        elif kind < 6:
            d[kind - 3] = 0.0
            d[(kind - 2) % 3] = 0.0
        else:
            axis = kind - 6
            d[axis] = 0.0
            rays[i, axis] = (lo, hi, lo)[axis][axis]
        rays[i, 3:6] = d / np.linalg.norm(d)
        assert (rays[i, 3:6] == 0.0).sum() == (2 if 3 <= kind < 6 else 1)


def _compare(gpu, orc, rays, what):
    """Both ray kinds of `rays` on the GPU and in the oracle: everything the kernels write or count."""
    hg, sg = gpu.trace(rays)
    ho, so = orc.trace(rays)
    assert np.array_equal(hg.view(np.uint8), ho.view(np.uint8)), what
    for k in ("rays_closest", "nodes_closest", "tris_closest"):
        assert sg[k] == so[k], (what, k)
    assert sg["rays_closest"] == len(rays), what
    ag, s2 = gpu.trace(rays, any_hit=True)
    ao, s3 = orc.trace(rays, any_hit=True)
    assert np.array_equal(ag, ao), what
    for k in ("rays_any", "nodes_any", "tris_any"):
        assert s2[k] == s3[k], (what, k)
    assert s2["rays_any"] == len(rays), what
    return ho, ao


def test_regularity_mixes_within_a_wave(env):
    """The rays go to Renderer.trace directly, so the queue is the identity and a wave's first refill is one 64-ray chunk: chunks that are all regular, all irregular,
    regular but for lane 0, regular but for lane 63, and alternating, in turn over 4 096 rays; then 40 000 rays with an irregular ray at every 97th index, which
    running regular waves take in by refill and retire again (the wave's regularity changes both ways while it traces)."""
    lib, oracle_py, render, scenes = env
    sc = scenes.cornell_box(lib, 32, 32)
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    rays = _rays(sc, 4096, 11, toward_centre=0.8)
    idx = []
    for chunk in range(4096 // 64):
        lanes = {0: [], 1: range(64), 2: [0], 3: [63], 4: range(0, 64, 2)}[chunk % 5]
        idx += [chunk * 64 + lane for lane in lanes]
    _make_irregular(rays, idx, sc)
    ho, ao = _compare(gpu, orc, rays, "chunk patterns")
    irregular = np.zeros(4096, bool)
    irregular[idx] = True
    assert (ho["prim"][irregular] >= 0).sum() > 50 and (ho["prim"][~irregular] >= 0).sum() > 50  # (both kinds of ray find the room)
    rays[:, 6] = 2.5
    _compare(gpu, orc, rays, "chunk patterns, t_max 2.5")
    rays = _rays(sc, 40000, 12)
    _make_irregular(rays, list(range(0, 40000, 97)), sc)
    _compare(gpu, orc, rays, "every 97th")
    gpu.close()
    orc.close()


_ARMS = {}  # scene name -> (scene, [(rays, what)]): the inputs of the next test, made once


def _arms_cases(scenes, lib):
    if not _ARMS:
        for name, sc in (("deep", scenes.ganesha_proxy(lib, 64, 64, n=96)), ("cornell", scenes.cornell_box(lib, 32, 32))):
            _ARMS[name] = (sc, [(_rays(sc, 20000, 21 + k, t_max, toward_centre=aim), f"{name}, t_max {t_max}") for k, (t_max, aim) in enumerate(((np.inf, 0.5), (2.5, 0.9)))])
    return _ARMS


@pytest.mark.parametrize("leaf_min", ["1", "64"])
@pytest.mark.parametrize("refill_min", ["1", "40", "64"])
def test_every_arm_of_the_loop(env, monkeypatch, refill_min, leaf_min):
    """A refill at the first idle lane, at the default and only when the whole wave is idle, crossed with a leaf phase per pending leaf and only when nothing else
    can run — on a tree deeper than the LDS stack levels of both triangle kernels (the spill arm of push and pop) and on a shallow one. The knobs are read when
    the scene is created."""
    lib, oracle_py, render, scenes = env
    for k in ("SHM_REFILL_MIN", "SHM_REFILL_MIN_ANY"):
        monkeypatch.setenv(k, refill_min)
    for k in ("SHM_LEAF_MIN", "SHM_LEAF_MIN_ANY"):
        monkeypatch.setenv(k, leaf_min)
    for name, (sc, cases) in _arms_cases(scenes, lib).items():
        gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
        if name == "deep":
            plan = orc.trace_plan()
            assert plan["spill_levels_closest"] >= 2 and plan["spill_levels_any"] >= 2
        for rays, what in cases:
            _compare(gpu, orc, rays, what)
        gpu.close()
        orc.close()


def test_queue_sizes_at_the_chunk_boundaries(env):
    """One ray, one short of a chunk, a chunk, one more, and the same around 64 chunks."""
    lib, oracle_py, render, scenes = env
    sc = scenes.cornell_box(lib, 32, 32)
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    rays = _rays(sc, 4097, 31, toward_centre=0.7)
    for n in (1, 63, 64, 65, 4095, 4097):
        _compare(gpu, orc, rays[:n], f"n = {n}")
    gpu.close()
    orc.close()


def test_general_and_instanced_scenes(env):
    """The general kernels (k_trace5<., GEN>) take the same loop: the parked round of a patch scene, and an instanced scene's marker push and pop."""
    lib, oracle_py, render, scenes = env
    for sc in (scenes.cornell_box(lib, 32, 32, patches=True), scenes.instanced_scene(lib, 32, 24)):
        gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
        for seed, t_max, aim in ((41, np.inf, 0.5), (42, 2.5, 0.9)):
            ho, _ = _compare(gpu, orc, _rays(sc, 20000, seed, t_max, toward_centre=aim), sc.name)
            assert (ho["prim"] >= 0).sum() > 100
        gpu.close()
        orc.close()


def test_a_small_render(env):
    """The kernels inside a render (queues compacted per bounce, shadow rays with deferred contributions): the f64 film and all seven counters equal the oracle's."""
    lib, oracle_py, render, scenes = env
    sc = scenes.ganesha_proxy(lib, 64, 64, n=32)
    p = render.make_params(seed=5, spp=4, max_depth=5)
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    fg, sg = gpu.render(p)
    fo, so = orc.render(p, n_threads=os.cpu_count() or 1)
    gpu.close()
    orc.close()
    assert np.array_equal(fg.view(np.uint64), fo.view(np.uint64))
    for k in COUNTERS:
        assert sg[k] == so[k], k
