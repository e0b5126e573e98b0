"""GPU parity tests proper (run with `pytest -m gpu` on an MI355X): libshimmer_hip.so through its C ABI against
the CPU oracle on identical seeded inputs — bit-exact for indices / hit records / counters / f64 film sums, and
the north-star tolerance L_inf < 1e-4 on the f32 film RGB (which bit-exactness implies).  At BASELINE sizes the
oracle is too slow, so size-independent properties are checked instead (determinism, tile/wave/batch
decomposition invariance, weight sums, agreement on an oracle-rendered crop)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L_INF_TOL = 1e-4  # BASELINE.json north_star: per-pixel L-infinity on f32 film RGB


def _rays(sc, n, seed, t_max=np.inf, toward_centre=0.5):
    rng = np.random.default_rng(seed)
    b = sc.info["bounds"]
    lo, hi = b[:, :3].min(0), b[:, 3:].max(0)
    c, r = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    o = c + (rng.random((n, 3)) * 2 - 1) * r * 1.5
    d = rng.normal(size=(n, 3))
    aim = rng.random(n) < toward_centre
    d[aim] = (c + (rng.random((int(aim.sum()), 3)) - 0.5) * r * 0.5) - o[aim]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3], rays[:, 3:6], rays[:, 6] = o, d, t_max
    return rays


@pytest.fixture(scope="module")
def env(gpu_lib):
    import oracle_py
    from shimmer_amd import render, scenes
    return gpu_lib, oracle_py, render, scenes


SCENES = {
    "S1_sphere_light": lambda scenes, lib: (scenes.sphere_light(lib, 64, 64), 8, 5),
    "S2_cornell": lambda scenes, lib: (scenes.cornell_box(lib, 96, 96), 16, 5),
    "S3_small": lambda scenes, lib: (scenes.ganesha_proxy(lib, 96, 96, n=48), 8, 5),
    "S4_small_depth32": lambda scenes, lib: (scenes.crown_proxy(lib, 60, 84, level=2, n_glass=12, n_gold=4), 8, 32),
    "three_spheres": lambda scenes, lib: (scenes.three_spheres(lib, 48, 32, camera=(0.75, 0.5, 9.0)), 4, 5),
    # LayeredBxDF materials (CoatedDiffuse with and without a scattering medium, CoatedConductor)
    "S2_cornell_coated": lambda scenes, lib: (scenes.cornell_box(lib, 64, 64, coated=True), 8, 5),
    "S3_small_coated": lambda scenes, lib: (scenes.ganesha_proxy(lib, 64, 64, n=32, coated=True), 4, 5),
    "S2_cornell_patches": lambda scenes, lib: (scenes.cornell_box(lib, 64, 64, patches=True), 8, 5),  # BilinearPatch: rectangle light + curved patch
    "S2_cornell_patches_skewed": lambda scenes, lib: (scenes.cornell_box(lib, 48, 48, patches=True, patch_skew=2e-3), 4, 5),  # area-sampled patch light
    "S2_cornell_glass": lambda scenes, lib: (scenes.cornell_box(lib, 64, 64, glass=True), 8, 14),  # smooth / rough / index-matched / thin dielectrics: k_scatter_specular + k_scatter_nonspecular, late-bounce overlap (6) and the fused tail launch (8)
    # emission at a vertex whose path goes on (a reflecting, two-sided emitter): the fused kernel defers it to k_emit_jobs — alone (all-diffuse scene) and as the
    # diverted kernel of a scene with coated materials
    "S2_cornell_reflecting_emitter": lambda scenes, lib: (scenes.cornell_box(lib, 64, 64, emitter_reflects=True), 8, 5),
    "S2_cornell_coated_reflecting_emitter": lambda scenes, lib: (scenes.cornell_box(lib, 48, 48, coated=True, emitter_reflects=True), 6, 5),
    # (round 6) the object as bilinear patches — what a quad PLY file becomes in the reference: every leaf of the object a parked non-triangle test
    "S3_small_smooth": lambda scenes, lib: (scenes.ganesha_proxy(lib, 64, 64, n=32, variant="smooth"), 6, 5),  # per-vertex normals + uv on the object (shading frames, dndu / dndv)
    "S3_small_mesh_emitter": lambda scenes, lib: (scenes.ganesha_proxy(lib, 64, 64, n=32, variant="mesh_emitter"), 6, 5),  # 8 192 area lights: the light tables beyond the LDS budget
    "S3_small_textured_object": lambda scenes, lib: (scenes.ganesha_proxy(lib, 64, 64, n=32, variant="textured_object"), 6, 5),  # an image texture over the object's uv: every object hit a textured vertex
    "S3_small_instance_grid": lambda scenes, lib: (scenes.ganesha_proxy(lib, 64, 64, n=32, variant="instance_grid"), 6, 5),  # 64 placements of one definition: rays cross several instance boxes
    "S3_small_quads": lambda scenes, lib: (scenes.ganesha_proxy(lib, 96, 96, n=48, variant="quads"), 8, 5),
    "S3_small_quads_coated": lambda scenes, lib: (scenes.ganesha_proxy(lib, 64, 64, n=32, variant="quads", coated=True), 4, 5),
    # (round 6, found by the kernel-coverage run — profiles/r06_kernel_coverage.txt: until then no test reached these instantiations)
    # the material-sorted fused all-materials kernel for GENERAL geometry: patches + glass (k_shade_fused_gen.hip), under a map (k_shade_fused_gen_env.hip), with textures (k_shade_fused_gen_tex.hip)
    "S2_cornell_patches_glass": lambda scenes, lib: (scenes.cornell_box(lib, 48, 48, patches=True, glass=True), 6, 8),
    "S2_cornell_patches_glass_env": lambda scenes, lib: (scenes.cornell_box(lib, 48, 48, patches=True, glass=True, environment=scenes.environment_image(32)), 6, 8),
    "S2_cornell_textured_nocoat_patches": lambda scenes, lib: (scenes.cornell_box(lib, 40, 40, textured=True, textured_coated_ceiling=False, patches=True), 4, 6),
    # coated + smooth and rough glass under a map: the dielectric class's K_ENV_LIGHT units (k_scatter_specular_env / k_scatter_nonspecular_env), triangles and with patches
    "S2_cornell_coated_glass_env": lambda scenes, lib: (scenes.cornell_box(lib, 48, 48, coated=True, glass_too=True, environment=scenes.environment_image(32)), 6, 8),
    "S2_cornell_coated_glass_env_patches": lambda scenes, lib: (scenes.cornell_box(lib, 48, 48, coated=True, glass_too=True, patches=True, environment=scenes.environment_image(32)), 6, 8),
    "S2_cornell_mix": lambda scenes, lib: (scenes.cornell_box(lib, 64, 64, mix=True), 8, 5),  # MixMaterial, nested, with a coated leaf
    # image textures (every mapping / filter / wrap / spectrum type), ray differentials through a mirror and glass
    "S2_cornell_textured": lambda scenes, lib: (scenes.cornell_box(lib, 64, 64, textured=True), 8, 6),
    "S2_cornell_textured_nocoat": lambda scenes, lib: (scenes.cornell_box(lib, 48, 48, textured=True, textured_coated_ceiling=False), 6, 6),  # k_shade<false, false, true>
    # ImageInfinitelight: compensated PiecewiseConstant2D sampling + MIS against BSDF-sampled escapes
    # TransformedPrimitive instancing: two-level traversal, inverse map for intersect, the reference's forward map for the predicate
    "instanced": lambda scenes, lib: (scenes.instanced_scene(lib, 64, 48), 8, 5),
    "three_spheres_environment": lambda scenes, lib: (scenes.three_spheres(lib, 64, 48, camera=(0.75, 0.5, 9.0), environment=scenes.environment_image(32)), 8, 5),
    # round 5: the headline scene with the shapes a real PBRT-v4 scene mixes into its triangles (bench.py's side results, small): k_trace5<., GEN> + the general fused kernel
    "S3_small_patch_emitter": lambda scenes, lib: (scenes.ganesha_proxy(lib, 64, 64, n=32, variant="patch_emitter"), 6, 5),
    "S3_small_one_sphere": lambda scenes, lib: (scenes.ganesha_proxy(lib, 64, 64, n=32, variant="one_sphere"), 6, 5),
    "S3_small_instanced": lambda scenes, lib: (scenes.ganesha_proxy(lib, 64, 64, n=32, variant="instanced"), 6, 5),
    "S3_small_textured_floor": lambda scenes, lib: (scenes.ganesha_proxy(lib, 64, 64, n=32, variant="textured_floor"), 6, 5),
    "S3_small_environment": lambda scenes, lib: (scenes.ganesha_proxy(lib, 64, 64, n=32, variant="environment"), 6, 5),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_trace_bitwise_parity(env, name):
    """K2/K3 alone: identical (prim, t, b0, b1, b2, phi) and identical node / primitive visit counts, i.e. the same
    traversal order as aggregate.rs:71-203."""
    lib, oracle_py, render, scenes = env
    sc, _, _ = SCENES[name](scenes, lib)
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    for seed, tmax in ((1, np.inf), (2, 3.0)):
        rays = _rays(sc, 30000, seed, tmax)
        hg, sg = gpu.trace(rays)
        ho, so = orc.trace(rays)
        for k in ("prim", "t", "b0", "b1", "b2", "phi", "instance"):
            hit = ho["prim"] >= 0  # (the record of a miss is only defined up to prim = -1)
            assert np.array_equal(hg[k].view(np.uint32)[hit], ho[k].view(np.uint32)[hit]), k
        assert np.array_equal(hg["prim"], ho["prim"])
        assert (hg["prim"] >= 0).sum() > 100
        assert sg["nodes_closest"] == so["nodes_closest"] and sg["tris_closest"] == so["tris_closest"] and sg["rays_closest"] == 30000
        ag, s2 = gpu.trace(rays, any_hit=True)
        ao, s3 = orc.trace(rays, any_hit=True)
        # any-hit: identical occlusion flags, primitive tests AND node visits — the pair-step kernel tests both children at the parent, and counts a
        # far child only if the reference's loop would have reached it before its early exit (phantom counts, k_trace.hip)
        assert np.array_equal(ag, ao) and s2["nodes_any"] == s3["nodes_any"] and s2["tris_any"] == s3["tris_any"]
    gpu.close()
    orc.close()


def test_trace_any_after_a_quirks_off_render_is_reference_exact(env):
    """shm_trace_any takes no render parameters: on an instanced scene it runs the reference-exact any-hit kernels whatever the scene's last render
    used — after a render with disable_reference_quirks too (that render's shadow rays took the STRICT instantiations)."""
    lib, oracle_py, render, scenes = env
    sc, spp, depth = SCENES["instanced"](scenes, lib)
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    gpu.render(render.make_params(seed=3, spp=spp, max_depth=depth, reference_quirks=False))
    rays = _rays(sc, 30000, 5)
    ag, sg = gpu.trace(rays, any_hit=True)
    ao, so = orc.trace(rays, any_hit=True)
    assert ag.any() and not ag.all()
    assert np.array_equal(ag, ao)
    for k in ("rays_any", "nodes_any", "tris_any"):
        assert sg[k] == so[k], k
    gpu.close()
    orc.close()


def _stacked_leaf_scene(scenes, lib, copies):
    """The Cornell box plus `copies` coincident triangles (identical centroids: BvhAggregate::new leaves them in ONE leaf, aggregate.rs:345-356) —
    a leaf of more primitives than the device link word's count field holds (15)."""
    from shimmer_amd.scene import SceneBuilder
    b = SceneBuilder()
    b.set_film(32, 32)
    rfw = b.set_camera_look_at(lib, (0, 1, 3.4), (0, 1, 0), (0, 1, 0), 39.0)
    white = b.material_diffuse(0.75)
    room_p, room_vi = scenes._merge([scenes._box((-1, 0, -1), (1, 2, 1), faces="xXyYz")])
    b.add_mesh(scenes._to_render(room_p, rfw), room_vi, white)
    tri = np.array([[-0.4, 0.6, 0.0], [0.4, 0.6, 0.1], [0.0, 1.4, -0.1]], np.float32)
    p = np.concatenate([tri] * copies)
    vi = np.arange(3 * copies, dtype=np.uint32).reshape(-1, 3)
    b.add_mesh(scenes._to_render(p, rfw), vi, white)
    pl, vil = scenes._quad((-0.3, 1.99, -0.3), (0.3, 1.99, -0.3), (0.3, 1.99, 0.3), (-0.3, 1.99, 0.3))
    from shimmer_amd.scene import blackbody_dense
    b.add_mesh(scenes._to_render(pl, rfw), vil, b.material_diffuse(0.0), emission=blackbody_dense(6500.0), emission_scale=10.0)
    return scenes._finish(b, lib, name=f"stacked leaf x{copies}")


def _tiny_tree_scene(scenes, lib, n_tris):
    """A tree of one node (n_tris = 1: the root IS a leaf) or three (two triangles): the smallest inputs of the traversal kernels' root handling."""
    from shimmer_amd.scene import SceneBuilder, blackbody_dense
    b = SceneBuilder()
    b.set_film(16, 16)
    rfw = b.set_camera_look_at(lib, (0, 0, 4), (0, 0, 0), (0, 1, 0), 40.0)
    p = np.array([[-1, -1, 0], [1, -1, 0.2], [0, 1, -0.1], [0.5, 0.5, 1.0], [1.5, 0.6, 1.1], [0.9, 1.5, 0.8]], np.float32)[: 3 * n_tris]
    vi = np.arange(3 * n_tris, dtype=np.uint32).reshape(-1, 3)
    b.add_mesh(scenes._to_render(p, rfw), vi, b.material_diffuse(0.5), emission=blackbody_dense(6500.0), emission_scale=5.0, two_sided=True)
    return scenes._finish(b, lib, name=f"{n_tris} triangle(s)")


def _deep_walk_scene(scenes, lib):
    """A coated floor whose coating is a thick, almost lossless scattering medium under an area light: LayeredBxDF walks of hundreds of steps (max_depth 1000)."""
    from shimmer_amd.scene import SceneBuilder, blackbody_dense
    b = SceneBuilder()
    b.set_film(40, 40)
    rfw = b.set_camera_look_at(lib, (0, 2.5, 4), (0, 0, 0), (0, 1, 0), 40.0)
    floor = np.array([[-2, 0, -2], [2, 0, -2], [2, 0, 2], [-2, 0, 2]], np.float32)
    lamp = np.array([[-0.7, 3, -0.7], [0.7, 3, -0.7], [0.7, 3, 0.7], [-0.7, 3, 0.7]], np.float32)
    quad = np.array([[0, 2, 1], [0, 3, 2]], np.uint32)
    m = b.material_coated_diffuse(reflectance=0.99, roughness=0.1, thickness=5.0, albedo=0.9999, g=0.2, max_depth=1000)
    b.add_mesh(scenes._to_render(floor, rfw), quad, m)
    b.add_mesh(scenes._to_render(lamp, rfw), quad[:, ::-1].copy(), b.material_diffuse(0.0), emission=blackbody_dense(6500.0), emission_scale=8.0)
    return scenes._finish(b, lib, name="deep layered walks")


def test_layered_walks_of_hundreds_of_steps(env):
    """The staged LayeredBxDF kernel (k_scatter_layered.inl) carries a walk's depth through its job buffer; walks longer than 255 steps (a thick, almost lossless
    medium, max_depth 1000: about one walk in 300 here) must come out as the oracle's one-piece layered_sample_f has them — film and counters bit for bit."""
    lib, oracle_py, render, scenes = env
    sc = _deep_walk_scene(scenes, lib)
    p = render.make_params(seed=4, spp=8, max_depth=4)
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    fg, sg = gpu.render(p)
    fo, so = orc.render(p)
    gpu.close(); orc.close()
    assert np.array_equal(fg.view(np.uint64), fo.view(np.uint64))
    for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
        assert sg[k] == so[k], k
    assert sg["rays_any"] > 1000  # (next-event estimation ran: the f and pdf walks too)


TRACE_TRI, TRACE_GEN, TRACE_GEN_HEAVY = 0, 1, 2  # host/render_plan.hpp: the rows of the traversal kernels' table


def _spilling_kernels(orc, gen_heavy_knob=-1):
    """The (variant, ray kind) pairs whose HBM stack spill this scene really sizes from its depth (host/render_plan.hpp through the oracle: no GPU): two levels or more."""
    plan = orc.trace_plan(gen_heavy_knob=gen_heavy_knob)
    return {(plan["variant"], kind) for kind in ("closest", "any") if plan[f"spill_levels_{kind}"] >= 2}


@pytest.mark.parametrize("other_min", ["16", "1", "64"])
def test_trace_tree_shapes_and_parked_tests(env, monkeypatch, other_min):
    """The traversal kernels (k_trace5 / k_trace5<., GEN>: the both-children step) against the oracle's scalar loop — hit records, occlusion flags and all four visit
    counters — on a deep tree (S3 proxy, stack spill exercised with depth beyond the LDS levels), a shallow one, a tree with leaves of 1, 6, 7, 8, 14, 16 and 40 coincident
    triangles (the link word's count field saturates at 7: ShmScene::d_big_leaf_n), one- and three-node trees, and the scenes with spheres, bilinear patches and instances
    (round 5: parked non-triangle tests, the marker on the stack, sub-trees of one leaf, spheres and patches INSIDE instances) — with the parked tests run as the default
    batches of 16, one at a time (SHM_OTHER_MIN=1) and only when nothing else can run (64). (Until round 5 this test also ran the one-node-step kernels k_trace3 as a
    second implementation; they are retired, the oracle is the checker.)"""
    lib, oracle_py, render, scenes = env
    monkeypatch.setenv("SHM_OTHER_MIN", other_min)
    cases = [scenes.ganesha_proxy(lib, 64, 64, n=96), scenes.cornell_box(lib, 32, 32)] + [_stacked_leaf_scene(scenes, lib, c) for c in (6, 7, 8, 14, 16, 40)] + \
            [_tiny_tree_scene(scenes, lib, 1), _tiny_tree_scene(scenes, lib, 2)] + \
            [scenes.instanced_scene(lib, 32, 24), scenes.three_spheres(lib, 32, 24, camera=(0.75, 0.5, 9.0)), scenes.cornell_box(lib, 32, 32, patches=True),
             scenes.ganesha_proxy(lib, 32, 32, n=64, variant="instanced"), scenes.ganesha_proxy(lib, 32, 32, n=24, variant="patch_emitter"),
             scenes.random_scene(lib, 3), scenes.random_scene(lib, 11)]
    spilling = set()
    for sc in cases:
        gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
        spilling |= _spilling_kernels(orc)
        for seed, tmax, aim in ((5, np.inf, 0.5), (6, 2.5, 0.9)):
            rays = _rays(sc, 40000, seed, tmax, toward_centre=aim)
            hg, sg = gpu.trace(rays)
            ho, so = orc.trace(rays)
            assert np.array_equal(hg.view(np.uint8), ho.view(np.uint8)), sc.name
            assert sg["nodes_closest"] == so["nodes_closest"] and sg["tris_closest"] == so["tris_closest"], sc.name
            ag, s2 = gpu.trace(rays, any_hit=True)
            ao, s3 = orc.trace(rays, any_hit=True)
            assert np.array_equal(ag, ao) and s2["nodes_any"] == s3["nodes_any"] and s2["tris_any"] == s3["tris_any"], sc.name
        p = render.make_params(seed=2, spp=4, max_depth=5)
        fg, st = gpu.render(p)
        fo, so = orc.render(p, n_threads=os.cpu_count() or 1)
        assert np.array_equal(fg, fo), sc.name
        for k in ("rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
            assert st[k] == so[k], (sc.name, k)
        gpu.close()
        orc.close()
    # the case list holds a tree deeper than the LDS stack levels for both ray kinds of the triangle and the general kernels (the five-wave ones: the next test)
    assert spilling >= {(v, kind) for v in (TRACE_TRI, TRACE_GEN) for kind in ("closest", "any")}


@pytest.mark.parametrize("heavy", ["0", "1"])
def test_both_occupancies_of_the_general_traversal_kernels(env, monkeypatch, heavy):
    """Scenes with spheres / bilinear patches trace with k_trace5<., GEN> at seven waves per SIMD, or — where those shapes are a sixth of the primitive records or more (a quad
    PLY file: every face a patch) — at five (k_trace5<., GEN, HEAVY>: the parked round's arithmetic in registers instead of spill code; round 6). The same body: whichever the
    scene would choose, forced either way (SHM_GEN_HEAVY), hit records, films and all seven counters equal the oracle's."""
    lib, oracle_py, render, scenes = env
    monkeypatch.setenv("SHM_GEN_HEAVY", heavy)
    cases = [(scenes.ganesha_proxy(lib, 64, 64, n=32, variant="quads"), 6, 5), (scenes.ganesha_proxy(lib, 48, 48, n=24, quad_fraction=0.3, coated=True), 4, 5),
             (scenes.cornell_box(lib, 48, 48, patches=True), 6, 5), (scenes.three_spheres(lib, 48, 32, camera=(0.75, 0.5, 9.0)), 4, 5), (scenes.instanced_scene(lib, 48, 36), 4, 6)]
    spilling = set()
    for sc, spp, depth in cases:
        gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
        spilling |= _spilling_kernels(orc, gen_heavy_knob=int(heavy))
        rays = _rays(sc, 20000, 5)
        hg, sg = gpu.trace(rays)
        ho, so = orc.trace(rays)
        assert all(np.array_equal(hg[k], ho[k]) for k in ("prim", "t", "b0", "b1", "b2", "phi")), sc.name
        assert sg["nodes_closest"] == so["nodes_closest"] and sg["tris_closest"] == so["tris_closest"], sc.name
        rays[:, 6] = 2.5
        ag, s2 = gpu.trace(rays, any_hit=True)
        ao, s3 = orc.trace(rays, any_hit=True)
        assert np.array_equal(ag, ao) and s2["nodes_any"] == s3["nodes_any"] and s2["tris_any"] == s3["tris_any"], sc.name
        p = render.make_params(seed=11, spp=spp, max_depth=depth)
        fg, stg = gpu.render(p)
        fo, sto = orc.render(p, n_threads=os.cpu_count() or 1)
        assert np.array_equal(fg, fo), sc.name
        for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
            assert stg[k] == sto[k], (sc.name, k)
        if sc.desc.n_instances:  # ... and with the reference quirks off: the any-hit kernels' STRICT instantiations (k_trace5_any_strict<heavy>), at this occupancy
            p = render.make_params(seed=11, spp=spp, max_depth=depth, reference_quirks=False)
            fg, stg = gpu.render(p)
            fo, sto = orc.render(p, n_threads=os.cpu_count() or 1)
            assert np.array_equal(fg, fo), sc.name
            for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
                assert stg[k] == sto[k], (sc.name, k)
        gpu.close(); orc.close()
    # ... and at the occupancy forced here, a tree deeper than the kernels' LDS stack levels for both ray kinds (the STRICT pair runs on the any-hit side's spill)
    assert spilling >= {(TRACE_GEN_HEAVY if heavy == "1" else TRACE_GEN, kind) for kind in ("closest", "any")}


def test_trace_edge_cases(env):
    """Degenerate inputs: a single ray, rays that start inside boxes, axis-parallel directions (inv_dir = inf), t_max = 0,
    rays grazing planes / shared edges (f64 edge-function fallback, triangle.rs:231-243)."""
    lib, oracle_py, render, scenes = env
    sc = scenes.cornell_box(lib, 32, 32)
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    cam_z = -3.4  # render space: camera at the origin, room centre at (0, 0, -3.4)
    rays = np.array([
        [0, 0, 0, 0, 0, -1, np.inf, 0],            # down the optical axis
        [0, 0, cam_z, 1, 0, 0, np.inf, 0],         # axis-parallel from inside the room
        [0, 0, cam_z, 0, 1, 0, np.inf, 0],
        [0, 0, cam_z, 0, -1, 0, np.inf, 0],
        [0, 0, cam_z, 0, 0, -1, 0.0, 0],           # t_max = 0: nothing can be hit
        [0, -1, cam_z, 0, 0, -1, np.inf, 0],       # along the floor plane (grazing)
        [-1, -1, 0, 0, 0, -1, np.inf, 0],          # along a room edge
        [1e3, 1e3, 1e3, 1, 1, 1, np.inf, 0],       # far away, pointing away
    ], np.float32)
    for any_hit in (False, True):
        hg, _ = gpu.trace(rays, any_hit=any_hit)
        ho, _ = orc.trace(rays, any_hit=any_hit)
        assert np.array_equal(hg.view(np.uint8), ho.view(np.uint8))
    one, _ = gpu.trace(rays[:1])
    assert one["prim"][0] >= 0
    # more rays than the lanes a small launch uses (a small queue takes part of the persistent grid: 4 rays per resident lane), hits and misses
    # mixed: every lane traces several rays in turn, and the record of a miss must not carry the barycentrics of the hit the lane found before it
    big = _rays(sc, 60000, 7, toward_centre=0.3)
    hg, sg = gpu.trace(big)
    ho, so = orc.trace(big)
    assert 0.05 < (ho["prim"] < 0).mean() < 0.95
    assert np.array_equal(hg.view(np.uint8), ho.view(np.uint8)) and sg["nodes_closest"] == so["nodes_closest"] and sg["tris_closest"] == so["tris_closest"]
    gpu.close()
    orc.close()


@pytest.mark.parametrize("name", list(SCENES))
def test_render_parity(env, name):
    """The whole hot path: every f64 film sum identical to the oracle's; L_inf on f32 RGB below the stated tolerance;
    identical ray / node / primitive counters (same paths, same traversals)."""
    lib, oracle_py, render, scenes = env
    sc, spp, depth = SCENES[name](scenes, lib)
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    params = render.make_params(seed=3, spp=spp, max_depth=depth)
    fg, sg = gpu.render(params)
    fo, so = orc.render(params, n_threads=os.cpu_count() or 1)
    a, b = render.film_to_rgb(fg), render.film_to_rgb(fo)
    assert np.isfinite(a).all() and a.max() > 0
    assert float(np.max(np.abs(a - b))) < L_INF_TOL
    assert np.array_equal(fg, fo)  # bit-exact f64 sums
    for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
        assert sg[k] == so[k], k
    gpu.close()
    orc.close()


def test_render_parity_options(env):
    """The option flags the path reads (options.rs): disable_pixel_jitter, disable_wavelength_jitter, regularize; and a
    non-zero pixel_bounds origin with ragged (remainder) tiles."""
    lib, oracle_py, render, scenes = env
    from shimmer_amd import scene as scn
    sc = scenes.crown_proxy(lib, 45, 37, level=1, n_glass=8, n_gold=4)
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    for kw in (dict(disable_pixel_jitter=True), dict(disable_wavelength_jitter=True), dict(regularize=True)):
        p = render.make_params(seed=8, spp=4, max_depth=8, **kw)
        fg, _ = gpu.render(p)
        fo, _ = orc.render(p, n_threads=os.cpu_count() or 1)
        assert np.array_equal(fg, fo), kw
    gpu.close()
    orc.close()
    # crop window: pixel_bounds (5,3)-(42,30) inside a 48x32 film -> remainder tiles on both axes
    b = scn.SceneBuilder()
    b.set_film(48, 32, pixel_bounds=(5, 3, 42, 30))
    rfw = b.set_camera_look_at(lib, (0, 1, 3.4), (0, 1, 0), (0, 1, 0), 39.0)
    m = b.material_diffuse(0.6)
    p, vi = scenes._box((-1, 0, -1), (1, 2, 1), faces="xXyYz")
    b.add_mesh(scenes._to_render(p, rfw), vi, m)
    q, qi = scenes._quad((-0.3, 1.98, -0.3), (0.3, 1.98, -0.3), (0.3, 1.98, 0.3), (-0.3, 1.98, 0.3))
    b.add_mesh(scenes._to_render(q, rfw), qi, b.material_diffuse(0.0), emission=scn.blackbody_dense(5000.0), emission_scale=15.0)
    desc, _ = b.build(lib)
    gpu, orc = render.Renderer(lib, desc, 0), oracle_py.Oracle(desc)
    pr = render.make_params(seed=1, spp=5, max_depth=4)
    fg, _ = gpu.render(pr)
    fo, _ = orc.render(pr, n_threads=4)
    assert fg.shape == (27, 37) and np.array_equal(fg, fo) and (fg["weight_sum"] == 5.0).all()
    gpu.close()
    orc.close()


def test_render_decomposition_invariance(env, monkeypatch):
    """Size-independent properties: (i) two runs are identical; (ii) rendering tile subsets wave by wave into the device
    film equals the whole render; (iii) the result does not depend on the path-batch capacity (SHM_BATCH_PATHS)."""
    lib, oracle_py, render, scenes = env
    from shimmer_amd import scene as scn
    sc = scenes.ganesha_proxy(lib, 160, 120, n=64)
    p = render.make_params(seed=21, spp=12, max_depth=5)
    gpu = render.Renderer(lib, sc.desc, 0)
    f1, s1 = gpu.render(p)
    f2, s2 = gpu.render(p)
    assert np.array_equal(f1, f2) and s1["rays_closest"] == s2["rays_closest"]
    assert (f1["weight_sum"] == 12.0).all()
    gpu.clear()
    idx = np.arange(gpu.n_tiles)
    for ws, we in scn.wave_schedule(12):
        gpu.render_waves(p, tile_indices=idx[idx % 3 != 0], waves=[(ws, we)])
        gpu.render_waves(p, tile_indices=idx[idx % 3 == 0], waves=[(ws, we)])
    assert np.array_equal(gpu.read_film(), f1)
    gpu.clear()
    gpu.render_device(p)  # shm_render_device fuses the 1,1,2,4,4-sample waves into one launch: same film
    assert np.array_equal(gpu.read_film(), f1)
    gpu.close()
    monkeypatch.setenv("SHM_BATCH_PATHS", "8192")  # forces many small batches per wave
    gpu_small = render.Renderer(lib, sc.desc, 0)
    f3, _ = gpu_small.render(p)
    gpu_small.close()
    assert np.array_equal(f3, f1)
    # (iv) ... nor on whether the any-hit kernel of bounce b runs on the second stream beside the closest-hit kernel of bounce
    # b+1 (the default for batches this small) or everything is serialised on one stream
    monkeypatch.delenv("SHM_BATCH_PATHS")
    monkeypatch.setenv("SHM_OVERLAP_PATHS", "0")
    gpu_serial = render.Renderer(lib, sc.desc, 0)
    f4, s4 = gpu_serial.render(p)
    gpu_serial.close()
    assert np.array_equal(f4, f1) and s4["rays_any"] == s1["rays_any"] and s4["nodes_any"] == s1["nodes_any"]


@pytest.mark.parametrize("kind", ["quads", "instance_grid", "coated_quads", "one_sphere"])
def test_batch_and_overlap_invariance_of_the_general_scene_classes(env, monkeypatch, kind):
    """The decomposition properties of the test above on the classes round 6 gave their own traversal instantiations or thresholds: an object of bilinear patches (five
    waves per SIMD, the LDS save area), the same coated (the staged LayeredBxDF pipeline beside it), a grid of instances (32 parked lanes), one sphere among triangles
    (seven waves): 8192-path batches and serialised streams render the same film and counters as the defaults, and the defaults equal the oracle."""
    lib, oracle_py, render, scenes = env
    sc = {"quads": lambda: scenes.ganesha_proxy(lib, 96, 72, n=40, variant="quads"),
          "coated_quads": lambda: scenes.ganesha_proxy(lib, 96, 72, n=40, variant="quads", coated=True),
          "instance_grid": lambda: scenes.ganesha_proxy(lib, 96, 72, n=40, variant="instance_grid"),
          "one_sphere": lambda: scenes.ganesha_proxy(lib, 96, 72, n=40, variant="one_sphere")}[kind]()
    p = render.make_params(seed=8, spp=6, max_depth=5)
    keys = ("paths", "rays_closest", "rays_any", "nodes_closest", "nodes_any", "tris_closest", "tris_any")
    gpu = render.Renderer(lib, sc.desc, 0)
    f1, s1 = gpu.render(p)
    gpu.close()
    orc = oracle_py.Oracle(sc.desc)
    fo, so = orc.render(p, n_threads=8)
    orc.close()
    assert f1.tobytes() == fo.tobytes() and all(s1[k] == so[k] for k in keys)
    for env_kv in (("SHM_BATCH_PATHS", "8192"), ("SHM_OVERLAP_PATHS", "0")):
        monkeypatch.setenv(*env_kv)
        g = render.Renderer(lib, sc.desc, 0)
        f, st = g.render(p)
        g.close()
        monkeypatch.delenv(env_kv[0])
        assert f.tobytes() == f1.tobytes(), env_kv
        assert all(st[k] == s1[k] for k in keys), env_kv


def test_full_size_properties_and_crop_parity(env):
    """BASELINE-scale geometry (S3: 4.3 M triangles, 8.5 M nodes) at a reduced frame: the oracle renders a 64x64 crop
    of tiles and the GPU must match it bit for bit; whole-frame invariants hold (weights, finiteness)."""
    lib, oracle_py, render, scenes = env
    from shimmer_amd import scene as scn
    sc = scenes.ganesha_proxy(lib, 256, 256)
    assert sc.info["n_primitives"] == 4305626
    p = render.make_params(seed=0, spp=4, max_depth=5)
    gpu = render.Renderer(lib, sc.desc, 0)
    fg, sg = gpu.render(p)
    assert (fg["weight_sum"] == 4.0).all() and np.isfinite(fg["rgb_sum"]).all() and sg["paths"] == 256 * 256 * 4
    orc = oracle_py.Oracle(sc.desc)
    crop = (96, 96, 160, 160)
    tiles, n = scn.tiles_for(lib, crop)
    fo, so = orc.render(p, n_threads=os.cpu_count() or 1, tiles=tiles, n_tiles=n)
    assert np.array_equal(fg[96:160, 96:160], fo[96:160, 96:160])
    # traversal statistics on this scene: tens of nodes per ray (the HBM-bound regime the roofline is quoted on)
    assert 20 < sg["nodes_closest"] / sg["rays_closest"] < 200
    rays = _rays(sc, 20000, 42)  # incoherent ray batch, bitwise
    hg, st_g = gpu.trace(rays)
    ho, st_o = orc.trace(rays)
    assert np.array_equal(hg.view(np.uint8), ho.view(np.uint8)) and st_g["nodes_closest"] == st_o["nodes_closest"]
    gpu.close()
    orc.close()


def test_headline_frame_at_full_size(env):
    """BASELINE.json configs[2] exactly as bench.py times it — S3 with 4 305 626 primitives, 1024 x 1024, 256 spp, maxdepth 5, one 268 M-path
    batch — through the size-independent properties the path offers, plus an oracle crop at the full sample count:
      (i)   two renders are identical (the persistent queues hand rays to lanes in a run-dependent order; nothing may depend on it);
      (ii)  every pixel holds exactly 256 samples and finite sums; paths = pixels x spp; closest-hit rays >= paths; shadow rays <= closest;
      (iii) the frame rendered as two interleaved tile sets into one device film equals the whole render, bit for bit;
      (iv)  a 16 x 16 pixel block in the object's silhouette at all 256 samples equals the oracle's film of those tiles, bit for bit,
            and the node / triangle visit counters of that block equal the oracle's."""
    lib, oracle_py, render, scenes = env
    from shimmer_amd import scene as scn
    sc = scenes.ganesha_proxy(lib, 1024, 1024)
    assert sc.info["n_primitives"] == 4305626
    p = render.make_params(seed=0, spp=256, max_depth=5)
    gpu = render.Renderer(lib, sc.desc, 0)
    gpu.clear()
    s1 = gpu.render_device(p)
    f1 = gpu.read_film()
    gpu.clear()
    s2 = gpu.render_device(p)
    f2 = gpu.read_film()
    assert np.array_equal(f1, f2)
    for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
        assert s1[k] == s2[k], k
    assert (f1["weight_sum"] == 256.0).all() and np.isfinite(f1["rgb_sum"]).all() and (f1["rgb_sum"] >= 0).all()
    assert s1["paths"] == 1024 * 1024 * 256 and s1["rays_closest"] >= s1["paths"] and 0 < s1["rays_any"] <= s1["rays_closest"]
    assert s1["rays_closest"] + s1["rays_any"] > 1_000_000_000  # the 1.2 G rays of the headline number
    gpu.clear()
    idx = np.arange(gpu.n_tiles)
    gpu.render_device(p, tile_indices=idx[idx % 2 == 0])
    gpu.render_device(p, tile_indices=idx[idx % 2 == 1])
    assert np.array_equal(gpu.read_film(), f1)
    crop = (504, 440, 520, 456)  # (x0, y0, x1, y1): on the displaced cube-sphere
    tiles, n = scn.tiles_for(lib, crop)
    orc = oracle_py.Oracle(sc.desc)
    fo, so = orc.render(p, n_threads=os.cpu_count() or 1, tiles=tiles, n_tiles=n)
    orc.close()
    assert np.array_equal(f1[440:456, 504:520], fo[440:456, 504:520])
    # the same tiles alone on the GPU: counters equal the oracle's
    sel = np.array([i for i in range(gpu.n_tiles) if (lambda t: t.x0 >= 504 and t.x1 <= 520 and t.y0 >= 440 and t.y1 <= 456)(gpu.tiles[i])])
    assert len(sel) == n == 4
    gpu.clear()
    sc_ = gpu.render_device(p, tile_indices=sel)
    for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
        assert sc_[k] == so[k], k
    gpu.close()


@pytest.mark.parametrize("variant,crop", [("patch_emitter", (504, 440, 520, 456)), ("one_sphere", (152, 920, 168, 936)), ("instanced", (504, 440, 520, 456)),
                                          ("environment", (504, 440, 520, 456)), ("textured_floor", (504, 840, 520, 856)),
                                          ("quads", (504, 440, 520, 456))])  # (round 6: the object as 2.15 M bilinear patches — the five-wave traversal kernels)
def test_mixed_shape_frames_at_full_size(env, variant, crop):
    """The headline frame with the shapes a real PBRT-v4 scene mixes into its triangles (bench.py's round-5 side results: the emitter as ONE bilinear patch, a sphere
    beside the object, the object as a TransformedPrimitive; and the object under an ImageInfinitelight: the sorted fused kernel's textured instantiation) at its own size — 4.3 M primitives, 1024 x 1024, 256 spp, one 268 M-path batch through k_trace5<., GEN> and the
    general fused kernel: two renders identical in film and counters; every pixel 256 samples, finite; a 16 x 16 block at all 256 samples — on the object, on the sphere
    where there is one — equal to the oracle's film bit for bit, with the block's node / primitive visit counters."""
    lib, oracle_py, render, scenes = env
    from shimmer_amd import scene as scn
    sc = scenes.ganesha_proxy(lib, 1024, 1024, variant=variant)
    p = render.make_params(seed=0, spp=256, max_depth=5)
    gpu = render.Renderer(lib, sc.desc, 0)
    gpu.clear()
    s1 = gpu.render_device(p)
    f1 = gpu.read_film()
    gpu.clear()
    s2 = gpu.render_device(p)
    assert np.array_equal(f1, gpu.read_film())
    for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
        assert s1[k] == s2[k], k
    assert (f1["weight_sum"] == 256.0).all() and np.isfinite(f1["rgb_sum"]).all() and s1["paths"] == 1024 * 1024 * 256
    x0, y0, x1, y1 = crop
    tiles, n = scn.tiles_for(lib, crop)
    orc = oracle_py.Oracle(sc.desc)
    fo, so = orc.render(p, n_threads=os.cpu_count() or 1, tiles=tiles, n_tiles=n)
    orc.close()
    assert np.array_equal(f1[y0:y1, x0:x1], fo[y0:y1, x0:x1])
    assert fo[y0:y1, x0:x1]["rgb_sum"].max() > 0
    sel = np.array([i for i in range(gpu.n_tiles) if (lambda t: t.x0 >= x0 and t.x1 <= x1 and t.y0 >= y0 and t.y1 <= y1)(gpu.tiles[i])])
    assert len(sel) == n == 4
    gpu.clear()
    sc_ = gpu.render_device(p, tile_indices=sel)
    for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
        assert sc_[k] == so[k], k
    gpu.close()


def test_c4_frame_at_full_size(env):
    """BASELINE.json configs[3] at its own size — the crown proxy (64 dispersive-glass + 16 rough-gold icospheres, 410 k triangles), 1000 x 1400,
    256 spp, maxdepth 32 (358 M paths in one batch, 33 bounces through the staged vertex / per-class scatter kernels): run-to-run identity,
    sample counts, and a 16 x 16 block through glass at all 256 samples against the oracle, film and counters bit for bit."""
    lib, oracle_py, render, scenes = env
    from shimmer_amd import scene as scn
    sc = scenes.crown_proxy(lib, 1000, 1400)
    p = render.make_params(seed=0, spp=256, max_depth=32)
    gpu = render.Renderer(lib, sc.desc, 0)
    gpu.clear()
    s1 = gpu.render_device(p)
    f1 = gpu.read_film()
    gpu.clear()
    s2 = gpu.render_device(p)
    assert np.array_equal(gpu.read_film(), f1)
    for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
        assert s1[k] == s2[k], k
    assert (f1["weight_sum"] == 256.0).all() and np.isfinite(f1["rgb_sum"]).all() and s1["paths"] == 1000 * 1400 * 256
    x0, y0 = 496, 696
    tiles, n = scn.tiles_for(lib, (x0, y0, x0 + 16, y0 + 16))
    orc = oracle_py.Oracle(sc.desc)
    fo, so = orc.render(p, n_threads=os.cpu_count() or 1, tiles=tiles, n_tiles=n)
    orc.close()
    assert np.array_equal(f1[y0:y0 + 16, x0:x0 + 16], fo[y0:y0 + 16, x0:x0 + 16])
    sel = np.array([i for i in range(gpu.n_tiles) if (lambda t: t.x0 >= x0 and t.x1 <= x0 + 16 and t.y0 >= y0 and t.y1 <= y0 + 16)(gpu.tiles[i])])
    assert len(sel) == n == 4
    gpu.clear()
    sb = gpu.render_device(p, tile_indices=sel)
    for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
        assert sb[k] == so[k], k
    assert so["rays_closest"] / so["paths"] > 3.0  # the block is on the glass: long specular chains
    gpu.close()


def test_c2_frame_at_full_size(env):
    """BASELINE.json configs[1] at its own size — the 32-triangle Cornell-style box, 512 x 512, 64 spp, maxdepth 5 (16.8 M paths) — WHOLE frame against the
    oracle (it renders the frame in seconds on the test box's host cores): every f64 film sum and all seven counters bit for bit, through the entry point
    bench.py times (shm_render_device, <= 64-spp launches) — and the same film once more through the reference's own spp-wave schedule (shm_render_wave)."""
    lib, oracle_py, render, scenes = env
    sc = scenes.cornell_box(lib, 512, 512)
    assert sc.info["n_primitives"] == 32
    p = render.make_params(seed=0, spp=64, max_depth=5)
    gpu = render.Renderer(lib, sc.desc, 0)
    gpu.clear()
    sg = gpu.render_device(p)
    fg = gpu.read_film()
    orc = oracle_py.Oracle(sc.desc)
    fo, so = orc.render(p, n_threads=os.cpu_count() or 1)
    orc.close()
    assert sg["paths"] == 512 * 512 * 64 and (fg["weight_sum"] == 64.0).all() and np.isfinite(fg["rgb_sum"]).all()
    assert np.array_equal(fg, fo)
    assert float(np.max(np.abs(render.film_to_rgb(fg) - render.film_to_rgb(fo)))) < L_INF_TOL
    for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
        assert sg[k] == so[k], k
    fw, sw = gpu.render(p)  # clear, the waves 1, 1, 2, 4, 8, 16, 32 one by one (integrator.rs:226-322), read back
    assert np.array_equal(fw, fo) and sw["rays_closest"] == so["rays_closest"] and sw["rays_any"] == so["rays_any"]
    gpu.close()


def test_instance_root_inside_another_tree_is_rejected(env):
    """An instance whose root node lies INSIDE the top-level tree (an instanced sub-tree) would get two device indices in the sibling-pair re-layout of the node array:
    scene creation names it instead of traversing something else (advisor, round 3). Whatever layer refuses it first, it is refused with a message, on the GPU path."""
    lib, oracle_py, render, scenes = env
    sc = scenes.instanced_scene(lib, 16, 16, n_instances=2)
    assert sc.desc.n_instances >= 1 and sc.desc.n_nodes > 3
    saved = sc.desc.instances[0].root_node
    try:
        sc.desc.instances[0].root_node = 1  # the first child of the top-level root: not a tree of its own
        with pytest.raises(Exception) as ei:
            render.Renderer(lib, sc.desc, 0).close()
        assert "instance" in str(ei.value).lower() or "tree" in str(ei.value).lower() or "unsupported" in str(ei.value).lower(), str(ei.value)
    finally:
        sc.desc.instances[0].root_node = saved
    r = render.Renderer(lib, sc.desc, 0)  # (and the untouched description still loads)
    r.close()


def test_two_primitives_sharing_one_instance_record_are_rejected(env):
    """The traversal finds an instance's leaf slot — what a hit inside it is named by — in the ShmInstance record itself: two instance primitives that name ONE record would
    overwrite each other's slot (advisor, round 5). Scene creation refuses the description with a message instead of reporting the other primitive's slot."""
    from shimmer_amd import abi
    lib, oracle_py, render, scenes = env
    sc = scenes.instanced_scene(lib, 16, 16, n_instances=2)
    prims = [i for i in range(sc.desc.n_primitives) if sc.desc.primitives[i].shape_kind == abi.SHM_SHAPE_INSTANCE]
    assert len(prims) >= 2 and sc.desc.primitives[prims[0]].shape_index != sc.desc.primitives[prims[1]].shape_index
    saved = sc.desc.primitives[prims[1]].shape_index
    try:
        sc.desc.primitives[prims[1]].shape_index = sc.desc.primitives[prims[0]].shape_index
        with pytest.raises(Exception) as ei:
            render.Renderer(lib, sc.desc, 0).close()
        assert "instance" in str(ei.value).lower(), str(ei.value)
    finally:
        sc.desc.primitives[prims[1]].shape_index = saved
    render.Renderer(lib, sc.desc, 0).close()  # (the untouched description still loads)


@pytest.mark.parametrize("first", ["-1", "0", "3"])
def test_fused_all_materials_kernel_from_any_bounce(env, monkeypatch, first):
    """Triangle scenes with several BxDF classes (no textures, no coated materials) shade with ONE fused all-materials launch per bounce from bounce
    SHM_TAIL_FUSED_BOUNCE on (k_shade_tail*.hip, k_shade_fused_*.hip) and with the staged kernels (k_vertex + one scatter kernel per class) before it: whichever bounce the switch
    is made at — never (-1), from the camera ray's hit on (0: the default), from bounce 3 — the films and the counters are the same bits. (The knob is read at scene creation.)"""
    lib, oracle_py, render, scenes = env
    cases = [(scenes.cornell_box(lib, 48, 48, glass=True), 6, 14), (scenes.crown_proxy(lib, 40, 56, level=1, n_glass=6, n_gold=3), 4, 12),
             # ... the same kernel's other instantiations: with textures (k_shade_fused_tex.hip), for scenes with spheres / patches / instances (k_shade_fused_gen.hip), both
             # (k_shade_fused_gen_tex.hip: the environment map is an image)
             (scenes.cornell_box(lib, 40, 40, textured=True, textured_coated_ceiling=False), 4, 6), (scenes.instanced_scene(lib, 48, 36), 4, 6),
             (scenes.three_spheres(lib, 48, 36, camera=(0.75, 0.5, 9.0), environment=scenes.environment_image(32)), 4, 5)]
    for sc, spp, depth in cases:
        p = render.make_params(seed=5, spp=spp, max_depth=depth)
        monkeypatch.delenv("SHM_TAIL_FUSED_BOUNCE", raising=False)
        g = render.Renderer(lib, sc.desc, 0)
        f_def, s_def = g.render(p)
        g.close()
        monkeypatch.setenv("SHM_TAIL_FUSED_BOUNCE", first)
        g = render.Renderer(lib, sc.desc, 0)
        f_alt, s_alt = g.render(p)
        g.close()
        assert np.array_equal(f_def, f_alt), (first, sc.name)
        for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
            assert s_def[k] == s_alt[k], (first, sc.name, k)


def test_workspace_is_not_reallocated_between_equal_renders(env):
    """A frame large enough to take the whole workspace budget (64 M paths: more than an eighth of it) rendered three times: the second and third render find
    the workspace of the first. Round 4 found the opposite — the per-path estimate of the budget was 16 bytes high, the budget crept from call to call, and every
    frame of a coated scene freed and re-allocated 150 GB (7 s against 0.1 s of rendering). Wall-clock, with a generous bound: allocation takes seconds."""
    import time
    lib, oracle_py, render, scenes = env
    sc = scenes.ganesha_proxy(lib, 1024, 1024, n=24, coated=True)
    p = render.make_params(seed=0, spp=64, max_depth=5)
    gpu = render.Renderer(lib, sc.desc, 0)
    times = []
    for _ in range(3):
        gpu.clear()
        t0 = time.perf_counter()
        st = gpu.render_device(p)
        times.append(time.perf_counter() - t0)
    gpu.close()
    assert st["paths"] == 1024 * 1024 * 64
    assert times[1] < 1.5 and times[2] < 1.5, times  # (the first one allocates: several seconds)


def test_layered_pdf_zero_over_zero_is_the_references(env):
    """LayeredBxDF::pdf (bxdf.rs:1491-1506) takes the reflecting interface's sample without testing its pdf: a cosine-hemisphere sample on the
    horizon gives power_heuristic(1, 0, 1, 0) = 0 / 0 and the NaN reaches the film (evaluate_pixel_sample leaves it, integrator.rs:377-382).
    Found on the coated S3 frame at pixel (714, 268), sample 83: the HIP path must poison the same pixel and match every other one, bit
    for bit."""
    lib, oracle_py, render, scenes = env
    from shimmer_amd import scene as scn
    sc = scenes.ganesha_proxy(lib, 1024, 1024, coated=True)
    p = render.make_params(seed=0, spp=128, max_depth=5)
    x, y, sample = 714, 268, 83
    x0, y0 = x & ~7, y & ~7
    tiles, n = scn.tiles_for(lib, (x0, y0, x0 + 8, y0 + 8))
    orc = oracle_py.Oracle(sc.desc)
    fo, _ = orc.render(p, n_threads=1, tiles=tiles, n_tiles=n, waves=[(sample, sample + 1)])
    orc.close()
    assert np.isnan(fo["rgb_sum"][y, x]).all() and np.isfinite(fo["rgb_sum"][y0:y0 + 8, x0:x0 + 8]).sum() == 3 * 63
    gpu = render.Renderer(lib, sc.desc, 0)
    sel = np.array([i for i in range(gpu.n_tiles) if (gpu.tiles[i].x0, gpu.tiles[i].y0) == (x0, y0)])
    gpu.clear()
    gpu.render_waves(p, tile_indices=sel, waves=[(sample, sample + 1)])
    fg = gpu.read_film()
    gpu.close()
    assert np.array_equal(fg[y0:y0 + 8, x0:x0 + 8].view(np.uint64), fo[y0:y0 + 8, x0:x0 + 8].view(np.uint64))  # NaN bits included


def test_reference_quirks_off_no_nan_and_still_bit_exact(env):
    """SHM_REFERENCE_QUIRKS off (ShmRenderParams::disable_reference_quirks = 1): the coated S3 tile whose pixel (714, 268) the reference
    poisons (previous test) renders finite at every one of its 128 samples, and the HIP path still equals the oracle bit for bit — the
    switch lives in the shared arithmetic, both sides take it from the render parameters."""
    lib, oracle_py, render, scenes = env
    from shimmer_amd import scene as scn
    sc = scenes.ganesha_proxy(lib, 1024, 1024, coated=True)
    x0, y0 = 714 & ~7, 268 & ~7
    tiles, n = scn.tiles_for(lib, (x0, y0, x0 + 8, y0 + 8))
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    sel = np.array([i for i in range(gpu.n_tiles) if (gpu.tiles[i].x0, gpu.tiles[i].y0) == (x0, y0)])
    films = {}
    for quirks in (True, False):
        p = render.make_params(seed=0, spp=128, max_depth=5, reference_quirks=quirks)
        fo, so = orc.render(p, n_threads=os.cpu_count() or 1, tiles=tiles, n_tiles=n)
        gpu.clear()
        sg = gpu.render_waves(p, tile_indices=sel)
        fg = gpu.read_film()
        assert np.array_equal(fg[y0:y0 + 8, x0:x0 + 8].view(np.uint64), fo[y0:y0 + 8, x0:x0 + 8].view(np.uint64))
        for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
            assert sg[k] == so[k], k
        films[quirks] = fg[y0:y0 + 8, x0:x0 + 8]["rgb_sum"]
    assert not np.isfinite(films[True]).all() and np.isfinite(films[False]).all()
    gpu.close(); orc.close()


@pytest.mark.parametrize("name", ["S1_sphere_light", "three_spheres_environment", "S2_cornell_textured", "S2_cornell_coated", "instanced", "S3_small_instance_grid",
                                  "S3_small_instanced", "S2_cornell_patches_skewed", "S3_small_mesh_emitter", "S3_small_quads", "S3_small_one_sphere"])
def test_render_parity_with_reference_quirks_off(env, name):
    """Every site the switch touches (sphere (u, v) through acos, SphericalMapping, LayeredBxDF::pdf's guard, the dropped non-finite
    samples; round 6: triangle and patch emitters sampled as PBRT-v4 samples them, the shadow ray's way into an instance — the any-hit kernels' STRICT instantiations, at
    both occupancies — and the instanced hit's interaction) through the wavefront pipeline == the scalar oracle, bit for bit, with the quirks off as with them on."""
    lib, oracle_py, render, scenes = env
    sc, spp, depth = SCENES[name](scenes, lib)
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    p = render.make_params(seed=3, spp=spp, max_depth=depth, reference_quirks=False)
    fg, sg = gpu.render(p)
    fo, so = orc.render(p, n_threads=os.cpu_count() or 1)
    assert np.array_equal(fg, fo) and np.isfinite(fg["rgb_sum"]).all()
    for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
        assert sg[k] == so[k], k
    gpu.close(); orc.close()


@pytest.mark.parametrize("integrator", ["simplepath", "randomwalk"])
def test_other_integrators_with_reference_quirks_off(env, integrator):
    """uniform_hemisphere_pdf (1/(2 pi) with the quirks off) is reached by SimplePath's uniform sampling and the uniform sky's sample_li."""
    lib, oracle_py, render, scenes = env
    sc = scenes.three_spheres(lib, 48, 32, camera=(0.75, 0.5, 9.0))
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    p = render.make_params(seed=4, spp=8, max_depth=4, integrator=integrator, sample_lights=False, sample_bsdf=False, reference_quirks=False)
    fg, _ = gpu.render(p)
    fo, _ = orc.render(p, n_threads=os.cpu_count() or 1)
    assert np.array_equal(fg, fo) and np.isfinite(fg["rgb_sum"]).all()
    gpu.close(); orc.close()


def test_no_silent_fallback(env):
    """The product never routes through the oracle: libshimmer_hip.so exports no orc_* symbol, and a Renderer holds a
    device film pointer."""
    lib, oracle_py, render, scenes = env
    from shimmer_amd import abi
    syms = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True).stdout
    assert "orc_" not in syms and "shm_render_wave" in syms
    sc = scenes.cornell_box(lib, 16, 16)
    gpu = render.Renderer(lib, sc.desc, 0)
    ptr, nbytes = gpu.film_device_ptr()
    assert ptr and nbytes == 16 * 16 * 32
    gpu.close()


def test_integrator_mirror_parity(env):
    """The C++ host mirror of the reference's interface (create_integrator("path", ...)->render(options), integrator.hpp):
    the reference's own spp-wave loop (1, 1, 2, 4, 8, ... over all 8x8 tiles) driving shm_render_wave gives the oracle's film
    bit for bit, the same counters, and the wave count of integrator.rs:231-233."""
    import ctypes as C
    from shimmer_amd import abi
    lib, oracle_py, render, scenes = env
    sc = scenes.cornell_box(lib, 72, 56)
    spp, depth, seed = 21, 5, 6
    film = np.zeros((56, 72), dtype=render.FILM_DTYPE)
    st, waves = abi.ShmStats(), C.c_int32(0)
    abi.check(lib, lib.shm_integrator_render(b"path", C.byref(sc.desc), 0, depth, 0, 1, 1, spp, seed, 0, 0, film.ctypes.data_as(C.c_void_p),
                                             C.byref(st), C.byref(waves)), "shm_integrator_render")
    fo, so = oracle_py.Oracle(sc.desc).render(render.make_params(seed=seed, spp=spp, max_depth=depth), n_threads=os.cpu_count() or 1)
    assert np.array_equal(film, fo)
    assert st.rays_closest == so["rays_closest"] and st.rays_any == so["rays_any"] and st.nodes_closest == so["nodes_closest"]
    assert waves.value == len(scn_wave_schedule(spp)) == 6  # [0,1) [1,2) [2,4) [4,8) [8,16) [16,21)


def scn_wave_schedule(spp):
    from shimmer_amd.scene import wave_schedule
    return wave_schedule(spp)


@pytest.mark.parametrize("sample_lights,sample_bsdf", [(True, True), (True, False), (False, True), (False, False)])
def test_simple_path_integrator_parity(env, sample_lights, sample_bsdf):
    """SimplePathIntegrator (integrator.rs:573-733; create_integrator("simplepath")): every combination of its two switches,
    on a random scene (all shape / material / light kinds, including the uniform infinite light sampled with
    allow_incomplete_pdf = false) — the oracle's film and counters bit for bit, through the render params and through the
    C++ integrator mirror."""
    import ctypes as C
    from shimmer_amd import abi
    lib, oracle_py, render, scenes = env
    sc = scenes.random_scene(lib, 1)  # seed 1: thin-lens camera + the sky light
    p = render.make_params(seed=8, spp=6, max_depth=4, integrator="simplepath", sample_lights=sample_lights, sample_bsdf=sample_bsdf)
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    fg, sg = gpu.render(p)
    fo, so = orc.render(p, n_threads=os.cpu_count() or 1)
    assert np.array_equal(fg, fo) and np.isfinite(render.film_to_rgb(fg)).all()
    for k in ("rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
        assert sg[k] == so[k], k
    assert (sg["rays_any"] > 0) == sample_lights
    film = np.zeros_like(fo)
    abi.check(lib, lib.shm_integrator_render(b"simplepath", C.byref(sc.desc), 0, 4, 0, int(sample_lights), int(sample_bsdf), 6, 8, 0, 0,
                                             film.ctypes.data_as(C.c_void_p), None, None), "shm_integrator_render")
    assert np.array_equal(film, fo)
    gpu.close(); orc.close()


def test_random_walk_integrator_parity(env):
    """RandomWalkIntegrator through create_integrator("randomwalk"): the GPU records (le, f cos) per depth and folds the recursion
    backwards; film sums and counters must equal the oracle's literal recursion bit for bit (random scene with the sky light,
    and the Cornell box at a depth where most walks reach the limit)."""
    import ctypes as C
    from shimmer_amd import abi
    lib, oracle_py, render, scenes = env
    for sc, spp, depth in ((scenes.random_scene(lib, 1), 6, 5), (scenes.cornell_box(lib, 48, 40), 9, 7)):
        p = render.make_params(seed=4, spp=spp, max_depth=depth, integrator="randomwalk")
        gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
        fg, sg = gpu.render(p)
        fo, so = orc.render(p, n_threads=os.cpu_count() or 1)
        assert np.array_equal(fg, fo) and np.isfinite(render.film_to_rgb(fg)).all() and render.film_to_rgb(fg).max() > 0
        for k in ("rays_closest", "rays_any", "nodes_closest", "tris_closest"):
            assert sg[k] == so[k], k
        assert sg["rays_any"] == 0
        film = np.zeros_like(fo)
        abi.check(lib, lib.shm_integrator_render(b"randomwalk", C.byref(sc.desc), 0, depth, 0, 1, 1, spp, 4, 0, 0,
                                                 film.ctypes.data_as(C.c_void_p), None, None), "shm_integrator_render")
        assert np.array_equal(film, fo)
        gpu.close(); orc.close()


@pytest.mark.parametrize("integrator", ["path", "simplepath", "randomwalk"])
@pytest.mark.parametrize("texture_filter", ["point", "bilinear", "trilinear", "ewa"])
def test_textured_parity_per_filter_and_integrator(env, integrator, texture_filter):
    """Image textures under each MIPMap filter and each integrator (the two general ones only carry the camera ray's
    differentials, every later vertex goes through Camera::approximate_dp_dxy), with and without pixel jitter (the differential
    scaling of integrator.rs:356-362 and camera.rs:344-348) and at an spp where that scale is not a power of two."""
    lib, oracle_py, render, scenes = env
    sc = scenes.cornell_box(lib, 40, 40, textured=True, texture_filter=texture_filter)
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    for dpj, spp, dtf in ((False, 6, False), (True, 2, False), (False, 3, True)):
        p = render.make_params(seed=5, spp=spp, max_depth=5, integrator=integrator, disable_pixel_jitter=dpj, disable_texture_filtering=dtf)
        fg, sg = gpu.render(p)
        fo, so = orc.render(p, n_threads=os.cpu_count() or 1)
        assert np.array_equal(fg, fo) and np.isfinite(render.film_to_rgb(fg)).all() and render.film_to_rgb(fg).max() > 0
        for k in ("rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
            assert sg[k] == so[k], k
    gpu.close(); orc.close()


@pytest.mark.parametrize("integrator", ["simplepath", "randomwalk"])
def test_environment_map_parity_other_integrators(env, integrator):
    """ImageInfinitelight under the two general integrators: SimplePathIntegrator samples the plain distribution
    (allow_incomplete_pdf = false), RandomWalkIntegrator only evaluates le on escape."""
    lib, oracle_py, render, scenes = env
    sc = scenes.three_spheres(lib, 48, 32, camera=(0.75, 0.5, 9.0), environment=scenes.environment_image(16))
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    p = render.make_params(seed=6, spp=6, max_depth=4, integrator=integrator)
    fg, sg = gpu.render(p)
    fo, so = orc.render(p, n_threads=os.cpu_count() or 1)
    assert np.array_equal(fg, fo) and np.isfinite(render.film_to_rgb(fg)).all() and render.film_to_rgb(fg).max() > 0
    for k in ("rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
        assert sg[k] == so[k], k
    gpu.close(); orc.close()


@pytest.mark.parametrize("integrator", ["path", "simplepath", "randomwalk"])
def test_force_diffuse_parity(env, integrator):
    """options.force_diffuse (the BSDF of every vertex replaced by DiffuseBxDF(rho_hd estimate), three more sampler dimensions per
    vertex) on scenes with specular, layered, textured and instanced materials."""
    lib, oracle_py, render, scenes = env
    for sc in (scenes.crown_proxy(lib, 30, 42, level=1, n_glass=6, n_gold=2), scenes.cornell_box(lib, 32, 32, textured=True), scenes.random_scene(lib, 13)):
        gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
        p = render.make_params(seed=9, spp=4, max_depth=6, integrator=integrator, force_diffuse=True)
        fg, sg = gpu.render(p)
        fo, so = orc.render(p, n_threads=os.cpu_count() or 1)
        assert np.array_equal(fg, fo) and np.isfinite(render.film_to_rgb(fg)).all()
        for k in ("rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
            assert sg[k] == so[k], k
        gpu.close(); orc.close()


@pytest.mark.parametrize("option", ["force_diffuse", "regularize"])
def test_rare_options_reach_the_one_pass_kernels(env, option):
    """options.force_diffuse / regularize change the BxDF INSIDE the scatter half: those renders run the one-pass kernels of each class — k_scatter<CLASS_LAYERED, *, *> for the
    coated materials (the staged stages have no such code), k_scatter<CLASS_DIELECTRIC, *, *> instead of the specular / general pair, and under a map with regularize their
    K_ENV_LIGHT units — on scenes WITHOUT textures, triangles and with patches (round 6: the kernel-coverage run found them unreached, profiles/r06_kernel_coverage.txt)."""
    lib, oracle_py, render, scenes = env
    cases = [scenes.cornell_box(lib, 40, 40, coated=True, glass_too=True), scenes.cornell_box(lib, 40, 40, coated=True, glass_too=True, patches=True),
             scenes.cornell_box(lib, 40, 40, coated=True, glass_too=True, environment=scenes.environment_image(32)),
             scenes.cornell_box(lib, 40, 40, coated=True, glass_too=True, patches=True, environment=scenes.environment_image(32))]
    for sc in cases:
        gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
        p = render.make_params(seed=4, spp=4, max_depth=8, force_diffuse=option == "force_diffuse", regularize=option == "regularize")
        fg, sg = gpu.render(p)
        fo, so = orc.render(p, n_threads=os.cpu_count() or 1)
        assert np.array_equal(fg, fo), (sc.name, option)
        for k in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
            assert sg[k] == so[k], (sc.name, option, k)
        gpu.close(); orc.close()


def test_textured_scenes_split_their_plain_diffuse_hits(env, monkeypatch):
    """A scene WITH material textures (round 5): the split pass (k_split_plain, render.hip) sends the hits on DiffuseMaterials that bind no texture to the lean fused kernel
    — their whole vertex, without the textured class's differentials: a diffuse bounce ends them (interaction.rs:430-514) — and everything else to the textured kernels.
    On by itself where a quarter of the primitives are plain diffuse (S3 with a textured floor); forced on (SHM_SPLIT_PASS=1) and off (0) on the textured Cornell boxes — with
    and without the coated ceiling, with an environment map shining in as well — and on a random scene: the same bits, equal to the oracle's."""
    lib, oracle_py, render, scenes = env
    cases = [(scenes.ganesha_proxy(lib, 64, 64, n=24, variant="textured_floor"), 6, 5), (scenes.cornell_box(lib, 40, 40, textured=True), 4, 6),
             (scenes.ganesha_proxy(lib, 48, 48, n=16, variant="textured_hidden"), 4, 5),  # (the textured material out of sight: every hit is plain, q_split holds the escaped rays only)
             (scenes.cornell_box(lib, 40, 40, textured=True, textured_coated_ceiling=False, environment=scenes.environment_image(32)), 4, 6),
             (scenes.random_scene(lib, 13), 4, 5),
             # ... and without textures (the same pass in front of k_vertex, which then diverts nothing itself): coated + diffuse, with patches, with glass
             (scenes.ganesha_proxy(lib, 64, 64, n=24, coated=True), 4, 5), (scenes.cornell_box(lib, 40, 40, coated=True, patches=True), 4, 5),
             (scenes.cornell_box(lib, 40, 40, coated=True, mix=True, environment=scenes.environment_image(32)), 4, 5)]
    for sc, spp, depth in cases:
        p = render.make_params(seed=17, spp=spp, max_depth=depth)
        orc = oracle_py.Oracle(sc.desc)
        fo, so = orc.render(p, n_threads=os.cpu_count() or 1)
        orc.close()
        for mode in ("1", "0", None):
            if mode is None: monkeypatch.delenv("SHM_SPLIT_PASS", raising=False)
            else: monkeypatch.setenv("SHM_SPLIT_PASS", mode)
            gpu = render.Renderer(lib, sc.desc, 0)
            fg, sg = gpu.render(p)
            gpu.close()
            assert np.array_equal(fg, fo), (sc.name, mode)
            for k in ("rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
                assert sg[k] == so[k], (sc.name, mode, k)
        monkeypatch.delenv("SHM_SPLIT_PASS", raising=False)


def test_environment_map_scenes_run_the_lean_class(env, monkeypatch):
    """A scene without coated materials whose only image is an ImageInfinitelight (light.rs:805-981) shades with the ENV_LIGHT instantiations of the lean fused kernel
    (all-diffuse: k_shade_lean_env.hip, k_shade_lean_gen_env.hip) or of the material-sorted fused kernel (glass, metal: k_shade_tail_sorted_env.hip,
    k_shade_fused_gen_env.hip) — no ray differentials, no auxiliary rays, bounce 0 on known constants — instead of the textured class's kernels:
    triangles and spheres / instances, every integrator, against the oracle; and
    one Renderer through path -> force_diffuse (a STAGED render: the textured class's kernels and their workspace arrays) -> path again."""
    lib, oracle_py, render, scenes = env
    cases = [scenes.ganesha_proxy(lib, 48, 48, n=24, variant="environment"),
             scenes.three_spheres(lib, 48, 36, camera=(0.75, 0.5, 9.0), environment=scenes.environment_image(32)),
             # ... and with other BxDF classes (glass and metal, the sorted fused kernel's ENV_LIGHT instantiations: k_shade_tail_sorted_env.hip, k_shade_fused_gen_env.hip)
             scenes.crown_proxy(lib, 40, 56, level=1, n_glass=6, n_gold=3, environment=scenes.environment_image(32)),
             scenes.instanced_scene(lib, 48, 36, environment=scenes.environment_image(32)),
             # ... and with coated materials — the reference's showcase class, a coated object under a map —: the staged kernels' K_ENV_LIGHT units (k_vertex_env.hip,
             # k_scatter_*_env.hip, k_scatter_layered*_env.hip), triangles / with bilinear patches / with glass beside the coated boxes
             scenes.ganesha_proxy(lib, 48, 48, n=24, coated=True, variant="environment"),
             scenes.cornell_box(lib, 40, 40, coated=True, patches=True, environment=scenes.environment_image(32)),
             scenes.cornell_box(lib, 40, 40, coated=True, mix=True, environment=scenes.environment_image(32))]
    for sc in cases:
        orc = oracle_py.Oracle(sc.desc)
        films = {}
        for integrator in ("path", "simplepath", "randomwalk"):
            p = render.make_params(seed=21, spp=6, max_depth=5, integrator=integrator)
            fo, so = orc.render(p, n_threads=os.cpu_count() or 1)
            gpu = render.Renderer(lib, sc.desc, 0)
            fg, sg = gpu.render(p)
            gpu.close()
            assert np.array_equal(fg, fo), (sc.name, integrator)
            for k in ("rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
                assert sg[k] == so[k], (sc.name, integrator, k)
            films[integrator] = fo
        assert render.film_to_rgb(films["path"]).max() > 0
        p = render.make_params(seed=21, spp=6, max_depth=5)
        # one scene object through the class change and back
        gpu = render.Renderer(lib, sc.desc, 0)
        pf = render.make_params(seed=21, spp=6, max_depth=5, force_diffuse=True)
        fo_f, so_f = orc.render(pf, n_threads=os.cpu_count() or 1)
        for params, want in ((p, films["path"]), (pf, fo_f), (p, films["path"])):
            fg, _ = gpu.render(params)
            assert np.array_equal(fg, want), sc.name
        gpu.close(); orc.close()


def test_extreme_render_parameters(env):
    """Edges of the parameter space: max_depth 0 (camera rays and emission only, no any-hit launch), 1 spp, a 5 x 3 film (one
    partial tile), maximum path depth 64 on a closed mirror-like box (paths that live long), a scene without any light, and the
    error returns for arguments the reference would panic on."""
    import ctypes as C
    from shimmer_amd import abi, scene as scn
    lib, oracle_py, render, scenes = env
    sc = scenes.cornell_box(lib, 40, 24)
    gpu, orc = render.Renderer(lib, sc.desc, 0), oracle_py.Oracle(sc.desc)
    for kw in (dict(spp=3, max_depth=0), dict(spp=1, max_depth=5), dict(spp=2, max_depth=64)):
        p = render.make_params(seed=12, **kw)
        fg, sg = gpu.render(p)
        fo, so = orc.render(p, n_threads=4)
        assert np.array_equal(fg, fo), kw
        assert sg["rays_closest"] == so["rays_closest"] and sg["rays_any"] == so["rays_any"]
        if kw["max_depth"] == 0:
            assert sg["rays_any"] == 0 and sg["rays_closest"] == 40 * 24 * 3
    # invalid arguments: codes, not crashes
    bad = render.make_params(seed=1, spp=2, max_depth=300)
    st = abi.ShmStats()
    assert lib.shm_render_wave(gpu.handle, C.byref(bad), gpu.tiles, gpu.n_tiles, 0, 2, C.byref(st)) == -1
    ok = render.make_params(seed=1, spp=2, max_depth=3)
    assert lib.shm_render_wave(gpu.handle, C.byref(ok), gpu.tiles, gpu.n_tiles, 2, 2, C.byref(st)) == -1  # empty sample range
    outside = (abi.ShmTile * 1)(abi.ShmTile(32, 16, 48, 32))
    assert lib.shm_render_wave(gpu.handle, C.byref(ok), outside, 1, 0, 1, C.byref(st)) == -1 and b"tile" in lib.shm_last_error()
    unknown = render.make_params(seed=1, spp=2, max_depth=3)
    unknown.integrator = 9
    assert lib.shm_render_wave(gpu.handle, C.byref(unknown), gpu.tiles, gpu.n_tiles, 0, 1, C.byref(st)) == -2
    gpu.close(); orc.close()
    # a tiny film and no light at all: everything black, still bit-identical and complete
    b = scn.SceneBuilder()
    b.set_film(5, 3)
    rfw = b.set_camera_look_at(lib, (0, 0, 4), (0, 0, 0), (0, 1, 0), 40.0)
    p_, vi = scenes._box((-1, -1, -1), (1, 1, 1))
    b.add_mesh(scenes._to_render(p_, rfw), vi, b.material_diffuse(0.5))
    desc, _ = b.build(lib)
    gpu, orc = render.Renderer(lib, desc, 0), oracle_py.Oracle(desc)
    pr = render.make_params(seed=2, spp=4, max_depth=3)
    fg, sg = gpu.render(pr)
    fo, so = orc.render(pr, n_threads=2)
    assert fg.shape == (3, 5) and np.array_equal(fg, fo) and (fg["rgb_sum"] == 0).all() and (fg["weight_sum"] == 4.0).all()
    assert sg["rays_any"] == 0 == so["rays_any"]
    gpu.close(); orc.close()
