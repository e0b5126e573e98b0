"""The prefetch of k_shade<lean> (shimmer_amd/csrc/k_shade.inl, K_SHADE_PREFETCH; its kernel: k_shade_lean_prefetch.hip): while a lane shades one vertex of its chunk it
fetches the path and the compact hit record of its next one and the queue entry of the one after. Only loads move, so films and counters are what they were: f64 film
sums and all seven counters are compared bit for bit

  against the CPU oracle, at path counts that put the prefetch's index clamps on their edges — fewer paths than one SHADE2_BLOCK (256: no lane has a second vertex), a
  count that is no multiple of 256 (the last block's lanes run out at different vertices), exactly SHADE_CHUNK (2048: every lane's eighth vertex is the queue's last
  block) and SHADE_CHUNK + 1 (a second workgroup with one path) —, each one batch: render_device fuses a small render's samples into one launch per kernel, so
  pixels of the tile subset x spp is the queue length at bounce 0 (the identity queue, rng0 / pixel0); depth 5 then walks the indirect queue, which Russian roulette
  and escaped rays thin to lengths of their own. Once with the independent sampler, once with ZSobol (the *_zs build of the kernel);

  against the same library with the prefetch switched off (SHM_SHADE_PREFETCH=0, read at scene creation: the launchers then take the plain instantiation) — a batch of
  more than 768 x SHADE_CHUNK paths, in which workgroups take a second chunk through the grid-stride loop, and a scene with a second material class, in which the
  kernel works the diverted queue off (n_in, q_lean).

The scene is all-diffuse, a few dozen triangles, with a reflecting emitter: the lean kernel and k_emit_jobs shade it."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTERS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")

SHADE2_BLOCK, SHADE_CHUNK = 256, 2048  # (wavefront.h)
W, H = 51, 43  # 6 x 5 whole 8x8 tiles, a column of five 3x8 ones, a row of six 8x3 ones and a 3x3 corner
DEPTH, SEED = 5, 13


def _tilted_quad(cx, cy, cz=0.0, half=0.24, yaw=0.35, pitch=0.2):
    """A quad facing the camera (+z in world space), turned a little about y and x so that no normal component is 0."""
    c, s, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    local = np.array([[-half, -half, 0], [half, -half, 0], [half, half, 0], [-half, half, 0]], np.float64)
    p = local @ (ry @ rx).T + np.array([cx, cy, cz])
    return p.astype(np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def _scene(lib, scenes, variant="diffuse", w=W, h=H):
    """variant "diffuse": every material a DiffuseMaterial; "coated": one quad coated (the staged pipeline; plain diffuse hits are diverted to the lean kernel)."""
    from shimmer_amd.scene import SceneBuilder, blackbody_dense
    b = SceneBuilder()
    b.set_film(w, h)
    rfw = b.set_camera_look_at(lib, (0, 1, 3.4), (0, 1, 0), (0, 1, 0), 39.0)
    white, grey = b.material_diffuse(0.7), b.material_diffuse(0.5)
    other = b.material_coated_diffuse(reflectance=0.6, roughness=0.2, thickness=0.02) if variant == "coated" else grey
    room_p, room_vi = scenes._box((-1, 0, -1), (1, 2, 1), faces="xXyYz")
    b.add_mesh(scenes._to_render(room_p, rfw), room_vi, white)
    for k, (cx, cy, yaw, mat) in enumerate([(-0.6, 0.45, 0.35, grey), (0.0, 0.45, -0.3, other), (0.6, 0.45, 0.5, white), (-0.6, 1.15, 0.1, white), (0.0, 1.15, 0.25, grey),
                                            (0.6, 1.15, -0.45, grey)]):
        p, vi = _tilted_quad(cx, cy, yaw=yaw, pitch=0.2 - 0.1 * k)
        b.add_mesh(scenes._to_render(p, rfw), vi, mat)
    # the emitter: reflecting, so that paths go on from it (k_emit_jobs: the hit itself, and the previous vertex rebuilt from its hit record)
    p, vi = scenes._quad((-0.35, 1.98, -0.35), (0.35, 1.98, -0.35), (0.35, 1.98, 0.35), (-0.35, 1.98, 0.35))
    b.add_mesh(scenes._to_render(p, rfw), vi, b.material_diffuse(0.4), emission=blackbody_dense(6500.0), emission_scale=12.0)
    desc, _ = b.build(lib)
    desc.keepalive = b  # (the description points into the builder's arrays)
    return desc


@pytest.fixture(scope="module")
def env(gpu_lib):
    import oracle_py
    from shimmer_amd import render, scenes
    return gpu_lib, oracle_py, render, scenes


def _tile_pixels(t):
    return (t.x1 - t.x0) * (t.y1 - t.y0)


def _pick_tiles(renderer, whole, edge, corner):
    """Indices of `whole` 64-pixel tiles, `edge` 24-pixel ones and `corner` 9-pixel ones of the film, in tile order."""
    want = {64: whole, 24: edge, 9: corner}
    out = []
    for i in range(renderer.n_tiles):
        n = _tile_pixels(renderer.tiles[i])
        if want.get(n, 0) > 0:
            want[n] -= 1
            out.append(i)
    assert not any(want.values()), want
    return out


# name: (whole tiles, edge tiles, corner tiles, spp) -> paths in the one batch
EDGE_CASES = {
    "below_one_block": (1, 0, 0, 3),         # 192 < SHADE2_BLOCK
    "no_multiple_of_256": (5, 0, 0, 7),      # 2240 = 8 x 256 + 192: a second workgroup whose last block is partial
    "exactly_one_chunk": (4, 0, 0, 8),       # 2048
    "one_chunk_and_one": (30, 5, 1, 1),      # 1920 + 120 + 9 = 2049
}


def _paths(case):
    whole, edge, corner, spp = EDGE_CASES[case]
    return (64 * whole + 24 * edge + 9 * corner) * spp


def test_the_cases_are_on_the_edges():
    assert _paths("below_one_block") < SHADE2_BLOCK
    assert _paths("no_multiple_of_256") % SHADE2_BLOCK != 0 and _paths("no_multiple_of_256") > SHADE_CHUNK
    assert _paths("exactly_one_chunk") == SHADE_CHUNK
    assert _paths("one_chunk_and_one") == SHADE_CHUNK + 1


def _render_device(render, lib, desc, params, tile_indices=None):
    """One clear + render_device + read-back on a fresh scene object: (film, stats)."""
    gpu = render.Renderer(lib, desc, 0)
    try:
        gpu.clear()
        stats = gpu.render_device(params, tile_indices)
        return gpu.read_film(), stats
    finally:
        gpu.close()


def _same(a, b, what):
    (fa, sa), (fb, sb) = a, b
    for field in ("rgb_sum", "weight_sum"):
        assert np.array_equal(fa[field].view(np.uint64), fb[field].view(np.uint64)), (what, field)
    for k in COUNTERS:
        assert sa[k] == sb[k], (what, k)


@pytest.mark.parametrize("sampler", ["independent", "zsobol"])
@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_edge_counts_equal_the_oracle(env, monkeypatch, case, sampler):
    lib, oracle_py, render, scenes = env
    monkeypatch.delenv("SHM_SHADE_PREFETCH", raising=False)
    whole, edge, corner, spp = EDGE_CASES[case]
    desc = _scene(lib, scenes)
    params = render.make_params(seed=SEED, spp=spp, max_depth=DEPTH, **({"sampler": "zsobol"} if sampler == "zsobol" else {}))
    gpu = render.Renderer(lib, desc, 0)
    try:
        idx = _pick_tiles(gpu, whole, edge, corner)
        assert sum(_tile_pixels(gpu.tiles[i]) for i in idx) * spp == _paths(case)
        gpu.clear()
        s_gpu = gpu.render_device(params, idx)
        f_gpu = gpu.read_film()
        tiles, n_tiles = gpu._tile_subset(idx)
    finally:
        gpu.close()
    assert s_gpu["paths"] == _paths(case)
    orc = oracle_py.Oracle(desc)
    try:
        f_cpu, s_cpu = orc.render(params, n_threads=min(16, os.cpu_count() or 1), tiles=tiles, n_tiles=n_tiles)
    finally:
        orc.close()
    assert np.isfinite(f_cpu["rgb_sum"]).all() and f_cpu["rgb_sum"].max() > 0
    assert s_cpu["rays_any"] > 0 and s_cpu["rays_closest"] > s_cpu["paths"]  # (next-event estimation ran, and paths went on past bounce 0)
    _same((f_gpu, s_gpu), (f_cpu, s_cpu), (case, sampler))


def _on_and_off(env, monkeypatch, variant, w, h, spp):
    lib, _, render, scenes = env
    params = render.make_params(seed=SEED, spp=spp, max_depth=DEPTH)
    monkeypatch.setenv("SHM_SHADE_PREFETCH", "0")
    off = _render_device(render, lib, _scene(lib, scenes, variant, w, h), params)
    monkeypatch.delenv("SHM_SHADE_PREFETCH")
    on = _render_device(render, lib, _scene(lib, scenes, variant, w, h), params)
    assert np.isfinite(on[0]["rgb_sum"]).all() and on[0]["rgb_sum"].max() > 0 and on[1]["rays_any"] > 0
    _same(on, off, variant)
    return on


def test_a_second_chunk_per_workgroup_equals_prefetch_off(env, monkeypatch):
    """160 x 120 at 96 spp is one batch of 1 843 200 paths: more than the 768 x SHADE_CHUNK a grid of three workgroups on each of 256 CUs covers in one round."""
    w, h, spp = 160, 120, 96
    assert w * h * spp > 768 * SHADE_CHUNK
    on = _on_and_off(env, monkeypatch, "diffuse", w, h, spp)
    assert on[1]["paths"] == w * h * spp


def test_the_diverted_queue_equals_prefetch_off(env, monkeypatch):
    """A coated quad beside the diffuse ones: the staged k_vertex diverts the plain diffuse hits, and the lean kernel works that queue off (its count is n_in's)."""
    _on_and_off(env, monkeypatch, "coated", W, H, 8)
