"""PBRT-v4's shape alpha (ShmTriangleMesh / ShmBilinearPatchMesh / ShmSphere::alpha; shimmer_amd/csrc/shm/alpha.h) on the CPU: the oracle's two traversals, which accept a
leaf primitive through prim_intersect and so run the text the traversal kernels run (tests/test_gpu_shape_alpha.py holds those to the oracle bit for bit).
Ray batches are 4096 rays, films 32 x 32 at 1 spp; every scene has a handful of primitives.

The scene of the ray tests: the camera at the origin (render space = world space), a wall at z = -3, and in front of it, at z = -2, the shape that is cut — by default a
quad of two triangles over [-1, 1]^2 with (u, v) = (0, 0) .. (1, 1). The rays start on the plane z = 0 and run towards -z."""
import ctypes as C
import json
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_py
from shimmer_amd import abi, render, scene as scn, scenes
from shimmer_amd.scene import blackbody_dense

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests" / "golden"))
ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -2  # (include/shimmer_hip.h)
STATS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")
N_RAYS = 4096
QUAD_P = np.array([(-1, -1, -2), (1, -1, -2), (1, 1, -2), (-1, 1, -2)], np.float32)
QUAD_VI = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
QUAD_UV = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
SHAPES = ("triangles", "patch", "sphere", "disk", "instance")


def build(lib, shape="triangles", alpha=None, present=True, material=None, make_alpha=None):
    """-> (builder, desc). `alpha`: None, a number, or — through `make_alpha(builder)` — a handle made on this builder. `present=False`: the scene without the cut shape
    (inside an instance: the object keeps its other triangle). The cut shape is added LAST, so every other shape keeps its index whether it is there or not."""
    b = scn.SceneBuilder()
    b.set_film(4, 4)
    b.set_camera_look_at(lib, (0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0)
    grey = b.material_diffuse(0.5)
    m = grey if material is None else material(b)
    wall = np.array([(-3, -3, -3), (3, -3, -3), (3, 3, -3), (-3, 3, -3)], np.float32)
    b.add_mesh(wall, QUAD_VI, grey)
    if make_alpha is not None:
        alpha = make_alpha(b)
    at = np.eye(4)
    at[:3, 3] = (0.0, 0.0, -2.0)
    if shape == "instance":
        b.begin_object("card")
        b.add_mesh(np.array([(-1.4, -0.2, 0), (-1.2, -0.2, 0), (-1.3, 0.2, 0)], np.float32), np.array([[0, 1, 2]], np.uint32), grey)
        if present:
            b.add_mesh(QUAD_P + np.float32([0, 0, 2]), QUAD_VI, m, uv=QUAD_UV, alpha=alpha)
        b.end_object()
        place = np.diag([1.0, 0.9, 1.0, 1.0])
        c, s = np.cos(0.3), np.sin(0.3)
        place[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ place[:3, :3]
        place[:3, 3] = (0.1, 0.0, -2.0)
        b.add_instance("card", place)
    elif present:
        if shape == "triangles":
            b.add_mesh(QUAD_P, QUAD_VI, m, uv=QUAD_UV, alpha=alpha)
        elif shape == "patch":
            b.add_patch_mesh(QUAD_P[[0, 1, 3, 2]] + np.float32([[0, 0, 0], [0, 0, 0.2], [0, 0, 0.1], [0, 0, -0.1]]), np.array([[0, 1, 2, 3]], np.uint32), m,
                             uv=QUAD_UV[[0, 1, 3, 2]], alpha=alpha)
        elif shape == "sphere":
            b.add_sphere(0.9, m, render_from_object=at, alpha=alpha)
        elif shape == "disk":
            b.add_disk(1.0, m, inner_radius=0.2, render_from_object=at, alpha=alpha)
    desc, _ = b.build(lib)
    desc.keep_alive = b  # (the builder owns the arrays the description points at)
    return b, desc


def rays_at(targets_xy, seed=5, spread=0.05):
    """One ray per target (x, y) on the plane z = -2, from a point of the plane z = 0 within `spread` of it: no two rays alike, all nearly parallel to -z."""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.asarray(targets_xy, np.float64)
    o = np.column_stack([t + rng.uniform(-spread, spread, t.shape), np.zeros(len(t))])
    d = np.column_stack([t, np.full(len(t), -2.0)]) - o
    rays = np.zeros((len(t), 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = o, d, np.inf
    return rays


def uniform_targets(n=N_RAYS, seed=3, half=0.95):
    return np.random.Generator(np.random.PCG64(seed)).uniform(-half, half, (n, 2))


def trace(desc, rays, any_hit=False):
    o = oracle_py.Oracle(desc)
    try:
        out, st = o.trace(rays, any_hit=any_hit)
    finally:
        o.close()
    return out, st


def shape_keys(desc, hits):
    """Per ray what the hit names, independent of the leaf order: (shape kind, shape index) of the primitive, -1s for a miss; and whether it lies inside an instance."""
    kinds = np.array([desc.primitives[i].shape_kind for i in range(desc.n_primitives)], np.int64)
    index = np.array([desc.primitives[i].shape_index for i in range(desc.n_primitives)], np.int64)
    prim = hits["prim"].astype(np.int64)
    miss = prim < 0
    return np.where(miss, -1, kinds[np.maximum(prim, 0)]), np.where(miss, -1, index[np.maximum(prim, 0)]), (hits["instance"] != 0)


def same_hits(desc_a, ha, desc_b, hb):
    ka, kb = shape_keys(desc_a, ha), shape_keys(desc_b, hb)
    return all(np.array_equal(x, y) for x, y in zip(ka, kb)) and all(np.array_equal(ha[f].view(np.uint32), hb[f].view(np.uint32)) for f in ("t", "b0", "b1", "b2", "phi"))


def on_cut_shape(desc, hits, shape):
    kind, index, inside = shape_keys(desc, hits)
    if shape == "instance":
        return inside & (index >= 3)  # (the wall's triangles are 0 and 1, the object's other triangle 2, the card's 3 and 4)
    if shape == "triangles":
        return (kind == abi.SHM_SHAPE_TRIANGLE) & (index >= 2)
    return kind == {"patch": abi.SHM_SHAPE_BILINEAR_PATCH, "sphere": abi.SHM_SHAPE_SPHERE, "disk": abi.SHM_SHAPE_SPHERE}[shape]


# ---- HashFloat, restated ------------------------------------------------------------------------------------------------------------------
def hash_float(o, d):
    """alpha_hash_float of shm/alpha.h in NumPy's wrapping uint64 arithmetic: hash_v3(hash_v3(0, o), d) >> 40, times 2^-24."""
    def mix(v):
        v = v ^ (v >> np.uint64(31))
        v = v * np.uint64(0x7fb5d329728ea185)
        v = v ^ (v >> np.uint64(27))
        v = v * np.uint64(0x81dadef4bc2dd44d)
        return v ^ (v >> np.uint64(33))
    h = np.zeros(len(o), np.uint64)
    with np.errstate(over="ignore"):
        for x in list(np.asarray(o, np.float32).T) + list(np.asarray(d, np.float32).T):
            h = mix(h ^ (np.ascontiguousarray(x).view(np.uint32).astype(np.uint64) + np.uint64(0x9e3779b97f4a7c15)))
    return (h >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


# ---- constants ----------------------------------------------------------------------------------------------------------------------------
def test_constant_one_changes_nothing(lib):
    """A texture that says 1 everywhere (kept as a texture: a handle, not the number the builder would drop): the hit records and the seven counters of both traversals
    equal, bit for bit, those of the scene without the parameter, and so does the BVH."""
    _, plain = build(lib)
    b, cut = build(lib, make_alpha=lambda b: b.ftex_constant(1.0))
    assert b.meshes[1]["alpha"] != 0 and cut.meshes[1].alpha == b.meshes[1]["alpha"] and plain.meshes[1].alpha == 0
    assert cut.n_nodes == plain.n_nodes and bytes(C.string_at(cut.nodes, cut.n_nodes * C.sizeof(abi.ShmBvhNode))) == bytes(C.string_at(plain.nodes, plain.n_nodes * C.sizeof(abi.ShmBvhNode)))
    rays = rays_at(uniform_targets(half=1.6))
    for any_hit in (False, True):
        a, sa = trace(plain, rays, any_hit)
        c, sc = trace(cut, rays, any_hit)
        assert a.tobytes() == c.tobytes() and sa == sc, any_hit
    hits, _ = trace(cut, rays)
    assert on_cut_shape(cut, hits, "triangles").sum() > 1000  # (the rays do meet the quad)
    # a NUMBER of 1 or more stores nothing at all, as PBRT-v4 drops it
    b1, d1 = build(lib, alpha=1.0)
    assert b1.meshes[1]["alpha"] == 0 and len(b1.float_textures) == 0


def test_constant_zero_is_absence(lib):
    """No ray reports the quad; every ray's hit — what it names, t, the barycentrics — is that of the scene built without the quad, and so is the any-hit answer.
    (The test fails on a build that ignores the field: there the quad stops three rays in four.)"""
    _, without = build(lib, present=False)
    _, cut = build(lib, alpha=0.0)
    assert cut.meshes[1].alpha != 0
    rays = rays_at(uniform_targets(half=1.6))
    hw, _ = trace(without, rays)
    hc, _ = trace(cut, rays)
    assert not on_cut_shape(cut, hc, "triangles").any()
    assert same_hits(without, hw, cut, hc)
    short = rays.copy()
    short[:, 6] = 1.2  # (t is about 1 at the quad and 1.5 at the wall: these rays end between the two)
    for r in (rays, short):
        aw, _ = trace(without, r, any_hit=True)
        ac, _ = trace(cut, r, any_hit=True)
        assert np.array_equal(aw, ac)
    assert trace(cut, short, any_hit=True)[0].sum() == 0 and trace(build(lib)[1], short, any_hit=True)[0].sum() > 1000


def test_constant_half_is_a_fair_and_repeatable_coin(lib):
    """Of the N = 4096 rays that geometrically hit the quad, the accepted share lies within 5 binomial standard deviations of one half: 0.5 +- 5 sqrt(0.25 / 4096) =
    0.5 +- 0.04. Which rays are accepted is HashFloat(o, d) <= 0.5, restated above — ray by ray, for both traversals — and the hash alone stays inside the same bound.
    Tracing the batch a second time gives the same bits."""
    _, cut = build(lib, alpha=0.5)
    rays = rays_at(uniform_targets())
    solid, _ = trace(build(lib)[1], rays)
    assert on_cut_shape(build(lib)[1], solid, "triangles").all()  # all N of them hit the quad
    hits, st = trace(cut, rays)
    accepted = on_cut_shape(cut, hits, "triangles")
    share = accepted.mean()
    print(f"accepted share {share:.4f} of {N_RAYS}")
    assert abs(share - 0.5) <= 0.04
    u = hash_float(rays[:, 0:3], rays[:, 3:6])
    assert abs((u <= 0.5).mean() - 0.5) <= 0.04 and 0.0 <= u.min() and u.max() < 1.0
    assert np.array_equal(accepted, u <= np.float32(0.5))
    short = rays.copy()
    short[:, 6] = 1.2
    occluded, _ = trace(cut, short, any_hit=True)
    assert np.array_equal(occluded.astype(bool), accepted)
    again, st2 = trace(cut, rays)
    assert again.tobytes() == hits.tobytes() and st == st2
    # a rejected candidate leaves the ray as it was: it goes on to the wall, with the wall's t
    wall, _ = trace(build(lib, present=False)[1], rays)
    assert np.array_equal(hits["t"][~accepted], wall["t"][~accepted]) and np.array_equal(hits["t"][accepted], solid["t"][accepted])


# ---- textures -----------------------------------------------------------------------------------------------------------------------------
def cell_targets(cells, margin, seed=9):
    """Targets on the quad [-1, 1]^2 whose (u, v) keep `margin` (in cells) away from every edge of a cells x cells grid."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cell = rng.integers(0, cells, (N_RAYS, 2))
    uv = (cell + rng.uniform(margin, 1.0 - margin, (N_RAYS, 2))) / cells
    return uv * 2.0 - 1.0


def quad_uv_of(desc, hits):
    idx = np.array([desc.primitives[i].shape_index for i in range(desc.n_primitives)], np.int64)[np.maximum(hits["prim"], 0)] - 2  # 0 or 1: which triangle of the quad
    corners = QUAD_UV.astype(np.float64)[QUAD_VI.astype(np.int64)[np.clip(idx, 0, 1)]]  # (n, 3, 2)
    b = np.stack([hits["b0"], hits["b1"], hits["b2"]], axis=1).astype(np.float64)
    return np.einsum("nk,nkc->nc", b, corners)


def test_checkerboard_cuts_where_numpy_says_so(lib):
    """A 4 x 4 checkerboard over the quad's (u, v): a ray is accepted exactly where an evaluation of the checker written here — PBRT-v4's: the value is 1 where
    floor(4 u) + floor(4 v) is odd — says 1 at the hit's (u, v), taken from the solid quad's hit record. Every target keeps 0.1 cell (0.025 in u, v; rounding moves a
    hit's (u, v) by 1e-6) away from the cell edges, and the test asserts that every ray's hit does."""
    make = lambda b: b.ftex_checkerboard(None, None, mapping=b.add_texture_mapping("uv", su=4.0, sv=4.0))
    _, solid = build(lib)
    _, cut = build(lib, make_alpha=make)
    rays = rays_at(cell_targets(4, 0.15), spread=0.02)
    hs, _ = trace(solid, rays)
    assert on_cut_shape(solid, hs, "triangles").all()
    st = 4.0 * quad_uv_of(solid, hs)
    assert (np.abs(st - np.round(st)) >= 0.1).all()
    want = ((np.floor(st[:, 0]) + np.floor(st[:, 1])) % 2) == 1
    hc, _ = trace(cut, rays)
    got = on_cut_shape(cut, hc, "triangles")
    assert np.array_equal(got, want) and 0.3 < want.mean() < 0.7
    assert np.array_equal(hc["t"][got], hs["t"][got])
    short = rays.copy()
    short[:, 6] = 1.2
    assert np.array_equal(trace(cut, short, any_hit=True)[0].astype(bool), want)


def test_cutout_lines_up_with_a_material_texture(lib):
    """The same 8 x 8 image of zeros and ones, point-sampled, as the alpha of the quad and as the reflectance of an uncut copy: the rays accepted by the cut quad are the
    rays at whose hit the copy's reflectance — SpectrumTexture::evaluate at the interaction hit_interaction builds, zero differentials — is not zero."""
    img = (np.random.Generator(np.random.PCG64(21)).random((8, 8)) < 0.5).astype(np.float32)
    assert 20 < img.sum() < 44
    _, cut = build(lib, make_alpha=lambda b: b.ftex_image(img, filter="point"))
    bs, solid = build(lib, material=lambda b: b.material_diffuse(b.add_image_texture(img, filter="point", color_space=False)))
    rays = rays_at(uniform_targets(), spread=0.02)
    hc, _ = trace(cut, rays)
    got = on_cut_shape(cut, hc, "triangles")
    o = oracle_py.Oracle(solid)
    F = C.c_float
    refl = bs.materials[-1].a
    assert refl.kind == abi.SHM_SPECTRUM_IMAGE_TEXTURE
    o.lib.orc_fn_hit_interaction.restype = C.c_int
    o.lib.orc_fn_spectrum_texture_evaluate.restype = None
    hs, _ = o.trace(rays)
    uv = quad_uv_of(solid, hs)
    lam = (F * 4)(500.0, 550.0, 600.0, 650.0)
    want = np.zeros(N_RAYS, bool)
    for i in range(N_RAYS):
        ray = abi.ShmRay()
        ray.o[:], ray.d[:], ray.t_max = [float(x) for x in rays[i, 0:3]], [float(x) for x in rays[i, 3:6]], float("inf")
        out, hit = (F * 12)(), abi.ShmHit()
        assert o.lib.orc_fn_hit_interaction(o.handle, C.byref(ray), out, C.byref(hit)) == 1
        # the interaction's (u, v) in the float32 operations triangle_interaction runs: b0 uv0 + b1 uv1 + b2 uv2
        tri = QUAD_VI[desc_tri(solid, hit.prim)]
        b = np.float32([hit.b0, hit.b1, hit.b2])
        uvf = (b[0] * QUAD_UV[tri[0]] + b[1] * QUAD_UV[tri[1]]).astype(np.float32) + b[2] * QUAD_UV[tri[2]]
        ctx = (F * 18)(*([out[0], out[1], out[2]] + [0.0] * 6 + [out[3], out[4], out[5]] + [float(uvf[0]), float(uvf[1])] + [0.0] * 4))
        val = (F * 4)()
        o.lib.orc_fn_spectrum_texture_evaluate(o.handle, C.byref(refl), ctx, lam, val)
        want[i] = any(v != 0.0 for v in val)
    o.close()
    assert np.array_equal(got, want) and 0.3 < want.mean() < 0.7
    # ... and with the image itself, read at the float64 (u, v): row 0 is the top (v = 1), away from texel edges
    st = uv * 8.0
    inner = (np.abs(st - np.round(st)) > 1e-3).all(axis=1)
    texel = img[np.clip(7 - np.floor(st[:, 1]).astype(int), 0, 7), np.clip(np.floor(st[:, 0]).astype(int), 0, 7)] != 0
    assert inner.sum() > N_RAYS - 64 and np.array_equal(got[inner], texel[inner])


def desc_tri(desc, prim):
    return desc.primitives[prim].shape_index - 2


# ---- every shape, and inside an instance -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s in SHAPES if s != "triangles"])
def test_shapes_and_instances(lib, shape):
    """Alpha on a sphere, a disk, a bilinear patch and a triangle mesh inside an instance: constant 0 is the scene without the shape, a texture that says 1 the scene
    without the parameter (hit records and counters of both traversals), and one half accepts by the hash of the ray the test ran with — inside the instance, the
    instance-space ray: not the hash of the ray that was sent."""
    rays = rays_at(uniform_targets(half=1.5))
    _, plain = build(lib, shape)
    _, one = build(lib, shape, make_alpha=lambda b: b.ftex_constant(1.0))
    _, zero = build(lib, shape, alpha=0.0)
    _, without = build(lib, shape, present=False)
    hp, sp = trace(plain, rays)
    n_on = on_cut_shape(plain, hp, shape).sum()
    assert n_on > 500, n_on
    for any_hit in (False, True):
        a, sa = trace(plain, rays, any_hit)
        c, sc = trace(one, rays, any_hit)
        assert a.tobytes() == c.tobytes() and sa == sc, (shape, any_hit)
    hz, _ = trace(zero, rays)
    hw, _ = trace(without, rays)
    assert not on_cut_shape(zero, hz, shape).any() and same_hits(without, hw, zero, hz)
    short = rays.copy()
    short[:, 6] = 1.2
    assert np.array_equal(trace(zero, short, any_hit=True)[0], trace(without, short, any_hit=True)[0])
    _, half = build(lib, shape, alpha=0.5)
    hh, _ = trace(half, rays)
    acc = on_cut_shape(half, hh, shape)
    # a sphere's far side stands behind a rejected near side: count the rays whose NEAREST candidate was accepted
    first = acc & (hh["t"].view(np.uint32) == hp["t"].view(np.uint32))
    cand = on_cut_shape(plain, hp, shape)
    share = first.sum() / cand.sum()
    print(f"{shape}: accepted share {share:.4f} of {cand.sum()}")
    assert abs(share - 0.5) <= 5.0 * np.sqrt(0.25 / cand.sum())
    u = hash_float(rays[:, 0:3], rays[:, 3:6])
    if shape == "instance":
        assert not np.array_equal(first[cand], (u <= 0.5)[cand])  # the instance-space ray is another ray
    else:
        assert np.array_equal(first[cand], (u <= 0.5)[cand])


# ---- shadows ------------------------------------------------------------------------------------------------------------------------------
def shadow_scene(lib, alpha, present=True):
    """A floor lit by a point light straight above it, a square occluder halfway up, and a camera below the occluder's height that looks at the floor under it."""
    b = scn.SceneBuilder()
    b.set_film(32, 32)
    rfw = np.asarray(b.set_camera_look_at(lib, (0.0, 0.9, 3.2), (0.0, 0.0, 0.0), (0, 1, 0), 36.0), np.float32).reshape(4, 4)
    to_r = lambda p: (np.asarray(p, np.float32) + rfw[:3, 3][None, :]).astype(np.float32)
    grey = b.material_diffuse(0.5)
    b.add_mesh(to_r([(-4, 0, -4), (-4, 0, 4), (4, 0, 4), (4, 0, -4)]), QUAD_VI, grey)
    b.light_point(tuple(float(x) for x in to_r([(0.0, 3.0, 0.0)])[0]), blackbody_dense(5000.0), scale=20.0)
    if present:
        b.add_mesh(to_r([(-0.7, 1.5, -0.7), (-0.7, 1.5, 0.7), (0.7, 1.5, 0.7), (0.7, 1.5, -0.7)]), QUAD_VI, grey, uv=QUAD_UV, alpha=alpha)
    desc, _ = b.build(lib)
    desc.keep_alive = b
    return b, desc


def test_half_alpha_occluder_casts_half_a_shadow(lib):
    """Direct lighting only (max depth 1), ONE sample per pixel, so that a pixel's value is its sample's contribution times the visibility of one shadow ray: under the
    0.5-alpha occluder every pixel equals, bit for bit, either the unoccluded film's or the fully occluded film's — it lies between them —, and over the pixel set
    S = {pixels the solid occluder leaves black and the unoccluded film lights} (its size M is printed and asserted > 150) the number of lit pixels is Binomial(M, 1/2):
    within 5 sqrt(M) / 2 of M / 2, which is the same statement as the film's sum over S being within that bound of the mean of the two films where the samples weigh alike."""
    p = render.make_params(seed=4, spp=1, max_depth=1)
    films = {}
    for name, (alpha, present) in dict(unoccluded=(None, False), solid=(None, True), half=(0.5, True)).items():
        _, desc = shadow_scene(lib, alpha, present)
        o = oracle_py.Oracle(desc)
        films[name], _ = o.render(p, n_threads=4)
        o.close()
    u, s, h = (films[k]["rgb_sum"] for k in ("unoccluded", "solid", "half"))
    assert np.isfinite(u).all() and (u >= s).all()
    shadow = (s.sum(axis=2) == 0.0) & (u.sum(axis=2) > 0.0)
    m = int(shadow.sum())
    print(f"shadowed pixels M = {m}")
    assert m > 150
    lit = (h == u).all(axis=2)
    dark = (h == s).all(axis=2)
    assert (lit | dark).all() and ((h >= s) & (h <= u)).all()
    k = int((lit & shadow).sum())
    print(f"lit under the half occluder: {k} of {m}")
    assert abs(k - m / 2.0) <= 5.0 * np.sqrt(m) / 2.0
    mean = 0.5 * (u[shadow].sum() + s[shadow].sum())
    assert abs(h[shadow].sum() - mean) <= 5.0 * np.sqrt((u[shadow].sum(axis=1) ** 2).sum()) / 2.0


# ---- rejections ---------------------------------------------------------------------------------------------------------------------------
def create(desc):
    orc = oracle_py.load()
    handle = C.c_void_p()
    rc = orc.orc_scene_create(C.byref(desc), C.byref(handle))
    msg = orc.orc_last_error().decode() if rc != 0 else ""
    if rc == 0:
        orc.orc_scene_destroy(handle)
    return rc, msg


def test_flatten_scene_rejects_what_is_out_of_scope(lib):
    em = dict(emission=blackbody_dense(5000.0), emission_scale=2.0)
    for add in (lambda b, m, kw: b.add_mesh(QUAD_P, QUAD_VI, m, **kw), lambda b, m, kw: b.add_patch_mesh(QUAD_P[[0, 1, 3, 2]], np.array([[0, 1, 2, 3]], np.uint32), m, **kw),
                lambda b, m, kw: b.add_sphere(0.5, m, **kw), lambda b, m, kw: b.add_disk(0.5, m, **kw), lambda b, m, kw: b.add_cylinder(0.5, m, **kw)):
        def scene(**kw):
            b = scn.SceneBuilder()
            b.set_film(4, 4)
            b.set_camera_look_at(lib, (0, 0, 0), (0, 0, -1), (0, 1, 0), 40.0)
            add(b, b.material_diffuse(0.5), kw)
            desc = b.build(lib)[0]
            desc.keep_alive = b
            return b, desc
        assert create(scene(alpha=0.5)[1])[0] == 0 and create(scene(**em)[1])[0] == 0
        rc, msg = create(scene(alpha=0.5, **em)[1])
        assert rc == ERR_UNSUPPORTED and "alpha" in msg and "area light" in msg, (rc, msg)
        b, desc = scene(alpha=0.5)
        for mesh in (desc.meshes, desc.patch_meshes, desc.spheres):
            if mesh:
                mesh[0].alpha = 3  # 1 + index 2 of a table of one
        rc, msg = create(desc)
        assert rc == ERR_INVALID_ARGUMENT and "alpha" in msg and "out of range" in msg, (rc, msg)
    # the library's own entry answers the same before it looks for a device
    b, desc = build(lib, alpha=0.5)
    desc.meshes[1].alpha = 9
    handle = C.c_void_p()
    assert lib.shm_scene_create(C.byref(desc), 0, C.byref(handle)) == ERR_INVALID_ARGUMENT and "alpha" in lib.shm_last_error().decode()


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def test_an_alpha_tested_triangle_is_a_non_triangle_record_to_the_plan(lib):
    TRACE_TRI, TRACE_GEN, TRACE_GEN_HEAVY = 0, 1, 2
    for alpha, variant in ((None, TRACE_TRI), (0.5, TRACE_GEN_HEAVY)):  # (two of four records: a twelfth or more)
        o = oracle_py.Oracle(build(lib, alpha=alpha)[1])
        facts, plan, plan7 = o.scene_facts(), o.trace_plan(), o.trace_plan(gen_heavy_knob=0)
        o.close()
        assert facts["has_spheres"] == (alpha is not None) and plan["variant"] == variant
        assert plan7["variant"] == (TRACE_TRI if alpha is None else TRACE_GEN)
    sc = scenes.cutout_scene(lib, "lean", n_leaves=0)
    many = scenes.cutout_scene(lib, "lean", n_leaves=40)
    for s in (sc, many):
        o = oracle_py.Oracle(s.desc)
        assert o.scene_facts()["has_spheres"] == 1 and o.trace_plan()["variant"] == TRACE_GEN_HEAVY and o.scene_facts()["extended"] == 0
        o.close()


def test_cutout_scene_renders_its_holes(lib):
    """The generator's scene through the oracle: finite, lit, and another film than the same shapes uncut (what a build that ignores the field renders)."""
    p = render.make_params(seed=7, spp=2, max_depth=3)
    out = []
    for cut in (True, False):
        sc = scenes.cutout_scene(lib, "lean", 24, 24, cut=cut)
        o = oracle_py.Oracle(sc.desc)
        out.append(o.render(p, n_threads=4))
        o.close()
    (f_cut, s_cut), (f_solid, s_solid) = out
    assert np.isfinite(f_cut["rgb_sum"]).all() and f_cut["rgb_sum"].max() > 0
    assert not np.array_equal(f_cut["rgb_sum"], f_solid["rgb_sum"])
    assert s_cut["paths"] == s_solid["paths"]


# ---- the PBRT front end -------------------------------------------------------------------------------------------------------------------
HEAD = ('LookAt 0 0 0  0 0 -1  0 1 0\nCamera "perspective" "float fov" 40\nFilm "rgb" "integer xresolution" 8 "integer yresolution" 8\n'
        'WorldBegin\nShape "trianglemesh" "point3 P" [ -4 -1 -4  -4 -1 4  4 -1 4  4 -1 -4 ] "integer indices" [ 0 1 2 0 2 3 ]\n')
QUAD = '"point3 P" [ -1 -1 -2  1 -1 -2  1 1 -2  -1 1 -2 ] "point2 uv" [ 0 0 1 0 1 1 0 1 ]'


def load(lib, tmp_path, text, name="s.pbrt"):
    (tmp_path / name).write_text(text)
    out = C.POINTER(abi.ShmPbrtScene)()
    rc = lib.shm_scene_load_pbrt(str(tmp_path / name).encode(), C.byref(out))
    return rc, out


def test_loader_takes_both_spellings_on_every_shape(lib, tmp_path):
    text = HEAD + ('Texture "holes" "float" "checkerboard" "float uscale" 4 "float vscale" 4\n'
                   f'Shape "trianglemesh" {QUAD} "integer indices" [ 0 1 2 0 2 3 ] "texture alpha" "holes"\n'
                   f'Shape "trianglemesh" {QUAD} "integer indices" [ 0 1 2 0 2 3 ] "float alpha" [ 0.25 ]\n'
                   f'Shape "trianglemesh" {QUAD} "integer indices" [ 0 1 2 0 2 3 ] "float alpha" 1\n'
                   f'Shape "trianglemesh" {QUAD} "integer indices" [ 0 1 2 0 2 3 ] "float alpha" 0\n'
                   f'Shape "bilinearmesh" {QUAD} "integer indices" [ 0 1 3 2 ] "texture alpha" "holes"\n'
                   'Shape "sphere" "float radius" 0.5 "texture alpha" "holes"\n'
                   'Shape "disk" "float radius" 0.5 "float alpha" 0.5\n'
                   'Shape "cylinder" "float radius" 0.5 "texture alpha" "holes"\n'
                   'Shape "sphere" "float radius" 0.25\n')
    rc, out = load(lib, tmp_path, text)
    assert rc == 0, lib.shm_last_error().decode()
    d = out.contents.desc
    # the same scene through the SceneBuilder: the loader's field values are the builder's
    b = scn.SceneBuilder()
    m = b.material_diffuse(0.5)
    b.add_mesh(np.float32([(-4, -1, -4), (-4, -1, 4), (4, -1, 4), (4, -1, -4)]), QUAD_VI, m)
    holes = b.ftex_checkerboard(1.0, 0.0, mapping=b.add_texture_mapping("uv", su=4.0, sv=4.0))  # (PBRT-v4's defaults tex1 = 1, tex2 = 0: two constant nodes in front of it)
    for a in (holes, 0.25, 1.0, 0.0):
        b.add_mesh(QUAD_P, QUAD_VI, m, uv=QUAD_UV, alpha=a)
    b.add_patch_mesh(QUAD_P, np.array([[0, 1, 3, 2]], np.uint32), m, uv=QUAD_UV, alpha=holes)
    b.add_sphere(0.5, m, alpha=holes)
    b.add_disk(0.5, m, alpha=0.5)
    b.add_cylinder(0.5, m, alpha=holes)
    b.add_sphere(0.25, m)
    assert d.n_meshes == 5 and d.n_patch_meshes == 1 and d.n_spheres == 4
    got = [d.meshes[i].alpha for i in range(5)] + [d.patch_meshes[0].alpha] + [d.spheres[i].alpha for i in range(4)]
    want = [mm["alpha"] for mm in b.meshes] + [b.patch_meshes[0]["alpha"]] + [s.alpha for s in b.spheres]
    assert got == want == [0, 3, 4, 0, 5, 3, 3, 6, 3, 0], (got, want)
    assert d.n_float_textures == len(b.float_textures) == 6
    for i, (kind, value) in enumerate(((abi.SHM_FLOATTEX_CONSTANT, 1.0), (abi.SHM_FLOATTEX_CONSTANT, 0.0), (abi.SHM_FLOATTEX_CHECKERBOARD, None), (abi.SHM_FLOATTEX_CONSTANT, 0.25),
                                       (abi.SHM_FLOATTEX_CONSTANT, 0.0), (abi.SHM_FLOATTEX_CONSTANT, 0.5))):
        for t in (d.float_textures[i], b.float_textures[i]):
            assert t.kind == kind and (value is None or t.value == value), (i, t.kind, t.value)
    # the loaded scene is accepted and traced: the invisible quad (alpha 0) and the dropped parameter (alpha 1) among them
    o = oracle_py.Oracle(d)
    film, _ = o.render(render.make_params(seed=1, spp=1, max_depth=2), n_threads=4)
    o.close()
    assert np.isfinite(film["rgb_sum"]).all()
    lib.shm_pbrt_free(out)


def test_loader_rejects_alpha_on_an_emissive_shape_with_the_line(lib, tmp_path):
    text = HEAD + ('AttributeBegin\nAreaLightSource "diffuse" "blackbody L" 5000\n'
                   f'Shape "trianglemesh" {QUAD} "integer indices" [ 0 1 2 0 2 3 ]\n'
                   'Shape "sphere" "float radius" 0.5 "float alpha" 0.5\nAttributeEnd\n')
    rc, out = load(lib, tmp_path, text, name="lamp.pbrt")
    msg = lib.shm_last_error().decode()
    assert rc == ERR_UNSUPPORTED and not out and "lamp.pbrt:9" in msg and "alpha" in msg and "emissive" in msg, (rc, msg)
    # a constant 1 is no alpha: the same shape loads
    rc, out = load(lib, tmp_path, text.replace('"float alpha" 0.5', '"float alpha" 1'), name="lamp1.pbrt")
    assert rc == 0, lib.shm_last_error().decode()
    lib.shm_pbrt_free(out)
    rc, out = load(lib, tmp_path, HEAD + 'Shape "sphere" "texture alpha" "nobody"\n', name="missing.pbrt")
    assert rc != 0 and "missing.pbrt:6" in lib.shm_last_error().decode() and "nobody" in lib.shm_last_error().decode()


def test_example_scene_loads(lib):
    out = C.POINTER(abi.ShmPbrtScene)()
    rc = lib.shm_scene_load_pbrt(str(ROOT / "examples" / "scenes" / "cutout.pbrt").encode(), C.byref(out))
    assert rc == 0, lib.shm_last_error().decode()
    d = out.contents.desc
    assert any(d.meshes[i].alpha for i in range(d.n_meshes)) and any(d.spheres[i].alpha for i in range(d.n_spheres))
    o = oracle_py.Oracle(d)
    assert o.scene_facts()["has_spheres"] == 1
    o.close()
    lib.shm_pbrt_free(out)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_the_three_structs_kept_their_layout(tmp_path):
    """tests/golden/shape_alpha_before.json (gen_shape_alpha_before.py, run on the parent commit): sizeof and every named field's offset, in abi.py and in the header; the
    new field sits inside the former padding, and a zeroed record has no alpha."""
    before = json.loads((ROOT / "tests" / "golden" / "shape_alpha_before.json").read_text())["abi"]
    assert abi.SHM_ABI_VERSION == before["version"] == 10
    names = list(before["structs"])
    assert names == ["ShmTriangleMesh", "ShmBilinearPatchMesh", "ShmSphere"]
    for name, lay in before["structs"].items():
        cls = getattr(abi, name)
        assert C.sizeof(cls) == lay["sizeof"], name
        for field, off in lay["offsets"].items():
            assert getattr(cls, field).offset == off, (name, field)
        last = max(off for off in lay["offsets"].values())
        assert last < cls.alpha.offset and cls.alpha.offset + 4 <= lay["sizeof"] and cls.alpha.offset % 4 == 0 and cls.alpha.size == 4 and cls().alpha == 0, name
    s = abi.ShmSphere()
    s.alpha = 0x01020304
    assert bytes(s.pad) == bytes([0, 4, 3, 2, 1]) and s.quadric == 0  # (`pad` still names the five bytes behind `quadric`; alpha is the last four)
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    fields = [(n, f) for n in names for f in list(before["structs"][n]["offsets"]) + ["alpha", "pad"]]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "shimmer_hip.h"\nint main(void) {\n  printf("%d %zu %zu %zu\\n", SHM_ABI_VERSION, '
           + ", ".join(f"sizeof({n})" for n in names) + ");\n"
           + "".join(f'  printf("%zu\\n", offsetof({n}, {f}));\n' for n, f in fields) + "  return 0;\n}\n")
    (tmp_path / "p.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "p.c"), "-o", str(tmp_path / "p")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "p")], check=True, capture_output=True, text=True).stdout.split()))
    assert got[:4] == [10] + [before["structs"][n]["sizeof"] for n in names]
    assert got[4:] == [getattr(getattr(abi, n), f).offset for n, f in fields]


def test_scenes_without_a_cutout_render_what_the_parent_commit_rendered(lib):
    """tests/golden/shape_alpha_before.json: the oracle's films and counters of four scenes without alpha under both samplers — prim_intersect returns what it returned."""
    import gen_shape_alpha_before as gen
    before = json.loads((ROOT / "tests" / "golden" / "shape_alpha_before.json").read_text())
    assert len(before["films"]) == 8
    for rec in before["films"]:
        film, st = gen.film_of(lib, rec)
        assert gen.film_sha256(film) == rec["sha256"], rec["scene"]
        assert [int(st[k]) for k in STATS] == rec["stats"], rec["scene"]
