"""The CPU oracle under ZSobol (oracle/oracle.cpp honours ShmRenderParams::sampler), made trustworthy on its own before the device is held to it
(tests/test_gpu_zsobol_oracle.py): its stream against the Python restatement of tests/test_zsobol_sampler.py; the camera ray's draw layout against a float64
restatement of the reference's evaluate_pixel_sample / get_camera_sample order; films invariant under threads and under cutting the work up; unbiased against
independent sampling; the stratification reaching the integrator; the library's argument checks; and the table of tests/zsobol_cases.py landing on the plan cells it
declares. No GPU."""
import math
import os
import random

import numpy as np
import pytest

import oracle_py
import test_pixel_filters as pf
import test_zsobol_sampler as ref
import zsobol_cases as zc
from shimmer_amd import abi, render, scene as scn, scenes
from shimmer_amd.scene import SceneBuilder, blackbody_dense

THREADS = min(16, os.cpu_count() or 1)


def rgb(film):
    return render.film_to_rgb(film).astype(np.float64)


# ---- the stream ----
def test_stream_equals_the_restatement():
    """400 random (pixel, index, spp, resolution, seed, randomization) cases, 1-D and 2-D draws mixed: the u32 values and the bits of the floats."""
    for c in ref.random_cases(400, random.Random(4321)):
        u, f = oracle_py.sampler_stream_zs(*c)
        want = ref.stream(*c)
        assert u == want, c
        assert f == [int(np.float32(ref.to_float(v)).view(np.uint32)) for v in want], c


# ---- the camera ray's draws ----
RES = (1024, 768)
FOV = 60.0
LENS_RADIUS, FOCAL = 0.2, 5.0
PIXELS = [(256, 256), (1000, 700), (777, 300), (5, 3)]
FILTERS = {"box": (0.5, ()), "triangle": (2.0, ()), "gaussian": (1.5, (0.5,))}  # PBRT-v4's default radii and parameters (SceneBuilder.FILTERS)


def camera_scene(lib, camera, filter_name):
    """A camera at the world's origin looking down +z with y up — render space is camera space — over one quad; the film is 1024 x 768."""
    b = SceneBuilder()
    b.set_film(*RES, filter=filter_name)
    kw = dict(orthographic=True) if camera == "orthographic" else (dict(lens_radius=LENS_RADIUS, focal_distance=FOCAL) if camera == "thin_lens" else {})
    rfw = b.set_camera_look_at(lib, (0, 0, 0), (0, 0, 1), (0, 1, 0), FOV, **kw)
    assert np.allclose(rfw, np.eye(4)) and np.allclose(np.array(b.camera.render_from_camera[:]).reshape(4, 4), np.eye(4))
    p, vi = scenes._quad((-50, -50, 10), (50, -50, 10), (50, 50, 10), (-50, 50, 10))
    b.add_mesh(p, vi, b.material_diffuse(0.5), emission=blackbody_dense(6500.0), emission_scale=1.0)
    desc, _ = b.build(lib)
    desc.keepalive = b
    return desc


def wavelengths_f64(lu):
    """sample_visible (sampled_wavelengths.rs:57-71) over sample_visible_wavelengths (sampling.rs:268-270): the stratified u and the argument of atanh in float32 as the
    reference forms them, atanh in float64 by the formula tests/test_oracle_golden.py::test_transcendentals holds the float32 one to. Returns (lambda, tolerance): that
    test's 2 ulp of the atanh, carried through the factor 138.888889, plus one rounding each of the product and of the difference."""
    lam, tol = [], []
    for i in range(4):
        up = np.float32(lu) + np.float32(i) / np.float32(4)
        if up > np.float32(1.0):
            up = up - np.float32(1.0)
        x = np.float32(0.85691062) - np.float32(1.82750197) * up
        at = 0.5 * np.log1p(np.float64(np.float32(np.float32(2.0) * x) / np.float32(np.float32(1.0) - x)))
        lam.append(538.0 - float(np.float32(138.888889)) * at)
        tol.append(138.888889 * 2.0 * float(np.spacing(np.float32(abs(at)))) + float(np.spacing(np.float32(abs(138.888889 * at)))) + float(np.spacing(np.float32(lam[-1]))))
    return np.array(lam), np.array(tol)


def concentric_disk_f64(u):
    ox, oy = 2.0 * u[0] - 1.0, 2.0 * u[1] - 1.0
    if ox == 0.0 and oy == 0.0:
        return np.zeros(2)
    if abs(ox) > abs(oy):
        r, theta = ox, (math.pi / 4.0) * (oy / ox)
    else:
        r, theta = oy, math.pi / 2.0 - (math.pi / 4.0) * (ox / oy)
    return r * np.array([math.cos(theta), math.sin(theta)])


@pytest.mark.parametrize("filter_name", list(FILTERS))
@pytest.mark.parametrize("camera", ["perspective", "orthographic", "thin_lens"])
def test_camera_ray_draw_layout(lib, camera, filter_name):
    """generate_camera_ray (shm/path.h) is shared by the oracle and the kernels: bit parity between them cannot see an error in its draw order. Here the draws come from
    the Python restatement of the stream, taken in the order and kinds of the reference's evaluate_pixel_sample (integrator.rs:338-362: the wavelength, one 1-D draw, none
    under disable_wavelength_jitter) and get_camera_sample (sampling.rs:347-371: the film point, one 2-D draw, always; then the lens, one 2-D draw, and the time, one 1-D
    draw, neither under disable_pixel_jitter), and everything after them is float64:
      the sampled wavelengths equal the oracle's (wavelengths_f64's tolerance);
      the oracle's ray passes through the film point — pixel + 0.5 + the filter's offset (tests/test_pixel_filters.py's float64 samplers), the pixel centre without
        jitter — at the tolerances of tests/test_camera_properties.py: 2e-5 (1 + tan(fov / 2)) on the direction's tangents, 2e-5 on an orthographic origin;
      the filter weight is 1 (box, triangle, and every filter without jitter) or the gaussian sampler's constant (1e-5 relative: that file's tolerance);
      the thin lens's ray starts at lens_radius * the concentric disk point of the lens draw, within 8 float32 ulp of the lens radius (the mapping is a handful of float32
        operations and a sine and cosine at 2 ulp each);
      the next draw is taken from the dimension the reference's call order gives.
    Pixels with coordinates above 255 in a 1024 x 768 film; spp 1, 6 and 16; both randomizations."""
    desc = camera_scene(lib, camera, filter_name)
    o = oracle_py.Oracle(desc)
    w, h = RES
    t = math.tan(math.radians(FOV) / 2.0)
    r, params = FILTERS[filter_name]
    tabulated = pf.FilterSampler2D(filter_name, pf.f32(r), pf.f32(r), tuple(pf.f32(v) for v in params)) if filter_name == "gaussian" else None
    rnd = random.Random(99)
    n = 0
    for px, py in PIXELS:
        for spp, index, none in ((1, 0, False), (6, 5, False), (16, 11, False), (16, 3, True)):
            for dwj in (False, True):
                for dpj in (False, True):
                    seed = rnd.getrandbits(64) | (1 << 44)
                    kinds = ([] if dwj else [1]) + [2] + ([] if dpj else [2, 1])
                    draws = [float(ref.to_float(v)) for v in ref.stream(px, py, index, spp, w, h, seed, none, kinds)]
                    got = o.camera_ray_zs(px, py, index, seed, spp, none=none, disable_wavelength_jitter=dwj, disable_pixel_jitter=dpj)
                    what = (camera, filter_name, px, py, spp, index, none, dwj, dpj)
                    assert got["dimension"] == sum(kinds), what
                    lam, tol = wavelengths_f64(0.5 if dwj else draws.pop(0))
                    assert (np.abs(got["lambda"].astype(np.float64) - lam) <= tol).all(), (what, got["lambda"], lam)
                    uf = np.array([draws[:2]])
                    if dpj:
                        fp, weight = np.zeros(2), 1.0
                    elif filter_name == "box":
                        fp, weight = (2.0 * uf[0] - 1.0) * r, 1.0
                    elif filter_name == "triangle":
                        fp, weight = pf.tent_inverse_cdf(uf[0], r), 1.0
                    else:
                        p_ref, w_ref = tabulated.sample(uf)
                        fp, weight = p_ref[0], float(w_ref[0])
                    assert got["weight"] == pytest.approx(weight, rel=1e-5), what
                    x, y = px + 0.5 + fp[0], py + 0.5 + fp[1]
                    d, org = got["d"].astype(np.float64), got["o"].astype(np.float64)
                    if camera == "orthographic":
                        pixel = 2.0 / min(w, h)
                        assert np.allclose(d, (0.0, 0.0, 1.0), atol=1e-6), what
                        assert org[0] == pytest.approx((x - w / 2) * pixel, abs=2e-5) and org[1] == pytest.approx(-(y - h / 2) * pixel, abs=2e-5), what
                    else:
                        k = 2.0 * t / min(w, h)
                        if camera == "thin_lens":  # the ray from the lens point through the point of the plane of focus that the pinhole ray meets
                            lens = LENS_RADIUS * concentric_disk_f64((0.5, 0.5) if dpj else draws[2:4])
                            assert np.abs(org[:2] - lens).max() <= 8 * float(np.spacing(np.float32(LENS_RADIUS))) and abs(org[2]) < 1e-7, (what, org, lens)
                            focus = org + d * ((FOCAL - org[2]) / d[2])
                            tx, ty = focus[0] / FOCAL, focus[1] / FOCAL
                        else:
                            assert np.allclose(org, 0.0), what
                            tx, ty = d[0] / d[2], d[1] / d[2]
                        assert tx == pytest.approx((x - w / 2) * k, abs=2e-5 * (1 + t)) and ty == pytest.approx(-(y - h / 2) * k, abs=2e-5 * (1 + t)), what
                    n += 1
    o.close()
    assert n == 64


def test_camera_hit_differentials_under_zsobol(lib):
    """The ZSobol form of orc_fn_camera_hit_differentials starts from the ZSobol camera ray (the same origin and direction as orc_fn_camera_ray_zs, bit for bit) and
    the existing form from the independent sampler's, as before."""
    desc = camera_scene(lib, "perspective", "box")
    o = oracle_py.Oracle(desc)
    for px, py, index in ((300, 400, 0), (1000, 5, 3)):
        ok, out = o.camera_hit_differentials_zs(px, py, index, 7, 4)
        ray = o.camera_ray_zs(px, py, index, 7, 4)
        assert ok and np.array_equal(out[0:3], ray["o"]) and np.array_equal(out[3:6], ray["d"])
        plain = (oracle_py.C.c_float * 44)()
        assert o.lib.orc_fn_camera_hit_differentials(o.handle, px, py, index, 7, 4, 0, 1, plain)
        ind = (oracle_py.C.c_float * 14)()
        o.lib.orc_fn_camera_ray(o.handle, px, py, index, 7, ind)
        assert list(plain[0:6]) == list(ind[0:6]) and list(plain[3:6]) != list(out[3:6])
    o.close()


# ---- the library's argument checks ----
def test_arguments_are_checked_as_the_library_checks_them(lib):
    sc = scenes.cornell_box(lib, 8, 8)
    o = oracle_py.Oracle(sc.desc)
    p = render.make_params(seed=1, spp=6, sampler="zsobol")  # log2spp = 3: indices 0 .. 7
    o.render(p, waves=[(6, 8)])
    with pytest.raises(RuntimeError, match=r"zsobol: sample index outside \[0, 2\^ceil\(log2\(samples_per_pixel\)\)\)"):
        o.render(p, waves=[(7, 9)])
    with pytest.raises(RuntimeError, match="zsobol: sample index outside"):
        o.render(p, waves=[(-1, 2)])
    o.render(render.make_params(seed=1, spp=6), waves=[(7, 9)])  # (the independent sampler has no such range)
    p.sampler = 2
    with pytest.raises(RuntimeError, match="unknown sampler or sampler randomization"):
        o.render(p)
    p.sampler, p.sampler_randomization = abi.SHM_SAMPLER_ZSOBOL, 2
    with pytest.raises(RuntimeError, match="unknown sampler or sampler randomization"):
        o.render(p)
    with pytest.raises(RuntimeError, match="reference stream"):
        o.render_reference_stream(render.make_params(seed=1, spp=2, sampler="zsobol"))
    o.close()


# ---- the film ----
def test_film_is_invariant_under_threads_and_decomposition(lib):
    """Cornell box, 24 x 24, spp 6: the same bits on 1, 3 and 16 threads and rendered wave by wave over two disjoint tile subsets; weight_sum == spp everywhere; the
    sampler and its randomization are used."""
    sc = scenes.cornell_box(lib, 24, 24)
    o = oracle_py.Oracle(sc.desc)
    p = render.make_params(seed=21, spp=6, max_depth=5, sampler="zsobol")
    f1, s1 = o.render(p, n_threads=1)
    for n in (3, 16):
        f, s = o.render(p, n_threads=n)
        assert np.array_equal(f, f1) and s["rays_any"] == s1["rays_any"] and s["nodes_closest"] == s1["nodes_closest"], n
    assert (f1["weight_sum"] == 6.0).all() and np.isfinite(f1["rgb_sum"]).all() and f1["rgb_sum"].max() > 0
    tiles, n_tiles = scn.tiles_for(lib, o.pixel_bounds)
    subsets = []
    for keep in (lambda i: i % 3 != 0, lambda i: i % 3 == 0):
        idx = [i for i in range(n_tiles) if keep(i)]
        sub = (abi.ShmTile * len(idx))()
        for k, i in enumerate(idx):
            sub[k] = tiles[i]
        subsets.append((sub, len(idx)))
    film = np.zeros_like(f1)
    for wave in scn.wave_schedule(6):
        for sub, n in subsets:
            o.render(p, n_threads=3, tiles=sub, n_tiles=n, waves=[wave], film=film)
    assert np.array_equal(film, f1)
    f_ind, _ = o.render(render.make_params(seed=21, spp=6, max_depth=5), n_threads=THREADS)
    f_none, _ = o.render(render.make_params(seed=21, spp=6, max_depth=5, sampler="zsobol", randomization="none"), n_threads=THREADS)
    assert not np.array_equal(f1["rgb_sum"], f_ind["rgb_sum"]) and not np.array_equal(f1["rgb_sum"], f_none["rgb_sum"])
    o.close()


def test_zsobol_is_unbiased(lib):
    """tests/test_gpu_zsobol.py::test_zsobol_is_unbiased on the oracle, Cornell box at 24 x 24, max_depth 5: against the mean of 64 independent 64-spp images, whose
    spread gives each pixel's standard error, ZSobol at 1 024 spp has the same image mean within 0.5 % and no pixel beyond 5 standard errors (the error of the
    reference plus that of a 1 024-spp independent estimate: ZSobol's own is smaller). Measured: mean ratio 0.99771, max |z - ref| / se 3.77."""
    sc = scenes.cornell_box(lib, 24, 24)
    o = oracle_py.Oracle(sc.desc)
    ind = np.stack([rgb(o.render(render.make_params(seed=1000 + s, spp=64, max_depth=5), n_threads=THREADS)[0]) for s in range(64)])
    z = rgb(o.render(render.make_params(seed=7, spp=1024, max_depth=5, sampler="zsobol"), n_threads=THREADS)[0])
    o.close()
    ref_img = ind.mean(axis=0)
    var64 = ind.var(axis=0, ddof=1)
    se = np.sqrt(var64 / 64.0 + var64 / 16.0)
    dev = np.abs(z - ref_img) / (se + 1e-12)
    print(f"[zsobol oracle] C2 24^2: mean ratio {z.mean() / ref_img.mean():.5f}, max |z - ref| / se {dev[se > 0].max():.2f}")
    assert abs(z.mean() / ref_img.mean() - 1.0) < 0.005, (z.mean(), ref_img.mean())
    assert (np.abs(z - ref_img) <= 5.0 * se + 1e-6).all(), float(dev.max())


@pytest.mark.parametrize("depth, bound", [(1, 0.6), (5, 1.0)])
def test_zsobol_has_lower_error(lib, depth, bound):
    """tests/test_gpu_zsobol.py::test_zsobol_has_lower_error on the oracle: MSE against 4 096-spp independent sampling, averaged over 4 seeds at 64 spp, on the Cornell
    box at 24 x 24: ZSobol / independent at most `bound` (that test's bounds): the stratification reaches the integrator. (What this does NOT see: with the light sample of `li`
    drawn as two 1-D draws instead of one 2-D draw the ratios stayed 0.082 and 0.099 — two stratified 1-D draws padded together integrate this scene as well. Such
    a slip shows as a film that differs from the kernels', which are written apart from the oracle: tests/test_gpu_zsobol_oracle.py.) Measured: 0.082 at max_depth 1 (2.99e-3 against 3.65e-2), 0.098 at max_depth 5 (3.65e-3 against 3.71e-2)."""
    sc = scenes.cornell_box(lib, 24, 24)
    o = oracle_py.Oracle(sc.desc)
    ref_img = rgb(o.render(render.make_params(seed=1000, spp=4096, max_depth=depth), n_threads=THREADS)[0])
    mse = {}
    for sampler in ("independent", "zsobol"):
        imgs = [rgb(o.render(render.make_params(seed=s, spp=64, max_depth=depth, sampler=sampler), n_threads=THREADS)[0]) for s in range(4)]
        mse[sampler] = float(np.mean([np.mean((im - ref_img) ** 2) for im in imgs]))
    o.close()
    ratio = mse["zsobol"] / mse["independent"]
    print(f"[zsobol oracle] C2 24^2 depth {depth}: MSE independent {mse['independent']:.4e} zsobol {mse['zsobol']:.4e} ratio {ratio:.3f}")
    assert ratio <= bound, ratio


# ---- the table of edge cases: where each row lands ----
def test_every_case_lands_on_the_cell_it_declares(lib):
    """Each row's scene and params through scene_facts and render_plan (host/render_plan.hpp, the code shm_render_wave runs): the row lands on the coordinates of its
    cell with zs == 1 and no plan error; the cells are pairwise distinct in those coordinates and every cell has a row. A change to the plan that moves a case onto
    other kernels fails here instead of thinning the GPU test's coverage silently."""
    cells = {name: tuple(c[k] for k in zc.COORDS) for name, c in zc.CELLS.items()}
    assert len(set(cells.values())) == len(cells), [a for a in cells for b in cells if a < b and cells[a] == cells[b]]
    assert {c.cell for c in zc.CASES} == set(cells)
    assert len({c.name for c in zc.CASES}) == len(zc.CASES)
    built = {}
    for c in zc.CASES:
        key = (c.scene, repr(sorted(c.scene_kw.items())))
        if key not in built:  # (a scene's facts do not depend on the render)
            sc = zc.build_scene(lib, c)  # (kept: the description points into the builder's arrays)
            o = oracle_py.Oracle(sc.desc)
            built[key] = o.scene_facts()
            assert 16 * 16 <= o.width * o.height <= 48 * 48 or c.name in ("crop_above_255", "smaller_than_a_tile"), c.name
            o.close()
        p = zc.make_params(c)
        assert p.samples_per_pixel <= 16, c.name
        split_knob, tail = zc.knobs(c)
        row = dict(built[key], split_knob=split_knob, tail_fused_bounce=tail, integrator=p.integrator, force_diffuse=p.force_diffuse, sampler=p.sampler,
                   disable_pixel_jitter=p.disable_pixel_jitter, max_depth=p.max_depth)
        plan = oracle_py.render_plans([[row[k] for k in oracle_py.PLAN_IN]])
        got = {k: int(plan[k][0]) for k in oracle_py.PLAN_OUT}
        got["fused_from_0"] = int(got["fused_from"] == 0)
        assert got["zs"] == 1 and got["error"] == 0, c.name
        assert {k: got[k] for k in zc.COORDS} == zc.CELLS[c.cell], (c.name, c.cell)


def test_scene_facts_of_real_scenes(lib):
    """orc_fn_scene_facts on scenes whose facts are known by construction."""
    sc = scenes.cornell_box(lib, 16, 16)
    o = oracle_py.Oracle(sc.desc)
    assert o.scene_facts() == dict(classes=1, diffuse_only=1, has_material_textures=0, has_image_light=0, has_spheres=0, has_instances=0, extended=0,
                                   has_plain_diffuse=1, plain_quarter=1, filter=abi.SHM_FILTER_BOX)
    o.close()
    sc = scenes.cornell_box(lib, 16, 16, coated=True, patches=True, environment=scenes.environment_image(8), film=dict(filter="gaussian"),
                            extra_lights=scenes.spot_and_distant())
    o = oracle_py.Oracle(sc.desc)
    f = o.scene_facts()
    assert f["classes"] == 0b1001 and (f["diffuse_only"], f["has_image_light"], f["has_spheres"], f["extended"], f["filter"]) == (0, 1, 1, 1, abi.SHM_FILTER_GAUSSIAN)
    o.close()
