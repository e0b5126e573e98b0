"""The state one ShmScene carries from render to render (run with `pytest -m gpu`): the path workspace — whose staging arrays an all-diffuse scene gains with its first
staged render and keeps —, the per-batch hit-record form set on the scene's PathArrays and taken back, the random-walk records, the regrown capacity. Seven renders in
sequence on ONE Renderer, each held bit for bit against a fresh Renderer given the same parameters; the ZSobol render also against the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(gpu_lib):
    from shimmer_amd import render, scenes
    return gpu_lib, render, scenes


SEQUENCE = [
    dict(),                          # path
    dict(force_diffuse=True),        # ... through the staged pipeline whatever the scene class
    dict(integrator="simplepath"),
    dict(integrator="randomwalk"),
    dict(sampler="zsobol"),
    dict(spp=64),                    # regrows the workspace
    dict(),                          # the first render again
]


@pytest.mark.parametrize("scene", ["all_diffuse", "coated_textured"])
def test_renders_in_sequence_on_one_scene_equal_fresh_scenes(env, scene):
    lib, render, scenes = env
    sc = scenes.cornell_box(lib, 64, 64) if scene == "all_diffuse" else scenes.cornell_box(lib, 64, 64, coated=True, textured=True)
    kept = render.Renderer(lib, sc.desc, device=0)
    films = []
    try:
        for step, opts in enumerate(SEQUENCE):
            params = render.make_params(**{"seed": 11, "spp": 4, "max_depth": 5, **opts})
            film, stats = kept.render(params)
            fresh = render.Renderer(lib, sc.desc, device=0)
            try:
                film_fresh, stats_fresh = fresh.render(params)
            finally:
                fresh.close()
            assert np.array_equal(film, film_fresh), f"step {step} {opts}: the kept scene's film differs from a fresh scene's"
            for key in ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any"):
                assert stats[key] == stats_fresh[key], f"step {step} {opts}: {key}"
            assert film["weight_sum"].min() == params.samples_per_pixel
            if opts.get("sampler") == "zsobol":
                import zsobol_cases as zc
                zc.assert_equals_oracle(sc.desc, params, film, stats, (scene, opts))
            films.append(film)
    finally:
        kept.close()
    assert np.array_equal(films[-1], films[0])
    assert not np.array_equal(films[4], films[0])  # (another sampler: another film)
