"""Every row of tests/zsobol_cases.py on the device against the CPU oracle under ZSobol: the film (rgb_sum, weight_sum) and the seven counters, bit for bit. The
oracle's li / li_simple_path / li_random_walk draw sequentially in the reference integrator's order, with no save / resume: a kernel that draws a dimension too many or
too few on some branch, splits a 2-D draw, or resumes one dimension off renders another film. tests/test_zsobol_oracle.py (no GPU) holds the oracle itself to the
restatement of the stream and checks that each row lands on the kernels it is meant for."""
import numpy as np
import pytest

import zsobol_cases as zc
from shimmer_amd import abi, render

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", zc.CASES, ids=[c.name for c in zc.CASES])
def test_case_equals_the_oracle(gpu_lib, monkeypatch, case):
    for var in ("SHM_TAIL_FUSED_BOUNCE", "SHM_SPLIT_PASS"):
        monkeypatch.delenv(var, raising=False)
    for var, val in case.env.items():  # (read at scene creation)
        monkeypatch.setenv(var, val)
    sc = zc.build_scene(gpu_lib, case)
    p = zc.make_params(case)
    g = render.Renderer(gpu_lib, sc.desc, 0)
    rects = zc.tile_rects(gpu_lib, case, g.pixel_bounds)
    indices, oracle_kw = None, {}
    if rects is not None:
        where = {(g.tiles[i].x0, g.tiles[i].y0, g.tiles[i].x1, g.tiles[i].y1): i for i in range(g.n_tiles)}
        indices = [where[r] for r in rects]
        sub = (abi.ShmTile * len(indices))()
        for k, i in enumerate(indices):
            sub[k] = g.tiles[i]
        oracle_kw = dict(tiles=sub, n_tiles=len(indices))
    if zc.waves(case) is not None:
        oracle_kw["waves"] = zc.waves(case)
    g.clear()
    s_gpu = g.render_waves(p, tile_indices=indices, waves=zc.waves(case))
    f_gpu = g.read_film()
    g.close()
    zc.assert_equals_oracle(sc.desc, p, f_gpu, s_gpu, case.name, **oracle_kw)
    assert f_gpu["rgb_sum"].max() > 0, case.name
    if rects is None and "film" not in case.scene_kw:  # (the box filter: every sample weighs 1)
        assert (f_gpu["weight_sum"] == p.samples_per_pixel).all(), case.name
    elif rects is not None:
        rendered = np.zeros(f_gpu.shape, bool)
        x0, y0 = g.pixel_bounds[:2]
        for rx0, ry0, rx1, ry1 in rects:
            rendered[ry0 - y0:ry1 - y0, rx0 - x0:rx1 - x0] = True
        assert (f_gpu["weight_sum"][rendered] == p.samples_per_pixel).all() and (f_gpu["weight_sum"][~rendered] == 0).all(), case.name
