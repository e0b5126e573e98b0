"""Writes tests/golden/quadrics_before.json: the films three EXISTING scenes — three_spheres, instanced_scene and the Cornell box as bilinear patches — rendered BEFORE
ShmSphere's spare byte became the quadric kind (PBRT-v4's disk and cylinder), as the CPU oracle of the parent commit computes them under both samplers: the sha256 of the
film's f64 sums and the seven counters. Uses nothing the parent commit lacks; run on the parent commit's tree with its libraries built:

    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/gen_quadrics_before.py

tests/test_quadrics.py (oracle) and tests/test_gpu_quadrics.py (device) assert the same hashes now: every sphere record of these scenes has a zeroed byte."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))
STATS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")
CASES = [dict(scene=s, sampler=smp, seed=11, spp=4, max_depth=5) for s in ("three_spheres", "instanced_scene", "cornell_patches") for smp in ("independent", "zsobol")]


def scene(lib, name):
    from shimmer_amd import scenes
    if name == "three_spheres":
        return scenes.three_spheres(lib, 32, 24, camera=(0.75, 0.5, 9.0))
    if name == "instanced_scene":
        return scenes.instanced_scene(lib, 32, 24)
    assert name == "cornell_patches"
    return scenes.cornell_box(lib, 32, 32, patches=True)


def params_of(case):
    from shimmer_amd import render
    return render.make_params(seed=case["seed"], spp=case["spp"], max_depth=case["max_depth"], sampler=case["sampler"])


def film_sha256(film):
    return hashlib.sha256(np.ascontiguousarray(film).tobytes()).hexdigest()


def film_of(lib, case):
    import oracle_py
    sc = scene(lib, case["scene"])  # (the builder owns the arrays the description points at)
    o = oracle_py.Oracle(sc.desc)
    try:
        film, st = o.render(params_of(case), n_threads=8)
    finally:
        o.close()
    return film, st


if __name__ == "__main__":
    from shimmer_amd import abi
    lib = abi.load_library()
    films = []
    for case in CASES:
        film, st = film_of(lib, case)
        films.append(dict(case, sha256=film_sha256(film), stats=[int(st[k]) for k in STATS]))
    out = dict(note="films of three_spheres, instanced_scene and cornell_box(patches=True) as the CPU oracle of the commit BEFORE the disk and cylinder rendered them",
               command="python -c \"import __graft_entry__ as g; g.build()\" && python tests/golden/gen_quadrics_before.py", films=films)
    (ROOT / "tests" / "golden" / "quadrics_before.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))
