"""Writes tests/golden/procedural_textures_before.json: the films two EXISTING textured scenes rendered BEFORE the procedural float textures were added, as the CPU
oracle computes them (which the device path equals bit for bit) — the sha256 of the film's f64 sums and the seven counters. Uses nothing the parent commit lacks:

    git checkout fab7bd4 && python -c "import __graft_entry__ as g; g.build()" && python tests/golden/gen_procedural_textures_before.py

tests/test_procedural_textures.py (oracle) and tests/test_gpu_procedural_textures.py (device) assert the same hashes now."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))
STATS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")


def scene(lib, name):
    """The two scenes: the image-textured Cornell box, and the coated Cornell box with a float-texture graph (constant / mix / directionmix / scale nodes, no image) on
    the floor's interface roughness and thickness."""
    from shimmer_amd import abi, scenes
    if name == "textured_cornell":
        sc = scenes.cornell_box(lib, 32, 32, textured=True)
        return sc.desc, sc  # (the builder owns the arrays the description points at)
    sc = scenes.cornell_box(lib, 32, 32, coated=True)
    b = sc.builder
    floor = max(i for i, m in enumerate(b.materials) if m.kind == abi.SHM_MATERIAL_COATED_DIFFUSE)
    b.set_float_texture(floor, abi.SHM_FLOATSLOT_U_ROUGHNESS, b.ftex_mix(0.05, 0.3, b.ftex_direction_mix(0.2, 0.8, dir=(0.0, 0.6, 0.8))))
    b.set_float_texture(floor, abi.SHM_FLOATSLOT_THICKNESS, b.ftex_scaled(0.1, b.ftex_constant(0.5)))
    desc, _ = b.build(lib)
    return desc, b


CASES = [dict(scene="textured_cornell", seed=5, spp=4, max_depth=5), dict(scene="float_texture_cornell", seed=5, spp=4, max_depth=5)]


def film_of(lib, case):
    import oracle_py
    from shimmer_amd import render
    desc, keep = scene(lib, case["scene"])
    o = oracle_py.Oracle(desc)
    try:
        film, st = o.render(render.make_params(seed=case["seed"], spp=case["spp"], max_depth=case["max_depth"]), n_threads=8)
    finally:
        o.close()
    return film, st


if __name__ == "__main__":
    from shimmer_amd import abi
    lib = abi.load_library()
    films = []
    for case in CASES:
        film, st = film_of(lib, case)
        films.append(dict(case, sha256=hashlib.sha256(np.ascontiguousarray(film).tobytes()).hexdigest(), stats=[int(st[k]) for k in STATS]))
    out = dict(note="32x32 films of two existing textured scenes as the library BEFORE the procedural float textures rendered them (CPU oracle; commit fab7bd4)",
               command="git checkout fab7bd4 && python -c \"import __graft_entry__ as g; g.build()\" && python tests/golden/gen_procedural_textures_before.py",
               films=films)
    (ROOT / "tests" / "golden" / "procedural_textures_before.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))
