"""Writes tests/golden/shape_alpha_before.json: what the commit BEFORE PBRT-v4's shape alpha (ShmTriangleMesh / ShmBilinearPatchMesh / ShmSphere::alpha, carved out of the
structs' padding) says about two things the feature must leave alone —
  abi    sizeof and every named field's offset of the three structs, from shimmer_amd/abi.py's ctypes mirrors (which tests hold to include/shimmer_hip.h), and SHM_ABI_VERSION;
  films  four EXISTING scenes without a cutout — three_spheres, instanced_scene, the Cornell box as bilinear patches and the lean disk-and-cylinder scene — under both
         samplers as the CPU oracle of that commit renders them: the sha256 of the film's f64 sums and the seven counters.
Uses nothing the parent commit lacks; run on the parent commit's tree with its libraries built:

    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/gen_shape_alpha_before.py

tests/test_shape_alpha.py (oracle) and tests/test_gpu_shape_alpha.py (device) assert the same numbers now."""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))
STATS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")
STRUCTS = ("ShmTriangleMesh", "ShmBilinearPatchMesh", "ShmSphere")
CASES = [dict(scene=s, sampler=smp, seed=11, spp=4, max_depth=5) for s in ("three_spheres", "instanced_scene", "cornell_patches", "quadrics_lean") for smp in ("independent", "zsobol")]


def scene(lib, name):
    from shimmer_amd import scenes
    if name == "three_spheres":
        return scenes.three_spheres(lib, 32, 24, camera=(0.75, 0.5, 9.0))
    if name == "instanced_scene":
        return scenes.instanced_scene(lib, 32, 24)
    if name == "quadrics_lean":
        return scenes.quadric_scene(lib, "lean", 32, 24)
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


def layout_of(abi, name):
    """sizeof and the offsets of the struct's named fields (the padding is what the feature carves its field out of: not a field to hold)."""
    cls = getattr(abi, name)
    return dict(sizeof=C.sizeof(cls), offsets={f[0]: getattr(cls, f[0]).offset for f in cls._fields_ if f[0] != "pad" and not f[0].startswith("_")})


if __name__ == "__main__":
    from shimmer_amd import abi
    lib = abi.load_library()
    films = []
    for case in CASES:
        film, st = film_of(lib, case)
        films.append(dict(case, sha256=film_sha256(film), stats=[int(st[k]) for k in STATS]))
    out = dict(note="the ABI layout of the three shape structs, and the films of four scenes without a cutout, as of the commit BEFORE shape alpha (the CPU oracle's films)",
               command="python -c \"import __graft_entry__ as g; g.build()\" && python tests/golden/gen_shape_alpha_before.py",
               abi=dict(version=int(abi.SHM_ABI_VERSION), structs={name: layout_of(abi, name) for name in STRUCTS}), films=films)
    (ROOT / "tests" / "golden" / "shape_alpha_before.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))
