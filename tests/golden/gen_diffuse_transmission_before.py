"""Writes tests/golden/diffuse_transmission_before.json: the films two EXISTING scenes — the Cornell box and the S3 proxy, 32 x 32 at 4 spp — rendered BEFORE the diffuse
transmission material was added, as the CPU oracle computes them (which the device path equals bit for bit): the sha256 of the film's f64 sums and the seven counters.
Uses nothing the parent commit lacks:

    git checkout 7cd5461 && python -c "import __graft_entry__ as g; g.build()" && python tests/golden/gen_diffuse_transmission_before.py

tests/test_diffuse_transmission.py (oracle) and tests/test_gpu_diffuse_transmission.py (device) assert the same hashes now."""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))
STATS = ("paths", "rays_closest", "rays_any", "nodes_closest", "tris_closest", "nodes_any", "tris_any")
CASES = [dict(scene="cornell_box", seed=5, spp=4, max_depth=5), dict(scene="s3_proxy", seed=5, spp=4, max_depth=5)]


def scene(lib, name):
    from shimmer_amd import scenes
    if name == "cornell_box":
        return scenes.cornell_box(lib, 32, 32)
    assert name == "s3_proxy"
    return scenes.ganesha_proxy(lib, 32, 32, n=24)


def film_of(lib, case):
    import oracle_py
    from shimmer_amd import render
    sc = scene(lib, case["scene"])  # (the builder owns the arrays the description points at)
    o = oracle_py.Oracle(sc.desc)
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
    out = dict(note="32x32 films of the Cornell box and the S3 proxy as the library BEFORE the diffuse transmission material rendered them (CPU oracle; commit 7cd5461)",
               command="git checkout 7cd5461 && python -c \"import __graft_entry__ as g; g.build()\" && python tests/golden/gen_diffuse_transmission_before.py",
               films=films)
    (ROOT / "tests" / "golden" / "diffuse_transmission_before.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out, indent=1))
