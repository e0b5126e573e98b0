"""Writes tests/golden/spherical_camera_before.json: SHA-256 of the scene descriptions the generators of shimmer_amd/scenes.py produced BEFORE they took a `camera=`
argument (and before ShmCamera::pad became `mapping`) — run on the parent commit's tree with its library built:

    python tests/golden/gen_spherical_camera_before.py /path/to/parent/checkout

tests/test_spherical_camera.py holds the generators, called without `camera=`, to these hashes (`description_sha256` below is what it calls)."""
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent

# the generators and the arguments they are called with: small, and every class of scene the GPU tests render
CASES = [("cornell_box", dict(width=40, height=40)), ("cornell_box", dict(width=32, height=32, textured=True)), ("cornell_box", dict(width=32, height=32, glass=True, patches=True)),
         ("ganesha_proxy", dict(width=48, height=48, n=24, coated=True)), ("three_spheres", dict(width=40, height=30, camera=(0.75, 0.5, 9.0))),
         ("three_spheres", dict()), ("crown_proxy", dict(width=30, height=42, level=1, n_glass=6, n_gold=2)), ("instanced_scene", dict(width=40, height=30))]


def _arr(ptr, n):
    return C.string_at(ptr, C.sizeof(ptr._type_) * n) if n and ptr else b""


def description_sha256(desc):
    """Everything of a ShmSceneDesc that the generators' common head (film, camera) and body (geometry, materials, lights, spectra) write, pointers followed."""
    h = hashlib.sha256()
    h.update(bytes(desc.camera))
    f = desc.film
    h.update(repr((list(f.pixel_bounds), list(f.full_resolution), list(f.filter_radius), f.filter, list(f.filter_params), f.imaging_ratio, f.max_component_value)).encode())
    for t in ("sensor_r_bar", "sensor_g_bar", "sensor_b_bar"):
        h.update(_arr(getattr(f, t), 471))
    h.update(_arr(desc.nodes, desc.n_nodes) + _arr(desc.primitives, desc.n_primitives) + _arr(desc.spheres, desc.n_spheres))
    for i in range(desc.n_meshes):
        m = desc.meshes[i]
        h.update(repr((m.n_triangles, m.n_vertices, m.reverse_orientation, m.transform_swaps_handedness)).encode())
        h.update(_arr(m.vertex_indices, 3 * m.n_triangles) + _arr(m.p, 3 * m.n_vertices) + _arr(m.n, 3 * m.n_vertices) + _arr(m.s, 3 * m.n_vertices) + _arr(m.uv, 2 * m.n_vertices))
    h.update(_arr(desc.materials, desc.n_materials) + _arr(desc.lights, desc.n_lights) + _arr(desc.spectrum_data, desc.n_spectrum_floats))
    return h.hexdigest()


def main(tree):
    sys.path.insert(0, str(tree))
    from shimmer_amd import abi, scenes
    lib = abi.load_library()
    out = []
    for name, kw in CASES:
        sc = getattr(scenes, name)(lib, **kw)
        out.append(dict(scene=name, args={k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}, sha256=description_sha256(sc.desc)))
    (HERE / "spherical_camera_before.json").write_text(json.dumps(dict(note="scene descriptions of the parent commit (gen_spherical_camera_before.py)", descriptions=out), indent=1) + "\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(Path(sys.argv[1]).resolve() if len(sys.argv) > 1 else HERE.parent.parent)
