#!/usr/bin/env python3
"""A light probe rendered inside one scene lights another: PBRT-v4's spherical camera closes the loop with the equal-area environment maps the library reads.

    python examples/probe_to_environment.py [--res 64] [--spp 256]

Renders the Cornell box through an equal-area spherical camera standing in the middle of the room (scenes.cornell_box(camera=...)), takes the square film — an equal-area
octahedral map is what an ImageInfinitelight's image is —, mirrors it left to right (scenes.environment_from_probe: the camera's y / z swap is a reflection, the
generators' light transform a rotation) and hands it to scenes.three_spheres(environment=...). Writes probe.pfm and lit.pfm.
Needs an MI355X: there is no CPU path."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shimmer_amd import abi, render, scenes  # noqa: E402


def render_rgb(lib, desc, spp):
    r = render.Renderer(lib, desc, 0)
    film, _ = r.render(render.make_params(seed=1, spp=spp, max_depth=5))
    r.close()
    return np.ascontiguousarray(render.film_get_image(lib, film, render.SRGB_FROM_XYZ), np.float32)  # (linear sRGB: what an environment image holds)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=64, help="the probe's (square) resolution")
    ap.add_argument("--spp", type=int, default=256)
    args = ap.parse_args()
    lib = abi.load_library()
    if lib.shm_device_count() < 1:
        raise SystemExit("no HIP device visible (there is no CPU fallback)")
    probe = scenes.cornell_box(lib, args.res, args.res, camera=dict(type="spherical", mapping="equalarea", pos=(0.0, 1.0, 0.2), look_at=(0.0, 1.0, -1.0)))
    # The probe looks down -z with y up. Its film is an equal-area octahedral map, but not yet THIS scene's: the camera's swap of y and z is a reflection and
    # three_spheres turns its map by a rotation, so the film is mirrored left to right on the way (scenes.environment_from_probe) — without that the ceiling would
    # still be overhead, but the red and the green wall would change sides.
    env = scenes.environment_from_probe(render_rgb(lib, probe.desc, args.spp))
    lit = scenes.three_spheres(lib, 256, 256, camera=(0.75, 0.5, 9.0), environment=env)
    img = render_rgb(lib, lit.desc, args.spp)
    for name, a in (("probe.pfm", env), ("lit.pfm", img)):
        abi.check(lib, lib.shm_write_pfm(name.encode(), a.ctypes.data_as(abi.c_float_p), a.shape[1], a.shape[0]), "shm_write_pfm")
        print("wrote", name, a.shape, "mean", float(a.mean()))


if __name__ == "__main__":
    main()
