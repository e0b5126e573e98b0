#!/usr/bin/env python3
"""The S3 proxy at 1024^2 x 64 spp with the camera moved inside the room, as a perspective camera or as PBRT-v4's equal-area probe at the same place: `--frames`
timed frames after `--warmup`, wall time and the library's own breakdown per frame. For the generate kernel alone run it under

    rocprofv3 --kernel-trace --stats -d OUT/stats -o stats -- python tools/generate_cost.py --camera spherical --frames 4

and read k_generate off the kernel statistics (python tools/summarize_prof.py OUT; profiles/spherical_camera.md)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shimmer_amd import abi, render, scenes  # noqa: E402

INSIDE = dict(pos=(1.2, 0.4, 2.4), look_at=(0.0, 0.0, 0.0))  # in front of the object, to the right of the scene's own camera: inside the room


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--camera", default="spherical", choices=["perspective", "spherical"])
    ap.add_argument("--mapping", default="equalarea", choices=["equalarea", "equirectangular"])
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=599)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--max-depth", type=int, default=5)
    args = ap.parse_args()
    lib = abi.load_library()
    if lib.shm_device_count() < 1:
        raise SystemExit("no HIP device visible (there is no CPU fallback)")
    cam = dict(INSIDE, type=args.camera, **(dict(mapping=args.mapping) if args.camera == "spherical" else {}))
    sc = scenes.ganesha_proxy(lib, args.res, args.res, n=args.n, camera=cam)
    r = render.Renderer(lib, sc.desc, 0)
    p = render.make_params(seed=0, spp=args.spp, max_depth=args.max_depth)
    rows = []
    for k in range(args.warmup + args.frames):
        r.clear()
        t0 = time.perf_counter()
        st = r.render_device(p)
        dt = time.perf_counter() - t0
        if k >= args.warmup:
            rows.append(dict(ms=dt * 1e3, ms_closest=st["ms_trace_closest"], ms_any=st["ms_trace_any"], ms_shade=st["ms_shade"], mrays=(st["rays_closest"] + st["rays_any"]) / 1e6))
    r.close()
    print(json.dumps(dict(camera=args.camera, mapping=args.mapping if args.camera == "spherical" else None, res=args.res, spp=args.spp, frames=rows)))


if __name__ == "__main__":
    main()
