#!/usr/bin/env python3
"""The G-buffer pass on the S3 proxy at 1024^2 x 16 spp beside the frame it guides: `--frames` timed passes after `--warmup` — wall time and the library's own
breakdown (closest-hit launch; K1 plus the pass's two kernels) — and, for scale, a beauty render of max depth 0 of the same frame: K1, the bounce-0 closest-hit
launch, one vertex and K6. For the two kernels alone run it under

    rocprofv3 --kernel-trace --stats -d OUT/stats -o stats -- python tools/gbuffer_cost.py --frames 4

and read k_gbuffer / k_gbuffer_accumulate off the kernel statistics (python tools/summarize_prof.py OUT; profiles/gbuffer.md)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shimmer_amd import abi, render, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=599)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--coated", action="store_true", help="the object as a coated material: LayeredBxDF under rho_hd")
    ap.add_argument("--space", default="render", choices=["render", "camera"])
    args = ap.parse_args()
    lib = abi.load_library()
    if lib.shm_device_count() < 1:
        raise SystemExit("no HIP device visible (there is no CPU fallback)")
    sc = scenes.ganesha_proxy(lib, args.res, args.res, n=args.n, coated=args.coated)
    r = render.Renderer(lib, sc.desc, 0)
    p = render.make_params(seed=0, spp=args.spp, max_depth=5)
    p0 = render.make_params(seed=0, spp=args.spp, max_depth=0)
    space = abi.SHM_GBUFFER_SPACE_CAMERA if args.space == "camera" else abi.SHM_GBUFFER_SPACE_RENDER
    passes, first_vertex = [], []
    for k in range(args.warmup + args.frames):
        r.gbuffer_clear()
        t0 = time.perf_counter()
        st = r.gbuffer_wave(p, 0, args.spp, space=space)
        dt = time.perf_counter() - t0
        r.clear()
        t1 = time.perf_counter()
        sb = r.render_device(p0)
        db = time.perf_counter() - t1
        if k >= args.warmup:
            passes.append(dict(ms=dt * 1e3, ms_device=st["ms_total"], ms_closest=st["ms_trace_closest"], ms_k1_and_pass=st["ms_shade"], mrays=st["rays_closest"] / 1e6))
            first_vertex.append(dict(ms=db * 1e3, ms_device=sb["ms_total"], ms_closest=sb["ms_trace_closest"], ms_shade=sb["ms_shade"]))
    g = r.read_gbuffer()
    r.close()
    covered = float((g["weight_hit"] != 0).mean())
    print(json.dumps(dict(res=args.res, spp=args.spp, coated=args.coated, space=args.space, covered=covered, gbuffer=passes, depth0_render=first_vertex)))


if __name__ == "__main__":
    main()
