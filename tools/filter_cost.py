#!/usr/bin/env python3
"""What a pixel filter costs on the headline scene (S3, 1024^2 x 256 spp, max_depth 5): each filter's frame against the box frame of the SAME build, alternating
(box, F1, box, F2, ...), one renderer per entry, `--warmup` frames then `--frames` timed ones. Prints one line per entry — wall time per frame and the
library's own breakdown (closest-hit launches, any-hit launches, everything else = shade + generate + film) — and a JSON summary last.

    python tools/filter_cost.py [--filters gaussian,mitchell,sinc,triangle] [--frames 2] [--n 599] [--res 1024] [--spp 256] [--sampler independent]

For the two kernels alone run it under `rocprofv3 --kernel-trace --stats -- python tools/filter_cost.py --frames 1 --warmup 0 --filters <one>` and read k_generate* / k_film*
off the kernel statistics (profiles/pixel_filters.md)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shimmer_amd import abi, render, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--filters", default="gaussian,mitchell,sinc,triangle")
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=599)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--max-depth", type=int, default=5)
    ap.add_argument("--sampler", default="independent", choices=["independent", "zsobol"])
    ap.add_argument("--no-box", action="store_true", help="only the named filters, without the box frames between them")
    args = ap.parse_args()
    lib = abi.load_library()
    if lib.shm_device_count() < 1:
        raise SystemExit("no HIP device visible (there is no CPU fallback)")
    order = []
    for name in [f for f in args.filters.split(",") if f]:
        order += [name] if args.no_box else ["box", name]
    p = render.make_params(seed=0, spp=args.spp, max_depth=args.max_depth, sampler=args.sampler)
    rows = []
    sc = scenes.ganesha_proxy(lib, args.res, args.res, n=args.n)  # (built once: only the film's filter fields change between the entries)
    for name in order:
        kind, radius, params = sc.builder.FILTERS[name]
        sc.desc.film.filter = kind
        sc.desc.film.filter_radius[:] = (radius, radius)
        sc.desc.film.filter_params[:] = (tuple(params) + (0.0, 0.0))[:2]
        r = render.Renderer(lib, sc.desc, 0)
        for _ in range(args.warmup):
            r.clear()
            r.render_device(p)
        for _ in range(args.frames):
            r.clear()
            t0 = time.perf_counter()
            st = r.render_device(p)
            wall = (time.perf_counter() - t0) * 1e3
            row = dict(filter=name, wall_ms=round(wall, 2), gpu_ms=round(st["ms_total"], 2), closest_ms=round(st["ms_trace_closest"], 2), any_ms=round(st["ms_trace_any"], 2),
                       shade_generate_film_ms=round(st["ms_shade"], 2), rays=st["rays_closest"] + st["rays_any"])
            rows.append(row)
            print(f"{name:9s} wall {wall:8.2f} ms | gpu {st['ms_total']:8.2f} = closest {st['ms_trace_closest']:7.2f} + any {st['ms_trace_any']:7.2f} + shade/generate/film "
                  f"{st['ms_shade']:7.2f} | {row['rays'] / 1e6:.1f} Mrays", flush=True)
        r.close()
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
