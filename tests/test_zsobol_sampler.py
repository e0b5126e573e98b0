"""The ZSobol sampler (shm/sampling.h; DESIGN.md "Sampler") on the CPU: a Python restatement of the stream — Morton index, per-digit permutation,
Sobol' dimensions 0 and 1, FastOwen, MurmurHash64A, float conversion — against the host build of the header, bit for bit; the (0, m, 2)-net
properties of the draws on their u32 values; the loader's `Sampler "zsobol"`; the two new ShmRenderParams fields."""
import ctypes as C
import itertools
import random
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from shimmer_amd import abi, render

ROOT = Path(__file__).resolve().parents[1]
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
PERMS = list(itertools.permutations(range(4)))  # lexicographic order


# ---- the restatement ----
def mix_bits(v):
    v ^= v >> 31
    v = (v * 0x7fb5d329728ea185) & M64
    v ^= v >> 27
    v = (v * 0x81dadef4bc2dd44d) & M64
    v ^= v >> 33
    return v


def ceil_log2(v):
    l = 0
    while (1 << l) < v:
        l += 1
    return l


def config(spp, rx, ry):
    log2spp = ceil_log2(max(spp, 1))
    return log2spp, ceil_log2(max(rx, ry, 1)) + (log2spp + 1) // 2


def morton2(x, y):
    return sum(((x >> i) & 1) << (2 * i) | ((y >> i) & 1) << (2 * i + 1) for i in range(32))


def sample_index(morton, dim, log2spp, n_digits):
    odd = log2spp & 1
    dmix = (0x55555555 * dim) & M32
    index = 0
    for i in range(n_digits - 1, odd - 1, -1):
        shift = 2 * i - odd
        digit = (morton >> shift) & 3
        higher = morton >> (shift + 2)
        p = (mix_bits(higher ^ dmix) >> 24) % 24
        index |= PERMS[p][digit] << shift
    if odd:
        index |= (morton & 1) ^ (mix_bits((morton >> 1) ^ dmix) & 1)
    return index


def sobol(a, d):
    v, c, k = 0, 0x80000000, 0
    while a:
        if a & 1:
            v ^= (1 << (31 - k) if k < 32 else 0) if d == 0 else c
        a >>= 1
        k += 1
        c ^= c >> 1
    return v


def rev32(v):
    return int(f"{v:032b}"[::-1], 2)


def fast_owen(v, s):
    v = rev32(v)
    v ^= (v * 0x3d20adea) & M32
    v = (v + s) & M32
    v = (v * ((s >> 16) | 1)) & M32
    v ^= (v * 0x05526c56) & M32
    v ^= (v * 0x53a22864) & M32
    return rev32(v)


def murmur64a(data, seed=0):
    m, r = 0xc6a4a7935bd1e995, 47
    h = (seed ^ (len(data) * m)) & M64
    n8 = len(data) // 8
    for i in range(n8):
        k = int.from_bytes(data[8 * i:8 * i + 8], "little")
        k = (k * m) & M64
        k ^= k >> r
        k = (k * m) & M64
        h ^= k
        h = (h * m) & M64
    tail = data[8 * n8:]
    if tail:
        for i in range(len(tail) - 1, -1, -1):
            h ^= tail[i] << (8 * i)
        h = (h * m) & M64
    h ^= h >> r
    h = (h * m) & M64
    h ^= h >> r
    return h


def zhash(dim, seed):
    return murmur64a(dim.to_bytes(4, "little", signed=False) + seed.to_bytes(8, "little"))


def to_float(v):
    return min(np.float32(v) * np.float32(2.0 ** -32), np.float32(0.99999994))


def stream(px, py, index, spp, rx, ry, seed, none, kinds):
    """The u32 values of the draws `kinds` (1: get_1d, 2: get_2d) from start_pixel_sample((px, py), index)."""
    log2spp, nd = config(spp, rx, ry)
    morton = (morton2(px, py) << log2spp) | index
    dim, out = 0, []
    for k in kinds:
        idx = sample_index(morton, dim, log2spp, nd)
        dim += k
        h = zhash(dim, seed)
        x = sobol(idx, 0)
        if k == 1:
            out.append(x if none else fast_owen(x, h & M32))
        else:
            y = sobol(idx, 1)
            out += [x, y] if none else [fast_owen(x, h & M32), fast_owen(y, h >> 32)]
    return out


# ---- the host build of shm/sampling.h ----
DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "shm/sampling.h"
using namespace shm;
int main() {
    unsigned px, py, idx, spp, rx, ry, none, n; unsigned long long seed;
    while (scanf("%u %u %u %u %u %u %llu %u %u", &px, &py, &idx, &spp, &rx, &ry, &seed, &none, &n) == 9) {
        Rng r = sampler_start_pixel_sample((int)px, (int)py, (int)idx, seed, zsobol_config((int)spp, (int)rx, (int)ry, none != 0));
        for (unsigned i = 0; i < n; ++i) {
            unsigned k; if (scanf("%u", &k) != 1) return 1;
            // half the draws through a save / resume round trip: what a path keeps between kernels
            if (i & 1) r = sampler_resume(sampler_save(r), px, py, seed, r.zs);
            if (k == 2) {
                Rng q = r;
                uint32_t x, y; zsobol_next_2d_bits(r, x, y);
                V2 f = sampler_get_2d(q);
                uint32_t fx, fy; memcpy(&fx, &f.x, 4); memcpy(&fy, &f.y, 4);
                printf("%u %u %u %u ", x, y, fx, fy);
            } else {
                Rng q = r;
                uint32_t x = zsobol_next_1d_bits(r);
                float f = sampler_get_1d(q);
                uint32_t fb; memcpy(&fb, &f, 4);
                printf("%u %u ", x, fb);
            }
        }
        printf("\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_stream(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("zsobol")
    (d / "drv.cpp").write_text(DRIVER)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", str(ROOT / "shimmer_amd" / "csrc"), str(d / "drv.cpp"),
                    "-o", str(d / "drv")], check=True)

    def run(cases):
        text = "".join(f"{px} {py} {i} {spp} {rx} {ry} {seed} {int(none)} {len(k)} " + " ".join(map(str, k)) + "\n" for px, py, i, spp, rx, ry, seed, none, k in cases)
        out = subprocess.run([str(d / "drv")], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
        res = []
        for line, c in zip(out, cases):
            w = list(map(int, line.split()))
            u, f, o = [], [], 0
            for k in c[8]:
                u += w[o:o + k]
                f += w[o + k:o + 2 * k]
                o += 2 * k
            res.append((u, f))
        return res
    return run


def random_cases(n, rng):
    cases = []
    for _ in range(n):
        spp = rng.choice([1, 2, 16, 32, 48, 256])
        rx, ry = rng.choice([(64, 64), (160, 120), (37, 300), (1024, 768), (5, 3)])
        px, py = rng.randrange(rx), rng.randrange(ry)
        seed = rng.getrandbits(64) | (1 << 40) if rng.random() < 0.5 else rng.getrandbits(64)
        kinds = [rng.choice([1, 2]) for _ in range(rng.randrange(1, 9))]
        cases.append((px, py, rng.randrange(spp), spp, rx, ry, seed, rng.random() < 0.3, kinds))
    return cases


def test_host_build_equals_the_restatement(host_stream):
    """3 000 random (pixel, index, spp, resolution, seed, randomization) cases, 1D and 2D draws mixed: u32 and float bits equal."""
    cases = random_cases(3000, random.Random(1234))
    for c, (u, f) in zip(cases, host_stream(cases)):
        want = stream(*c)
        assert u == want, c
        assert f == [int(np.float32(to_float(v)).view(np.uint32)) for v in want], c


def test_every_seed_bit_changes_the_stream(host_stream):
    base = (3, 5, 1, 16, 64, 64, 0x0123456789abcdef, False, [1, 2, 2])
    cases = [base] + [base[:6] + (base[6] ^ (1 << b),) + base[7:] for b in range(64)]
    res = [tuple(u) for u, _ in host_stream(cases)]
    assert len(set(res)) == len(res)


def test_sobol_dimension_one_is_the_pascal_matrix():
    """The header computes dimension 1 by Lucas' theorem (a superset sum over index bits); the columns by the recurrence c_k = c_{k-1} ^ (c_{k-1} >> 1)."""
    c = 0x80000000
    for k in range(40):
        lucas = sum(1 << (31 - j) for j in range(32) if (j & k) == j)
        assert c == lucas and sobol(1 << k, 1) == c
        c ^= c >> 1


@pytest.mark.parametrize("m", [0, 1, 2, 3, 4, 5, 6, 8])
@pytest.mark.parametrize("none", [False, True])
def test_draws_of_a_pixel_are_nets(host_stream, m, none):
    """spp = 2^m: over the pixel's samples, each of its first 12 draws is a (0, m, 1)-net (1D: one sample per [k / 2^m, (k + 1) / 2^m)) or a (0, m, 2)-net
    (2D: one per elementary interval 2^-a x 2^-b, a + b = m). On the u32 values: a float can round 0x7fffffff up to 0.5."""
    spp = 1 << m
    kinds = [1, 2, 2, 1, 2, 1, 1, 2, 2, 2, 1, 2]
    for px, py in [(0, 0), (7, 3), (63, 62), (20, 41)]:
        cases = [(px, py, i, spp, 64, 64, 99, none, kinds) for i in range(spp)]
        rows = [u for u, _ in host_stream(cases)]
        assert rows == [stream(*c) for c in cases]
        o = 0
        for k in kinds:
            vals = [r[o:o + k] for r in rows]
            if k == 1:
                assert sorted(v[0] >> (32 - m) if m else 0 for v in vals) == list(range(spp))
            else:
                for a in range(m + 1):
                    b = m - a
                    cells = {((v[0] >> (32 - a)) if a else 0, (v[1] >> (32 - b)) if b else 0) for v in vals}
                    assert len(cells) == spp, (px, py, k, a, b)
            o += k


def test_unscrambled_first_draws_at_4spp(host_stream):
    """Randomization "none", spp = 4, pixel (0, 0) of a 1x1 film: the four samples' first 2D draw is the Sobol' net {0, 1/2} x {0, 1/2} pattern,
    visited in the order the digit permutation gives."""
    cases = [(0, 0, i, 4, 1, 1, 0, True, [2, 1]) for i in range(4)]
    rows = [u for u, _ in host_stream(cases)]
    assert rows == [stream(*c) for c in cases]
    pts = sorted((r[0], r[1]) for r in rows)
    assert pts == [(0, 0), (0x40000000, 0xc0000000), (0x80000000, 0x80000000), (0xc0000000, 0x40000000)]
    assert sorted(r[2] >> 30 for r in rows) == [0, 1, 2, 3]


# ---- the ABI ----
def test_render_params_fields():
    assert C.sizeof(abi.ShmRenderParams) == 32
    assert abi.ShmRenderParams.sampler.offset == 25 and abi.ShmRenderParams.sampler_randomization.offset == 26
    assert abi.ShmRenderParams.pad.offset == 27 and abi.ShmRenderParams.pad.size == 5
    p = render.make_params()
    assert p.sampler == abi.SHM_SAMPLER_INDEPENDENT == 0 and p.sampler_randomization == abi.SHM_SAMPLER_FASTOWEN == 0
    p = render.make_params(sampler="zsobol", randomization="none")
    assert p.sampler == abi.SHM_SAMPLER_ZSOBOL == 1 and p.sampler_randomization == abi.SHM_SAMPLER_RANDOMIZE_NONE == 1
    with pytest.raises(KeyError):
        render.make_params(sampler="halton")


def test_header_agrees_with_abi_py(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no C compiler")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "shimmer_hip.h"\nint main(void) {\n'
           '  printf("%zu %zu %zu %zu %d %d %d %d\\n", sizeof(ShmRenderParams), offsetof(ShmRenderParams, sampler), offsetof(ShmRenderParams, sampler_randomization),'
           ' offsetof(ShmRenderParams, pad), SHM_SAMPLER_INDEPENDENT, SHM_SAMPLER_ZSOBOL, SHM_SAMPLER_FASTOWEN, SHM_SAMPLER_RANDOMIZE_NONE);\n  return 0;\n}\n')
    (tmp_path / "p.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "p.c"), "-o", str(tmp_path / "p")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "p")], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [32, abi.ShmRenderParams.sampler.offset, abi.ShmRenderParams.sampler_randomization.offset, abi.ShmRenderParams.pad.offset,
                   abi.SHM_SAMPLER_INDEPENDENT, abi.SHM_SAMPLER_ZSOBOL, abi.SHM_SAMPLER_FASTOWEN, abi.SHM_SAMPLER_RANDOMIZE_NONE]


# ---- the loader ----
SCENE = 'WorldBegin\nLightSource "point" "rgb I" [1 1 1]\nShape "sphere" "float radius" 1\n'


def parse(lib, text):
    out = C.POINTER(abi.ShmPbrtScene)()
    rc = lib.shm_scene_parse_pbrt(text.encode(), None, C.byref(out))
    return rc, out


@pytest.mark.parametrize("line, sampler, rnd, spp, seed", [
    ('Sampler "zsobol" "integer pixelsamples" 64 "integer seed" 7', abi.SHM_SAMPLER_ZSOBOL, abi.SHM_SAMPLER_FASTOWEN, 64, 7),
    ('Sampler "zsobol" "string randomization" "fastowen"', abi.SHM_SAMPLER_ZSOBOL, abi.SHM_SAMPLER_FASTOWEN, 16, 0),
    ('Sampler "zsobol" "integer pixelsamples" 8 "string randomization" "none"', abi.SHM_SAMPLER_ZSOBOL, abi.SHM_SAMPLER_RANDOMIZE_NONE, 8, 0),
    ('Sampler "independent" "integer pixelsamples" 8', abi.SHM_SAMPLER_INDEPENDENT, abi.SHM_SAMPLER_FASTOWEN, 8, 0),
    ('', abi.SHM_SAMPLER_INDEPENDENT, abi.SHM_SAMPLER_FASTOWEN, 4, 0),
])
def test_loader_fills_the_sampler(lib, line, sampler, rnd, spp, seed):
    rc, out = parse(lib, line + "\n" + SCENE)
    assert rc == 0, lib.shm_last_error()
    p = out.contents.params
    assert (p.sampler, p.sampler_randomization, p.samples_per_pixel, p.seed) == (sampler, rnd, spp, seed)
    lib.shm_pbrt_free(out)


@pytest.mark.parametrize("line, needle", [
    ('Sampler "zsobol" "string randomization" "owen"', "randomization \"owen\" is not supported"),
    ('Sampler "zsobol" "string randomization" "permutedigits"', "randomization \"permutedigits\" is not supported"),
] + [(f'Sampler "{s}"', f'sampler "{s}" is not supported') for s in ("halton", "sobol", "paddedsobol", "pmj02bn", "stratified")])
def test_loader_rejects_other_samplers(lib, line, needle):
    rc, out = parse(lib, "\n" + line + "\n" + SCENE)
    assert rc == -2 and not out  # SHM_ERR_UNSUPPORTED
    msg = lib.shm_last_error().decode()
    assert needle in msg and "<string>:2" in msg, msg
