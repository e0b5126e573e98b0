#!/usr/bin/env python3
"""Are the kernels of two builds of libshimmer_hip.so the same code? Disassembles every gfx950 code object embedded in each library (llvm-objdump) and compares, per kernel
symbol, the instruction text with addresses, branch targets and the padding behind s_endpgm stripped. Prints how many of the FIRST library's symbols are identical, different or
missing in the second, and the second's new symbols. A symbol that several code objects define (an anonymous-namespace kernel or a noinline device function of a
unit that is compiled more than once) is compared as the SET of its distinct texts: more copies of the same texts are the same code. With tools/kernel_resources.py (registers, spills, LDS, scratch) this is the check that a change left existing kernels alone.

With --without SUBSTRING the comparison is per CODE OBJECT instead: every code object of the first library that defines no symbol containing SUBSTRING must have a twin in
the second — the same symbols with the same instruction texts, one to one — and the second may hold no further such object. This is the form for a change that lives in the
*_dl builds only (--without _dl): a noinline device function that every unit defines (base_f_v, get_bsdf_general, ...) then counts with the object it is linked into, where
the comparison by name above can only say that the library as a whole holds more distinct texts of it.

    python tools/kernel_isa_diff.py parent/libshimmer_hip.so shimmer_amd/csrc/libshimmer_hip.so
    python tools/kernel_isa_diff.py --without _dl parent/libshimmer_hip.so shimmer_amd/csrc/libshimmer_hip.so"""
import collections
import hashlib
import os
import re
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def kernels(lib, per_object=False):
    data = open(lib, "rb").read()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, m in enumerate(re.finditer(b"\x7fELF\x02\x01\x01", data)):
            o = m.start()
            if int.from_bytes(data[o + 18:o + 20], "little") != 224:  # EM_AMDGPU
                continue
            shoff = int.from_bytes(data[o + 40:o + 48], "little")
            size = shoff + int.from_bytes(data[o + 58:o + 60], "little") * int.from_bytes(data[o + 60:o + 62], "little")
            fn = os.path.join(tmp, f"co{k}.elf")
            open(fn, "wb").write(data[o:o + size])
            text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", fn], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in text.splitlines():
                head = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line.strip())
                if head:
                    cur = (head.group(1), k)  # (one text per code object that defines the symbol)
                    out.setdefault(cur, [])
                    continue
                ins = re.sub(r"//.*", "", line).strip()
                if cur is None or not ins or ins == "...":
                    continue
                ins = re.sub(r"<[^>]*>", "<L>", ins)
                out[cur].append(re.sub(r"\b(s_c?branch\w*|s_call\w*)\s+\S+", r"\1 T", ins))
    if per_object:  # one {symbol: text} table per code object
        objs = collections.defaultdict(dict)
        for (name, k), v in out.items():
            objs[k][name] = hashlib.sha1("\n".join(v).encode()).hexdigest()
        return list(objs.values())
    by_name = {}
    for (name, _), v in out.items():
        texts, n_ins, n_copies = by_name.setdefault(name, (set(), 0, 0))
        texts.add(hashlib.sha1("\n".join(v).encode()).hexdigest())
        by_name[name] = (texts, max(n_ins, len(v)), n_copies + 1)
    return {name: (frozenset(texts), n_ins, n_copies) for name, (texts, n_ins, n_copies) in by_name.items()}


def objects_main(sub, lib_a, lib_b):
    def untouched(lib):
        return collections.Counter(tuple(sorted(o.items())) for o in kernels(lib, per_object=True) if not any(sub in n for n in o))
    a, b = untouched(lib_a), untouched(lib_b)
    twins, extra = sum((a & b).values()), sum((b - a).values())
    print(f"code objects without a symbol containing '{sub}': {sum(a.values())} in the first library ({sum(len(k) * c for k, c in a.items())} symbol definitions), "
          f"{sum(b.values())} in the second — {twins} with an identical twin, {sum((a - b).values())} without one, {extra} only in the second")
    for k in (a - b):  # name the symbols that keep it from matching the second library's closest object (the one that shares most definitions)
        best = max(b - a, key=lambda o: len(set(k) & set(o)), default=())
        theirs = dict(best)
        changed = [n for n, h in k if n in theirs and theirs[n] != h]
        absent = [n for n, _ in k if n not in theirs]
        print(f"NO TWIN: the object of {', '.join(n for n, _ in k[:3])} ... ({len(k)} symbols) — against the closest object of the second library: "
              f"different text: {', '.join(changed) or 'none'}; not defined there: {', '.join(absent) or 'none'}; only there: {', '.join(n for n in theirs if n not in dict(k)) or 'none'}")
    return 1 if (a - b) or extra else 0


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--without":
        return objects_main(*sys.argv[2:])
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    same = [k for k in a if k in b and a[k][0] == b[k][0]]
    diff = [k for k in a if k in b and a[k][0] != b[k][0]]
    gone = [k for k in a if k not in b]
    new = [k for k in b if k not in a]
    print(f"symbols of the first library: {len(a)} — identical {len(same)}, different {len(diff)}, missing {len(gone)}; new in the second: {len(new)}")
    for k in same:
        if a[k][2] != b[k][2]:
            print(f"IDENTICAL {k}: {a[k][2]} -> {b[k][2]} copies of the same {len(a[k][0])} text(s)")
    for k in diff:
        print(f"DIFFERENT {k}: {a[k][1]} -> {b[k][1]} instructions, {len(a[k][0])} -> {len(b[k][0])} distinct texts in {a[k][2]} -> {b[k][2]} copies")
    for k in gone:
        print("MISSING", k)
    for k in new:
        print(f"NEW {k}: {b[k][1]} instructions")
    return 1 if diff or gone else 0


if __name__ == "__main__":
    sys.exit(main())
