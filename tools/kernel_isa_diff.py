#!/usr/bin/env python3
"""Are the kernels of two builds of libshimmer_hip.so the same code? Disassembles every gfx950 code object embedded in each library (llvm-objdump) and compares, per kernel
symbol, the instruction text with addresses, branch targets and the padding behind s_endpgm stripped. Prints how many of the FIRST library's symbols are identical, different or
missing in the second, and the second's new symbols. A symbol that several code objects define (an anonymous-namespace kernel or a noinline device function of a
unit that is compiled more than once) is compared as the SET of its distinct texts: more copies of the same texts are the same code. With tools/kernel_resources.py (registers, spills, LDS, scratch) this is the check that a change left existing kernels alone.

    python tools/kernel_isa_diff.py parent/libshimmer_hip.so shimmer_amd/csrc/libshimmer_hip.so"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def kernels(lib):
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
    by_name = {}
    for (name, _), v in out.items():
        texts, n_ins, n_copies = by_name.setdefault(name, (set(), 0, 0))
        texts.add(hashlib.sha1("\n".join(v).encode()).hexdigest())
        by_name[name] = (texts, max(n_ins, len(v)), n_copies + 1)
    return {name: (frozenset(texts), n_ins, n_copies) for name, (texts, n_ins, n_copies) in by_name.items()}


def main():
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
