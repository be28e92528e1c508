#!/usr/bin/env python3
"""Device code of two builds of libldt_hip.so, kernel by kernel (no GPU): the disassembly with addresses, encodings and branch offsets
dropped, plus VGPR / AGPR / SGPR counts, LDS, scratch and spills of the code objects' metadata.  Prints one line per kernel
(verdict, instruction count, resources, name), then the totals.   usage: lib_codegen_diff.py libA.so libB.so"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "ldt_amd", "csrc"))
import isa_lint

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count",
        ".sgpr_spill_count")


def kernels_of(lib):
    out = {}
    for elf in isa_lint.code_objects(lib):
        code, meta = isa_lint.disassemble(elf)
        for name, m in meta.items():
            text = tuple(i.op if i.target is not None else i.text for i in code[name])
            assert name not in out, name
            out[name] = (text, tuple(m.get(k) for k in META))
    return out


a, b = kernels_of(sys.argv[1]), kernels_of(sys.argv[2])
names = isa_lint.demangle(sorted(set(a) | set(b)))
differ = 0
print("verdict  instructions  " + " ".join(k[1:].replace("_count", "").replace("_segment_fixed_size", "") for k in META) + "  kernel")
for n in sorted(set(a) | set(b), key=lambda n: names[n]):
    if n not in a or n not in b:
        print("only in %s: %s" % (sys.argv[1 if n in a else 2], names[n]))
        continue
    differ += a[n] != b[n]
    verdict = "same" if a[n] == b[n] else "INSTRUCTIONS" if a[n][0] != b[n][0] else "RESOURCES"
    res = " ".join(str(x) if x == y else "%s->%s" % (x, y) for x, y in zip(a[n][1], b[n][1]))
    print("%-8s %6d%s  %s  %s" % (verdict, len(a[n][0]), "" if len(a[n][0]) == len(b[n][0]) else "->%d" % len(b[n][0]), res, names[n]))
print("kernel symbols: %d in %s, %d in %s, %d in both; instructions compared: %d; kernels that differ: %d"
      % (len(a), sys.argv[1], len(b), sys.argv[2], len(set(a) & set(b)), sum(len(a[n][0]) for n in set(a) & set(b)), differ))
print("resources compared per kernel: " + " ".join(k[1:] for k in META))
