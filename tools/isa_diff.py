#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 code in two builds of libbspgemm.so (or two objects); needs no GPU.
    tools/isa_diff.py OLD.so NEW.so [-v] [--rename 'REGEX=REPLACEMENT' ...]
Every code object is disassembled; per kernel the addresses, the encodings and the padding behind the last instruction are
dropped.  Kernels are paired by demangled name without the argument list; a kernel that was renamed is paired through
--rename, a regular expression for the whole old name (behind its namespace) and what it becomes, e.g.
    --rename 'k_rank_rows<(true|false)>=k_rank_rows<\1, (bsp::MaskMode)0>'
Per kernel: `identical`, `identical but for s_load offsets` (the same instructions and registers; only immediates of
s_load_dword*, i.e. places in the argument list, differ) or `DIFFERENT`; kernels on one side only are listed.  Prints the
kernels that are not identical (-v: all) and the totals; exit status 1 on any DIFFERENT or unpaired kernel."""
import re
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
# what may follow a kernel's last instruction: padding, elided zeros, an all-zero dword
PADDING = r"s_code_end|s_nop|\.\.\.|v_cndmask_b32_e32 v0, s0, v0, vcc$"


def kernels(path):
    """{demangled name without arguments: [instruction, ...]} over the gfx950 entries of every offload bundle in the file"""
    data, out, body = open(path, "rb").read(), {}, None
    at = data.find(MAGIC)
    while at >= 0:
        p = at + len(MAGIC) + 8
        for _ in range(struct.unpack_from("<Q", data, p - 8)[0]):
            off, size, idlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + idlen]
            p += 24 + idlen
            if b"gfx950" not in triple or not size:
                continue
            with tempfile.NamedTemporaryFile(suffix=".co") as f:
                f.write(data[at + off:at + off + size])
                f.flush()
                text = subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump", "-d", "--no-show-raw-insn", f.name],
                                      capture_output=True, text=True, check=True).stdout
            for line in text.splitlines():
                m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
                if m:
                    body = out.setdefault(m.group(1), [])
                elif body is not None and line.startswith("\t"):
                    body.append(" ".join(line.split("//")[0].split()))          # (the comment holds address and encoding)
        at = data.find(MAGIC, at + 1)
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.splitlines()
    res = {}
    for name, body in zip(names, out.values()):
        while body and re.match(PADDING, body[-1]):
            body.pop()
        name = re.sub(r"^void ", "", name)
        res[name[:name.find(">(") + 1] if ">(" in name else name.split("(")[0]] = body
    return res


verbose = "-v" in sys.argv
args = [a for a in sys.argv[1:] if a != "-v"]
renames = []
while "--rename" in args:
    i = args.index("--rename")
    renames.append(args[i + 1].split("=", 1))
    del args[i:i + 2]
old, new = kernels(args[0]), kernels(args[1])
for pat, rep in renames:
    old = {re.sub(r"\b" + pat + "$", rep, k): v for k, v in old.items()}


def masked(body):
    return [re.sub(r"^(s_load_dword\w* .*, )\S+$", r"\1#", i) for i in body]


tally = {"identical": 0, "identical but for s_load offsets": 0, "DIFFERENT": 0}
for k in sorted(old.keys() & new.keys()):
    verdict = "identical" if old[k] == new[k] else "identical but for s_load offsets" if masked(old[k]) == masked(new[k]) else "DIFFERENT"
    tally[verdict] += 1
    if verbose or verdict != "identical":
        print("%-34s %s" % (verdict, k))
for side, only in (("old", old.keys() - new.keys()), ("new", new.keys() - old.keys())):
    for k in sorted(only):
        print("%-34s %s" % ("only in " + side, k))
unpaired = len(old.keys() ^ new.keys())
print("kernels: %d old, %d new; %s; %d unpaired" % (len(old), len(new), ", ".join("%d %s" % (v, k) for k, v in tally.items()), unpaired))
sys.exit(1 if tally["DIFFERENT"] or unpaired else 0)
