#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two objects, up to the order of the functions: what stands in for byte
identity (tools/fatbin_digest.py) when a host-side change only moved the point where kernel templates are first instantiated.

    python tools/fatbin_kernel_diff.py other/_obj/knn.o neuralsampleid_amd/csrc/_obj/knn.o

Equal means: the same set of functions, every kernel's resource metadata (registers, LDS, scratch, spills, kernel arguments) equal,
and every function's instructions equal, encodings included. Two things that follow from the position of a function are taken out
first: the padding behind its last instruction, and the literal of a pc-relative address (s_getpc_b64 + s_add_u32), which is
replaced by the symbol (or, for constants without one, the section) and offset it resolves to. Exit status 0 when equal."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
META = (".agpr_count", ".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
        ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size", ".vgpr_spill_count", ".sgpr_spill_count")


def run(*cmd) -> str:
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def load(obj: str, tmp: str, tag: str):
    fb, co = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".co")
    run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(tmp, "null"))
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}",
        f"--output={co}")
    syms = []                                   # (address, size, name) of everything defined
    for line in run(f"{LLVM}/llvm-readelf", "-sW", co).splitlines():
        p = line.split()
        if len(p) >= 8 and p[0].rstrip(":").isdigit() and p[6] != "UND":
            syms.append((int(p[1], 16), int(p[2], 0), p[7]))

    secs = []                                   # (address, size, name) of the allocated sections: constants have no symbol
    for m in re.finditer(r"^\s*\[\s*\d+\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+[0-9a-f]+\s+([0-9a-f]+)", run(f"{LLVM}/llvm-readelf", "-SW", co), re.M):
        if int(m.group(2), 16):
            secs.append((int(m.group(2), 16), int(m.group(3), 16), m.group(1)))

    def resolve(addr):
        hit = [(n, addr - a) for a, sz, n in syms + secs if a <= addr < a + max(sz, 1)]
        return hit[0] if hit else ("?", addr)

    funcs, cur = {}, None
    for line in run(f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif cur is not None and "//" in line:
            ins, rest = line.split("//", 1)
            addr, enc = rest.split(":", 1)
            cur.append([ins.strip(), enc.strip(), int(addr.strip(), 16)])
    for body in funcs.values():
        while body and body[-1][0].split()[0] in ("s_code_end", "s_nop"):
            body.pop()
        for i in range(1, len(body)):           # s_getpc_b64 at A returns A + 4; the s_add_u32 at A + 4 adds target - (A + 4)
            m = re.match(r"s_add_u32 (s\d+), \1, (0x[0-9a-f]+|\d+)$", body[i][0])
            if m and body[i - 1][0].startswith("s_getpc_b64") and len(body[i][1].split()) == 2:
                target = (body[i][2] + int(m.group(2), 0)) & 0xFFFFFFFF
                body[i][:2] = [f"s_add_u32 {m.group(1)}, {m.group(1)}, <{resolve(target)}>", ""]
    meta = {}
    for blk in re.split(r"\n\s*- \.agpr_count", run(f"{LLVM}/llvm-readelf", "--notes", co))[1:]:
        kv = dict(re.findall(r"^\s*(\.[a-z_]+):\s*(\S+)\s*$", ".agpr_count" + blk, re.M))
        meta[kv.get(".name")] = {k: kv.get(k) for k in META}
    return {k: [(i, e) for i, e, _ in v] for k, v in funcs.items()}, meta


def main() -> int:
    with tempfile.TemporaryDirectory() as tmp:
        fa, ma = load(sys.argv[1], tmp, "a")
        fb, mb = load(sys.argv[2], tmp, "b")
    differ = sorted(k for k in fa if k in fb and fa[k] != fb[k])
    print(f"functions {len(fa)} / {len(fb)}, same set: {set(fa) == set(fb)}, same order: {list(fa) == list(fb)}")
    print(f"kernels {len(ma)} / {len(mb)}, same set: {set(ma) == set(mb)}, metadata equal: {ma == mb}")
    print(f"functions whose instructions differ: {len(differ)}")
    for k in differ:
        print("  " + k)
    return 0 if set(fa) == set(fb) and ma == mb and not differ else 1


if __name__ == "__main__":
    sys.exit(main())
