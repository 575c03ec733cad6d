"""Compare the gfx950 kernels of two builds of the library, kernel by kernel (the acceptance check of a
refactor that must not change device code).

Instruction streams: the disassembly of every code object (disassemble() of check_dma_hazards.py),
comments stripped, lines that are not instructions dropped, a branch's target kept as its offset from
the kernel's start; each kernel is compared to the kernel of the same name in the other library.
Resources: each kernel's VGPR, AGPR and SGPR counts, LDS bytes, scratch bytes and kernarg size from
the code objects' metadata notes.

    python tools/kernel_isa_diff.py OLD.so NEW.so
Prints the kernels present on one side only, the kernels that differ (with the first differing
instruction or the differing resources) and the number of identical kernels. Exit status 1 unless
every kernel name is on both sides and every kernel is identical. Needs objcopy,
clang-offload-bundler, llvm-objdump and llvm-readelf (ROCm).
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_dma_hazards import LLVM, disassemble  # noqa: E402

RES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
       "kernarg_segment_size")


def streams(lib):
    """-> {kernel: [instruction text]}"""
    out, cur = {}, None
    for raw in disassemble(lib):
        m = re.match(r"^[0-9a-f]+ <(.+)>:", raw)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        code, _, comment = raw.partition("//")
        code = " ".join(code.split())
        # (not instructions: blank lines, "...", "file format" and "Disassembly of section" headers)
        if cur is None or not code or code == "..." or not raw.startswith((" ", "\t")):
            continue
        t = re.search(r"<[^>+]+(\+0x[0-9a-f]+)?>", comment)
        cur.append(code + (" -> " + (t.group(1) or "+0x0") if t else ""))
    return out


def resources(lib):
    """-> {kernel: {resource: value}} from the metadata notes of every code object in the library"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat")
        subprocess.run(["objcopy", "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(d, "copy.so")],
                       check=True, capture_output=True)
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)]
        for a, b in zip(starts, starts[1:] + [len(data)]):
            part, co = os.path.join(d, "part"), os.path.join(d, "co")
            open(part, "wb").write(data[a:b])
            r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}",
                                "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True)
            if r.returncode != 0 or not os.path.getsize(co):
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True,
                                   capture_output=True, text=True).stdout
            # one "  - .agpr_count: ..." entry per kernel; its argument list is indented deeper
            for entry in re.split(r"\n  - ", notes)[1:]:
                keys = dict(re.findall(r"^(?:    |)\.(\w+): +(\S+)$", entry, re.M))
                if "name" in keys:
                    out[keys["name"]] = {k: keys.get(k) for k in RES}
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = sys.argv[1:]
    so, sn, ro, rn = streams(old), streams(new), resources(old), resources(new)
    kernels = sorted(set(ro) | set(rn))
    only = [(k, "OLD" if k in ro else "NEW") for k in kernels if (k in ro) != (k in rn)]
    for k, side in only:
        print(f"only in {side}: {k}")
    same = differ = 0
    for k in kernels:
        if k not in ro or k not in rn:
            continue
        a, b = so.get(k, []), sn.get(k, [])
        why = None
        if ro[k] != rn[k]:
            why = "resources " + ", ".join(f"{r} {ro[k][r]} -> {rn[k][r]}" for r in RES if ro[k][r] != rn[k][r])
        elif a != b or not a:
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            why = f"instruction {i} of {len(a)} / {len(b)}: {a[i] if i < len(a) else '<end>'} | {b[i] if i < len(b) else '<end>'}"
        if why:
            differ += 1
            print(f"differs: {k}: {why}")
        else:
            same += 1
    print(f"kernel_isa_diff: {same} identical, {differ} differ, {len(only)} on one side only "
          f"({len(ro)} kernels in OLD, {len(rn)} in NEW)")
    return 0 if not differ and not only else 1


if __name__ == "__main__":
    sys.exit(main())
