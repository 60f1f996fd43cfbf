#!/usr/bin/env python3
"""Is the device code of this tree's build the same as another build's?  For a host-only change: every gfx950 code object of both
libraries (bf16: csrc/*.o, fp16 storage: csrc/obj_f16/*.o) against the same object of another checkout built with the same compiler
and flags -- kernel names, register / LDS / scratch metadata, and the sha256 of the `llvm-objdump -d` text of the code object.

    python scripts/device_code_diff.py <other checkout>/difashion_amd/csrc

Exit status 0 when everything is equal."""
import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr  # noqa: E402


def disasm_sha(obj):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        r = subprocess.run([os.path.join(kr.LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj], capture_output=True)
        if r.returncode != 0 or not os.path.exists(fat):
            return None
        subprocess.run([os.path.join(kr.LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}", f"--targets={kr.TARGET}",
                        f"--output={co}"], check=True, capture_output=True)
        text = subprocess.run([os.path.join(kr.LLVM, "llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
    text = "\n".join(l for l in text.splitlines() if "file format" not in l and not l.startswith(co))      # drop the temporary path
    return hashlib.sha256(text.encode()).hexdigest()[:16]


def compare(mine, other, title):
    print(title)
    print(f"{'object':<24} kernels  names  metadata  device code (llvm-objdump -d of the gfx950 code object, sha256 of the text)")
    ok, total = True, 0
    objs = sorted(f for f in os.listdir(mine) if f.endswith(".o"))
    theirs = sorted(f for f in os.listdir(other) if f.endswith(".o"))
    for f in sorted(set(objs) ^ set(theirs)):      # an object of one build only is fine when it holds no device code (a new host-only file)
        path = os.path.join(mine if f in objs else other, f)
        host_only = disasm_sha(path) is None and not dict(kr.object_kernels(path))
        print(f"{f:<24} only in {'this tree' if f in objs else 'the other build'}: " + ("host-only object, no gfx950 code object" if host_only else "HOLDS DEVICE CODE"))
        ok = ok and host_only
    for f in sorted(set(objs) & set(theirs)):
        a, b = dict(kr.object_kernels(os.path.join(mine, f))), dict(kr.object_kernels(os.path.join(other, f)))
        sa, sb = disasm_sha(os.path.join(mine, f)), disasm_sha(os.path.join(other, f))
        if sa is None and sb is None and not a and not b:
            continue                                                                                        # host-only object
        names, meta, code = sorted(a) == sorted(b), a == b, sa == sb
        total += len(a)
        ok = ok and names and meta and code
        print(f"{f:<24} {len(a):7d}  {'equal' if names else 'DIFFER':<6} {'equal' if meta else 'DIFFER':<8}  {sb} {'==' if code else '!='} {sa}")
    print(f"kernels: {total}; names, metadata and device code of every object identical: {ok}\n")
    return ok


if __name__ == "__main__":
    here = os.path.join(kr.ROOT, "difashion_amd", "csrc")
    other = sys.argv[1]
    good = compare(here, other, "bf16 library (the default): this tree against the other build, object by object")
    good = compare(os.path.join(here, "obj_f16"), os.path.join(other, "obj_f16"), "fp16-storage library (-DDFH_F16)") and good
    sys.exit(0 if good else 1)
