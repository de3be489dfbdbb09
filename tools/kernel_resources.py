#!/usr/bin/env python3
"""Register / scratch / LDS budget of every kernel in the built library, read from the code objects' metadata (no GPU needed).
usage: tools/kernel_resources.py [--digest] [--lib LIB] [--against LIB2] [regex]
columns: vgpr agpr sgpr scratch-bytes static-LDS-bytes max-workgroup [digest] name
--digest        adds a hash of the kernel's disassembly: instruction text, encoding and branch targets relative to the kernel's own
                start - where the kernel lies in the code object does not enter
--against LIB2  compares the selected kernels of LIB (default: the built library) with those of LIB2: resource rows and digests side by
                side, the instruction diff of every kernel that differs; exit status 1 if any differs or is missing on one side"""
import difflib
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin/"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
DEFAULT_LIB = os.path.join(ROOT, "gtsam-vslam_amd", "libvslam_hip.so")


def code_objects(lib, td):
    """the gfx950 code objects of the library's .hip_fatbin section, unbundled into td"""
    fat = os.path.join(td, "fat.bin")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(MAGIC, blob)] + [len(blob)]
    out = []
    for i in range(len(starts) - 1):
        part = os.path.join(td, "b%d.bin" % i); co = os.path.join(td, "b%d.co" % i)
        open(part, "wb").write(blob[starts[i]:starts[i + 1]])
        r = subprocess.run([LLVM + "clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + part, "--output=" + co, "--unbundle"],
                           capture_output=True)
        if r.returncode == 0 and os.path.exists(co):
            out.append(co)
    return out


def demangle(name):
    try:
        return subprocess.run([LLVM + "llvm-cxxfilt", name], capture_output=True, text=True).stdout.strip().split("(")[0]
    except Exception:      # noqa: BLE001
        return name


def kernel_rows(lib=None):
    """[(demangled name, vgpr, agpr, sgpr, scratch bytes, static LDS bytes, max workgroup size)] of every kernel in the library"""
    with tempfile.TemporaryDirectory() as td:
        rows = []
        for co in code_objects(lib or DEFAULT_LIB, td):
            notes = subprocess.run([LLVM + "llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            for blk in notes.split("- .agpr_count:")[1:]:
                def g(k):
                    m = re.search(r"\." + k + r":\s*(\S+)", blk)
                    return m.group(1) if m else "?"
                rows.append((demangle(g("name")), g("vgpr_count"), blk.split()[0], g("sgpr_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size"), g("max_flat_workgroup_size")))
        return sorted(rows)


def kernel_code(lib=None):
    """{demangled name: [normalised instruction lines]} of every kernel: 'text | encoding | <symbol+offset>' without the address"""
    line = re.compile(r"^\s+(.*?)\s*// [0-9A-F]+: ([0-9A-F ]+?)\s*(<.*>)?$")
    with tempfile.TemporaryDirectory() as td:
        code = {}
        for co in code_objects(lib or DEFAULT_LIB, td):
            notes = subprocess.run([LLVM + "llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            kernels = set(re.findall(r"\.name:\s*(\S+)", notes))
            cur = None
            for ln in subprocess.run([LLVM + "llvm-objdump", "-d", co], capture_output=True, text=True).stdout.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
                if m:
                    cur = code.setdefault(demangle(m.group(1)), []) if m.group(1) in kernels else None
                    continue
                m = line.match(ln) if cur is not None else None
                if m:
                    cur.append("%s | %s | %s" % (m.group(1), m.group(2), m.group(3) or ""))
        return code


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def main():
    args = sys.argv[1:]
    want_digest = "--digest" in args
    opt = {}
    for k in ("--lib", "--against"):
        if k in args:
            opt[k] = args[args.index(k) + 1]
            del args[args.index(k):args.index(k) + 2]
    args = [a for a in args if a != "--digest"]
    pat = re.compile(args[0]) if args else None
    lib = opt.get("--lib")
    rows = [r for r in kernel_rows(lib) if pat is None or pat.search(r[0])]
    if "--against" not in opt:
        code = kernel_code(lib) if want_digest else {}
        print("%5s %5s %5s %8s %8s %6s  %s%s" % ("vgpr", "agpr", "sgpr", "scratch", "lds", "wg", "digest            " if want_digest else "", "kernel"))
        for name, v, a, s, p, l, w in rows:
            print("%5s %5s %5s %8s %8s %6s  %s%s" % (v, a, s, p, l, w, digest(code.get(name, [])) + "  " if want_digest else "", name))
        return 0
    other = {r[0]: r[1:] for r in kernel_rows(opt["--against"]) if pat is None or pat.search(r[0])}
    code, code2 = kernel_code(lib), kernel_code(opt["--against"])
    print("%5s %5s %5s %8s %8s %6s  %-16s  %-9s %-16s  %s" % ("vgpr", "agpr", "sgpr", "scratch", "lds", "wg", "digest", "resources", "digest there", "kernel"))
    differ = []
    for r in rows:
        name = r[0]
        d1, d2 = digest(code.get(name, [])), digest(code2[name]) if name in code2 else "missing"
        same_rows = other.get(name) == r[1:]
        print("%5s %5s %5s %8s %8s %6s  %-16s  %-9s %-16s  %s" % (r[1:] + (d1, "same" if same_rows else "DIFFER", "same" if d1 == d2 else d2, name)))
        if not same_rows or d1 != d2:
            differ.append(name)
    missing = sorted(set(other) - {r[0] for r in rows})
    for name in differ:
        print("\n--- %s: instruction diff" % name)
        for ln in difflib.unified_diff(code2.get(name, []), code.get(name, []), "there", "here", lineterm="", n=1):
            print(ln)
    print("\n%d kernels compared, %d differ, %d only in the other library%s" % (len(rows), len(differ), len(missing), (": " + ", ".join(missing)) if missing else ""))
    return 1 if differ or missing else 0


if __name__ == "__main__":
    sys.exit(main())
