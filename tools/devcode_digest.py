"""Digests of the gfx950 device code inside object files: is a build's device code the same as
another's, kernel by kernel?

    python tools/devcode_digest.py BUILD            one JSON line per kernel
    python tools/devcode_digest.py PARENT BRANCH    the kernels added, removed and differing; exit 1 on any

BUILD is an object file or a directory of them (advanced-cpu-raytracing_amd/build).  Of each object
with a .hip_fatbin section the gfx950 code object is taken out (llvm-objcopy --dump-section,
clang-offload-bundler --unbundle) and read with llvm-readelf -S -s: a kernel is a FUNC symbol `k`
with a 64-byte descriptor object `k.kd`.  Per kernel: the object file, the symbol, the body's size
and sha256, and the sha256 of the descriptor with its code-entry offset (bytes 16-23) zeroed -- the
offset moves when the kernels' order inside .text does, which a change of host code alone can cause;
the rest of the descriptor (registers, scratch, LDS, launch bounds' effect) must not.  Whole files,
whole code objects and the __hip_cuid_* symbol differ between two builds of the same source and
are not compared.  Hashes only: no instruction is decoded.
"""
import argparse
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ARCH = "gfx950"


def tool(name):
    for d in (os.path.join(ROCM, "llvm", "bin"), os.path.join(ROCM, "lib", "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    path = shutil.which(name)
    if not path:
        sys.exit("devcode_digest: %s not found under %s or on PATH" % (name, ROCM))
    return path


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """The object's gfx950 code object as bytes; None: the object holds no device code."""
    fatbin, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    for p in (fatbin, co):
        if os.path.exists(p):
            os.remove(p)
    r = subprocess.run([tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fatbin, obj,
                        os.path.join(tmp, "copy.o")], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(fatbin) or os.path.getsize(fatbin) == 0:
        return None
    targets = [t for t in run(tool("clang-offload-bundler"), "--list", "--type=o", "--input=" + fatbin).split()
               if t.endswith(ARCH)]
    if not targets:
        return None
    run(tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + targets[0], "--input=" + fatbin,
        "--output=" + co)
    return co


def kernels(co):
    """{symbol: (size, body sha256, descriptor sha256)} of one code object."""
    data = open(co, "rb").read()
    sections = {}                                    # index -> (address, file offset)
    symbols = {}                                     # name -> (value, size, section index)
    for line in run(tool("llvm-readelf"), "-S", "-s", "--wide", co).splitlines():
        f = line.split()
        if line.lstrip().startswith("[") and "]" in line:
            f = line.split("]", 1)[1].split()        # name type address off size ...
            nr = line.split("]", 1)[0].strip(" [")
            if nr.isdigit() and len(f) >= 5 and f[1] != "NULL":
                sections[int(nr)] = (int(f[2], 16), int(f[3], 16))
        elif len(f) == 8 and f[0].endswith(":") and f[0][:-1].isdigit() and f[6].isdigit():
            symbols[f[7]] = (int(f[1], 16), int(f[2], 0), int(f[6]))

    def content(name):
        value, size, ndx = symbols[name]
        addr, off = sections[ndx]
        return data[off + value - addr: off + value - addr + size]

    out = {}
    for name in symbols:
        if name.startswith("__hip_cuid_") or name.endswith(".kd") or name + ".kd" not in symbols:
            continue
        body, kd = content(name), bytearray(content(name + ".kd"))
        if len(kd) != 64:
            sys.exit("devcode_digest: %s.kd of %d bytes in %s" % (name, len(kd), co))
        kd[16:24] = bytes(8)                         # KERNEL_CODE_ENTRY_BYTE_OFFSET
        out[name] = (len(body), hashlib.sha256(body).hexdigest(), hashlib.sha256(bytes(kd)).hexdigest())
    return out


def digest(path):
    """{(object file, kernel): (size, body, kd)} of an object file or a directory of them."""
    objs = sorted(glob.glob(os.path.join(path, "*.o"))) if os.path.isdir(path) else [path]
    if not objs:
        sys.exit("devcode_digest: no object files in " + path)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in objs:
            co = code_object(obj, tmp)
            if co:
                for k, v in kernels(co).items():
                    out[(os.path.basename(obj), k)] = v
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("build", nargs="+", help="an object file or a build directory; two of them: compare")
    a = ap.parse_args()
    if len(a.build) > 2:
        ap.error("one build to list, two to compare")
    d = [digest(p) for p in a.build]
    if len(d) == 1:
        for (obj, k), (size, body, kd) in sorted(d[0].items()):
            print(json.dumps({"object": obj, "kernel": k, "size": size, "body": body, "kd": kd}))
        return 0
    removed = sorted(set(d[0]) - set(d[1]))
    added = sorted(set(d[1]) - set(d[0]))
    differing = sorted(k for k in set(d[0]) & set(d[1]) if d[0][k] != d[1][k])
    for what, keys in (("removed", removed), ("added", added), ("differing", differing)):
        for obj, k in keys:
            print(json.dumps({"change": what, "object": obj, "kernel": k, "first": d[0].get((obj, k)),
                              "second": d[1].get((obj, k))}))
    print(json.dumps({"kernels": [len(d[0]), len(d[1])], "objects": [len({o for o, _ in x}) for x in d],
                      "removed": len(removed), "added": len(added), "differing": len(differing)}))
    return 1 if removed or added or differing else 0


if __name__ == "__main__":
    sys.exit(main())
