"""Sorted list of the GPU kernels compiled into a libcxrk.so (no GPU needed): every kernel descriptor symbol (`*.kd`) of every
gfx code object in the library's offload bundles, demangled.  Two builds launch-compatible in their kernel set print equal lists:
    python scripts/kernel_symbols.py A/libcxrk.so > a.txt; python scripts/kernel_symbols.py B/libcxrk.so > b.txt; diff a.txt b.txt"""
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
READELF = "/opt/rocm/llvm/bin/llvm-readelf"


def code_objects(blob):
    pos = blob.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", blob, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "amdgcn" in triple and size:
                yield blob[pos + off:pos + off + size]
        pos = blob.find(MAGIC, pos + 1)


def main(path):
    names = []
    for obj in code_objects(open(path, "rb").read()):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(obj)
            f.flush()
            out = subprocess.run([READELF, "-sW", f.name], check=True, capture_output=True, text=True).stdout
        names += [ln.split()[-1][:-3] for ln in out.splitlines() if ln.rstrip().endswith(".kd")]
    demangled = subprocess.run(["c++filt"], input="\n".join(names), check=True, capture_output=True, text=True).stdout
    print("\n".join(sorted(demangled.splitlines())))


if __name__ == "__main__":
    main(sys.argv[1])
