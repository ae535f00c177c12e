"""sha1 of every gfx950 code object embedded in a built library (default: moshi_amd/libmoshi_mi.so).

    python scripts/device_code_hash.py [lib.so ...]
    python scripts/device_code_hash.py --kernels [lib.so ...]
    python scripts/device_code_hash.py --kernels --against parent.so lib.so

Used to show that a host-side change (error codes, test hooks) leaves the GPU code that a committed GPU run validated untouched:
profiles/r05_logs/device_code_sha1.txt holds the hashes of the library the round's last GPU suite ran on.

`--kernels`: one sha1 per kernel (the bytes of its function in .text) instead of one per code object - a change that ADDS kernels to
a source file moves that file's code object but must leave every kernel that existed as it was.  `--against`: each kernel is marked
same / DIFFERENT / NEW against that library.  Build both libraries at the same path: kernels in anonymous namespaces carry a hash of
their file's path in their names."""
import hashlib
import re
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = "/opt/rocm/lib/llvm/bin/"


def code_objects(path, with_bytes=False):
    data = Path(path).read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out = []
    for m in re.finditer(magic, data):
        i = m.start()
        p = i + len(magic)
        num = struct.unpack_from("<Q", data, p)[0]
        p += 8
        for _ in range(num):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            p += 24
            triple = data[p:p + tlen].decode()
            p += tlen
            if "gfx950" in triple and size > 0:
                blob = data[i + off:i + off + size]
                out.append((triple, size, blob if with_bytes else hashlib.sha1(blob).hexdigest()))
    return out


def kernel_hashes(path):
    """{mangled kernel name: sha1 of its function's bytes} over every gfx950 code object of the library."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for n, (_, _, blob) in enumerate(code_objects(path, with_bytes=True)):
            co = Path(d) / f"co{n}.o"
            co.write_bytes(blob)
            text = None
            for ln in subprocess.run([LLVM + "llvm-readelf", "-SW", str(co)], capture_output=True, text=True).stdout.splitlines():
                p = ln.replace("[", " ").replace("]", " ").split()
                if len(p) > 5 and p[1] == ".text":
                    text = (int(p[3], 16), int(p[4], 16))          # address, file offset
            if text is None:
                continue
            for ln in subprocess.run([LLVM + "llvm-readelf", "-sW", str(co)], capture_output=True, text=True).stdout.splitlines():
                p = ln.split()
                if len(p) >= 8 and p[3] == "FUNC" and int(p[2]) > 0:
                    off = int(p[1], 16) - text[0] + text[1]
                    out[p[7]] = hashlib.sha1(blob[off:off + int(p[2])]).hexdigest()
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    per_kernel = "--kernels" in args
    against = None
    if "--against" in args:
        against = kernel_hashes(args[args.index("--against") + 1])
        del args[args.index("--against"):args.index("--against") + 2]
    libs = [a for a in args if a != "--kernels"] or [str(Path(__file__).resolve().parent.parent / "moshi_amd" / "libmoshi_mi.so")]
    for lib in libs:
        if not per_kernel:
            for triple, size, h in code_objects(lib):
                print(f"{h}  {size:9d}  {triple}")
            continue
        mine = kernel_hashes(lib)
        names = subprocess.run(["c++filt"], input="\n".join(sorted(mine)), capture_output=True, text=True).stdout.splitlines()
        for k, n in zip(sorted(mine), names):
            mark = "" if against is None else ("NEW        " if k not in against else "same       " if against[k] == mine[k] else "DIFFERENT  ")
            print(f"{mine[k]}  {mark}{re.sub(r'^void ', '', n)}")
        if against is not None:
            gone = [k for k in against if k not in mine]
            print(f"# {len(mine)} kernels: {sum(k in against and against[k] == mine[k] for k in mine)} same, "
                  f"{sum(k in against and against[k] != mine[k] for k in mine)} different, {sum(k not in against for k in mine)} new; "
                  f"{len(gone)} of the other library's kernels are gone", file=sys.stderr)
