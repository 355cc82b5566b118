#!/usr/bin/env python3
"""One line per gfx950 device function of a build, so that two builds `diff`: mangled name, size, SHA-256 of its bytes
in .text and, for kernels, the resource fields of the code-object notes.  CPU only.

    make -C fem-fct-pdeco_amd/csrc OBJDIR=/tmp/fp OUT=/tmp/fp/libfemfct.so EXTRA=-save-temps=obj
    python3 tools/kernel_fingerprint.py /tmp/fp [--build-id ID] > listing.txt

The arguments are object directories (every *-hip-amdgcn-amd-amdhsa-gfx950.out in them) or code objects.  The first
line names the build: --build-id, else the FEMFCT_BUILD_ID of a build_id.h found next to the code objects (EXTRA is
part of that hash: pass the product build's id to label a listing made with -save-temps)."""
import argparse
import glob
import hashlib
import os
import re
import subprocess

READELF = os.environ.get("LLVM_READELF", "/opt/rocm/lib/llvm/bin/llvm-readelf")
FIELDS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
          ".group_segment_fixed_size")


def readelf(*args):
    return subprocess.run([READELF, "--wide", *args], check=True, capture_output=True, text=True).stdout


def kernel_notes(path):
    """{kernel name: {field: value}} from the amdhsa.kernels list of the metadata note"""
    out, cur = {}, None
    for line in readelf("--notes", path).splitlines():
        if line.startswith("  - "):            # next entry of a top-level list
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"    (\.\w+): +(\S+)$", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2).strip("'\"")
            if m.group(1) == ".name":
                out[cur[".name"]] = cur
    return out


def fingerprints(path):
    text = None
    for line in readelf("-S", path).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\] \.text\s+PROGBITS\s+([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+)", line)
        if m:
            text = (m.group(1), int(m.group(2), 16), int(m.group(3), 16), int(m.group(4), 16))
    if text is None:
        raise SystemExit(f"{path}: no .text section")
    ndx, addr, off, size = text
    with open(path, "rb") as f:
        f.seek(off)
        code = f.read(size)
    notes = kernel_notes(path)
    symtab = readelf("--symbols", path).split("Symbol table '.symtab'")[-1]
    for line in symtab.splitlines():
        col = line.split()
        if len(col) == 8 and col[3] == "FUNC" and col[6] == ndx:
            lo, n, name = int(col[1], 16) - addr, int(col[2]), col[7]
            if lo < 0 or lo + n > size:
                raise SystemExit(f"{path}: {name} lies outside .text")
            res = "".join(f" {k}={notes[name].get(k, '?')}" for k in FIELDS) if name in notes else ""
            yield f"{name} {n} {hashlib.sha256(code[lo:lo + n]).hexdigest()}{res}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("paths", nargs="+", help="object directories or gfx950 code objects")
    ap.add_argument("--build-id")
    a = ap.parse_args()
    files, build_id = [], a.build_id
    for p in a.paths:
        files += sorted(glob.glob(os.path.join(p, "*-hip-amdgcn-amd-amdhsa-gfx950.out"))) if os.path.isdir(p) else [p]
        hdr = os.path.join(p if os.path.isdir(p) else os.path.dirname(p), "build_id.h")
        if build_id is None and os.path.exists(hdr):
            build_id = re.search(r'"(.*)"', open(hdr).read()).group(1)
    if not files:
        raise SystemExit("no gfx950 code objects found (build with EXTRA=-save-temps=obj)")
    lines = sorted(l for f in files for l in fingerprints(f))
    print(f"# build {build_id or 'unknown'}: {len(lines)} device functions; name size sha256(.text bytes) [kernel resources]")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
