#!/usr/bin/env python3
"""Is the gfx950 device code of two builds of the library the same?  Runs without a GPU.

    python tools/compare_code_objects.py <object dir A> <object dir B> [--json out.json]

For every object file of A there must be one of the same name in B; the gfx950 code object is taken out of each, and the
disassembly (without the line that names the file and without absolute addresses) and the notes (kernel metadata: names,
registers, LDS, arguments) are compared by digest.  Prints one line per object that differs; exit status 1 if any does.
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
ADDRESS = re.compile(r"^[0-9a-f]{16} (?=<)|(?<=// )[0-9A-F]{12}(?=:)")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name)] + list(args), check=True, capture_output=True, text=True).stdout


def digests(obj, tmp):
    fatbin, co = os.path.join(tmp, "x.fatbin"), os.path.join(tmp, "x.co")
    tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fatbin, obj)
    tool("clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fatbin, "--targets=" + TARGET, "--output=" + co)
    # without the absolute addresses: a code object carries one symbol named after a hash of its source text, whose printed length
    # varies, and a byte more or less in the string table moves .text as a whole (branch targets print as <kernel+offset>)
    code = "\n".join(ADDRESS.sub("", l) for l in tool("llvm-objdump", "-d", co).splitlines() if "file format" not in l)
    notes = "\n".join(l for l in tool("llvm-readelf", "--notes", co).splitlines() if not l.startswith("File:"))
    return hashlib.sha256(code.encode()).hexdigest(), hashlib.sha256(notes.encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--json")
    a = ap.parse_args()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(f for f in os.listdir(a.dir_a) if f.endswith(".o")):
            other = os.path.join(a.dir_b, name)
            row = {"object": name, "equal": False}
            if os.path.exists(other):
                row["code_a"], row["notes_a"] = digests(os.path.join(a.dir_a, name), tmp)
                row["code_b"], row["notes_b"] = digests(other, tmp)
                row["equal"] = row["code_a"] == row["code_b"] and row["notes_a"] == row["notes_b"]
            if not row["equal"]:
                print("DIFFERS" if os.path.exists(other) else "MISSING", name)
            rows.append(row)
    print("%d objects, %d equal" % (len(rows), sum(r["equal"] for r in rows)))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"objects": rows}, fh, indent=1)
    return 0 if rows and all(r["equal"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
