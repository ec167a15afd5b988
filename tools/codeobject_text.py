#!/usr/bin/env python3
"""Size and SHA-256 of the .text section of the gfx950 code object in every built object:
    python3 tools/codeobject_text.py [build dir, default ntracer_amd/build] [other build dir]
With two directories (two builds with the same flags, say a commit and its parent) the units are compared and the exit status is
1 if the device code of any differs: how a change that should leave the kernels alone is shown to have done so
(profiles/var_dispatch_codeobjects.txt).  The code object is taken out as tools/kernel_resources.py takes it out."""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def text_of(obj):
    """the bytes of .text of the object's gfx950 code object, or None where the unit has no device code"""
    with tempfile.TemporaryDirectory() as td:
        fat, co, text = (os.path.join(td, f) for f in ("fat.bin", "dev.co", "text.bin"))
        r = subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(td, "copy.o")], capture_output=True)
        if r.returncode or not os.path.exists(fat):
            return None
        r = subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], capture_output=True)
        if r.returncode or not os.path.exists(co) or os.path.getsize(co) == 0:
            return None
        r = subprocess.run([LLVM + "/llvm-objcopy", "-O", "binary", "--only-section=.text", co, text], capture_output=True)
        if r.returncode or not os.path.exists(text):
            return None
        with open(text, "rb") as f:
            return f.read()


def units(build):
    """{unit name without the flag tag: (size, sha256)}"""
    out = {}
    for o in sorted(glob.glob(os.path.join(build, "*.o"))):
        t = text_of(o)
        if t is not None:
            out[re.sub(r"\.[0-9a-f]{8}\.o$", "", os.path.basename(o))] = (len(t), hashlib.sha256(t).hexdigest())
    return out


def _key(name):
    m = re.match(r"(.*?)_(\d+)$", name)
    return (m.group(1), int(m.group(2))) if m else (name, 0)


if __name__ == "__main__":
    dirs = sys.argv[1:3] or [os.path.join(ROOT, "ntracer_amd", "build")]
    tables = [units(d) for d in dirs]
    differ = 0
    for name in sorted(set().union(*tables), key=_key):
        cells = [t.get(name) for t in tables]
        same = len(cells) == 1 or cells[0] == cells[1]
        differ += not same
        print("%-18s %s%s" % (name, "  ".join("%8d %s" % c if c else "%8s %s" % ("-", "-" * 64) for c in cells),
                              "" if len(cells) == 1 else ("  same" if same else "  DIFFERENT")))
    if len(tables) == 2:
        print("%d units, %d with different device code" % (len(set().union(*tables)), differ))
    sys.exit(1 if differ else 0)
