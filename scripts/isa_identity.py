#!/usr/bin/env python3
"""Is the gfx950 device assembly of two source trees the same text?  (the identity rule of a refactor)
    python scripts/isa_identity.py <tree A> [<tree B, default: this repository>] [extra -D flags]
Compiles walker_hip.hip and es_hip.hip of each tree with build.py's compiler and flags (device only, -S), replaces the
__hip_cuid_<hash> symbol (a hash of the input) by a fixed token, and prints each file's sha256 and line count and
`identical` or the first differing lines.  It hashes and diffs text; it does not look at the instructions.
(A -DWG_STAMPS build has two device globals that hipcc emits in either order from run to run: a difference at those two
.bss objects alone is that; run it again.  profiles/r12_isa_identity.txt has the case.)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from walker_gym_amd import build  # noqa: E402

trees = [os.path.abspath(a) for a in sys.argv[1:] if not a.startswith("-")]
extra = [a for a in sys.argv[1:] if a.startswith("-")]
if not 1 <= len(trees) <= 2:
    sys.exit(__doc__)
trees = (trees + [ROOT])[:2]
flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")] + ["--offload-device-only", "-S", *extra]
same = True
with tempfile.TemporaryDirectory() as tmp:
    for unit in ("walker_hip.hip", "es_hip.hip"):
        texts = []
        for i, tree in enumerate(trees):
            out = os.path.join(tmp, f"{i}_{unit}.s")
            subprocess.run([build.hipcc(), f"--offload-arch={build.ARCH}", *flags, "-I", os.path.join(tree, "include"),
                            "-o", out, os.path.join(tree, "walker_gym_amd", "csrc", unit)], check=True)
            with open(out) as f:
                text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", f.read())
            texts.append(text.splitlines())
            print(f"{unit} {'AB'[i]} sha256 {hashlib.sha256(text.encode()).hexdigest()} lines {len(texts[-1])}")
        if texts[0] == texts[1]:
            print(f"{unit}: identical")
            continue
        same = False
        n = next((k for k, (x, y) in enumerate(zip(*texts)) if x != y), min(map(len, texts)))
        print(f"{unit}: DIFFERENT from line {n + 1}")
        for k in range(n, min(n + 5, max(map(len, texts)))):
            for i in (0, 1):
                print(f"  {'AB'[i]} {k + 1}: {texts[i][k] if k < len(texts[i]) else '<end of file>'}")
sys.exit(0 if same else 1)
