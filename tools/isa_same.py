#!/usr/bin/env python3
"""CPU: is the gfx950 device code of the working tree the same as that of a git revision?

    python tools/isa_same.py [rev] [--sub PATTERN REPLACEMENT]...          (default HEAD)

Every jepa_amd/csrc/*.hip of the revision (extracted with `git archive` into a temporary directory) and of the working tree is
compiled device-only to assembly with the flags of jepa_amd/build.py, as tests/test_build_no_spills.py does; lines that contain
`__hip_cuid_` (a hash of the source text) are dropped and the rest is compared per file.  The gate of a refactor of csrc/:
instructions, register counts, LDS sizes, kernel names and kernel-argument sizes must not move.  Exit status 1 on any difference.
A kernel that lost a template parameter has a new mangled name and nothing else: each --sub (a regular expression and its replacement,
re.sub) is applied to the REVISION's assembly before the comparison, and is printed with the number of replacements it made."""
import concurrent.futures
import difflib
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from jepa_amd import build as vb  # noqa: E402

REL = os.path.relpath(vb.CSRC, ROOT)


def asm(src):
    cmd = [vb._hipcc()] + vb.CXXFLAGS + vb.EXTRA_FLAGS.get(os.path.basename(src), []) + ["-x", "hip", "--cuda-device-only", "-S", src, "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return [ln for ln in r.stdout.splitlines() if "__hip_cuid_" not in ln]


def main(rev, subs=()):
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, REL, "include"], capture_output=True, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
        old_dir = os.path.join(tmp, REL)
        names = sorted(f for f in set(os.listdir(old_dir)) | set(os.listdir(vb.CSRC)) if f.endswith(".hip"))
        jobs = [os.path.join(d, n) for n in names for d in (old_dir, vb.CSRC)]
        with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
            outs = list(ex.map(lambda p: asm(p) if os.path.exists(p) else None, jobs))
    bad = 0
    for pat, repl in subs:
        hits = 0
        for old in outs[0::2]:
            for k, ln in enumerate(old or ()):
                old[k], c = re.subn(pat, repl, ln)
                hits += c
        print(f"--sub {pat} -> {repl}: {hits} replacements in the assembly of {rev}")
    for i, n in enumerate(names):
        old, new = outs[2 * i], outs[2 * i + 1]
        same = old == new
        bad += not same
        print(f"{n:16s} {'same' if same else 'DIFFERENT'}  ({0 if new is None else len(new)} lines)")
        if not same and old is not None and new is not None:
            print("\n".join(list(difflib.unified_diff(old, new, "old/" + n, "new/" + n, lineterm="", n=1))[:60]))
    print(f"{len(names) - bad} of {len(names)} files emit the same device code as {rev}")
    return 1 if bad else 0


if __name__ == "__main__":
    argv, subs = sys.argv[1:], []
    while "--sub" in argv:
        k = argv.index("--sub")
        subs.append((argv[k + 1], argv[k + 2]))
        del argv[k:k + 3]
    sys.exit(main(argv[0] if argv else "HEAD", subs))
