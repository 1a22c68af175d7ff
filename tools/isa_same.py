#!/usr/bin/env python3
"""CPU: is the gfx950 device code of the working tree the same as that of a git revision?

    python tools/isa_same.py [rev] [--per-kernel] [--sub PATTERN REPLACEMENT]...          (default HEAD)

Every jepa_amd/csrc/*.hip of the revision (extracted with `git archive` into a temporary directory) and of the working tree is
compiled device-only to assembly with the flags of jepa_amd/build.py, as tests/test_build_no_spills.py does; lines that contain
`__hip_cuid_` (a hash of the source text) are dropped and the rest is compared per file.  The gate of a refactor of csrc/:
instructions, register counts, LDS sizes, kernel names and kernel-argument sizes must not move.  Exit status 1 on any difference.
A kernel that lost a template parameter has a new mangled name and nothing else: each --sub (a regular expression and its replacement,
re.sub) is applied to the REVISION's assembly before the comparison, and is printed with the number of replacements it made.

--per-kernel is the gate of a refactor that moves kernels between files: the assembly of both trees is cut into one piece per kernel,
keyed by its symbol -- the function from `-- Begin function` to the end of its `Kernel info` comment (instructions, the
`.amdhsa_kernel` descriptor, the resource `.set`s) plus its entry of `amdhsa.kernels` in the metadata -- with the per-file function
index taken out of the local labels (`.LBB3_7` -> `.LBB_7`, `.Lfunc_end3` -> `.Lfunc_end`, in the label comments too).  Every kernel is
listed as same or DIFFERENT with the file it lives in on either side; a kernel on one side only is listed and counts as a difference."""
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


FUNC_INDEX = re.compile(r"(\.L(?:BB|func_begin|func_end|JTI|CPI)|\bBB)\d+")
COUNTED = ((".vgpr_count:", "VGPRs"), (".agpr_count:", "AGPRs"), (".sgpr_count:", "SGPRs"), (".group_segment_fixed_size:", "LDS bytes"),
           (".private_segment_fixed_size:", "scratch bytes"))


def kernels(lines):
    """{symbol: lines of the kernel's function piece + lines of its metadata entry}, function indices normalised."""
    out, name, seen_info = {}, None, False
    for ln in lines:
        m = re.search(r"; -- Begin function (\S+)", ln)
        if m:
            name, seen_info = m.group(1), False
            out[name] = []
        elif name is not None and seen_info and not ln.startswith(";"):
            name = None                                  # the `Kernel info` comment block is over
        if name is not None:
            seen_info |= ".AMDGPU.csdata" in ln
            ln = FUNC_INDEX.sub(r"\1", ln)
            out[name].append(re.sub(r"^(\.L\w+:)\s+;", r"\1 ;", ln))      # the comment column of a label line moves with the index's width
    if "amdhsa.kernels:" in lines:
        k, entries = lines.index("amdhsa.kernels:") + 1, []
        while k < len(lines) and lines[k].startswith(" "):          # the table ends at the next top-level key
            if lines[k].startswith("  - "):
                entries.append([])
            entries[-1].append(lines[k])
            k += 1
        for entry in entries:
            sym = next(m.group(1) for m in (re.match(r"\s+\.name:\s+(\S+)", ln) for ln in entry) if m)
            out.setdefault(sym, []).extend(entry)
    return out


def counts(piece):
    """The resource figures of a kernel piece (from its metadata entry) and its instruction count."""
    res = {}
    for ln in piece:
        for key, label in COUNTED:
            if ln.strip().lstrip("- ").startswith(key):
                res[label] = int(ln.split(":")[1])
    end = next((i for i, ln in enumerate(piece) if ".amdhsa_kernel" in ln or ".section" in ln), len(piece))
    res["instructions"] = sum(1 for ln in piece[:end] if ln.startswith("\t") and not ln.startswith("\t.") and not ln.startswith("\t;"))
    return res


def compare_kernels(names, outs, rev):
    """Per-kernel comparison across files: returns the number of kernels that differ or live on one side only."""
    old, new = {}, {}
    for i, n in enumerate(names):
        for side, lines in ((old, outs[2 * i]), (new, outs[2 * i + 1])):
            for sym, piece in kernels(lines or []).items():
                assert sym not in side, f"{sym} is defined twice"
                side[sym] = (n, piece)
    bad = 0
    for sym in sorted(set(old) | set(new)):
        if sym not in old or sym not in new:
            bad += 1
            print(f"ONLY IN {rev if sym in old else 'THE TREE'}  {sym}  ({(old.get(sym) or new.get(sym))[0]})")
            continue
        (fo, po), (fn, pn) = old[sym], new[sym]
        where = fo if fo == fn else f"{fo} -> {fn}"
        print(f"{'same     ' if po == pn else 'DIFFERENT'}  {sym}  ({where}, {len(pn)} lines)")
        if po != pn:
            bad += 1
            co, cn = counts(po), counts(pn)
            print("    " + ", ".join(f"{k} {co.get(k)} -> {cn.get(k)}" for k in cn))
            print("\n".join(list(difflib.unified_diff(po, pn, "old/" + fo, "new/" + fn, lineterm="", n=1))))      # whole: the diff of a kernel is the evidence a refactor note quotes
    print(f"{len(set(old) | set(new)) - bad} of {len(set(old) | set(new))} kernels emit the same device code as {rev}")
    return bad


def main(rev, subs=(), per_kernel=False):
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
    if per_kernel:
        return 1 if compare_kernels(names, outs, rev) else 0
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
    per_kernel = "--per-kernel" in argv
    argv = [a for a in argv if a != "--per-kernel"]
    sys.exit(main(argv[0] if argv else "HEAD", subs, per_kernel))
