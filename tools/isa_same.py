#!/usr/bin/env python
"""Is a kernel's machine code unchanged by an edit?  Compiles one .hip source of dream_amd/csrc (or, with `all`, every one) at a git
revision and in the working tree for gfx950 and compares the assembly kernel by kernel (comments stripped, basic-block labels
renumbered).  Runs without a GPU.

    python tools/isa_same.py HEAD~1 conv_wino.hip [substring of the mangled kernel names to report]
    python tools/isa_same.py HEAD~1 all
    python tools/isa_same.py --renamed HEAD~1 conv_f16.hip

The revision's source is compiled against the revision's own headers (dream_amd/csrc and include/ extracted into a temporary
directory), the working tree's source in place, both with the flags the product library is built with (__graft_entry__: plain fp32
VALU for most units); nothing is written into the source tree.  With `all`: one summary line per file, plus
every kernel that is not SAME.  Exit status 0 when every kernel of the revision is SAME in the working tree.

--renamed tolerates a rename (a wrapper folded into a template: another mangled name, the same code): a kernel's own symbol is masked
inside its body, and kernels present on one side only are paired one-to-one by body; a pair prints as `SAME (renamed) old -> new` and
counts as SAME, whatever stays unpaired as `only in old` / `only in new`.

Why: kernels written against the edge of the register file (conv_wino_kernel<4,1,0>: 253-255 VGPRs) change their register
allocation when code is merely PRESENT in the translation unit -- round 4 added a BatchNorm-folding variant of the Winograd kernel
in the last hours, with no GPU time left to re-measure the plain kernels; this check showed all 15 of them instruction-identical to
the measured library (the body is included twice, conv_wino_body.inc, instead of being templated on the new feature)."""
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import SCALAR_F32_FLAGS, SCALAR_F32_SOURCES      # noqa: E402  (the product's per-unit flags)
CSRC_REL = os.path.join("dream_amd", "csrc")


def kernels(asm_path, mask_own_symbol=False):
    txt = open(asm_path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*;\s*@\1\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        body = re.sub(r"[ \t]*;.*", "", m.group(2))         # (with the padding in front of it: its width follows the label's digits)
        body = re.sub(r"[ \t]+$", "", body, flags=re.M)
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        body = re.sub(r"\.Ltmp\d+", ".Ltmp", body)
        if mask_own_symbol:
            body = body.replace(m.group(1), "<kernel>")
        out[m.group(1)] = (hashlib.md5(body.encode()).hexdigest()[:12], body.count("\n"))
    return out


def compile_to_asm(root, name, out_dir, mask_own_symbol=False):
    """Kernels of root/dream_amd/csrc/name, compiled against root's headers; every product goes to out_dir."""
    csrc = os.path.join(root, CSRC_REL)
    os.makedirs(out_dir)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-I", os.path.join(csrc, "include"), "-I", csrc,
             "-I", os.path.join(root, "include"), "-Wno-unused-result", "-x", "hip"] + (SCALAR_F32_FLAGS if name in SCALAR_F32_SOURCES else [])
    subprocess.check_call(["/opt/rocm/bin/hipcc"] + flags + ["-c", os.path.join(csrc, name), "-save-temps=obj", "-o", os.path.join(out_dir, "out.o")],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return kernels(os.path.join(out_dir, os.path.splitext(name)[0] + "-hip-amdgcn-amd-amdhsa-gfx950.s"), mask_own_symbol)


def compare(a, b, want="", renamed=False):
    """[(state, kernel)] over the kernels of either side whose name contains `want`, and whether nothing of `a` changed or went.
    renamed: each kernel of one side only is paired with one of the other side only that has the same body, -> "old -> new"."""
    rows = []
    new_only = {}
    for k in sorted(set(b) - set(a)) if renamed else ():
        new_only.setdefault(b[k], []).append(k)
    for k in sorted(set(a) | set(b)):
        if want not in k:
            continue
        if k in a and k in b:
            rows.append(("SAME" if a[k] == b[k] else "DIFFERENT", k))
        elif k in a and new_only.get(a[k]):
            rows.append(("SAME (renamed)", "%s -> %s" % (k, new_only[a[k]].pop(0))))
        elif k in a:
            rows.append(("only in old", k))
    paired = {r[1].split(" -> ")[1] for r in rows if r[0] == "SAME (renamed)"}
    rows += [("only in new", k) for k in sorted(set(b) - set(a) - paired) if want in k]
    return rows, all(s in ("SAME", "SAME (renamed)", "only in new") for s, _ in rows)


def hip_sources(root):
    return sorted(f for f in os.listdir(os.path.join(root, CSRC_REL)) if f.endswith(".hip"))


def main():
    argv = [a for a in sys.argv[1:] if a != "--renamed"]
    renamed = "--renamed" in sys.argv[1:]
    rev, name = argv[0], argv[1]
    want = argv[2] if len(argv) > 2 else ""
    with tempfile.TemporaryDirectory() as tmp:
        old_root = os.path.join(tmp, "old")
        os.makedirs(old_root)
        archive = subprocess.Popen(["git", "-C", ROOT, "archive", rev, "dream_amd/csrc", "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", old_root], stdin=archive.stdout)
        if archive.wait():
            sys.exit("git archive %s failed" % rev)
        names = sorted(set(hip_sources(old_root)) | set(hip_sources(ROOT))) if name == "all" else [name]
        jobs = {}
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            for n in names:
                for tag, root in (("old", old_root), ("new", ROOT)):
                    if os.path.exists(os.path.join(root, CSRC_REL, n)):
                        jobs[n, tag] = pool.submit(compile_to_asm, root, n, os.path.join(tmp, "obj", tag, n), renamed)
        ok = True
        for n in names:
            if (n, "old") not in jobs or (n, "new") not in jobs:
                print("%-20s only in %s" % (n, "old" if (n, "old") in jobs else "new"))
                ok &= (n, "new") in jobs
                continue
            rows, same = compare(jobs[n, "old"].result(), jobs[n, "new"].result(), want, renamed)
            ok &= same
            if name == "all":
                print("%-20s %d kernels, %d SAME%s" % (n, len(rows), sum(s == "SAME" for s, _ in rows),
                                                        ", %d SAME (renamed)" % sum(s == "SAME (renamed)" for s, _ in rows) if renamed else ""))
                rows = [r for r in rows if r[0] != "SAME"]
            for state, k in rows:
                print("%-14s %s" % (state, k) if renamed else "%-11s %s" % (state, k))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
