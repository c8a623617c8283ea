#!/usr/bin/env python3
"""Device-code identity of the working tree against a git revision (default HEAD): for every file of _lib.SOURCES both trees are
compiled with `hipcc --offload-arch=gfx950 -O3 -std=c++17 <EXTRA_FLAGS> --cuda-device-only -S` and the assembly is compared.

A file is `identical` when the two .s files are equal (after the per-translation-unit id `__hip_cuid_<hash of the path>` is
normalised).  Otherwise every kernel of the working tree's file is compared with the revision's kernel of the same symbol: the text
from its symbol to its end label (the file-wide function index inside local labels normalised), and its .amdhsa_kernel block;
kernels only one side has are listed.  Needs no GPU.
usage: scripts/isa_identity.py [rev]      exit status 1 when a kernel that exists on both sides differs
"""
import ast
import concurrent.futures as cf
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = "unet-watermark_amd/csrc"


def lib_lists(text):
    """SOURCES and EXTRA_FLAGS of a _lib.py"""
    ns = {}
    for node in ast.parse(text).body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") in ("SOURCES", "EXTRA_FLAGS"):
            exec(compile(ast.Module([node], []), "_lib.py", "exec"), ns)
    return ns["SOURCES"], ns["EXTRA_FLAGS"]


def compile_s(src: Path, flags, out: Path):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", *flags, "--cuda-device-only", "-S", src.name, "-o", str(out)]
    r = subprocess.run(cmd, cwd=src.parent, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}\n{r.stdout.decode(errors='replace')}")
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", out.read_text())


def kernels(asm):
    """symbol -> (text from the symbol's label to its .Lfunc_end label, its .amdhsa_kernel block)"""
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n.*?^\s*\.end_amdhsa_kernel", asm, re.M | re.S):
        sym = m.group(1)
        body = re.search(r"^" + re.escape(sym) + r":.*?^\.Lfunc_end\d+:", asm, re.M | re.S)
        # (local labels and the loop comments carry the function's INDEX in its file, .LBB<index>_<block>: it moves when a kernel before it goes)
        out[sym] = (re.sub(r"\b(L?BB|Lfunc_end|Lfunc_begin)\d+", r"\1", body.group(0)) if body else None, m.group(0))
    return out


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    new_sources, new_flags = lib_lists((ROOT / "unet-watermark_amd/_lib.py").read_text())
    old_sources, old_flags = lib_lists(subprocess.check_output(["git", "show", f"{rev}:unet-watermark_amd/_lib.py"], cwd=ROOT).decode())
    bad = 0
    with tempfile.TemporaryDirectory() as t:
        t = Path(t)
        subprocess.run(f"git archive {rev} {CSRC} include | tar -x -C {t}", shell=True, check=True, cwd=ROOT)
        (t / "old").mkdir(); (t / "new").mkdir()
        with cf.ThreadPoolExecutor(8) as ex:
            old = {f: ex.submit(compile_s, t / CSRC / f, old_flags.get(f, []), t / "old" / (f + ".s")) for f in old_sources}
            new = {f: ex.submit(compile_s, ROOT / CSRC / f, new_flags.get(f, []), t / "new" / (f + ".s")) for f in new_sources}
        for f in new_sources:
            a = new[f].result()
            if f not in old:
                print(f"{f}: new file, {len(kernels(a))} kernels")
                continue
            b = old[f].result()
            if a == b:
                print(f"{f}: identical ({len(kernels(a))} kernels)")
                continue
            ka, kb = kernels(a), kernels(b)
            same = [s for s in ka if s in kb and ka[s] == kb[s] and ka[s][0] is not None]
            differ = [s for s in ka if s in kb and s not in same]
            print(f"{f}: {len(same)} surviving kernels identical (body and .amdhsa_kernel block), {len(differ)} differ, "
                  f"{len(kb.keys() - ka.keys())} removed, {len(ka.keys() - kb.keys())} added")
            for s in sorted(kb.keys() - ka.keys()):
                print(f"    removed {s}")
            for s in sorted(ka.keys() - kb.keys()):
                print(f"    added   {s}")
            for s in differ:
                print(f"    DIFFERS {s}")
            bad += len(differ)
        for f in old_sources:
            if f not in new_sources:
                print(f"{f}: removed file")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
