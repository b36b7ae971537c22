"""Compare the gfx950 device code of two source trees, kernel by kernel (no GPU needed).

    python tools/device_code_diff.py <tree_a> <tree_b> [--jobs N]

Every file of build.py's SOURCES and DIAG_ONLY_SOURCES is compiled to device-only assembly (build.py's FLAGS plus
--offload-device-only -S), once plain and once with -DDGVIT_DIAG, in both trees.  A diagnostic-only file that does not compile plain in
EITHER tree (diag_api.hip stops at its own #error without -DDGVIT_DIAG) is reported and left out of the plain pass.

Per translation unit the assembly is cut into kernels (the text between a kernel's label and its descriptor, and the .amdhsa_kernel
descriptor block) and the two trees are compared as plain text: the set of kernel symbols must be the same and every kernel's
instruction stream and descriptor must be identical; only the order of kernels inside a file may differ.  The instructions themselves
are not interpreted.  The file list, the flags and the sources come from tree_a's and tree_b's own build.py respectively.

Prints one line per difference and ends with "N kernels, M differ"; exit status 1 when M > 0 or the symbol sets differ.
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = "dgvit-depth-goal-guided-vision-transformer-_amd"


def _build_module(tree):
    spec = importlib.util.spec_from_file_location("dgvit_build_" + str(abs(hash(tree))), os.path.join(tree, PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _jobs(mod):
    return [(s, d) for d in (False, True) for s in mod.SOURCES + mod.DIAG_ONLY_SOURCES]


def _assembly(mod, job):
    """the device assembly, or None where a diagnostic-only file does not compile without -DDGVIT_DIAG"""
    src, diag = job
    flags = [f for f in mod.FLAGS if not f.startswith("-Rpass")]
    r = subprocess.run(["hipcc", *flags, *(["-DDGVIT_DIAG"] if diag else []), "--offload-device-only", "-S", os.path.join(mod.CSRC, src), "-o", "-"],
                       capture_output=True, text=True)
    if r.returncode != 0:
        if not diag and src in mod.DIAG_ONLY_SOURCES:
            return None
        sys.stderr.write(r.stderr)
        raise RuntimeError(f"hipcc failed on {src}{' [diag]' if diag else ''} in {mod.HERE}")
    return r.stdout


_DESC = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)\s*$")


def kernels(asm):
    """{kernel symbol: (instruction stream, descriptor block)} of one device-only assembly file: the stream runs from the kernel's label
    to its descriptor, which the assembly places behind the last instruction"""
    lines = asm.split("\n")
    label = {l.split(":", 1)[0]: i for i, l in enumerate(lines) if l[:1] not in ("", "\t", " ", ";", ".") and ":" in l}
    out, i = {}, 0
    while i < len(lines):
        m = _DESC.match(lines[i])
        if m:
            j = i
            while ".end_amdhsa_kernel" not in lines[j]:
                j += 1
            out[m.group(1)] = ("\n".join(lines[label[m.group(1)]:i]), "\n".join(lines[i:j + 1]))
            i = j
        i += 1
    return out


def _neutral(text):
    # local labels carry the function's ordinal in the file (.LBB12_3, .Lfunc_end12): it moves with the order of instantiation
    return re.sub(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+", r".L\1", text)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    mods = [_build_module(os.path.abspath(t)) for t in (args.tree_a, args.tree_b)]
    jobs = [_jobs(m) for m in mods]
    bad = 0
    if jobs[0] != jobs[1]:
        print(f"the trees list different sources: {sorted(set(jobs[0]) ^ set(jobs[1]))}")
        bad += 1
    common = [j for j in jobs[0] if j in jobs[1]]
    with ThreadPoolExecutor(max_workers=args.jobs) as ex:
        asm = [list(ex.map(lambda j, m=m: _assembly(m, j), common)) for m in mods]
    total = differ = 0
    for job, a, b in zip(common, asm[0], asm[1]):
        what = job[0] + (" [diag]" if job[1] else "")
        if a is None or b is None:
            if a is None and b is None:
                print(f"{what}: does not compile without -DDGVIT_DIAG in either tree, left out")
            else:
                print(f"{what}: compiles without -DDGVIT_DIAG in only one of the trees")
                bad += 1
            continue
        ka, kb = kernels(a), kernels(b)
        for name in sorted(set(ka) ^ set(kb)):
            print(f"{what}: kernel {name} only in {args.tree_a if name in ka else args.tree_b}")
            bad += 1
        for name in sorted(set(ka) & set(kb)):
            total += 1
            same_code = _neutral(ka[name][0]) == _neutral(kb[name][0])
            same_desc = ka[name][1] == kb[name][1]
            if not (same_code and same_desc):
                differ += 1
                print(f"{what}: {name}: {'instructions' if not same_code else ''}{' and ' if not (same_code or same_desc) else ''}"
                      f"{'descriptor' if not same_desc else ''} differ")
    print(f"{total} kernels, {differ} differ")
    return 1 if (differ or bad) else 0


if __name__ == "__main__":
    sys.exit(main())
