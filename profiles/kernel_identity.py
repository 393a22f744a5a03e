"""Per-kernel comparison of the gfx950 device code of two source trees (no GPU needed): the check a refactor that must not change
a kernel is held to.

    python profiles/kernel_identity.py <csrc of the old tree> <csrc of the new tree>

Every .hip file of the Makefile's SRCS is compiled with the Makefile's flags plus `--cuda-device-only -S`.  Per kernel symbol the
instruction text (comments and directives removed, the function index inside local branch labels removed) and every .amdhsa_
value of its kernel descriptor (VGPRs, SGPRs, LDS, scratch, ...) are compared.  A kernel whose text differs while its descriptor
values and its sequence of mnemonics (and labels) are equal, line for line, is reported as "same opcodes, registers renamed" and
counted on its own: the compiler numbered registers or ordered the operands of a commutative instruction differently.  Exit status 0:
same symbols and nothing worse than that."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -fvisibility=hidden -Wall -Wno-unused-function -DGLP_LDE_NO_HOIST".split()
SRCS = "api.hip ntt.hip merkle.hip prover.hip verifier.hip witness.hip circuit_file.hip".split()
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def kernels(csrc, src, tmp):
    """{symbol: (instruction lines, {amdhsa key: value})} of one translation unit"""
    out = os.path.join(tmp, src + ".s")
    subprocess.check_call([HIPCC] + FLAGS + ["--cuda-device-only", "-S", src, "-o", out], cwd=csrc)
    text, meta, func, desc, body = {}, {}, None, None, []      # the kernel descriptor block sits inside its function's text
    for line in open(out):
        s = line.split(";")[0].strip()
        m = re.match(r"\.amdhsa_kernel (\S+)", s)
        if m:
            desc = meta.setdefault(m.group(1), {})
        elif s == ".end_amdhsa_kernel":
            desc = None
        elif desc is not None:
            k, _, v = s.partition(" ")
            desc[k] = v.strip()
        elif re.match(r"\.Lfunc_end\d+:", s):
            text[func], func = body, None
        elif func is None and re.match(r"[A-Za-z_][\w$.]*:$", s):
            func, body = s[:-1], []
        elif func is not None and s and (not s.startswith(".") or s.startswith(".LBB")):
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return {k: (text[k], meta[k]) for k in meta}


def tree(csrc, tmp):
    os.makedirs(tmp)
    with ThreadPoolExecutor(len(SRCS)) as ex:
        parts = list(ex.map(lambda s: kernels(csrc, s, tmp), SRCS))
    return {(s, k): v for s, p in zip(SRCS, parts) for k, v in p.items()}


def main(old_dir, new_dir):
    with tempfile.TemporaryDirectory() as tmp:
        with ThreadPoolExecutor(2) as ex:
            fo, fn = ex.submit(tree, old_dir, os.path.join(tmp, "old")), ex.submit(tree, new_dir, os.path.join(tmp, "new"))
            old, new = fo.result(), fn.result()
    bad = 0
    for k in sorted(set(old) ^ set(new)):
        bad += 1
        print("only in the %s tree: %s %s" % ("old" if k in old else "new", k[0], k[1]))
    both = sorted(set(old) & set(new))
    ninstr = renamed = 0
    for k in both:
        (to, mo), (tn, mn) = old[k], new[k]
        ninstr += len(to)
        if to == tn and mo == mn:
            continue
        if mo == mn and [x.split()[0] for x in to] == [x.split()[0] for x in tn]:
            renamed += 1
            print("same opcodes, registers renamed: %s %s: %d instructions, %d lines differ" % (k[0], k[1], len(to), sum(a != b for a, b in zip(to, tn))))
        else:
            bad += 1
            keys = [x for x in sorted(set(mo) | set(mn)) if mo.get(x) != mn.get(x)]
            print("differs: %s %s: %d -> %d instructions%s" % (k[0], k[1], len(to), len(tn), "".join(", %s %s -> %s" % (x, mo.get(x), mn.get(x)) for x in keys)))
    print("%d kernel symbols in the old tree, %d in the new, %d in both; %d instructions compared; %d same opcodes, registers renamed; %d differences"
          % (len(old), len(new), len(both), ninstr, renamed, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
