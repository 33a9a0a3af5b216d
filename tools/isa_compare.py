"""Compare the instruction streams of kernels in two builds of libbdd_mma_hip.so (addresses and encodings stripped).
A kernel of OLD is matched in NEW by its exact demangled name, or else by that name with one template argument `false` appended to its
argument list (a kernel template that gained a defaulted flag: the instantiation with the flag at its default).  A name that occurs in
several device code objects of a library (a template instantiated in more than one translation unit) must have the same instructions in
each, or the same sequence of differing copies in both libraries; otherwise it is reported as AMBIGUOUS.
python tools/isa_compare.py OLD.so NEW.so [name-substring ...]   (default: k_fwd_narrow3 k_bwd_narrow3)
Prints one line per kernel (identical / DIFFERENT / MISSING / AMBIGUOUS, instruction counts; NEW-ONLY for a kernel OLD has no match for)
and exits 1 unless all are identical."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_lint import OBJDUMP  # noqa: E402

FUNC = re.compile(r"^[0-9a-f]+ <(.+)>:$")


def kernels(lib):
    """demangled function name -> [its instructions in each device code object of the library that has it]"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.run([OBJDUMP, "--offloading", "lib.so"], check=True, capture_output=True, cwd=tmp)
        for f in sorted(f for f in os.listdir(tmp) if "amdgcn" in f):
            text = subprocess.run([OBJDUMP, "-d", "-C", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
            cur = None
            for ln in text.splitlines():
                m = FUNC.match(ln.strip())
                if m:
                    cur = []
                    out.setdefault(m.group(1), []).append(cur)
                    continue
                if cur is None or not ln.startswith("\t"):
                    continue
                ins = ln.split("//")[0].strip()
                if ins and ins != "...":  # "...": objdump's mark for the zero padding between two functions, not an instruction
                    cur.append(ins)
    return out


def with_default_flag(name):
    """the same kernel with `false` appended to its template argument list (the list closes right before the parameter list)"""
    i = name.find(">(")
    return None if i < 0 else name[:i] + ", false" + name[i:]


def unique(copies):
    """the instructions when every copy agrees, else None"""
    return copies[0] if all(c == copies[0] for c in copies) else None


def main():
    old, new = sys.argv[1], sys.argv[2]
    pats = sys.argv[3:] or ["k_fwd_narrow3", "k_bwd_narrow3"]
    ko, kn = kernels(old), kernels(new)
    bad = 0
    matched = set()
    for d in sorted(ko):
        if not any(p in d for p in pats):
            continue
        n = d if d in kn else with_default_flag(d)
        if n not in kn:
            print(f"MISSING    {d}")
            bad += 1
            continue
        matched.add(n)
        a, b = unique(ko[d]), unique(kn[n])
        if (a is None or b is None) and ko[d] == kn[n]:  # the copies differ from each other, but both libraries have the same ones
            print(f"identical  {len(ko[d])} differing copies, the same in both  {d}")
            continue
        if a is None or b is None:
            print(f"AMBIGUOUS  {d}: copies in several code objects differ")
            bad += 1
            continue
        same = a == b
        bad += not same
        print(f"{'identical' if same else 'DIFFERENT'}  {len(a):6d} / {len(b):6d} instructions  {d}  ->  {n}")
    for n in sorted(kn):
        if n not in matched and any(p in n for p in pats):
            print(f"NEW-ONLY   {n}")
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
