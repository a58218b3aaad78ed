"""tools/isa_same.py OLD.s NEW.s [NEW.s ...] -- do two builds hold the same kernels, instruction for instruction?

The inputs are device-side assembly listings of the GEMM sources (the FLAGS of gpt4roi_amd/build.py plus
`--cuda-device-only -S`; add `-DG4R_F16 -include include/g4r_f16_names.h` for the fp16 copy): OLD.s from the tree before a
change that must not alter machine code (moving kernels between files, host-side clean-up), NEW.s... from the tree after
it.  Kernels are keyed by their demangled name without the parameter list; a kernel is "identical" when its text from the
label to .Lfunc_end -- the body and the .amdhsa_kernel descriptor (register counts, LDS, scratch) -- matches after
block-label numbers and comments are dropped.  Prints names and counts only; exit status 1 on any difference.
"""
import re
import subprocess
import sys


def kernels(path):
    text = open(path, errors="replace").read().split("\n")
    bodies, i = {}, 0
    while i < len(text):
        m = re.match(r"(_Z\w+):\s*(;.*)?$", text[i])
        if m:
            j = i + 1
            while j < len(text) and not re.match(r"\.Lfunc_end\d+:", text[j]):
                j += 1
            if any(re.match(r"\s*\.amdhsa_kernel\s", ln) for ln in text[i:j]):      # a device function has no descriptor
                bodies[m.group(1)] = text[i + 1:j]
            i = j
        i += 1
    names = sorted(bodies)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for mangled, name in zip(names, dem):
        key = name.replace("(anonymous namespace)::", "")
        key = key[:key.rindex("(")]
        assert key not in out, key
        lines = (re.sub(r"\.L(BB|tmp)\d+(_\d+)?", ".L", ln.split(";")[0].rstrip()).replace(mangled, "<self>") for ln in bodies[mangled])
        out[key] = [ln for ln in lines if ln.strip()]
    return out


def main(argv):
    old, new = kernels(argv[1]), {}
    for p in argv[2:]:
        k = kernels(p)
        assert not set(k) & set(new), sorted(set(k) & set(new))
        new.update(k)
    for name in sorted(set(old) - set(new)):
        print("only in OLD:", name)
    for name in sorted(set(new) - set(old)):
        print("only in NEW:", name)
    differ = [n for n in sorted(set(old) & set(new)) if old[n] != new[n]]
    for name in differ:
        print("DIFFERS:", name)
    same = len(set(old) & set(new)) - len(differ)
    print(f"{same} / {len(old)} kernels of OLD identical in NEW ({len(new)} kernels in NEW)")
    return 0 if same == len(old) == len(new) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
