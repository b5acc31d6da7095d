"""sha256 of every kernel's gfx950 instruction stream in hipcc -S output (make -C ray-tracing-ultrasound_amd/csrc asm), local labels
normalised: two builds whose listings give the same digests run the same instructions.  Usage:
    python scripts/asm_body_digest.py DIR_A DIR_B      # compares the .s files of two directories function by function
    python scripts/asm_body_digest.py DIR              # prints the digests"""
import glob
import hashlib
import os
import re
import sys

LABEL = re.compile(r"\.L(BB|tmp|func_end)\w*")


def digests(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w.$]*):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = hashlib.sha256("".join(body).encode()).hexdigest()
            name = None
            continue
        s = line.split(";")[0].rstrip()
        if s.strip():
            body.append(LABEL.sub(".L", s) + "\n")
    return out


def tree(d):
    return {f"{os.path.basename(p)}:{k}": v for p in sorted(glob.glob(os.path.join(d, "*.s"))) for k, v in digests(p).items()}


if __name__ == "__main__":
    a = tree(sys.argv[1])
    if len(sys.argv) == 2:
        for k, v in a.items():
            print(v, k)
        sys.exit(0)
    b = tree(sys.argv[2])
    same = [k for k in a if k in b and a[k] == b[k]]
    diff = [k for k in a if k in b and a[k] != b[k]]
    print(f"{len(a)} functions in {sys.argv[1]}, {len(b)} in {sys.argv[2]}: {len(same)} identical, {len(diff)} differ, "
          f"{len(set(a) - set(b))} only in the first, {len(set(b) - set(a))} only in the second")
    for k in diff:
        print("DIFFERS", k)
    sys.exit(1 if diff or set(a) - set(b) else 0)
