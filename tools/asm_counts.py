#!/usr/bin/env python3
"""Static instruction counts per kernel of a gfx950 assembly file (hipcc -S --cuda-device-only):

    python tools/asm_counts.py <file.s> [--against <parent.s>] [name filter ...]

Whole kernel text, every instruction counted once however often it runs: VALU (v_* without the MFMAs), SALU (s_*),
LDS (ds_*), VMEM (global_* / buffer_* / flat_* / scratch_*), MFMA; and the VGPR / AGPR / scratch / occupancy figures the
compiler prints after each kernel.  --against prints "parent new" in every column.  Names are demangled with llvm-cxxfilt
where it is on the PATH; template arguments are spelled out where it does not know a type code."""
import re
import shutil
import subprocess
import sys


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or "llvm-cxxfilt"
    try:
        out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    if name.startswith("_Z"):          # the demangler does not know the bf16 type code: keep the name, spell the template arguments
        m = re.match(r"_ZN\d+_GLOBAL__N_1\d+([A-Za-z_0-9]+?)I((?:L[ib]\d+E)+)E", name)
        if m:
            args = [("true" if a[2:-1] == "1" else "false") if a[1] == "b" else a[2:-1] for a in re.findall(r"L[ib]\d+E", m.group(2))]
            return m.group(1) + "<" + ", ".join(args) + ">"
        m = re.match(r"_ZN\d+_GLOBAL__N_1\d+([A-Za-z_0-9]+?)E", name)
        return m.group(1) if m else name
    name = re.sub(r"^void \(anonymous namespace\)::", "", name)
    return re.sub(r"\(.*$", "", name)


def parse(path):
    kernels, cur, order = {}, None, []
    res = re.compile(r";\s*(NumVgprs|NumAgprs|NumSgprs|ScratchSize|LDSByteSize|Occupancy):\s*(\d+)")
    for line in open(path):
        s = line.strip()
        m = re.match(r"^([A-Za-z_][\w$.]*):", s)
        if m and not s.startswith(".L"):
            cur = m.group(1)
            kernels[cur] = dict(VALU=0, SALU=0, LDS=0, VMEM=0, MFMA=0)
            order.append(cur)
            continue
        if cur is None:
            continue
        m = res.search(s)
        if m:
            kernels[cur][m.group(1)] = int(m.group(2))
            continue
        if not s or s[0] in ".;" or s.startswith(".L"):
            continue
        op = s.split()[0]
        k = kernels[cur]
        if op.startswith("v_mfma") or op.startswith("v_smfma"):
            k["MFMA"] += 1
        elif op.startswith("v_"):
            k["VALU"] += 1
        elif op.startswith("s_"):
            k["SALU"] += 1
        elif op.startswith("ds_"):
            k["LDS"] += 1
        elif op.split("_")[0] in ("global", "buffer", "flat", "scratch"):
            k["VMEM"] += 1
    return [(n, kernels[n]) for n in order if "NumVgprs" in kernels[n]]


COLS = (("VALU", "VALU"), ("SALU", "SALU"), ("LDS", "LDS"), ("VMEM", "VMEM"), ("MFMA", "MFMA"), ("VGPR", "NumVgprs"), ("AGPR", "NumAgprs"),
        ("scr", "ScratchSize"), ("occ", "Occupancy"))


def main():
    args = sys.argv[1:]
    old = None
    if "--against" in args:
        i = args.index("--against")
        old = dict(parse(args[i + 1]))
        del args[i:i + 2]
    rows = parse(args[0])
    names = demangle([n for n, _ in rows])
    flt = args[1:]
    wd = 11 if old is not None else 5
    print(f"{'kernel':58s}" + "".join(f"{c:>{wd}s}" for c, _ in COLS))
    for n, k in rows:
        d = short(names[n])
        if flt and not any(f in d for f in flt):
            continue
        cells = [f"{old[n].get(key, 0)} {k.get(key, 0)}" if old is not None and n in old else str(k.get(key, 0)) for _, key in COLS]
        print(f"{d[:58]:58s}" + "".join(f"{c:>{wd}s}" for c in cells))


if __name__ == "__main__":
    sys.exit(main())
