#!/usr/bin/env python3
"""Are the kernels of a HIP source the same machine code as at an earlier revision?  (the check behind a pure refactor)

Exports csrc/ and include/ of <rev> with `git archive`, compiles each named source from both trees to device assembly with the
library's own recipe (lcv_hip/build.py: HIPCC, FLAGS, EXTRA, plus --cuda-device-only -S), normalises both listings and compares
them kernel by kernel: instructions, labels, the .amdhsa_* descriptor (register counts, LDS, kernarg size) and the code-object
metadata.  Normalising means: comments, blank lines, `.file` / `.ident` go; a mangled symbol becomes its function name plus
template arguments (the parameter types - a renamed struct - drop out); basic-block labels lose their function index.

Where a kernel differs, the report also says whether its arithmetic does: "same fp ops" when the multiset of its floating-point
VALU mnemonics (v_*_f32, v_pk_*_f32, the v_rcp* and v_div* families; encoding suffixes dropped, v_fmac counted as v_fma) is
unchanged, "fp ops differ" with the mnemonics gained and lost otherwise; and whether .amdhsa_next_free_vgpr and the LDS size
(.amdhsa_group_segment_fixed_size) are unchanged.  The exit code does not depend on it.

A kernel that was renamed or moved to another file is compared with --map: the old kernel's listing, with its name replaced
by the new one, against the new kernel's.  Kernel names are the normalised ones, as the report prints them.

Usage: python tools/isa_equal.py <rev> [--map old.hip:old_kernel=new.hip:new_kernel ...] [file.hip ...]
       (default without --map: csrc/attn_*.hip; exit code 1 on any difference)
"""
import re
import subprocess
import sys
import tempfile
from collections import Counter
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import Dict, List, Optional

ROOT = Path(__file__).resolve().parents[1]
PKG = "longcat-video-tta_amd"
_MANGLED = re.compile(r"_Z(\d+)(\w+)")
# literal template arguments and parameter packs of named types: <8, 0, true, 0> = ILi8ELi0ELb1ELi0EE, <8, drop_args> = ILi8EJ9drop_argsEE
_TEMPLATE = re.compile(r"I(?:L[a-z]\w*?E|J\w*?E)+E")
_LABEL = re.compile(r"\.L(BB|func_end|func_begin)\d+")
_FP_VALU = re.compile(r"(v_(?:pk_)?\w+_f32|v_rcp\w*|v_div\w*)\b")
_ENCODING = re.compile(r"_(e32|e64|dpp|sdwa)\b")
_RESOURCES = {".amdhsa_next_free_vgpr": "next_free_vgpr", ".amdhsa_group_segment_fixed_size": "LDS bytes"}


def _plain(m: "re.Match") -> str:
    n, rest = int(m.group(1)), m.group(2)
    if n > len(rest):
        return m.group(0)
    name, tail = rest[:n], rest[n:]
    t = _TEMPLATE.match(tail)
    return name + (t.group(0) if t else "")


def normalise(text: str) -> Dict[str, List[str]]:
    """hipcc -S text -> {kernel: its lines from the entry label to .end_amdhsa_kernel}, plus "(metadata)"."""
    out: Dict[str, List[str]] = {}
    cur, functions = None, set()
    for raw in text.splitlines():
        line = raw.split(";", 1)[0].rstrip()
        line = _LABEL.sub(r".L\1", _MANGLED.sub(_plain, line))
        s = line.strip()
        if not s or s.startswith((".file", ".ident")):
            continue
        m = re.fullmatch(r"\.type\s+(\S+),@function", s)
        if m:
            functions.add(m.group(1) + ":")
        if s == ".amdgpu_metadata":
            cur = out.setdefault("(metadata)", [])
        elif s in functions:
            cur = out.setdefault(s[:-1], [])
        if cur is not None:
            cur.append(s)
            if s in (".end_amdhsa_kernel", ".end_amdgpu_metadata") or s.startswith(".Lfunc_end"):
                cur = None
    return out


def fp_ops(lines: List[str]) -> Counter:
    """The multiset of a kernel's floating-point VALU mnemonics, without encoding suffixes; v_fmac is v_fma with a tied register."""
    ops = Counter()
    for line in lines:
        m = _FP_VALU.match(_ENCODING.sub("", line.split(None, 1)[0]) if line else "")
        if m:
            ops[m.group(1).replace("v_fmac_", "v_fma_")] += 1
    return ops


def arithmetic_verdict(a: List[str], b: List[str]) -> str:
    """One line for a kernel that differs: `same fp ops` or `fp ops differ`, then the register and LDS figures."""
    fa, fb = fp_ops(a), fp_ops(b)
    if fa == fb:
        out = f"same fp ops ({sum(fa.values())} floating-point VALU instructions)"
    else:
        out = "fp ops differ: " + " ".join([f"-{n}x{k}" for k, n in sorted((fa - fb).items())] + [f"+{n}x{k}" for k, n in sorted((fb - fa).items())])
    res = []
    for key, label in _RESOURCES.items():
        va, vb = ([line.split()[1] for line in side if line.startswith(key + " ")] for side in (a, b))
        res.append(f"{label} {'/'.join(va) or '?'}" + ("" if va == vb else f" -> {'/'.join(vb) or '?'}"))
    same = all("->" not in r for r in res)
    return f"{out}; {', '.join(res)} ({'unchanged' if same else 'CHANGED'})"


def compare(old: str, new: str, show: int = 4, rename: Optional[Dict[str, str]] = None) -> List[str]:
    """-> one report line per kernel: `identical`, or where the two listings part.  With `rename` {old kernel: new kernel} only
    those kernels are compared, the old one under its new name."""
    a, b = normalise(old), normalise(new)
    if rename:
        a = {n: [line.replace(o, n) for line in a[o]] for o, n in rename.items() if o in a}
        b = {k: v for k, v in b.items() if k in rename.values()}
    report = []
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            report.append(f"{k}: only in the {'new' if k in b else 'old'} listing")
        elif a[k] == b[k]:
            report.append(f"{k}: identical ({len(a[k])} lines)")
        else:
            i = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
            report.append(f"{k}: DIFFERS at line {i} of {len(a[k])} / {len(b[k])}\n" +
                          "\n".join(f"    - {x}" for x in a[k][i:i + show]) + "\n" + "\n".join(f"    + {y}" for y in b[k][i:i + show]) +
                          ("" if k == "(metadata)" else "\n    " + arithmetic_verdict(a[k], b[k])))
    return report


def device_asm(csrc: Path, include: Path, name: str, dst: Path) -> str:
    sys.path.insert(0, str(ROOT / PKG))
    from lcv_hip import build as B
    flags = [str(include) if f == str(B.INCLUDE) else f for f in B.FLAGS]
    cmd = [B.HIPCC, *flags, *B.EXTRA.get(name, []), "--cuda-device-only", "-S", str(csrc / name), "-o", str(dst)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {csrc / name}:\n{r.stderr[-2000:]}")
    return dst.read_text()


def main(argv: List[str]) -> int:
    if not argv:
        print(__doc__)
        return 2
    rev, argv = argv[0], argv[1:]
    maps: Dict[tuple, Dict[str, str]] = {}                # (old file, new file) -> {old kernel: new kernel}
    while "--map" in argv:
        i = argv.index("--map")
        (old_file, old_kernel), (new_file, new_kernel) = (side.split(":", 1) for side in argv[i + 1].split("=", 1))
        maps.setdefault((old_file, new_file), {})[old_kernel] = new_kernel
        del argv[i:i + 2]
    names = argv or ([] if maps else sorted(p.name for p in (ROOT / PKG / "csrc").glob("attn_*.hip")))
    jobs = [(n, n, None) for n in names] + [(o, n, r) for (o, n), r in maps.items()]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        tar = subprocess.run(["git", "-C", str(ROOT), "archive", rev, f"{PKG}/csrc", "include"], capture_output=True, check=True)
        subprocess.run(["tar", "-x", "-C", str(tmp)], input=tar.stdout, check=True)

        def one(job):
            old_name, name, rename = job
            stem = f"{Path(old_name).stem}-{Path(name).stem}"
            old = device_asm(tmp / PKG / "csrc", tmp / "include", Path(old_name).name, tmp / f"{stem}.old.s")
            new = device_asm(ROOT / PKG / "csrc", ROOT / "include", Path(name).name, tmp / f"{stem}.new.s")
            return (f"{old_name} -> {name}" if rename else name), compare(old, new, rename=rename)
        with ThreadPoolExecutor(max_workers=6) as ex:
            for name, report in ex.map(one, jobs):
                print(f"== {name}")
                print("\n".join("  " + line for line in report))
                bad += sum("identical" not in line.split("\n")[0] for line in report)
    print(f"{'DIFFERENT' if bad else 'all identical'} against {rev}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
