#!/usr/bin/env python3
"""Are the kernels of this tree the same device code as those of another checkout?  No GPU needed.

Compiles every csrc/*.hip of both trees to gfx950 device assembly with the flags of the library
build (_build.FLAGS + --cuda-device-only -S, plus -DISR_TUNING with --tuning) and compares every
kernel present in both: the instruction text between the kernel's label and its end marker, and the
kernel descriptor (.amdhsa_* fields and the compiler's resource comment: registers, spills, scratch,
LDS, occupancy).  Two normalisations only: mangled symbol names (template parameters may have
gone; --rename maps the other tree's demangled kernel names onto this tree's) and the numbering of
local labels.

    python tools/isa_diff.py OTHER_ROOT [--tuning] [--rename REGEX=REPL ...] [--asm-dir DIR] [--files X.hip ...]

OTHER_ROOT is a checkout of the commit to compare against (e.g. a `git worktree`).  --asm-dir
keeps the assembly (an existing .s of the other tree is reused).  Exit status 1 on any difference.
"""
from __future__ import annotations

import argparse
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from image_super_resolution_amd import _build  # noqa: E402

RESOURCE = re.compile(r"^; (NumSgprs|NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|Occupancy|SGPRSpill|VGPRSpill|"
                      r"LDSByteSize|SGPRBlocks|VGPRBlocks|codeLenInByte|COMPUTE_PGM_RSRC\w*)\b")


def device_asm(root: Path, src: str, defines: list[str], out: Path) -> str:
    if not out.exists():
        out.write_text(_build.device_asm(root / "image_super_resolution_amd" / "csrc" / src, defines, root=root))
    return out.read_text()


def demangle(names: list[str]) -> dict[str, str]:
    if not names:
        return {}
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if tool is None:  # no demangler: kernels whose mangled names are unchanged still match
        return {n: n for n in names}
    r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def normalise(lines: list[str]) -> list[str]:
    """Instruction text: comments and blank lines dropped, symbols and local label numbers normalised."""
    labels: dict[str, str] = {}

    def label(m):
        return labels.setdefault(m.group(0), f".L{len(labels)}")

    out = []
    for line in lines:
        s = line.split(";")[0].strip() if not line.lstrip().startswith(";;#ASM") else line.strip()
        if not s:
            continue
        s = re.sub(r"\.L\w+", label, s)
        out.append(re.sub(r"\b_Z\w+", "SYM", s))
    return out


def kernels(asm: str) -> dict[str, dict]:
    """Mangled kernel name -> {"text": normalised instructions, "desc": descriptor and resource lines}."""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    out: dict[str, dict] = {n: {"text": [], "desc": []} for n in names}
    body = desc = None
    last = None
    for line in asm.splitlines():
        m = re.match(r"^(\w+):", line)
        if m and m.group(1) in names and not out[m.group(1)]["text"]:
            body, last = [], m.group(1)
            continue
        if m and body is None:
            last = None  # a device function that is no kernel: its resource comment is not the kernel's
        if body is not None:
            if line.startswith(".Lfunc_end"):
                out[last]["text"] = normalise(body)
                body = None
            else:
                body.append(line)
            continue
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            desc = out[m.group(1)]["desc"]
        elif line.strip() == ".end_amdhsa_kernel":
            desc = None
        elif desc is not None:
            desc.append(line.strip())
        elif last and RESOURCE.match(line):
            out[last]["desc"].append(line.strip())
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("other", type=Path)
    ap.add_argument("--tuning", action="store_true")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL",
                    help="applied to the other tree's demangled kernel names before matching")
    ap.add_argument("--asm-dir", type=Path)
    ap.add_argument("--files", nargs="*", help="csrc file names (default: every .hip)")
    a = ap.parse_args()
    defines = ["-DISR_TUNING"] if a.tuning else []
    tag = "_tuning" if a.tuning else ""
    tmp = None if a.asm_dir else tempfile.TemporaryDirectory()
    base = a.asm_dir or Path(tmp.name)
    srcs = a.files or [p.name for p in _build.sources()]
    jobs = []
    with ThreadPoolExecutor(max_workers=8) as ex:
        for which, root in (("other", a.other.resolve()), ("new", ROOT)):
            d = base / (which + tag)
            d.mkdir(parents=True, exist_ok=True)
            for s in srcs:
                out = d / (Path(s).stem + ".s")
                if which == "new":
                    out.unlink(missing_ok=True)
                if (root / "image_super_resolution_amd" / "csrc" / s).exists():
                    jobs.append((which, s, ex.submit(device_asm, root, s, defines, out)))
        asm = {(w, s): f.result() for w, s, f in jobs}
    bad = 0
    print(f"# {'tuning' if a.tuning else 'production'} build: {' '.join(_build.FLAGS[:5] + defines)} --cuda-device-only -S")
    for s in srcs:
        if ("other", s) not in asm:
            continue
        old, new = kernels(asm[("other", s)]), kernels(asm[("new", s)])
        dm_old, dm_new = demangle(list(old)), demangle(list(new))
        for rule in a.rename:
            pat, repl = rule.split("=", 1)
            dm_old = {k: re.sub(pat, repl, v) for k, v in dm_old.items()}
        by_name = {v: k for k, v in dm_new.items()}
        print(f"== {s}: {len(old)} kernels in the other tree, {len(new)} in this one")
        for k, name in sorted(dm_old.items(), key=lambda kv: kv[1]):
            if name not in by_name:
                print(f"   only-other  {name}")
                continue
            o, n = old[k], new[by_name.pop(name)]
            same_text, same_desc = o["text"] == n["text"], o["desc"] == n["desc"]
            bad += not (same_text and same_desc)
            res = " ".join(x[2:] for x in n["desc"] if re.match(r"^; (NumVgprs|NumAgprs|NumSgprs|SGPRSpill|VGPRSpill|"
                                                               r"ScratchSize|LDSByteSize|Occupancy)\b", x))
            print(f"   {'IDENTICAL' if same_text and same_desc else 'DIFFERENT'}   {name}\n"
                  f"               {len(n['text'])} instruction lines{'' if same_text else ' (text differs: ' + str(len(o['text'])) + ' before)'}; "
                  f"descriptor {'equal' if same_desc else 'DIFFERS'}; {res}")
            if not same_desc:
                for x in sorted(set(o["desc"]) ^ set(n["desc"])):
                    print(f"               {'-' if x in o['desc'] else '+'} {x}")
        for name in sorted(by_name):
            print(f"   only-new    {name}")
    print(f"# {bad} kernel(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
