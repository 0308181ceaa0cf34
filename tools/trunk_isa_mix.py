#!/usr/bin/env python3
"""Static instruction mix of the persistent trunk kernel (csrc/trunk.hip), no GPU needed.

Compiles trunk.hip to gfx950 device assembly with the flags of the library build (_build.FLAGS,
_build.HIPCC) and prints, for each production instantiation of trunk_kernel (the fp16 and the bf16
pair form): per basic block that holds MFMAs or vector-memory instructions the instruction count by
class, the totals over the whole kernel, and the compiler's resource lines
(-Rpass-analysis=kernel-resource-usage: registers, spills, scratch, occupancy).

    python tools/trunk_isa_mix.py [--csrc DIR] [-D NAME=VALUE ...] [--all-blocks]

--csrc lists another copy of the sources (e.g. an export of an earlier commit) with the same flags.
These are static facts about the code, not timings."""
from __future__ import annotations

import argparse
import re
import subprocess
import sys
import tempfile
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from image_super_resolution_amd import _build  # noqa: E402

CLASSES = ("mfma", "valu", "lane", "salu", "smem", "wait", "branch", "lds", "vmem")
# production instantiations: trunk_kernel<TK<4,4,2,16,XM,0>, H> (XM = the ISR_TRUNK_XCD build option)
PROD = re.compile(r"^_ZN3isr12trunk_kernelINS_2TKILi4ELi4ELi2ELi16ELi[01]ELi0EEELb([01])EEEvNS_9TrunkArgsE$")


def classify(op: str) -> str | None:
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith(("s_waitcnt", "s_nop", "s_sleep", "s_barrier")):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_endpgm", "s_call")):
        return "branch"
    if op.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    return None


def device_asm(csrc: Path, defines: list[str]) -> tuple[str, str]:
    """(assembly text, compiler remarks) of trunk.hip in `csrc`."""
    flags = [f for f in _build.FLAGS]
    i = flags.index(str(_build.CSRC))
    flags[i] = str(csrc)
    with tempfile.TemporaryDirectory() as td:
        out = Path(td) / "trunk.s"
        cmd = [_build.HIPCC, *flags, *defines, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
               str(csrc / "trunk.hip"), "-o", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{r.stderr}")
        return out.read_text(), r.stderr


def kernels(asm: str) -> dict[str, list[str]]:
    """Kernel symbol -> its assembly lines (label line to .Lfunc_end)."""
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m and PROD.match(m.group(1)):
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            else:
                cur.append(line)
    return out


def blocks(lines: list[str]) -> list[tuple[str, Counter]]:
    res, name, cnt = [], "entry", Counter()
    for line in lines:
        s = line.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", s) or re.match(r"^; %bb\.(\d+):", s)
        if m:
            res.append((name, cnt))
            name, cnt = m.group(1), Counter()
            continue
        if not s or s.startswith((";", ".", "//")):
            continue
        c = classify(s.split()[0])
        if c:
            cnt[c] += 1
    res.append((name, cnt))
    return res


def resources(remarks: str) -> dict[str, list[str]]:
    out, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: (.*) \[-Rpass-analysis", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            name = t.split(":", 1)[1].strip()
            cur = out.setdefault(name, []) if PROD.match(name) else None
        elif cur is not None:
            cur.append(t)
    return out


def fmt(cnt: Counter) -> str:
    return " ".join(f"{cnt.get(c, 0):6d}" for c in CLASSES)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", type=Path, default=_build.CSRC)
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--all-blocks", action="store_true", help="list every basic block, not only MFMA / VMEM ones")
    a = ap.parse_args()
    asm, remarks = device_asm(a.csrc.resolve(), [f"-D{d}" for d in a.defines])
    res = resources(remarks)
    ks = kernels(asm)
    if not ks:
        print("no production trunk_kernel instantiation found", file=sys.stderr)
        return 1
    for name, lines in ks.items():
        storage = "fp16" if PROD.match(name).group(1) == "1" else "bf16"
        bl = blocks(lines)
        print(f"== {name} ({storage} storage)")
        for t in res.get(name, []):
            print(f"   {t}")
        print(f"   basic blocks: {len(bl)}")
        print(f"   {'block':>12} " + " ".join(f"{c:>6}" for c in CLASSES))
        total = Counter()
        for bname, cnt in bl:
            total.update(cnt)
            if a.all_blocks or cnt.get("mfma") or cnt.get("vmem"):
                print(f"   {bname:>12} {fmt(cnt)}")
        print(f"   {'total':>12} {fmt(total)}")
        mf = [c for _, c in bl if c.get("mfma")]
        lane_in = sum(c.get("lane", 0) for c in mf)
        print(f"   MFMA blocks: {len(mf)}, lane moves (v_readlane / v_writelane / v_readfirstlane) inside them: {lane_in}")
        print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
