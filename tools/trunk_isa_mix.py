#!/usr/bin/env python3
"""Static instruction mix of the persistent trunk kernel (csrc/trunk.hip), no GPU needed.

Compiles trunk.hip to gfx950 device assembly with the flags of the library build (_build.FLAGS,
_build.HIPCC) and prints, for each production instantiation of trunk_kernel (the fp16 and the bf16
pair form): per basic block that holds MFMAs or vector-memory instructions the instruction count by
class, the totals over the whole kernel, the compiler's resource lines
(-Rpass-analysis=kernel-resource-usage: registers, spills, scratch, occupancy), and one line per
basic block that holds vector-memory stores (the tile epilogues): instructions, stores, VALU
instructions per stored value, and which specialised epilogue form the block belongs to.

    python tools/trunk_isa_mix.py [--csrc DIR] [-D NAME=VALUE ...] [--all-blocks]

--csrc lists another copy of the sources (e.g. an export of an earlier commit) with the same flags.
These are static facts about the code, not timings."""
from __future__ import annotations

import argparse
import re
import sys
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from image_super_resolution_amd import _build  # noqa: E402

CLASSES = ("mfma", "valu", "lane", "salu", "smem", "wait", "branch", "lds", "vmem")
# production instantiations: trunk_kernel<H> (in a --csrc copy from before the A/B forms were removed:
# trunk_kernel<TK<4,4,2,16,XM,0>, H>)
PROD = re.compile(r"^_ZN3isr12trunk_kernelI(?:NS_2TKILi4ELi4ELi2ELi16ELi[01]ELi0EEE)?Lb([01])EEEvNS_9TrunkArgsE$")


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


EPI_FORMS = {1: "growth", 2: "final", 3: "final_s2", 4: "final_r2"}  # trunk_common.h EPI_*
EPI_MARK = re.compile(r"^; trunk epilogue form (\d+) full (\d+)")
STORE = re.compile(r"^(?:buffer|global|flat)_store_(\w+)")
STORE_BYTES = {"byte": 1, "short": 2, "dword": 4, "dwordx2": 8, "dwordx3": 12, "dwordx4": 16}
PACKED_CVT = {"fp16": "v_cvt_pk_f16_f32", "bf16": "v_cvt_pk_bf16_f32"}


def store_blocks(lines: list[str]) -> list[dict]:
    """One entry per basic block that holds vector-memory stores: its instruction count, stores,
    stored 16-bit values per lane, VALU instructions (MFMAs and lane moves apart) per stored value,
    the packed fp32 -> 16-bit converts in it, and the epilogue form whose marker comment
    (run_tile's specialised bodies emit one) lies in the block: (name, full tile) or None."""
    res, cur = [], None

    def new(name):
        return {"block": name, "insts": 0, "stores": 0, "values": 0, "valu": 0, "ops": Counter(), "form": None}

    def close(b):
        # tile-epilogue blocks only: a block whose stores are single dwords holds a progress word
        if b and b["values"] >= 8:
            b["valu_per_value"] = b["valu"] / b["values"]
            res.append(b)

    cur = new("entry")
    for line in lines:
        s = line.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", s) or re.match(r"^; %bb\.(\d+):", s)
        if m:
            close(cur)
            cur = new(m.group(1))
            continue
        m = EPI_MARK.match(s)
        if m:
            cur["form"] = (EPI_FORMS.get(int(m.group(1)), m.group(1)), bool(int(m.group(2))))
            continue
        if not s or s.startswith((";", ".", "//")):
            continue
        op = s.split()[0]
        c = classify(op)
        if not c:
            continue
        cur["insts"] += 1
        cur["ops"][op.removesuffix("_e32").removesuffix("_e64")] += 1
        if c == "valu":
            cur["valu"] += 1
        m = STORE.match(op)
        if m:
            cur["stores"] += 1
            cur["values"] += STORE_BYTES.get(m.group(1), 0) // 2
    close(cur)
    return res


def storage_of(name: str) -> str:
    return "fp16" if PROD.match(name).group(1) == "1" else "bf16"


def production_store_blocks(csrc: Path = _build.CSRC, defines: tuple[str, ...] = ()) -> dict[str, list[dict]]:
    """storage ("fp16" / "bf16") -> store_blocks() of that production instantiation."""
    asm = _build.device_asm(Path(csrc).resolve() / "trunk.hip", defines)
    return {storage_of(name): store_blocks(lines) for name, lines in kernels(asm).items()}


def fmt_store_block(b: dict, storage: str) -> str:
    form = "-" if b["form"] is None else f"{b['form'][0]}/{'full' if b['form'][1] else 'ragged'}"
    return (f"{b['block']:>12} {form:>16} {b['insts']:6d} {b['stores']:6d} {b['values']:6d} {b['valu']:6d} "
            f"{b['valu_per_value']:8.2f} {b['ops'].get(PACKED_CVT[storage], 0):6d}")


def fmt(cnt: Counter) -> str:
    return " ".join(f"{cnt.get(c, 0):6d}" for c in CLASSES)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--csrc", type=Path, default=_build.CSRC)
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--all-blocks", action="store_true", help="list every basic block, not only MFMA / VMEM ones")
    a = ap.parse_args()
    src, defines = a.csrc.resolve() / "trunk.hip", [f"-D{d}" for d in a.defines]
    asm, remarks = _build.device_asm(src, defines, remarks=True)
    res = _build.kernel_resources(src, defines, remarks=remarks)
    ks = kernels(asm)
    if not ks:
        print("no production trunk_kernel instantiation found", file=sys.stderr)
        return 1
    for name, lines in ks.items():
        storage = storage_of(name)
        bl = blocks(lines)
        print(f"== {name} ({storage} storage)")
        for field, value in res.get(name, {}).items():
            print(f"   {field}: {value}")
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
        print("   store-holding blocks (values = stored 16-bit values per lane; pk_cvt = packed fp32 converts):")
        print(f"   {'block':>12} {'epilogue form':>16} {'insts':>6} {'stores':>6} {'values':>6} {'valu':>6} "
              f"{'valu/val':>8} {'pk_cvt':>6}")
        for b in store_blocks(lines):
            print("   " + fmt_store_block(b, storage))
        print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
