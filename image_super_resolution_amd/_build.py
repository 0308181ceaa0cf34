"""Builds libisr.so (the HIP kernels + C-ABI) in-tree with hipcc for gfx950.

No cmake/ninja: one hipcc invocation per .hip file (run in parallel), then a
link.  The output lands in image_super_resolution_amd/lib/ so it travels with
the repository snapshot to the GPU box.

`python -m image_super_resolution_amd._build --tuning` builds lib/libisr_tuning.so
with -DISR_TUNING (the shipping kernels instrumented: stamps, ablation knobs, ring-protocol
checks; plus A/B forms of the per-conv and weight-gradient kernels); tools load it with
ISR_LIB=<path>.  The production libisr.so never contains them.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
LIBDIR = PKG / "lib"
LIB = LIBDIR / "libisr.so"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", f"--offload-arch={ARCH}", "-fPIC", "-Wall", "-Wno-unused-function",
         "-I", str(ROOT / "include"), "-I", str(CSRC)]


# sources whose kernels read LDS through inline asm with hand-counted waits: their device assembly
# is checked on every full build (tools/check_lds_waits.py)
WAIT_CHECKED = ("wgrad3x3.hip", "conv9x9.hip")


def sources() -> list[Path]:
    return sorted(CSRC.glob("*.hip"))


def device_asm(src, defines=(), root: Path = ROOT, remarks: bool = False):
    """The gfx950 device assembly hipcc makes of one .hip with the library's FLAGS (`defines`: further
    options such as -DISR_TUNING); with remarks, (assembly, the compiler's kernel-resource remarks).  For
    another checkout, `root` re-roots the public include path; csrc headers are taken from beside `src`."""
    src = Path(src)
    swap = {str(ROOT / "include"): str(Path(root) / "include"), str(CSRC): str(src.parent)}
    cmd = [HIPCC, *(swap.get(f, f) for f in FLAGS), *defines, "--cuda-device-only", "-S", str(src), "-o", "-"]
    r = subprocess.run(cmd + (["-Rpass-analysis=kernel-resource-usage"] if remarks else []), capture_output=True,
                       text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc -S failed on {src}:\n{r.stderr}")
    return (r.stdout, r.stderr) if remarks else r.stdout


def kernel_resources(src, defines=(), remarks: str | None = None) -> dict[str, dict[str, str]]:
    """{mangled kernel name: {remark field: value}} from hipcc's kernel-resource remarks on one .hip
    (fields such as "VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]").
    `remarks`: those of a device_asm(..., remarks=True) already made, to save the compile."""
    out, cur = {}, None
    for line in (device_asm(src, defines, remarks=True)[1] if remarks is None else remarks).splitlines():
        m = re.search(r"remark: (.*) \[-Rpass-analysis", line)
        if m:
            key, _, val = m.group(1).strip().partition(":")
            if key == "Function Name":
                cur = out.setdefault(val.strip(), {})
            elif cur is not None:
                cur[key.strip()] = val.strip()
    return out


def _needs_build() -> bool:
    if not LIB.exists():
        return True
    t = LIB.stat().st_mtime
    deps = sources() + list(CSRC.glob("*.h")) + [ROOT / "include" / "isr.h", Path(__file__)]
    return any(p.stat().st_mtime > t for p in deps)


def build(force: bool = False, verbose: bool = False, tuning: bool = False) -> Path:
    lib_path = LIBDIR / "libisr_tuning.so" if tuning else LIB
    if not tuning and not force and not _needs_build():
        return LIB
    objdir = PKG / ("build_tuning" if tuning else "build")
    flags = FLAGS + (["-DISR_TUNING"] if tuning else [])
    objdir.mkdir(exist_ok=True)
    LIBDIR.mkdir(exist_ok=True)

    headers = list(CSRC.glob("*.h")) + [ROOT / "include" / "isr.h", Path(__file__)]
    newest_header = max(p.stat().st_mtime for p in headers)

    def compile_one(src: Path) -> Path:
        obj = objdir / (src.stem + ".o")
        if not force and obj.exists() and obj.stat().st_mtime > max(src.stat().st_mtime, newest_header):
            return obj  # incremental: object newer than its source and every header
        cmd = [HIPCC, *flags, "-c", str(src), "-o", str(obj)]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src.name}:\n{r.stderr}")
        if verbose and r.stderr:
            print(r.stderr, file=sys.stderr)
        return obj

    def check_waits(src: Path) -> list[str]:
        """the hand-counted LDS waits of the asm-read kernels, checked on the gfx950
        assembly hipcc produces for them (tools/check_lds_waits.py: no read of an LDS destination
        before its wait, no SMEM load under a counted wait, no scratch)."""
        sys.path.insert(0, str(ROOT / "tools"))
        try:
            import check_lds_waits
        finally:
            sys.path.pop(0)
        errs = check_lds_waits.check_asm(device_asm(src, ["-DISR_TUNING"] if tuning else []), src.name)
        if tuning and errs:
            # the tuning library also carries A/B forms of the weight-gradient kernels that never ship
            # (measured slower): a hazard there is reported, and fatal only in a production kernel
            prod = set(check_lds_waits.kernels(device_asm(src))[0])
            for e in errs:
                if e.split(":", 1)[0] not in prod:
                    print(f"[build] tuning-only kernel, not fatal: {e}", file=sys.stderr)
            errs = [e for e in errs if e.split(":", 1)[0] in prod]
        return errs

    checked = [CSRC / n for n in WAIT_CHECKED] if (force or tuning or not LIB.exists()) else []
    with ThreadPoolExecutor(max_workers=min(8, len(sources()) + len(checked))) as ex:
        waits = [ex.submit(check_waits, src) for src in checked]
        objs = list(ex.map(compile_one, sources()))
        errs = [e for w in waits for e in w.result()]
    if errs:
        raise RuntimeError("LDS wait check failed (tools/check_lds_waits.py):\n" + "\n".join(errs))
    tmp = lib_path.with_suffix(".so.tmp")
    cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(tmp), *map(str, objs)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stderr}")
    os.replace(tmp, lib_path)
    return lib_path


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True, tuning="--tuning" in sys.argv))
