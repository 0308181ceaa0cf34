"""Host-only C++ programs of the suite (a csrc header with a main of its own, no GPU and nothing loaded
into Python): built with g++ plain and with the address and undefined-behaviour sanitizers, run both
ways; the two builds must run clean and print the same."""
import shutil
import subprocess
from pathlib import Path

CSRC = Path(__file__).resolve().parents[1] / "image_super_resolution_amd" / "csrc"
GXX = shutil.which("g++")
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")


def run_plain_and_sanitized(src, tmp_path, *, extra_flags=(), runs=((),), timeout=300) -> list[str]:
    """The standard output of the program `src` for each argument list of `runs`.  Every run of either
    build must exit with status 0 and an empty stderr, and the sanitizer build must print what the
    plain one prints."""
    out = {}
    for tag, san in (("plain", ()), ("san", SANITIZE)):
        exe = Path(tmp_path) / f"{Path(src).stem}_{tag}"
        cmd = [GXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *extra_flags, *san, "-I", str(CSRC),
               str(src), "-o", str(exe)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        for args in runs:
            r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=timeout)
            assert r.returncode == 0 and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-4000:]
            out.setdefault(tag, []).append(r.stdout)
    assert out["plain"] == out["san"], "the sanitizer build computes something else"
    return out["plain"]
