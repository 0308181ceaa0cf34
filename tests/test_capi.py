"""C-ABI checks that need no GPU: libisr.so loads, exports every symbol
include/isr.h declares, and every ctypes mirror matches its C struct's layout (probed
with gcc).  What the entry points refuse is in tests/test_capi_refusals.py."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest

from conftest import ROOT
from image_super_resolution_amd import _lib

HEADER = ROOT / "include" / "isr.h"


def declared_functions():
    txt = HEADER.read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(isr_[a-z0-9_]+)\s*\(", txt)))


def test_all_header_symbols_exported(built_lib):
    names = declared_functions()
    assert len(names) >= 12
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (isr_[a-z0-9_]+)\b", nm))
    missing = [n for n in names if n not in exported]
    assert not missing, f"declared but not exported: {missing}"
    # and the ctypes binding knows every one of them
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)


def c_name(cls):
    """IsrHlsMomentsDesc -> isr_hls_moments_desc, IsrWgrad9Desc -> isr_wgrad9_desc."""
    return re.sub(r"(?<!^)(?=[A-Z])", "_", cls.__name__).lower()


MIRRORS = {c_name(c): c for c in vars(_lib).values() if isinstance(c, type) and issubclass(c, ctypes.Structure)}
UNMIRRORED = ("isr_mt_tensor", "isr_mt_chunk", "isr_pack_item")  # written as bytes by ops.py / optim.py
MACROS = {"ISR_HLS_PARTIAL_BLOCKS": _lib.HLS_PARTIAL_BLOCKS, "ISR_TILE_H": _lib.TILE_H, "ISR_TILE_W": _lib.TILE_W}


def probe_source():
    """A C program that prints sizeof of every mirrored struct, offsetof and sizeof of every field the mirror
    names, the sizes of the structs Python writes as bytes, and the macros _lib restates."""
    out = ["#include <stdio.h>", "#include <stddef.h>", '#include "isr.h"', "int main(void) {"]
    for name, cls in MIRRORS.items():
        out.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        out += [f'  printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));'
                for f, _ in cls._fields_]
    out += [f'  printf("{name} %zu\\n", sizeof({name}));' for name in UNMIRRORED]
    out += [f'  printf("isr_pack_item.{f} %zu\\n", offsetof(isr_pack_item, {f}));' for f in ("scale", "src_n0", "src_cin")]
    out += [f'  printf("{m} %d\\n", {m});' for m in MACROS]
    return "\n".join(out + ["  return 0;", "}", ""])


def test_struct_layouts_match_c(tmp_path):
    """Every ctypes.Structure of _lib against the C struct of the same name: size, and offset and size of every
    field (arrays included); every struct of the header has a mirror or is one of the three written as bytes."""
    txt = HEADER.read_text()
    assert set(re.findall(r"typedef struct (isr_\w+) \{", txt)) == set(MIRRORS) | set(UNMIRRORED)
    src = tmp_path / "probe.c"
    src.write_text(probe_source())
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    c = {k: [int(v) for v in vals] for k, *vals in map(str.split, lines)}
    wrong = []
    for name, cls in MIRRORS.items():
        if c[name] != [ctypes.sizeof(cls)]:
            wrong.append((name, c[name], ctypes.sizeof(cls)))
        for f, _ in cls._fields_:
            py = [getattr(cls, f).offset, getattr(cls, f).size]
            if c[f"{name}.{f}"] != py:
                wrong.append((f"{name}.{f}", c[f"{name}.{f}"], py))
    assert not wrong, wrong
    # isr_pack_item is written by ops.pack_batch_table with struct "<QQiiiifiii"
    assert c["isr_pack_item"] == [48]
    assert (c["isr_pack_item.scale"], c["isr_pack_item.src_n0"], c["isr_pack_item.src_cin"]) == ([32], [36], [40])
    assert c["isr_mt_tensor"] == [_lib.MT_TENSOR_BYTES] and c["isr_mt_chunk"] == [_lib.MT_CHUNK_BYTES]
    for m, v in MACROS.items():
        assert c[m] == [v], m


def test_version(built_lib):
    assert built_lib.isr_version() >= 1


def test_packed_sizes(built_lib):
    lib = built_lib
    assert lib.isr_conv3x3_packed_bytes(64, 192) == 64 * 192 * 9 * 2
    assert lib.isr_head9x9_packed_bytes(64, 3) == 9 * 3 * 64 * 16 * 2
    assert lib.isr_tail9x9_packed_bytes(3, 64) == 9 * 2 * 2 * 32 * 32


def test_product_path_refuses_cpu_tensors():
    import torch
    from image_super_resolution_amd import models
    m = models.ResNet(1, 0.2, scaleRate=2).eval()
    with pytest.raises(RuntimeError, match="HIP"):
        with torch.no_grad():
            m(torch.zeros(1, 3, 16, 16))
