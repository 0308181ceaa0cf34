#!/usr/bin/env python3
"""The phase-2 hand-off of the trunk kernel's growth pairs, from the tuning build's stamps
(ISR_LIB=.../libisr_tuning.so): for the second layers of the pairs among layers 75..89 and every
tile, stamp 0 (phase-2 entry), 4 (stores drained and progress published: first poll issued), 5
(neighbourhood met) and 1 (first chunk in LDS for every wave, barrier passed), s_memrealtime at
100 MHz.  Prints one JSON line per layer and one over all of them: percentiles in microseconds of
drain + publish (4 - 0), poll (5 - 4), fetch issue to landed (1 - 5) and the whole hand-off (1 - 0).
usage: python tools/trunk_handoff.py [fp16 0/1] [batch] [lr]"""
from __future__ import annotations

import ctypes
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from image_super_resolution_amd import _lib, engine, models  # noqa: E402
from image_super_resolution_amd.weights import normalize, synth_lr_batch, synth_state_dict  # noqa: E402


def pct(v, qs=(0.1, 0.5, 0.9, 1.0)):
    v = sorted(v)
    return [round(v[min(len(v) - 1, int(q * len(v)))], 2) for q in qs] if v else []


def main():
    lib = _lib.load()
    f16 = bool(int(sys.argv[1])) if len(sys.argv) > 1 else True
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    lrs = int(sys.argv[3]) if len(sys.argv) > 3 else 128
    dev = torch.device("cuda")
    sd = synth_state_dict(models.ResNet(16, 0.2, scaleRate=4).state_dict(), seed=0)
    gw = engine.pack_generator({k: v.to(dev) for k, v in sd.items()}, enchant=False, device=dev, f16=f16)
    lr, _ = synth_lr_batch(n, lrs, lrs, seed=1234)
    x = normalize(lr).to(dev).contiguous()
    plan = engine.GeneratorPlan(gw, n, lrs, lrs, dev, False, False, (0.485, 0.456, 0.406),
                                (0.229, 0.224, 0.225), chain=True, chain_acquire=False)
    out = torch.empty(plan.out_shape, device=dev)
    for _ in range(3):
        plan.run(x, out)
    torch.cuda.synchronize()
    ntiles = n * (plan.bufs.feat.ha // 16) * (plan.bufs.feat.wa // 32)
    st = torch.zeros(15 * ntiles * 8, dtype=torch.int64, device=dev)
    _lib.check(lib.isr_tuning_trunk_stamps(ctypes.c_void_p(st.data_ptr())), "stamps")
    plan.run(x, out)
    torch.cuda.synchronize()
    _lib.check(lib.isr_tuning_trunk_stamps(None), "stamps off")
    assert not plan.chain.failed()
    a = st.view(15, ntiles, 8).cpu().double() / 100.0  # 100 MHz ticks -> us
    tot = {"drain_publish": [], "poll": [], "fetch": [], "handoff": []}
    for L in range(15):
        if L % 5 not in (1, 3):  # the second layers of (conv0, conv1) and (conv2, conv3)
            continue
        e, c0, w0, w1 = a[L, :, 0], a[L, :, 1], a[L, :, 4], a[L, :, 5]
        ok = ((w0 > 0) & (c0 > 0)).nonzero().flatten()
        parts = {"drain_publish": (w0 - e)[ok].tolist(), "poll": (w1 - w0)[ok].tolist(),
                 "fetch": (c0 - w1)[ok].tolist(), "handoff": (c0 - e)[ok].tolist()}
        row = {"layer": 75 + L, "tiles": len(ok)}
        for k, v in parts.items():
            tot[k] += v
            row[k + "_p10_p50_p90_max"] = pct(v)
        print(json.dumps(row), flush=True)
    row = {"layer": "all", "tiles": len(tot["poll"])}
    for k, v in tot.items():
        row[k + "_p10_p50_p90_max"] = pct(v)
        row[k + "_mean"] = round(sum(v) / max(1, len(v)), 3)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
