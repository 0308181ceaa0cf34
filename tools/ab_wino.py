#!/usr/bin/env python3
"""A/B the opt-in fp16 Winograd F(2,3) RDB convs (isr_conv3x3_wino_fwd) against the direct form on
the cfg2 forward (ResNet(16, 0.2, x4), 16 x 128², fp16, synthetic weights), one process.

Pass 1: HIP-graph replays, interleaved rounds, device events — (a) the production chained
forward, for scale; (b) per-conv direct (chain=False); (c) wino="final"; (d) wino="rdb".  One JSON
line per form: median / min ms per forward and PSNR of its output against (b)'s.
Pass 2: eager forwards of (b) and (d), alternated, every RDB conv bracketed by events
(GeneratorPlan.run's around hook): per (cin, cout) shape the summed time of its 48 launches per
forward under each form and their ratio — the direct per-conv launch of the same shape in the
same process is what the Winograd form is measured against.
usage: python tools/ab_wino.py [--rounds 7 --steps 5] > profiles/wino_ab.jsonl"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from image_super_resolution_amd import engine, metrics, models  # noqa: E402
from image_super_resolution_amd.weights import normalize, synth_lr_batch, synth_state_dict  # noqa: E402

RDB_SHAPES = [(64, 32), (96, 32), (128, 32), (160, 32), (192, 64)]


def psnr(a: torch.Tensor, b: torch.Tensor) -> float | None:
    """PSNR in dB on the [-1, 1] output (peak 2); None when identical."""
    m = metrics.image_metrics(a, b, sr_space="tanh", hr_space="tanh", border=0, clamp=False)
    mse = m.mse.mean()  # pooled over the batch, on [0, 1]: peak 1 there is peak 2 on [-1, 1]
    return None if mse.item() == 0 else round(-10 * torch.log10(mse).item(), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--lr-size", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=16)
    args = ap.parse_args()
    dev = torch.device("cuda")
    n, hw = args.batch, args.lr_size
    sd = synth_state_dict(models.ResNet(args.blocks, 0.2, scaleRate=4).state_dict(), seed=0)
    gw = engine.pack_generator({k: v.to(dev) for k, v in sd.items()}, enchant=False, device=dev, wino="rdb")
    lr, _ = synth_lr_batch(n, hw, hw, seed=1234)
    x = normalize(lr).to(dev).contiguous()
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    forms = {"chain": dict(chain=True, wino="off"), "direct": dict(chain=False, wino="off"),
             "wino_final": dict(chain=False, wino="final"), "wino_rdb": dict(chain=False, wino="rdb")}
    plans, runs = {}, {}
    for name, kw in forms.items():
        plans[name] = engine.GeneratorPlan(gw, n, hw, hw, dev, False, False, mean, std, **kw)
        out = torch.empty(plans[name].out_shape, device=dev)
        runs[name] = (engine.GraphedPlan(plans[name], x, out), out)
    for g, _ in runs.values():  # warm up every form
        for _ in range(2):
            g.run()
    torch.cuda.synchronize()
    t = {name: [] for name in runs}
    for _ in range(args.rounds):
        for name, (g, _) in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                g.run()
            e1.record()
            torch.cuda.synchronize()
            t[name].append(e0.elapsed_time(e1) / args.steps)
    ref = runs["direct"][1]
    for name, (g, o) in runs.items():
        print(json.dumps({"form": name, "batch": n, "lr": hw, "rounds": args.rounds, "steps": args.steps,
                          "ms_median": round(statistics.median(t[name]), 4), "ms_min": round(min(t[name]), 4),
                          "psnr_vs_direct_db": psnr(o, ref), "finite": bool(torch.isfinite(o).all())}), flush=True)

    # pass 2: per-shape summed time of the RDB convs, direct vs Winograd, eager forwards alternated
    tags = {("conv3x3", ci, co) for ci, co in RDB_SHAPES}
    sums = {name: {s: [] for s in RDB_SHAPES} for name in ("direct", "wino_rdb")}
    for _ in range(args.rounds):
        for name in sums:
            evs = []

            def around(tag):
                if tag not in tags:
                    return None
                e = (tag, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                evs.append(e)
                return e[1:]

            out = runs[name][1]
            for _ in range(args.steps):
                plans[name].run(x, out, around=around)
            torch.cuda.synchronize()
            per = {s: 0.0 for s in RDB_SHAPES}
            for tag, a, b in evs:
                per[tag[1:]] += a.elapsed_time(b)
            for s in RDB_SHAPES:
                sums[name][s].append(per[s] / args.steps)
    launches = 3 * args.blocks
    for s in RDB_SHAPES:
        d_ms, w_ms = statistics.median(sums["direct"][s]), statistics.median(sums["wino_rdb"][s])
        print(json.dumps({"shape": list(s), "launches_per_forward": launches, "direct_ms_sum": round(d_ms, 4),
                          "wino_ms_sum": round(w_ms, 4), "direct_us_per_launch": round(1e3 * d_ms / launches, 2),
                          "wino_us_per_launch": round(1e3 * w_ms / launches, 2),
                          "direct_over_wino": round(d_ms / w_ms, 3)}), flush=True)


if __name__ == "__main__":
    main()
