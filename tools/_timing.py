"""Timing helpers of the bench_*.py tools of the training-data stack."""
from __future__ import annotations

import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import torch

TOOLS = Path(__file__).resolve().parent


def timed(fn, iters: int, runs: int, warmup: int = 10) -> float:
    """Median over `runs` of the µs per call of `fn` (device events around `iters` calls)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / iters)
    return round(statistics.median(out), 2)


def host_ms(fn, runs: int) -> float:
    """Median wall clock of `fn` on the host, in ms."""
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * statistics.median(ts), 3)


def train_step_ms(tool: str = "bench_train.py", args=("--steps", "3", "--warmup", "2"), key: str = "ms_per_step",
                  timeout: int = 900) -> float:
    """One training step as another tool of this directory measures it, in a fresh child process: `key`
    of the JSON on the last line it prints."""
    r = subprocess.run([sys.executable, str(TOOLS / tool), *args], capture_output=True, text=True, check=True,
                       timeout=timeout)
    return json.loads(r.stdout.strip().splitlines()[-1])[key]
