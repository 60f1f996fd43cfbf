"""What the row benchmarks (bench_clip_vision.py, bench_eval_scores.py, bench_image_processor.py, bench_lpips.py) share: the timing
routine, the device header of a result and its one JSON line.  Importing it puts the repository root on the path."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from difashion_amd import _lib  # noqa: E402


def spread(per):
    """median, min, max of per-window ms figures"""
    return dict(ms=round(statistics.median(per), 4), ms_min=round(min(per), 4), ms_max=round(max(per), 4))


def timed(fn, windows=5, min_window_ms=200.0):
    """ms per call: median, min, max over `windows` event-timed windows, each long enough to swamp the launch overhead."""
    fn(); fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    reps = max(1, int(min_window_ms / max(a.elapsed_time(b), 1e-3)) + 1)
    per = []
    for _ in range(windows):
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) / reps)
    return dict(**spread(per), calls_per_window=reps)


def randomise(module, g):
    """Small random matrices drawn on the device: the speed does not depend on them."""
    for p in module.parameters():
        if p.dim() >= 2:
            p.copy_(torch.randn(p.shape, generator=g, device="cuda") * (0.7 / p[0].numel() ** 0.5))


def header(card=False):
    """Which device and which build a result came from; card: the marketing name alone does not identify the card"""
    res = dict(device=torch.cuda.get_device_name(0))
    if card:
        prop = torch.cuda.get_device_properties(0)
        res.update(gcn_arch=getattr(prop, "gcnArchName", ""), compute_units=prop.multi_processor_count, hbm_gib=round(prop.total_memory / 2 ** 30, 1))
    res["build_info"] = _lib.raw().dfh_build_info().decode()
    return res


def emit(res, out):
    """One JSON line, to the file `out` and to stdout."""
    line = json.dumps(res)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)
