#!/usr/bin/env python3
"""ms per outfit of the sampling loop at the SD-1.5 shape (one 4-item outfit, full guidance: U-Net batch 16) for four schedulers, reported
and not gated: one JSON line to profiles/sched_multistep_bench.json.

  * ``ddim50``         DDIMScheduler, 50 steps (dfh_cfg_step, the flagship path of bench.py);
  * ``plms50_parent``  PNDMScheduler, 50 steps (51 entries), on the path every scheduler took before dfh_cfg_multistep: dfh_cfg_step with
                       STEP_NONE, a clone, and the scheduler's own ``step`` (up to four blend launches and the transfer, each behind a clone).
                       OutfitSampler still takes it for a scheduler object it does not know, which is how it is reached here;
  * ``plms50_fused``   the same scheduler through dfh_cfg_multistep: one launch per entry, nothing allocated;
  * ``dpmpp20``        DPMSolverMultistepScheduler, 20 steps.

Device events around the whole step loop of one outfit (``prepare`` is outside the window), after a warm-up loop of every case; the cases
alternate inside every window so that all four see the same minutes of the same card; the figure is the median of --windows windows and
the spread (min .. max) is kept.  Synthetic weights: the time does not depend on the values, and nothing here says anything about image
quality at 20 steps.

    python scripts/bench_sampler_schedulers.py [--windows 3] [--out profiles/sched_multistep_bench.json]
"""
import argparse
import os

import torch
from _rowbench import ROOT, emit, header, spread

import difashion_amd as da  # noqa: E402
from bench import build_models, outfit_inputs  # noqa: E402


class ParentPath:
    """A scheduler object OutfitSampler does not know: everything is forwarded to the wrapped PNDMScheduler."""

    def __init__(self, sched):
        self._sched = sched

    def __getattr__(self, name):
        return getattr(self._sched, name)


CASES = {"ddim50": (lambda: da.DDIMScheduler(), 50), "plms50_parent": (lambda: ParentPath(da.PNDMScheduler()), 50),
         "plms50_fused": (lambda: da.PNDMScheduler(), 50), "dpmpp20": (lambda: da.DPMSolverMultistepScheduler(), 20)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sched_multistep_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    unet, enc = build_models(dev, "sd15")
    inp = outfit_inputs(dev, unet.config.cross_attention_dim, 0, 1)
    samplers = {k: (da.OutfitSampler(unet, enc, make()), n) for k, (make, n) in CASES.items()}

    def loop(name):
        s, n = samplers[name]
        s.prepare(num_inference_steps=n, cate_scale=12.0, hist_scale=4.0, mutual_scale=5.0, eta=0.1, **inp)
        torch.cuda.synchronize()
        a0, b0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        for i in range(len(s.ts)):
            s.step(i)
        b0.record()
        torch.cuda.synchronize()
        assert torch.isfinite(s.latents).all(), name
        return a0.elapsed_time(b0), len(s.ts)

    per, entries = {k: [] for k in CASES}, {}
    for name in CASES:                               # warm-up: workspaces, packed weights, code-object load
        loop(name)
    for _ in range(a.windows):
        for name in CASES:
            ms, entries[name] = loop(name)
            per[name].append(ms)
    res = dict(**header(card=True), shape="SD-1.5, one 4-item outfit, full guidance (U-Net batch 16), 64x64 latents", windows=a.windows,
               cases={k: dict(ms_per_outfit=spread(per[k])["ms"], **spread(per[k]), unet_calls=entries[k],
                              ms_per_unet_call=round(spread(per[k])["ms"] / entries[k], 4), windows_ms=[round(v, 3) for v in per[k]]) for k in CASES})
    c = res["cases"]
    res["plms50_fused_over_parent"] = round(c["plms50_fused"]["ms"] / c["plms50_parent"]["ms"], 4)
    res["dpmpp20_over_ddim50"] = round(c["dpmpp20"]["ms"] / c["ddim50"]["ms"], 4)
    unet.end_run()
    emit(res, a.out)


if __name__ == "__main__":
    main()
