#!/usr/bin/env python3
"""Throughput of the grounding retrieval, reported and not gated: one JSON line to profiles/grounding_bench.json.

Shapes:
  * single: 8 192 generated rows x ONE 20 000-item candidate set x dim 1024 (one large category);
  * mixed:  8 192 rows spread evenly over 64 sets of 200 .. 20 000 items (log-uniform lengths) drawn from a 40 000-row table.
Per shape:
  * ``rank_candidates`` at top 100, the whole call (host-side set bookkeeping and the upload of the flat id list included), table norms
    given -- a caller ranks many batches against one table;
  * the only route the parent of this row offers: ``CLIPScore.retrieval`` over the rectangular [rows, K] block (one call per set in
    the mixed shape) followed by ``torch.topk``;
  * the kernels of the new call one by one, from ``rocprofv3 --kernel-trace --stats`` over a child process that makes the same call:
    the GEMM against the 157.3 TFLOP/s fp32 matrix peak (2 rows len dim flops), the selection against the bytes it reads (rows x len
    fp32) and the 8 TB/s HBM peak.
Calls are warmed up twice, then timed with device events over five windows of >= 0.2 s; the figure is the median, the spread is kept.

    python scripts/bench_grounding.py [--out profiles/grounding_bench.json]
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

import torch
from _rowbench import ROOT, emit, header, timed

import difashion_amd as da  # noqa: E402

PEAK_F32_MATRIX_TFLOPS, PEAK_HBM_GBPS = 157.3, 8000.0
ROWS, DIM, TOP = 8192, 1024, 100
KERNELS = {"gemm": "embed_rank_gemm_kernel", "select": "embed_rank_select_kernel"}


class Recorded:
    def encode_image(self, x):
        return x


def shape_inputs(name):
    """-> (gen [ROWS, DIM], table, per-row candidate lists on the CPU sharing one tensor per set, [(set tensor, its rows)])"""
    g = torch.Generator(device="cuda").manual_seed(1)
    gc = torch.Generator().manual_seed(2)
    gen = torch.randn(ROWS, DIM, generator=g, device="cuda")
    if name == "single":
        table = torch.randn(20000, DIM, generator=g, device="cuda")
        sets = [torch.randperm(20000, generator=gc)]
    else:
        table = torch.randn(40000, DIM, generator=g, device="cuda")
        lens = (200.0 * (100.0 ** torch.rand(64, generator=gc))).long().clamp(200, 20000)
        lens[0], lens[1] = 200, 20000
        sets = [torch.randperm(40000, generator=gc)[:int(n)] for n in lens]
    per = ROWS // len(sets)
    rows_of = [list(range(s * per, (s + 1) * per)) for s in range(len(sets))]
    cands = [sets[r // per] for r in range(ROWS)]
    return gen, table, cands, list(zip(sets, rows_of))


def new_call(gen, table, cands, norms):
    return da.rank_candidates(gen, table, cands, TOP, table_norms=norms)


def parent_route(cs, gen, table, groups_dev):
    out = []
    for cand_block, rows in groups_dev:
        sims, _ = cs.retrieval(gen[rows[0]:rows[-1] + 1], table, cand_block)
        out.append(torch.topk(sims, min(TOP, sims.shape[1]), dim=1))
    return out


def child(name):
    gen, table, cands, _ = shape_inputs(name)
    norms = da.embed_row_norms(table)
    for _ in range(3):
        new_call(gen, table, cands, norms)
    torch.cuda.synchronize()


def kernel_stats(name):
    """{kernel: (calls, total ns)} of three calls of the new route in a profiled child process, or {"error": ...}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", name]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
        except (OSError, subprocess.TimeoutExpired) as e:
            return {"error": f"{type(e).__name__}: {e}"}
        if r.returncode != 0:
            return {"error": f"rocprofv3 exit {r.returncode}: {r.stderr[-400:]}"}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "rocprofv3 wrote no kernel_stats.csv"}
        out = {}
        for row in csv.DictReader(open(files[0])):
            for key, kname in KERNELS.items():
                if kname in row["Name"]:
                    out[key] = (int(row["Calls"]), int(row["TotalDurationNs"]))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grounding_bench.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    if a.child:
        return child(a.child)
    res = header()
    res.update(rows=ROWS, dim=DIM, top_n=TOP, peak_f32_matrix_tflops=PEAK_F32_MATRIX_TFLOPS, peak_hbm_gbps=PEAK_HBM_GBPS)
    cs = da.CLIPScore(Recorded())
    for name in ("single", "mixed"):
        gen, table, cands, groups = shape_inputs(name)
        norms = da.embed_row_norms(table)
        pairs = float(sum(len(s) * len(rows) for s, rows in groups))
        ranked = new_call(gen, table, cands, norms)
        # the two routes agree on the best item of a row unless its two best stand closer than the routes' rounding (random data: the
        # best similarities of both routes are reported side by side, so a near-tie and a wrong row cannot be confused)
        groups_dev = [(s.to("cuda")[None].expand(len(rows), -1).contiguous(), rows) for s, rows in groups]
        old = parent_route(cs, gen, table, groups_dev)
        best_old = torch.cat([g[0][0, idx[:, 0]] for g, (_, idx) in zip(groups_dev, old)])
        entry = dict(sets=len(groups), set_len_min=min(len(s) for s, _ in groups), set_len_max=max(len(s) for s, _ in groups), row_candidate_pairs=pairs,
                     gflop=round(2.0 * pairs * DIM / 1e9, 2), rows_whose_best_item_differs_from_parent_route=int((best_old != ranked.preds).sum()),
                     max_abs_diff_of_best_similarity_vs_parent_route=float((torch.cat([v[:, 0] for v, _ in old]) - ranked.sims[:, 0]).abs().max()))
        del old
        entry["rank_candidates"] = timed(lambda: new_call(gen, table, cands, norms))
        entry["parent_route_retrieval_topk"] = timed(lambda: parent_route(cs, gen, table, groups_dev))
        entry["speedup_over_parent_route"] = round(entry["parent_route_retrieval_topk"]["ms"] / entry["rank_candidates"]["ms"], 2)
        del groups_dev
        torch.cuda.empty_cache()
        ks = kernel_stats(name)
        if "error" in ks or "gemm" not in ks or "select" not in ks:
            entry["kernels"] = dict(not_measured=ks.get("error", f"kernels missing from the trace: {sorted(ks)}"))
        else:
            calls = 3.0
            gemm_ms, sel_ms = ks["gemm"][1] / calls / 1e6, ks["select"][1] / calls / 1e6
            tf = 2.0 * pairs * DIM / (gemm_ms * 1e-3) / 1e12
            gbs = pairs * 4 / (sel_ms * 1e-3) / 1e9
            entry["kernels"] = dict(source="rocprofv3 --kernel-trace --stats, three calls in a child process, per call",
                                    gemm_ms=round(gemm_ms, 4), gemm_launches_per_call=ks["gemm"][0] / calls, gemm_tflops=round(tf, 2),
                                    gemm_fraction_of_f32_matrix_peak=round(tf / PEAK_F32_MATRIX_TFLOPS, 3),
                                    select_ms=round(sel_ms, 4), select_launches_per_call=ks["select"][0] / calls, select_read_gbps=round(gbs, 1),
                                    select_fraction_of_hbm_peak=round(gbs / PEAK_HBM_GBPS, 3),
                                    long_pole="gemm" if gemm_ms >= sel_ms else "select")
        res[name] = entry
    emit(res, a.out)


if __name__ == "__main__":
    main()
