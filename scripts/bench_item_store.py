#!/usr/bin/env python3
"""What the item store buys, reported and not gated: one JSON line to profiles/item_store_bench.json.

  * input_stage: everything ``DiFashion.forward`` does BEFORE ``train_forward`` for 8 outfits x 4 items -- ``train_forward`` is replaced
    by a stub that returns at once -- with the SD-size AutoencoderKL (seeded random weights; the speed does not depend on them) at
    512 x 512, through
      - images + dict: the parent's only path -- 32 images picked one by one from an IN-MEMORY fp32 tensor data set (no JPEG decode,
        no transform: the real loader adds both on top), stacked, copied, encoded and sampled; the null image encoded; 32 history rows
        picked from a host dict of pre-averaged latents and copied one by one;
      - store + table: two ``dfh_item_gather`` launches and one ``dfh_history_rows`` launch.
    The text side is a table stand-in, the same in both; categories are Python ints so that the dict path's lookups hit.
  * kernels: call time of the two kernels at a size beyond the Infinity Cache (4 096 rows of 4 x 64 x 64 from a 40 000-item table,
    history segments of 8 items, every id distinct so that no read is served by a cache) as bytes moved per second, beside
    ``torch``'s device copy of the same byte count (read + written) in the same process; and at the step's own size (32 rows), where
    the launch is the cost.
  * vae_encode_batch_invariance: the tiny AutoencoderKL on five images together against one by one (a store equals the image path
    bit for bit only for batches that give the same moments); input_stage.sd_vae_encode_batch_invariance: the same question at the
    SD size, four images at 512 x 512.
Calls are warmed up twice, then timed with device events over five windows of >= 0.2 s; the figure is the median, the spread is kept.

    python scripts/bench_item_store.py [--out profiles/item_store_bench.json]
"""
import argparse
import os
import types

import torch
from _rowbench import ROOT, emit, header, timed

import difashion_amd as da  # noqa: E402
from difashion_amd import _lib, difashion as difashion_module  # noqa: E402

BSZ, OLEN, ITEMS_STAGE, CATES = 8, 4, 256, 10
TABLE_ITEMS, ROWS, SEG_LEN, LATENT = 40000, 4096, 8, (4, 64, 64)
E = LATENT[0] * LATENT[1] * LATENT[2]


def input_stage(res):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1)
    vae = da.AutoencoderKL().to(dev)
    dataset = torch.rand(ITEMS_STAGE, 3, 512, 512, generator=g) * 2 - 1
    store = da.data.build_item_store(vae, dataset, dev, batch_size=16)
    uids = torch.arange(BSZ) + 100
    raw = {int(u): {c: torch.randint(0, ITEMS_STAGE, (8,), generator=g).tolist() for c in range(CATES)} for u in uids}
    table = da.data.history_table(store, raw)
    host_dict = da.data.history_latents(store.modes(torch.arange(ITEMS_STAGE)).cpu(), raw)      # what preprocess_dataset hands the reference
    prompt = torch.zeros(BSZ * OLEN, 77, 768, device=dev)
    prompts = types.SimpleNamespace(null_prompt=prompt[:1], lookup=lambda cats: prompt)
    unet = torch.nn.Linear(1, 1).to(dev)                                                        # forward reads its device only
    args = types.SimpleNamespace(use_history=True, use_mutual_guidance=False, eta=0.1, noise_offset=0)
    model = da.DiFashion(args, vae=vae, unet=unet, fashion_encoder=types.SimpleNamespace(training=False),
                         noise_scheduler=da.DDIMScheduler(), prompt_table=prompts)
    batch = dict(uids=uids, outfits=torch.randint(0, ITEMS_STAGE, (BSZ, OLEN), generator=g),
                 category=[[int(c) for c in row] for row in torch.randint(0, CATES, (BSZ, OLEN), generator=g)], input_ids=None)
    seen = {}
    difashion_module.train_forward = lambda *a, **kw: seen.update(kw) or kw["latents"]            # the input stage alone
    gen = torch.Generator(device=dev).manual_seed(3)
    parent = lambda: model(batch, dataset, host_dict, dataset[0], 0.2, 0.3, 0.2, torch.float32, gen)
    cached = lambda: model(batch, store, table, None, 0.2, 0.3, 0.2, torch.float32, gen)
    with torch.no_grad():
        torch.manual_seed(5)
        parent()
        a = {k: seen[k].clone() for k in ("latents", "hist_latents", "null_latent")}
        torch.manual_seed(5)
        cached()
        b = {k: seen[k].clone() for k in ("latents", "hist_latents", "null_latent")}
        entry = dict(outfits=BSZ, items_per_outfit=OLEN, image_size=512, data_set="in-memory fp32 tensor, no JPEG decode, no transform",
                     store_items=len(store), store_bytes=store.nbytes,
                     # latents: equal bits only where the encoder gives the same moments in a batch of 32 as in the build batches of 16
                     latents_max_abs_diff_between_paths=float((a["latents"] - b["latents"]).abs().max()),
                     latents_max_abs=float(a["latents"].abs().max()),
                     null_latent_max_abs_diff_between_paths=float((a["null_latent"] - b["null_latent"]).abs().max()),
                     # history: the host dict averages with torch.mean on the CPU, the table sums in list order
                     hist_latents_max_abs_diff_between_paths=float((a["hist_latents"] - b["hist_latents"]).abs().max()))
        four = dataset[:4].to(dev)
        together = vae.encode(four).latent_dist.parameters
        singly = torch.cat([vae.encode(four[i:i + 1]).latent_dist.parameters for i in range(4)])
        entry["sd_vae_encode_batch_invariance"] = dict(config="the SD-size AutoencoderKL, 512 x 512 images, 4 together against one by one",
                                                       equal_bits=bool(torch.equal(together, singly)),
                                                       max_abs_diff=float((together - singly).abs().max()), max_abs_moment=float(together.abs().max()))
        entry["images_and_dict"] = timed(parent)
        entry["store_and_table"] = timed(cached)
    entry["speedup"] = round(entry["images_and_dict"]["ms"] / entry["store_and_table"]["ms"], 1)
    res["input_stage"] = entry
    del vae, store, dataset
    torch.cuda.empty_cache()


def device_copy(nbytes_moved):
    """torch's device-to-device copy that moves `nbytes_moved` in all (half read, half written)"""
    n = nbytes_moved // 8
    src, dst = torch.empty(n, dtype=torch.float32, device="cuda").normal_(), torch.empty(n, dtype=torch.float32, device="cuda")
    t = timed(lambda: dst.copy_(src))
    return dict(**t, gbps=round(nbytes_moved / (t["ms"] * 1e-3) / 1e9, 1))


def kernels(res):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(2)
    gc = torch.Generator().manual_seed(4)
    table = torch.randn(TABLE_ITEMS, 2 * E, generator=g, device=dev)
    store = da.ItemLatentStore(table, LATENT, 0.18215, 0.18215, True)
    entry = dict(table_items=TABLE_ITEMS, table_bytes=store.nbytes, row_bytes=E * 4, source="call time from device events (one launch a call)")
    for rows in (ROWS, BSZ * OLEN):
        ids = torch.randperm(TABLE_ITEMS, generator=gc)[:rows].to(dev)
        eps = torch.randn((rows,) + LATENT, generator=g, device=dev)
        distinct = torch.randperm(TABLE_ITEMS, generator=gc)[:rows * SEG_LEN].reshape(rows, SEG_LEN)
        raw = {0: {s: distinct[s].tolist() for s in range(rows)}}
        hist = da.HistoryTable(raw, store)
        null = store.null_latent()
        uids, cates = [0] * rows, list(range(rows))
        row_seg = torch.tensor(hist.segment_ids(uids, cates), dtype=torch.int32, device=dev)
        out = torch.empty((rows,) + LATENT, device=dev)

        def history_launch():
            _lib.call("dfh_history_rows", _lib.ptr(table), len(store), 2 * E, E, _lib.ptr(hist.seg_items), _lib.ptr(hist.seg_offsets),
                      _lib.ptr(row_seg), rows, _lib.ptr(null), store.scale, _lib.ptr(out), _lib.stream_ptr())

        moved = dict(gather_sample=rows * E * 4 * 4, gather_mode=rows * E * 4 * 2, history_rows=rows * E * 4 * (SEG_LEN + 1))
        calls = dict(gather_sample=lambda: store.sample(ids, eps=eps), gather_mode=lambda: store.modes(ids), history_rows=history_launch)
        sized = dict(rows=rows, history_segment_items=SEG_LEN)
        for name, fn in calls.items():
            t = timed(fn)
            sized[name] = dict(**t, bytes_moved=moved[name], gbps=round(moved[name] / (t["ms"] * 1e-3) / 1e9, 1))
            if rows == ROWS:
                sized[name]["torch_device_copy_of_the_same_bytes"] = device_copy(moved[name])
                sized[name]["fraction_of_the_copy_rate"] = round(sized[name]["gbps"] / sized[name]["torch_device_copy_of_the_same_bytes"]["gbps"], 3)
        entry["rows_%d" % rows] = sized
    res["kernels"] = entry


def batch_invariance(res):
    vae = da.AutoencoderKL(block_out_channels=(32, 64, 64, 64), sample_size=32).to("cuda")
    imgs = (torch.rand(5, 3, 32, 32, generator=torch.Generator().manual_seed(6)) * 2 - 1).to("cuda")
    together = vae.encode(imgs).latent_dist.parameters
    singly = torch.cat([vae.encode(imgs[i:i + 1]).latent_dist.parameters for i in range(5)])
    diff = float((together - singly).abs().max())
    res["vae_encode_batch_invariance"] = dict(config="block_out_channels (32, 64, 64, 64), 32 x 32 images, 5 together against one by one",
                                              equal_bits=bool(torch.equal(together, singly)), max_abs_diff=diff,
                                              max_abs_moment=float(together.abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "item_store_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    res = header(card=True)
    batch_invariance(res)
    kernels(res)
    input_stage(res)
    emit(res, a.out)


if __name__ == "__main__":
    main()
