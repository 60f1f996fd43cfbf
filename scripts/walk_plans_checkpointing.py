"""Prints what gradient checkpointing does to the training workspace, without a GPU (the dry plan only): the bytes of every region --
head (zero page, GroupNorm partials, split-K slabs), persistent activations, layer-internal gradient stack, recompute region -- for the
three modes of dfh_unet_set_checkpointing (0 off, 1 recompute, 2 recompute but keep the attention outputs), and from the same numbers
the largest batch of an SD-1.5 / SD-2-base training job that fits one 288 GB MI355X.

    python scripts/walk_plans_checkpointing.py > profiles/checkpointing_plans.txt

profiles/checkpointing_plans.txt is this tree's output (tests/test_checkpointing_cpu.py compares them line by line).

What "fits" counts, in bytes, for n parameters:
    weight arenas      arena16 + arena32 (packed bf16 / fp32 kernel layouts) + arena16t (transposed packs of the backward)
    gradient arenas    grad16 + grad32 (fp32, packed layouts)
    inference walk     dfh_unet_workspace_bytes at batch 1 (bound with the context; the training step does not run it)
    FusedAdamW state   flat_param + flat_grad + exp_avg + exp_avg_sq = 16 n (difashion_amd/training.py)
    workspace          dfh_unet_train_workspace_bytes(batch) of the mode
The VAE, the CLIP towers and the MutualEncoder of a DiFashion step are not counted: they are frozen or small."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from difashion_amd import _lib  # noqa: E402
from walk_plans import UNETS, unet_ctx  # noqa: E402

HBM_BYTES = 288 * 10**9
MODES = (0, 1, 2)
# tests/test_gpu_train.py LINEAR_CFG
UNETS = dict(UNETS, linear_proj=(16, (64, 128, 256, 256), 64, (2, 2, 4, 4), 1))
SHAPES = [("tiny", 3), ("tiny", 4), ("glue", 3), ("glue", 4), ("linear_proj", 3), ("linear_proj", 4),
          ("sd15", 32), ("sd2base", 32), ("sd15", 64), ("sd15", 128)]
FITS = ("sd15", "sd2base")


def regions(lib, h, batch):
    r = (C.c_size_t * 4)()
    _lib.call("dfh_unet_train_workspace_regions", h, batch, r)
    total = lib.dfh_unet_train_workspace_bytes(h, batch)
    assert total == sum(r) + 256
    return tuple(r), total


def largest_batch(lib, h, fixed):
    """largest B with fixed + workspace(B) <= HBM_BYTES (the workspace grows with B): doubling, then bisection"""
    fits = lambda b: fixed + lib.dfh_unet_train_workspace_bytes(h, b) <= HBM_BYTES
    lo, hi = 0, 1
    while fits(hi):
        lo, hi = hi, hi * 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


def main():
    lib = _lib.raw()
    ctxs = {}
    for name in dict.fromkeys(n for n, _ in SHAPES):
        ctxs[name] = unet_ctx(UNETS[name])
    print("# training workspace by region and checkpointing mode (bytes); total = head + persist + temp + recompute + 256")
    for name, b in SHAPES:
        h = ctxs[name]
        base = None
        for mode in MODES:
            _lib.call("dfh_unet_set_checkpointing", h, mode)
            (head, persist, temp, recomp), total = regions(lib, h, b)
            base = base or (persist, total)
            print(f"unet {name} B={b} mode={mode} head {head} persist {persist} temp {temp} recompute {recomp} total {total}"
                  f" persist/mode0 {persist / base[0]:.4f} total/mode0 {total / base[1]:.4f}")
        _lib.call("dfh_unet_set_checkpointing", h, 0)
    print(f"# largest training batch on one {HBM_BYTES // 10**9} GB device: fixed = weight arenas + gradient arenas + inference walk (B=1)"
          " + FusedAdamW state (16 bytes a parameter); fixed + workspace(batch) <= capacity")
    for name in FITS:
        h = ctxs[name]
        n = 0
        for i in range(lib.dfh_unet_num_params(h)):
            k = 1
            for d in range(lib.dfh_unet_param_ndim(h, i)):
                k *= lib.dfh_unet_param_dim(h, i, d)
            n += k
        arenas = lib.dfh_unet_arena16_bytes(h) + lib.dfh_unet_arena32_bytes(h) + lib.dfh_unet_arena16t_bytes(h)
        grads = lib.dfh_unet_grad16_bytes(h) + lib.dfh_unet_grad32_bytes(h)
        fixed = arenas + grads + lib.dfh_unet_workspace_bytes(h, 1) + 16 * n
        print(f"fits {name} parameters {n} weight_arenas {arenas} gradient_arenas {grads} adamw_state {16 * n} fixed {fixed}")
        for mode in MODES:
            _lib.call("dfh_unet_set_checkpointing", h, mode)
            b = largest_batch(lib, h, fixed)
            print(f"fits {name} mode={mode} largest_batch {b} workspace {lib.dfh_unet_train_workspace_bytes(h, b)}"
                  f" next_batch_workspace {lib.dfh_unet_train_workspace_bytes(h, b + 1)}")
    for h in ctxs.values():
        lib.dfh_unet_destroy(h)


if __name__ == "__main__":
    main()
