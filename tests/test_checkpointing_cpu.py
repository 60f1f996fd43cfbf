"""No GPU: gradient checkpointing of the training walk as far as the host decides it -- the mode of a context (dfh_unet_set_checkpointing /
dfh_unet_checkpointing), what it does to the planned training workspace, the recorded plans of profiles/checkpointing_plans.txt, and the
Python switch of UNet2DConditionModel.  The gradients themselves: tests/test_gpu_checkpointing.py."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import difashion_amd as da
from difashion_amd import _lib
from oracle import unet_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import walk_plans  # noqa: E402


@pytest.fixture()
def ctx():
    made = []

    def make(name):
        made.append(walk_plans.unet_ctx(walk_plans.UNETS[name]))
        return made[-1]
    yield make
    for h in made:
        _lib.raw().dfh_unet_destroy(h)


def test_a_fresh_context_is_in_mode_0_and_bad_modes_are_refused(ctx):
    lib, h = _lib.raw(), ctx("tiny")
    assert lib.dfh_unet_checkpointing(h) == 0
    before = lib.dfh_unet_train_workspace_bytes(h, 3)
    _lib.call("dfh_unet_set_checkpointing", h, 0)
    assert lib.dfh_unet_checkpointing(h) == 0 and lib.dfh_unet_train_workspace_bytes(h, 3) == before > 0
    for bad in (3, -1):
        assert lib.dfh_unet_set_checkpointing(h, bad) != 0
        assert b"checkpointing mode must be 0" in lib.dfh_last_error()
        with pytest.raises(_lib.DfhError, match="checkpointing mode"):
            _lib.call("dfh_unet_set_checkpointing", h, bad)
        assert lib.dfh_unet_checkpointing(h) == 0 and lib.dfh_unet_train_workspace_bytes(h, 3) == before
    for mode in (1, 2, 0):
        _lib.call("dfh_unet_set_checkpointing", h, mode)
        assert lib.dfh_unet_checkpointing(h) == mode
    assert lib.dfh_unet_train_workspace_bytes(h, 3) == before          # and back: mode 0 plans what it planned


@pytest.mark.parametrize("name,batch", [("tiny", 3), ("sd15", 32), ("sd2base", 32)])
def test_workspace_bytes_are_ordered_mode1_mode2_mode0(ctx, name, batch):
    lib, h = _lib.raw(), ctx(name)
    total, regions = {}, {}
    for mode in (0, 1, 2):
        _lib.call("dfh_unet_set_checkpointing", h, mode)
        total[mode] = lib.dfh_unet_train_workspace_bytes(h, batch)
        r = (C.c_size_t * 4)()
        _lib.call("dfh_unet_train_workspace_regions", h, batch, r)
        regions[mode] = tuple(r)
        assert sum(r) + 256 == total[mode]
    assert total[1] < total[2] < total[0], total
    head, persist, temp, recomp = zip(*(regions[m] for m in (0, 1, 2)))
    assert head[0] == head[1] == head[2] and temp[0] == temp[1] == temp[2]           # slabs and the gradient stack are not touched
    assert recomp[0] == 0 and 0 < recomp[2] < recomp[1]                              # mode 2 moves the attention outputs out of the region
    assert persist[1] < persist[2] < persist[0]
    # the region holds one layer, the persistent part what all layers kept: together still under half of what mode 0 keeps
    assert persist[1] + recomp[1] < persist[0] // 2


def test_plans_equal_the_recorded_text():
    env = {k: v for k, v in os.environ.items() if not k.startswith("DFH_")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "walk_plans_checkpointing.py")], capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    recorded = open(os.path.join(ROOT, "profiles", "checkpointing_plans.txt")).read().splitlines()
    printed = r.stdout.splitlines()
    assert len(printed) == len(recorded) >= 30 + 8
    differ = [(i, a, b) for i, (a, b) in enumerate(zip(printed, recorded)) if a != b]
    assert not differ, f"{len(differ)} lines differ from profiles/checkpointing_plans.txt, the first: {differ[0]}"
    # the mode-0 lines are the training workspace the default plans record (profiles/walk_common_plans.txt pins those byte counts)
    plans = open(os.path.join(ROOT, "profiles", "walk_common_plans.txt")).read()
    line = next(l for l in printed if l.startswith("unet tiny B=4 mode=0 "))
    assert f"train_workspace_bytes B=4 {line.split(' total ')[1].split()[0]}\n" in plans


def test_python_switch_records_the_mode():
    cfg = unet_ref.TINY
    m = da.UNet2DConditionModel(sample_size=cfg.sample_size, in_channels=cfg.in_channels, block_out_channels=cfg.block_out_channels,
                                cross_attention_dim=cfg.cross_attention_dim, attention_head_dim=cfg.num_heads, init_seed=None)
    assert m.is_gradient_checkpointing is False and m._ckpt_mode == 0
    assert m.enable_gradient_checkpointing() is None
    assert m.is_gradient_checkpointing is True and m._ckpt_mode == 1
    assert m.enable_gradient_checkpointing(keep_attention=True) is None
    assert m.is_gradient_checkpointing is True and m._ckpt_mode == 2
    assert m.disable_gradient_checkpointing() is None
    assert m.is_gradient_checkpointing is False and m._ckpt_mode == 0
    assert m._ctx is None and m._train_buffers is None               # only recorded: nothing was created or bound for it
