"""Gradient checkpointing of the training walk (dfh_unet_set_checkpointing; UNet2DConditionModel.enable_gradient_checkpointing): the
backward runs each resnet / transformer layer's forward launches again, into one recompute region, and must produce the gradients of
the default walk -- the same kernels on the same operands, so bit for bit wherever the default walk is itself reproducible (every
matrix gradient, the output and d_sample); vector gradients (biases, norm scales) are summed with float atomics in every mode and are
held to the project's bound for those, rtol 1e-5 (test_gpu_train.py, the side-stream test)."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from oracle import unet_ref
from tests.gpu_util import DEV
from tests.helpers import GLUE_CFG
from tests.test_gpu_train import LINEAR_CFG
from tests.test_gpu_unet import hip_unet, inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = {"tiny": unet_ref.TINY, "glue": GLUE_CFG, "linear_proj": LINEAR_CFG}


def set_mode(m, mode):
    if mode:
        m.enable_gradient_checkpointing(keep_attention=mode == 2)
    else:
        m.disable_gradient_checkpointing()
    return m


def step(m, x, t, e, dout, need_dx=True):
    """one training forward + backward from cleared gradients -> (output, d_sample or None, {name: grad})"""
    for p in m.parameters():
        p.grad = None
    xd = x.clone().requires_grad_(need_dx)
    out = m(xd, t, e).sample
    out.backward(dout)
    torch.cuda.synchronize()
    return out.detach().clone(), (xd.grad.clone() if need_dx else None), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def assert_same_gradients(got, ref, what):
    assert set(got) == set(ref)
    mats = 0
    for k, r in ref.items():
        if r.ndim >= 2:
            assert torch.equal(got[k], r), (what, k, float((got[k] - r).abs().max()))
            mats += 1
        else:
            torch.testing.assert_close(got[k], r, rtol=1e-5, atol=1e-6 * float(r.abs().max() + 1e-30), msg=f"{what} {k}")
    return mats


def case(name, B=3):
    cfg = CFGS[name]
    params = unet_ref.init_params(cfg, seed=3, w_std=0.05, affine_jitter=0.1)
    x, e = inputs(cfg, B, 11)
    t = torch.tensor([7, 500, 981, 130][:B], device=DEV)
    dout = torch.randn(B, cfg.out_channels, cfg.sample_size, cfg.sample_size, generator=torch.Generator().manual_seed(5)).to(DEV)
    return cfg, params, x.to(DEV), t, e.to(DEV), dout


_MODE0 = {}


def mode0(name):
    """the default walk's step of a config: computed once, shared, never modified"""
    if name not in _MODE0:
        cfg, params, x, t, e, dout = case(name)
        m = hip_unet(cfg, params, max_batch=3).train()
        _MODE0[name] = step(m, x, t, e, dout) + (m._train_buffers[3].numel(),)
    return _MODE0[name]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", list(CFGS))
def test_gradients_equal_those_of_the_default_walk(name, mode):
    ref_out, ref_dx, ref_g, ref_ws = mode0(name)
    cfg, params, x, t, e, dout = case(name)
    m = set_mode(hip_unet(cfg, params, max_batch=3).train(), mode)
    out, dx, g = step(m, x, t, e, dout)
    assert _lib.raw().dfh_unet_checkpointing(m._ctx) == mode and m._train_buffers[3].numel() < ref_ws
    assert torch.equal(out, ref_out) and torch.equal(dx, ref_dx)
    assert float(ref_dx.abs().max()) > 0 and sum(float(v.abs().max()) > 0 for v in ref_g.values()) > 100
    assert assert_same_gradients(g, ref_g, f"{name} mode {mode}") > 100


@pytest.mark.parametrize("need_dx", [True, False], ids=["d_sample", "no_d_sample"])
def test_two_steps_on_one_model_give_the_same_bits(need_dx):
    """the recompute region, the gradient states and the tape are re-used from step to step; one parameter is frozen"""
    cfg, params, x, t, e, dout = case("tiny")
    m = set_mode(hip_unet(cfg, params, max_batch=3).train(), 1)
    m.get_parameter("mid_block.attentions.0.proj_in.weight").requires_grad_(False)
    first = step(m, x, t, e, dout, need_dx)
    second = step(m, x, t, e, dout, need_dx)
    assert torch.equal(first[0], second[0]) and len(first[2]) == len(list(m.parameters())) - 1
    if need_dx:
        assert torch.equal(first[1], second[1]) and torch.equal(first[1], mode0("tiny")[1])
    else:
        assert first[1] is None
    assert_same_gradients(second[2], first[2], "second step")
    ref = {k: v for k, v in mode0("tiny")[2].items() if k in first[2]}
    assert_same_gradients(first[2], ref, "against the default walk")


def test_side_stream_reads_of_recomputed_tensors_are_ordered(tmp_path):
    """Every weight-gradient launch on the side stream (DFH_TRAIN_SIDE_MIN_FLOP=0), modes 0 / 1 / 2, twice each, in one child process:
    the side stream reads tensors the recompute wrote, and the next layer's recompute overwrites them -- a missing join shows up as a
    matrix gradient that differs between modes or repeats."""
    from tests.gpu_util import release_cached_gpu_memory
    release_cached_gpu_memory()
    out = tmp_path / "grads.pt"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checkpointing_child.py"), str(out)],
                       env={**os.environ, "DFH_TRAIN_SIDE_MIN_FLOP": "0"}, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = torch.load(out)
    assert sorted(got) == [(mode, rep) for mode in (0, 1, 2) for rep in (0, 1)]
    mats = sum(assert_same_gradients(g, got[(0, 0)], f"mode {key[0]} repeat {key[1]}") for key, g in got.items())
    assert mats > 6 * 100


def test_segmented_backward_in_mode_1_equals_the_monolithic_default():
    """dfh_unet_backward_begin / _next / _finish (the data-parallel exchange's pieces) with the recompute in front of every entry: the ranges
    are disjoint, bucket-aligned and inside the arena, and the master gradients equal those of dfh_unet_backward in mode 0 (the bounds of
    test_segmented_backward_equals_the_monolithic_one)."""
    cfg = unet_ref.TINY
    params = unet_ref.init_params(cfg, seed=3)
    x, e = inputs(cfg, 4, 9)
    grads = []
    for segmented in (False, True):
        m = set_mode(hip_unet(cfg, params, max_batch=4).train(), 1 if segmented else 0)
        out = m(x.to(DEV), torch.tensor([7, 100, 500, 900], device=DEV), e.to(DEV)).sample
        dout = torch.ones_like(out) * 0.01
        if not segmented:
            out.backward(dout)
        else:
            plist = m.grad_views()
            arr = (C.c_void_p * len(plist))(*[p.grad.data_ptr() for p in plist])
            sp = _lib.stream_ptr()
            n = _lib.call_count("dfh_unet_backward_begin", m._ctx, _lib.ptr(dout.contiguous().float()), None, 4096, sp)
            assert n > 10
            lo, hi, seen = C.c_size_t(0), C.c_size_t(0), []
            while True:
                rc = _lib.raw().dfh_unet_backward_next(m._ctx, C.byref(lo), C.byref(hi), sp)
                assert rc >= 0, _lib.last_error()
                if rc == 0:
                    break
                seen.append((lo.value, hi.value))
            _lib.call("dfh_unet_backward_finish", m._ctx, arr, len(plist), 1, sp)
            seen.sort()
            assert len(seen) > 3 and all(a[1] <= b[0] for a, b in zip(seen, seen[1:])) and all(h > l and l % 4096 == 0 for l, h in seen)
            total = m._train_buffers[1].numel() // 4
            assert seen[-1][1] <= total
        torch.cuda.synchronize()
        grads.append({n_: p.grad.clone() for n_, p in m.named_parameters()})
    for k in grads[0]:
        torch.testing.assert_close(grads[1][k], grads[0][k], rtol=1e-5, atol=1e-7, msg=k)


def test_the_mode_changes_between_steps_but_not_inside_one():
    ref_out, ref_dx, ref_g, ref_ws = mode0("tiny")
    cfg, params, x, t, e, dout = case("tiny")
    m = hip_unet(cfg, params, max_batch=3).train()
    sizes = {}
    for mode in (1, 0, 2, 1):                       # shrink, grow, shrink, shrink
        set_mode(m, mode)
        assert m._train_buffers is None             # dropped: the next training forward binds the workspace of the new mode
        out, dx, g = step(m, x, t, e, dout)
        assert torch.equal(out, ref_out) and torch.equal(dx, ref_dx)
        assert_same_gradients(g, ref_g, f"after switching to mode {mode}")
        sizes[mode] = m._train_buffers[3].numel()
        assert sizes[mode] == _lib.raw().dfh_unet_train_workspace_bytes(m._ctx, 3)
    assert sizes[1] < sizes[2] < sizes[0] == ref_ws
    # between a training forward and its backward
    for p in m.parameters():
        p.grad = None
    xd = x.clone().requires_grad_(True)
    out = m(xd, t, e).sample
    ws = m._train_buffers[3]
    with pytest.raises(da.DfhError, match="between dfh_unet_forward_train and its backward"):
        m.enable_gradient_checkpointing(keep_attention=True)
    with pytest.raises(da.DfhError, match="between dfh_unet_forward_train and its backward"):
        m.disable_gradient_checkpointing()
    assert _lib.raw().dfh_unet_set_checkpointing(m._ctx, 0) != 0 and b"between dfh_unet_forward_train" in _lib.raw().dfh_last_error()
    assert m._ckpt_mode == 1 and m.is_gradient_checkpointing and m._train_buffers[3] is ws and _lib.raw().dfh_unet_checkpointing(m._ctx) == 1
    out.backward(dout)                              # the refused calls changed nothing: the step in flight finishes ...
    torch.cuda.synchronize()
    assert torch.equal(xd.grad, ref_dx)
    assert_same_gradients({k: p.grad for k, p in m.named_parameters()}, ref_g, "the step in flight")
    set_mode(m, 2)                                  # ... and now the switch is taken, and the following step runs
    out, dx, g = step(m, x, t, e, dout)
    assert torch.equal(out, ref_out) and torch.equal(dx, ref_dx) and m._train_buffers[3].numel() == sizes[2]
    assert_same_gradients(g, ref_g, "the following step")
