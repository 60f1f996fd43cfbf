"""GPU tier: the FID / Inception Score row on the MI355X.

  * parity: the rule and the factor of tests/test_gpu_eval_scores.py for the evaluation rows, FACTOR = 3.0: the HIP path, fp32 end to
    end, must sit within 3 x the restatement's own fp32 distance of the fp64 values -- per case and per tap on the pooled features
    (relative L2 over the 4 images x C values of a tap; nothing is pooled over cases), and on the classifier's probabilities.
  * the conv, prep, average-pool and head ops: the same 3 x rule against a live fp64 run on the CPU, the yardstick being torch's own
    fp32 run.  The statistics: relative L2 <= 1e-12 against numpy's fp64.
  * the max pools, prep's indices and pass-through, and every invariance: bit equality.
Every measured ratio is printed before it is asserted (profiles/inception_parity.txt holds one run's "inception parity" lines).

Measured on an MI355X (profiles/inception_parity.txt): taps 0.56 - 1.01 x the yardstick over the three cases (where the
image is resized both runs share the fp32 source index, which dominates: 0.98 - 1.01), probabilities 0.99 x, the conv op 0.35 - 0.85 x
for K = 27 ... 4032 under the compensated k-tiles, the statistics <= 1.2e-16.
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import difashion_amd as da
from difashion_amd import _lib
from tests import helpers_inception as H
from tests.gpu_util import DEV, nchw, nhwc, release_cached_gpu_memory

pytestmark = pytest.mark.gpu
FACTOR = 3.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL_MAX_S2, POOL_MAX_S1, POOL_AVG_INCL, POOL_AVG_EXCL = range(4)


def held(tag, dist):
    """dist: {output: (measured, yardstick)}; prints every pair, then asserts measured <= FACTOR x yardstick."""
    print(f"inception parity {tag}", " ".join(f"{k}: hip {e:.2e} ref_fp32 {r:.2e} ratio {e / r if r else float('inf'):.2f};" for k, (e, r) in dist.items()))
    for k, (e, r) in dist.items():
        assert e <= FACTOR * r, (tag, k, e, r)


@functools.lru_cache(maxsize=None)
def case_model(name, blocks=(0, 1, 2, 3), max_workspace_bytes=4 << 30):
    variant, params, _, _ = H.load_case(name)
    if variant == "fid":
        m = da.FIDInceptionV3(blocks, init_seed=None, max_workspace_bytes=max_workspace_bytes)
    else:
        m = da.InceptionV3(num_classes=H.CASES[name][3], init_seed=None, resize_input=True, normalize_input=True, tap_blocks=blocks,
                           max_workspace_bytes=max_workspace_bytes)
    m.load_state_dict(params)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def case_run(name):
    """-> ([four pooled taps [4, C] on the host], probs or None) of the fixture case on the HIP path."""
    m = case_model(name)
    x = H.case_inputs(name).to(DEV)
    if H.CASES[name][0] == "fid":
        taps, probs = [t.reshape(t.shape[0], -1).cpu() for t in m(x)], None
    else:
        taps = m.pooled_taps(x)
        taps, probs = [taps[b].cpu() for b in range(4)], m(x).cpu()
    torch.cuda.synchronize()
    return taps, probs


# ------------------------------------------------------------------ 1. the network against the fixtures
@pytest.mark.parametrize("name", list(H.CASES))
def test_pooled_features_hold_the_fp32_rule(name):
    fx = H.load_fixture("inception_" + name)
    taps, probs = case_run(name)
    held(f"{name} taps", {f"tap{b}": (H.rel(taps[b], fx[f"tap{b}_64"]), H.rel(fx[f"tap{b}_32"], fx[f"tap{b}_64"])) for b in range(4)})
    assert all(bool(torch.isfinite(t).all()) and t.shape == (H.IMAGES, H.BLOCK_DIMS[b]) for b, t in enumerate(taps))
    if probs is not None:
        held(f"{name} probs", {"probs": (H.rel(probs, fx["probs_64"]), H.rel(fx["probs_32"], fx["probs_64"]))})
        assert torch.argmax(probs, 1).tolist() == fx["labels"].tolist()
        label, _, _, _ = da.inception_rows(probs.to(DEV))
        assert label.cpu().tolist() == fx["labels"].tolist()
        feat = case_model(name).feature_extract(H.case_inputs(name).to(DEV)).cpu()
        assert torch.equal(feat, taps[3])


# ------------------------------------------------------------------ 2. the conv op
# (C_in, C_out, (KH, KW), stride, (padH, padW), H, W, ldc, offset)
CONV_CASES = [(3, 32, (3, 3), 2, (0, 0), 9, 11, 32, 0), (32, 64, (3, 3), 1, (1, 1), 5, 7, 64, 0), (64, 80, (1, 1), 1, (0, 0), 6, 5, 80, 0),
              (48, 64, (5, 5), 1, (2, 2), 4, 6, 64, 0), (160, 160, (1, 7), 1, (0, 3), 5, 6, 160, 0), (160, 192, (7, 1), 1, (3, 0), 6, 5, 192, 0),
              (288, 384, (3, 3), 2, (0, 0), 7, 9, 768, 0), (448, 384, (3, 3), 1, (1, 1), 8, 8, 384, 0), (2048, 320, (1, 1), 1, (0, 0), 3, 3, 2048, 0),
              (64, 32, (1, 1), 1, (0, 0), 6, 7, 256, 224), (96, 96, (3, 3), 2, (0, 0), 9, 9, 768, 384)]


def conv_op(x, w, bn, stride, pad, ldc, offset):
    """x [n, C_in, H, W] on the host -> the op's output tensor [n, OH, OW, ldc] (NaN outside the slice) on the host."""
    n, cin, Hh, Ww = x.shape
    cout, _, kh, kw = w.shape
    cin_pad = (cin + 3) // 4 * 4
    xd = torch.zeros((n, Hh, Ww, cin_pad), dtype=torch.float32, device=DEV)
    xd[..., :cin] = nhwc(x).to(DEV)
    oh, ow = (Hh + 2 * pad[0] - kh) // stride + 1, (Ww + 2 * pad[1] - kw) // stride + 1
    out = torch.full((n, oh, ow, ldc), float("nan"), dtype=torch.float32, device=DEV)
    packed = torch.empty((cout * (kh * kw * cin_pad + 2),), dtype=torch.float32, device=DEV)
    wd = w.contiguous().to(DEV)
    bnd = [t.contiguous().to(DEV) for t in bn]
    arr = (C.c_void_p * 4)(*[t.data_ptr() for t in bnd])
    _lib.call("dfh_incep_conv_bn_relu", _lib.ptr(xd), _lib.ptr(wd), cin, arr, _lib.ptr(packed), _lib.ptr(out), n, Hh, Ww, cin_pad, cout, kh, kw, stride,
              pad[0], pad[1], ldc, offset, _lib.stream_ptr())
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: f"{c[0]}to{c[1]}_k{c[2][0]}x{c[2][1]}_s{c[3]}_{c[5]}x{c[6]}_off{c[8]}")
def test_conv_bn_relu_op_against_fp64(case):
    cin, cout, k, stride, pad, Hh, Ww, ldc, offset = case
    n = 3
    g = torch.Generator().manual_seed(cin * 131 + cout)
    x = torch.randn((n, cin, Hh, Ww), generator=g)
    w = torch.randn((cout, cin, k[0], k[1]), generator=g) * (2.0 / (cin * k[0] * k[1])) ** 0.5
    bn = [0.75 + 0.5 * torch.rand(cout, generator=g), 0.1 * torch.randn(cout, generator=g), 0.2 * torch.randn(cout, generator=g),
          0.5 + torch.rand(cout, generator=g)]

    def ref(dt):
        y = F.conv2d(x.to(dt), w.to(dt), None, stride, pad)
        return F.relu(F.batch_norm(y, bn[2].to(dt), bn[3].to(dt), bn[0].to(dt), bn[1].to(dt), False, 0.0, 1e-3))

    r64, r32 = ref(torch.float64), ref(torch.float32)
    out = conv_op(x, w, bn, stride, pad, ldc, offset)
    got = nchw(out[..., offset:offset + cout])
    assert got.shape == r64.shape and 0.2 < float((r64 > 0).double().mean()) < 0.8
    held(f"conv {cin}->{cout} k{k} s{stride} p{pad} {Hh}x{Ww} slice {offset}/{ldc}", {"out": (H.rel(got, r64), H.rel(r32, r64))})
    outside = torch.cat([out[..., :offset].flatten(), out[..., offset + cout:].flatten()])
    assert bool(torch.isnan(outside).all()), "the op wrote outside its channel slice"
    assert bool(torch.isfinite(got).all())


# ------------------------------------------------------------------ 3. prep
def prep_op(x, resize, normalize, affine):
    n, _, Hh, Ww = x.shape
    oh, ow = (H.SIDE, H.SIDE) if resize else (Hh, Ww)
    out = torch.full((n, oh, ow, 4), float("nan"), dtype=torch.float32, device=DEV)
    xd = x.contiguous().to(DEV)
    _lib.call("dfh_incep_prep", _lib.ptr(xd), n, Hh, Ww, int(resize), int(normalize), int(affine), _lib.ptr(out), _lib.stream_ptr())
    torch.cuda.synchronize()
    out = out.cpu()
    assert bool((out[..., 3] == 0).all())
    return nchw(out[..., :3])


@pytest.mark.parametrize("Hh,Ww", [(75, 91), (320, 300), (299, 299), (1, 1)])
def test_prep_against_torch_interpolate(Hh, Ww):
    g = torch.Generator().manual_seed(Hh)
    x = torch.rand((2, 3, Hh, Ww), generator=g)
    # index-valued images: pixel (y, x) holds y, x and y * W + x.  The resize alone must give torch's fp32 bits, which it can only with
    # torch's i0 / i1 and weights at every output pixel
    yy = torch.arange(Hh, dtype=torch.float32).view(Hh, 1).expand(Hh, Ww)
    xx = torch.arange(Ww, dtype=torch.float32).view(1, Ww).expand(Hh, Ww)
    idx = torch.stack([yy, xx, yy * Ww + xx])[None].contiguous()
    want = F.interpolate(idx, size=(H.SIDE, H.SIDE), mode="bilinear", align_corners=False)
    got = prep_op(idx, True, False, False)
    assert torch.equal(got, want), f"index images differ from torch's at {int((got != want).sum())} values"
    for variant in ("fid", "tv"):
        r64, r32 = H.prep(x.double(), variant), H.prep(x, variant)
        got = prep_op(x, True, True, variant == "tv")
        e, r = H.rel(got, r64), H.rel(r32, r64)
        print(f"inception parity prep {variant} {Hh}x{Ww} hip {e:.2e} ref_fp32 {r:.2e}")
        assert e <= FACTOR * r or torch.equal(got, r32)                  # at 299 x 299 the resize is the identity and both distances may be 0
    # both flags off: the input passes through bit for bit
    assert torch.equal(prep_op(x, False, False, False), x)
    assert torch.equal(prep_op(x, False, True, False), 2 * x - 1)


# ------------------------------------------------------------------ 4. pools and the global mean
def pool_op(x, mode, ldc=None, offset=0):
    n, c, Hh, Ww = x.shape
    oh, ow = ((Hh - 3) // 2 + 1, (Ww - 3) // 2 + 1) if mode == POOL_MAX_S2 else (Hh, Ww)
    ldc = ldc or c
    out = torch.full((n, oh, ow, ldc), float("nan"), dtype=torch.float32, device=DEV)
    xd = nhwc(x).to(DEV)
    _lib.call("dfh_incep_pool", _lib.ptr(xd), _lib.ptr(out), mode, n, Hh, Ww, c, ldc, offset, _lib.stream_ptr())
    torch.cuda.synchronize()
    out = out.cpu()
    outside = torch.cat([out[..., :offset].flatten(), out[..., offset + c:].flatten()])
    assert bool(torch.isnan(outside).all())
    return nchw(out[..., offset:offset + c])


@pytest.mark.parametrize("Hh,Ww", [(7, 9), (8, 6)])
def test_pools_against_torch(Hh, Ww):
    g = torch.Generator().manual_seed(Hh * 10 + Ww)
    x = torch.randn((3, 24, Hh, Ww), generator=g)
    xn = x.clone()
    xn[0, 1, 0, 0] = xn[1, 5, Hh // 2, Ww // 2] = xn[2, 7, Hh - 1, Ww - 1] = float("nan")
    for t in (x, xn):
        for mode, ref in ((POOL_MAX_S2, F.max_pool2d(t, 3, 2)), (POOL_MAX_S1, F.max_pool2d(t, 3, 1, 1))):
            got = pool_op(t, mode, 40, 12)
            assert got.shape == ref.shape and torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got.nan_to_num(7.0), ref.nan_to_num(7.0)), mode
    dist = {}
    for mode, kw in ((POOL_AVG_INCL, {}), (POOL_AVG_EXCL, dict(count_include_pad=False))):
        r64, r32 = F.avg_pool2d(x.double(), 3, 1, 1, **kw), F.avg_pool2d(x, 3, 1, 1, **kw)
        got = pool_op(x, mode, 40, 16)
        dist[f"avg{mode}"] = (H.rel(got, r64), H.rel(r32, r64))
        border = lambda t: torch.cat([t[..., 0, :].flatten(), t[..., -1, :].flatten(), t[..., :, 0].flatten(), t[..., :, -1].flatten()])
        dist[f"avg{mode}_border"] = (H.rel(border(got), border(r64)), H.rel(border(r32), border(r64)))
    held(f"pools {Hh}x{Ww}", dist)


def test_global_mean_is_the_fp64_mean():
    g = torch.Generator().manual_seed(3)
    for n, hw, c in [(2, 73 * 73, 64), (3, 64, 2048), (2, 5, 100)]:
        x = torch.rand((n, hw, c), generator=g)
        out = torch.empty((n, c), dtype=torch.float32, device=DEV)
        xd = x.to(DEV)
        _lib.call("dfh_incep_global_mean", _lib.ptr(xd), _lib.ptr(out), n, hw, c, _lib.stream_ptr())
        torch.cuda.synchronize()
        # the sum runs in fp64 and is rounded once: the correctly rounded mean up to the fp64 sum's own error
        want = x.double().mean(1)
        assert float((out.cpu().double() - want).abs().max()) <= 2.0 ** -24 * float(want.abs().max())


# ------------------------------------------------------------------ 5. the statistics
@pytest.mark.parametrize("N,D", [(2, 64), (77, 192), (50, 2048)])
def test_statistics_against_numpy(N, D):
    g = torch.Generator().manual_seed(N + D)
    act = (torch.rand((N, D), generator=g) * torch.rand((1, D), generator=g) + 0.3 * torch.rand((1, D), generator=g)).contiguous()
    mu = torch.empty((D,), dtype=torch.float64, device=DEV)
    sigma = torch.empty((D, D), dtype=torch.float64, device=DEV)
    ad = act.to(DEV)
    _lib.call("dfh_incep_stats", _lib.ptr(ad), N, D, _lib.ptr(mu), _lib.ptr(sigma), _lib.stream_ptr())
    torch.cuda.synchronize()
    a64 = act.numpy().astype(np.float64)
    e_mu, e_sigma = H.rel(mu.cpu(), np.mean(a64, axis=0)), H.rel(sigma.cpu(), np.cov(a64, rowvar=False))
    print(f"inception parity stats N={N} D={D} mu {e_mu:.2e} sigma {e_sigma:.2e}")
    assert e_mu <= 1e-12 and e_sigma <= 1e-12
    assert torch.equal(sigma, sigma.T)
    with pytest.raises(_lib.DfhError, match="at least two rows"):
        _lib.call("dfh_incep_stats", _lib.ptr(ad), 1, D, _lib.ptr(mu), _lib.ptr(sigma), _lib.stream_ptr())


# ------------------------------------------------------------------ 6. the head and the score
def test_fc_softmax_op_against_fp64():
    g = torch.Generator().manual_seed(8)
    n, K, classes = 70, 2048, 50
    feat = torch.rand((n, K), generator=g)
    w, b = 0.1 * torch.randn((classes, K), generator=g), 0.1 * torch.randn((classes,), generator=g)
    logits = torch.empty((n, classes), dtype=torch.float32, device=DEV)
    probs = torch.empty((n, classes), dtype=torch.float32, device=DEV)
    fd, wd, bd = feat.to(DEV), w.to(DEV), b.to(DEV)
    _lib.call("dfh_incep_fc_softmax", _lib.ptr(fd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(logits), _lib.ptr(probs), n, K, classes, _lib.stream_ptr())
    torch.cuda.synchronize()
    l64, l32 = F.linear(feat.double(), w.double(), b.double()), F.linear(feat, w, b)
    p64, p32 = torch.softmax(l64, 1), torch.softmax(l32, 1)
    held("fc + softmax", {"logits": (H.rel(logits.cpu(), l64), H.rel(l32, l64)), "probs": (H.rel(probs.cpu(), p64), H.rel(p32, p64))})


@pytest.mark.parametrize("splits", [1, 2])
def test_inception_score_equals_the_restatement_on_the_hip_probabilities(splits):
    name = "tv_down_320x300"
    m = case_model(name, (3,))
    x = H.case_inputs(name)
    # 12 images, batches of 5 (the batch loop runs too).  The second half is dark noise, which the stand-in classifier is far surer of
    # (restatement: mean entropy 2.2 against 0.3): with two splits the standard deviations are differences of unlike numbers, so the
    # 1e-6 holds them too -- two like splits would cancel to the fp32 rounding of the sums
    dark = 0.15 * torch.rand((4, 3, 320, 300), generator=torch.Generator().manual_seed(11))
    data = torch.cat([x, x.roll(1, 3)[:2], dark, dark.flip(3)[:2]]).to(DEV)
    cate = torch.tensor([22, 22, 22, 0, 0, 0, 22, 22, 12, 12, 5, 5])
    got = da.inception_score_given_data(m, data, cate.to(DEV), batch_size=5, num_splits=splits)
    probs = torch.cat([m(data[i:i + 5]) for i in range(0, 12, 5)]).cpu()
    want = H.inception_score(probs, cate, splits)
    print(f"inception parity score splits={splits} hip {got} restatement {want}")
    assert got[0] == want[0]
    for a, b in zip(got[1:], want[1:]):
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-6 * abs(b), (got, want)
    assert np.isnan(got[2]) == (splits == 1)
    # a NaN row and ties: torch.argmax's order
    p = torch.tensor([[0.2, 0.5, 0.5, 0.1], [0.1, float("nan"), 0.9, float("nan")], [0.25, 0.25, 0.25, 0.25]]).to(DEV)
    assert da.inception_rows(p)[0].cpu().tolist() == torch.argmax(p.cpu(), 1).tolist() == [1, 1, 0]


# ------------------------------------------------------------------ 7. FID plumbing
def test_fid_given_data_is_the_frechet_distance_of_the_statistics():
    g = torch.Generator().manual_seed(4)
    gen = torch.rand((80, 3, 35, 35), generator=g).to(DEV)
    grd = (0.7 * torch.rand((80, 3, 35, 35), generator=g) + 0.2).to(DEV)
    m = da.FIDInceptionV3((0,), init_seed=3).to(DEV)
    fid = da.fid_given_data(gen, grd, batch_size=50, dims=64, model=m)
    m1, s1 = da.activation_statistics(m, gen, 50, 64)
    m2, s2 = da.activation_statistics(m, grd, 50, 64)
    assert m1.dtype == s1.dtype == torch.float64 and m1.device.type == "cuda" and s1.shape == (64, 64)
    assert fid == da.frechet_distance(m1, s1, m2, s2) and fid > 0
    same = da.fid_given_data(gen, gen, batch_size=50, dims=64, model=m)
    # sqrtm(s1 s1) = s1 up to the conditioning of s1 x 2^-53 (64 correlated features of 80 images: allow a condition of 1e10)
    assert abs(same) <= 1e-6 * 2 * float(s1.trace())
    # the images as a list of per-image tensors, another batch size: the same statistics, bit for bit
    m1b, s1b = da.activation_statistics(m, list(gen), 33, 64)
    assert torch.equal(m1, m1b) and torch.equal(s1, s1b)


# ------------------------------------------------------------------ 8. invariances, bitwise
def test_chunking_rerun_and_output_blocks_do_not_change_a_bit():
    name = "fid_up_75x91"
    taps, _ = case_run(name)
    x = H.case_inputs(name).to(DEV)
    m = case_model(name)
    again = [t.reshape(4, -1).cpu() for t in m(x)]
    assert all(torch.equal(a, b) for a, b in zip(again, taps))
    only3 = case_model(name, (3,))
    assert torch.equal(only3(x)[0].reshape(4, -1).cpu(), taps[3])
    # one image a call, and another batch order
    need = _lib.raw().dfh_incep_workspace_bytes(only3._context(), 1, 75, 91)
    small = case_model(name, (3,), need)
    assert small.images_per_call(75, 91) == 1
    assert torch.equal(small(x)[0].reshape(4, -1).cpu(), taps[3])
    assert torch.equal(only3(x.flip(0))[0].reshape(4, -1).cpu(), taps[3].flip(0))
    # the packed copy follows the masters
    m2 = da.FIDInceptionV3((0,), init_seed=1).to(DEV)
    before = m2(x)[0].clone()
    with torch.no_grad():
        m2.Conv2d_2b_3x3.bn.bias.add_(0.5)
    assert not torch.equal(before, m2(x)[0])


def test_fp16_storage_library_gives_the_same_bits():
    """The row is fp32 only: libdifashion_hip_f16.so, in a process of its own, gives the bits of the bf16 build."""
    name = "fid_up_75x91"
    taps, _ = case_run(name)
    release_cached_gpu_memory()
    env = dict(os.environ, DFH_STORAGE="fp16")
    env.pop("DFH_LIB", None)
    r = subprocess.run([sys.executable, "-m", "tests.inception_fp16_child", name], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("INCEPTION_FP16_RESULT ")]
    assert line, r.stdout[-2000:]
    res = json.loads(line[-1][len("INCEPTION_FP16_RESULT "):])
    assert res["storage"] == "fp16" and "storage=fp16" in res["build_info"]
    for b in range(4):
        assert res["taps"][b] == taps[b].flatten().view(torch.int32).tolist(), b
