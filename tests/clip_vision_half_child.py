"""The measurements of tests/test_gpu_clip_vision_half.py, in the storage format the process runs (a process holds one): called in
process for bf16, and as a child under ``DFH_STORAGE=fp16``, which prints one ``CLIPVH_RESULT {json}`` line.

    DFH_STORAGE=fp16 python -m tests.clip_vision_half_child

Op-level bounds (the reference is fp64 torch on the SAME 16-bit-rounded operands, so operand rounding is not part of them).  u16 is the
unit roundoff of the storage format (bf16: 2^-8, fp16: 2^-11), u32 = 2^-24.

GEMM  out = round16(act(sum_k a_k w_k + bias) + resid):
  * the products of two 16-bit numbers are exact in fp32; a sum of K + 1 fp32 terms in ANY order is off by at most
    (K + 1) u32 S with S = sum_k |a_k w_k| + |bias| (Higham, Accuracy and Stability, eq. 4.4, first order; the 1.01 below covers the rest);
  * the activation runs in fp32 on that value: both have a derivative of at most 1.13, gelu's polynomial erfc is within 5.5e-7
    absolute (dfh_common.h), the hardware exp2 / rcp of quick_gelu within a few ulp: 1e-6 + 2^-20 |pre| covers either;
  * the residual add is one more fp32 rounding: u32 (|act| + |resid|), inside the 2^-20 term;
  * the 16-bit store rounds to nearest: u16 |want| (+ half a subnormal step of fp16, 2^-25; 2^-24 is used).
  bound[m][n] = u16 |want| + 1.01 (1.13 (K + 1) u32 S + 1e-6 + 2^-20 (|pre| + |resid|)) + 2^-24.

Attention  O[q][:] = sum_j p_j v_j / sum_j p_j,  p_j = exp(scale q.k_j - m):
  * the scores are fp32 sums of exact products: error at most (d + 2) u32 smax, smax = scale max_j sum_c |q_c k_jc|;
  * every probability is ROUNDED to the storage format before it multiplies V (it is an MFMA operand): relative error u16; the
    32x32x16 kernel also rounds the pre-scaled Q to the storage format, which moves a score by at most u16 smax and its
    probability by the same relative amount (first order).  eps_p = u16 (1 + smax [x32 only]) + 4 (d + 2) u32 smax + 8 u32;
  * numerator and denominator each carry eps_p (worst case: no cancellation) and an fp32 accumulation error of Nk u32:
    |O~ - O| <= 1.05 (2 eps_p + 4 Nk u32) A,  A[q][c] = sum_j softmax_j |v_jc|  (the same average over |V|);
  * an fp16 probability below 2^-14 is subnormal and rounds with an ABSOLUTE error of at most 2^-25.  The denominator is at least 1/2:
    the running offset m is set from the first tile's maximum (rounded up to an integer in the 32x32x16 kernel) and is only ever
    raised to a later tile's maximum, so the largest probability under the final offset is at least 1/2.  Numerator and denominator
    together: at most 2 Nk 2^-25 max|v| / (1/2) = Nk 2^-23 max|v|;
  * the store: u16 |want|.
"""
import ctypes as C
import json

import numpy as np
import torch

from tests.helpers_clip_half import FACTOR, GUARD, _bands_untouched, _guarded, u16  # noqa: F401

ATTENTION_CASES = [(2, 3, 64, 197), (2, 3, 80, 257), (2, 2, 64, 50), (1, 2, 80, 129)]      # (B, H, d, Nq = Nk)
GEMM_ROWS = (50, 257, 771)
GEMM_NK = (320, 192)               # N: two column tiles of 160; K: three 64-deep k-steps, LEAN


def hip_model(cfg, params, dtype):
    import difashion_amd as da
    m = da.CLIPVisionModelWithProjection(**cfg.kwargs(), init_seed=None, torch_dtype=dtype)
    m.load_state_dict(params)
    return m.to("cuda").eval().requires_grad_(False)


def parity(name):
    """One 16-bit encode of a case -> {output: (hip distance from fp64, the real class's)}, the census and the structural facts."""
    from difashion_amd import _lib
    from tests.helpers_clip_vision import checksum, rel
    from tests.helpers_clip_vision_half import YARDSTICKS, case_inputs, load_fixture, max_one_minus_cos, output_keys, yardstick
    fmt, sd = _lib.storage(), _lib.storage_dtype()
    cfg, params, pixels = case_inputs(name)
    fx, ys = load_fixture(name), dict(np.load(YARDSTICKS))
    ok = bool(np.allclose(fx["checksum"], checksum(params, pixels), rtol=1e-12) and np.allclose(ys[f"{name}/checksum"], fx["checksum"], rtol=1e-12))
    m = hip_model(cfg, params, sd)
    del params
    _lib.census_reset()
    out = m(pixels.to("cuda"), output_hidden_states=True)
    torch.cuda.synchronize()
    census = _lib.census()
    B, T, D, L = pixels.shape[0], cfg.num_tokens, cfg.hidden_size, cfg.num_hidden_layers
    tensors = (out.image_embeds, out.pooler_output, out.last_hidden_state) + tuple(out.hidden_states)
    facts = {
        "checksum": ok,
        "shapes": out.last_hidden_state.shape == (B, T, D) and out.pooler_output.shape == (B, D) and out.image_embeds.shape == (B, cfg.projection_dim)
                  and len(out.hidden_states) == L + 1,
        "fp32_outputs": all(t.dtype == torch.float32 and t.device.type == "cuda" for t in tensors),
        "finite": all(bool(torch.isfinite(t).all()) for t in tensors),
        # last_hidden_state and the taps are exact upcasts of the 16-bit stream
        "exact_upcasts": all(torch.equal(t.to(sd).float(), t) for t in (out.last_hidden_state,) + tuple(out.hidden_states)),
        "last_is_last_tap": torch.equal(out.hidden_states[-1], out.last_hidden_state),
        "encode_image": torch.equal(m.encode_image(pixels.to("cuda")), out.image_embeds),
        "compute_dtype_pixels": True,
    }
    again = m(pixels.to("cuda").to(sd).float(), output_hidden_states=True)       # pixels that are exact in the compute dtype ...
    in16 = m(pixels.to("cuda").to(sd), output_hidden_states=True)               # ... give the same bits when passed in it
    facts["compute_dtype_pixels"] = all(torch.equal(a, b) for a, b in zip(again.to_tuple()[:2] + again.hidden_states, in16.to_tuple()[:2] + in16.hidden_states))
    rows = torch.from_numpy(fx["rows"]).long()
    got = {"image_embeds": out.image_embeds.cpu(), "pooler_output": out.pooler_output.cpu(), "last_hidden_state": out.last_hidden_state.cpu()[:, rows]}
    for t in fx["taps"]:
        got[f"hidden_{int(t)}"] = out.hidden_states[int(t)].cpu()[:, rows]
    assert sorted(got) == sorted(output_keys(fx))
    dist = {k: (rel(got[k], torch.from_numpy(fx[k])), yardstick(ys, name, fmt, k)) for k in output_keys(fx)}
    dist["cos"] = (max_one_minus_cos(got["image_embeds"], torch.from_numpy(fx["image_embeds"])), yardstick(ys, name, fmt, "cos"))
    print(f"clipvh parity {name} {fmt} " + " ".join(f"{k}: hip {e:.2e} real_{fmt} {r:.2e} ratio {e / r:.2f};" for k, (e, r) in dist.items()), flush=True)
    return {"dist": dist, "census": {k: census[k] for k in ("attention_16", "attention_x32", "clipv_attention", "clipv_embed", "layernorm", "splitk_reduce")
                                     if k in census}, "layers": L, "facts": {k: bool(v) for k, v in facts.items()}}


def attention_check(B, H, d, N):
    """dfh_attention at Nq = Nk = N against fp64 torch on the same rounded operands -> facts about bound, guard bands and reruns."""
    from difashion_amd import _lib
    sd, u, u32 = _lib.storage_dtype(), u16(), 2.0 ** -24
    g = torch.Generator().manual_seed(7000 + 10 * N + d)
    q = (torch.randn(B, N, H * d, generator=g) * 1.5).to(sd)                    # peaked, not one-hot, softmaxes
    k, v = torch.randn(B, N, H * d, generator=g).to(sd), torch.randn(B, N, H * d, generator=g).to(sd)
    ldvt, scale = (N + 7) // 8 * 8, d ** -0.5
    vt = torch.full((B, H * d, ldvt), float("nan"), dtype=sd)                    # the padding keys of every V^T row hold NaN
    vt[:, :, :N] = v.transpose(1, 2)
    split = lambda t: t.double().reshape(B, N, H, d).transpose(1, 2)            # [B][H][N][d]
    q64, k64, v64 = split(q), split(k), split(v)
    p = torch.softmax(q64 @ k64.transpose(-1, -2) * scale, dim=-1)
    want = (p @ v64).transpose(1, 2).reshape(B, N, H * d)
    A = (p @ v64.abs()).transpose(1, 2).reshape(B, N, H * d)
    smax = (scale * (q64.abs() @ k64.abs().transpose(-1, -2)).amax(-1)).transpose(1, 2)      # [B][N][H]
    smax = smax.unsqueeze(-1).expand(B, N, H, d).reshape(B, N, H * d)
    sentinel = -1234.0
    dq, dk, dvt = q.cuda(), k.cuda(), vt.cuda()
    res = {}
    outs = []
    for _ in range(2):
        buf, o = _guarded((B, N, H * d), sd, sentinel)
        _lib.census_reset()
        _lib.call("dfh_attention", _lib.ptr(dq), H * d, _lib.ptr(dk), H * d, _lib.ptr(dvt), ldvt, _lib.ptr(o), H * d, B, H, d, N, N, scale,
                  _lib.stream_ptr())
        torch.cuda.synchronize()
        res["bands_untouched"] = _bands_untouched(buf, sentinel) and res.get("bands_untouched", True)
        outs.append(o.clone())
    x32 = _lib.census()["attention_x32"] == 1
    eps_p = u * (1.0 + (smax if x32 else 0.0)) + 4.0 * (d + 2) * u32 * smax + 8.0 * u32
    bound = u * want.abs() + 1.05 * (2.0 * eps_p + 4.0 * N * u32) * A + N * 2.0 ** -23 * float(v64.abs().max()) + 2.0 ** -24
    err = (outs[0].cpu().double() - want).abs()
    res.update(x32=bool(x32), finite=bool(torch.isfinite(outs[0]).all()), rerun_identical=torch.equal(outs[0], outs[1]),
               worst_ratio=float((err / bound).max()), rel_l2=float(err.norm() / want.norm()))
    print(f"clipvh attention {_lib.storage()} B={B} H={H} d={d} N={N} x32={int(x32)}: max err/bound {res['worst_ratio']:.3f} rel L2 {res['rel_l2']:.2e}", flush=True)
    return res


def gemm_check(M, act, with_resid):
    """dfh_gemm with bias and one of the two new activations (5 gelu, 6 quick_gelu) against fp64 torch on the same rounded operands."""
    from difashion_amd import _lib
    from tests.gpu_util import gemm_desc
    sd, u, u32 = _lib.storage_dtype(), u16(), 2.0 ** -24
    N, K = GEMM_NK
    g = torch.Generator().manual_seed(9000 + 10 * M + act)
    a = torch.randn(M, K, generator=g).to(sd)
    w = (torch.randn(N, K, generator=g) * K ** -0.5 * 1.5).to(sd)
    bias = torch.randn(N, generator=g) * 0.3
    resid = torch.randn(M, N, generator=g).to(sd) if with_resid else None
    pre = a.double() @ w.double().T + bias.double()
    S = a.double().abs() @ w.double().abs().T + bias.double().abs()
    actd = torch.nn.functional.gelu(pre) if act == 5 else pre * torch.sigmoid(1.702 * pre)
    want = actd + (resid.double() if with_resid else 0.0)
    rabs = resid.double().abs() if with_resid else 0.0
    bound = u * want.abs() + 1.01 * (1.13 * (K + 1) * u32 * S + 1e-6 + 2.0 ** -20 * (pre.abs() + rabs)) + 2.0 ** -24
    sentinel = -1234.0
    da_, dw, db = a.cuda(), w.cuda(), bias.cuda()
    dres = resid.cuda() if with_resid else None
    outs, bands = [], True
    for _ in range(2):
        buf, o = _guarded((M, N), sd, sentinel)
        d = gemm_desc(M=M, N=N, W=dw, ldw=K, a0=da_, a0_c=K, bias=db, resid=dres, act=act, out=o, ld_out=N)
        _lib.census_reset()
        _lib.call("dfh_gemm", C.byref(d), _lib.stream_ptr())
        torch.cuda.synchronize()
        bands = bands and _bands_untouched(buf, sentinel)
        outs.append(o.clone())
    c = _lib.census()
    err = (outs[0].cpu().double() - want).abs()
    res = dict(bands_untouched=bands, finite=bool(torch.isfinite(outs[0]).all()), rerun_identical=torch.equal(outs[0], outs[1]),
               lean_tile=c["gemm_lean"] == 1 and c["splitk_reduce"] == 0, worst_ratio=float((err / bound).max()), rel_l2=float(err.norm() / want.norm()))
    print(f"clipvh gemm {_lib.storage()} M={M} act={act} resid={int(with_resid)}: max err/bound {res['worst_ratio']:.3f} rel L2 {res['rel_l2']:.2e}", flush=True)
    return res


def main():
    from difashion_amd import _lib
    from tests.helpers_clip_vision_half import HALF_CASES
    res = {"storage": _lib.storage(), "build_info": _lib.raw().dfh_build_info().decode(), "parity": {}, "attention": {}, "gemm": {}}
    for name in HALF_CASES:
        res["parity"][name] = parity(name)
        torch.cuda.empty_cache()
    for case in ATTENTION_CASES:
        res["attention"]["x".join(map(str, case))] = attention_check(*case)
    for M in GEMM_ROWS:
        for act in (5, 6):
            for with_resid in (False, True):
                res["gemm"][f"{M}x{act}x{int(with_resid)}"] = gemm_check(M, act, with_resid)
    print("CLIPVH_RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
