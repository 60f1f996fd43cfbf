"""The measurements of tests/test_gpu_clip_text_half.py, in the storage format the process runs (a process holds one): called in
process for bf16, and as a child under ``DFH_STORAGE=fp16``, which prints one ``CLIPTH_RESULT {json}`` line.

    DFH_STORAGE=fp16 python -m tests.clip_text_half_child

Op-level bound of the causal attention kernel (the reference is fp64 torch on the SAME 16-bit-rounded operands, so operand rounding is
not part of it).  u16 is the unit roundoff of the storage format (bf16: 2^-8, fp16: 2^-11), u32 = 2^-24.

  O[i][:] = sum_{j <= i} p_j v_j / sum_{j <= i} p_j,  p_j = exp(scale q_i.k_j - m_i),  m_i = max_{j <= i} scale q_i.k_j  (exact: the row is resident)

  * a score is an fp32 sum of d exact products (two 16-bit numbers multiply exactly in fp32), in any order off by at most d u32 S
    with S = sum_c |q_c k_jc| (Higham, Accuracy and Stability, eq. 4.4, first order); the multiplication by the rounded constant
    scale x log2(e) and the subtraction of the maximum add three more roundings of numbers no larger than 2 smax:
    |error of (s_j - m_i)| <= 2 (d + 3) u32 smax,  smax = scale max_{j <= i} sum_c |q_ic k_jc|  (s_j and m_i each carry one share);
  * p_j = 2^(t_j - m) on the hardware exp2 (v_exp_f32: 1 ulp = 2 u32 relative), so p_j is off by the score error (first order,
    relative) + 2 u32; the factor 4 below instead of 2 covers the higher orders for smax up to 2^12;
  * every probability is ROUNDED to the storage format before it multiplies V (an MFMA operand): relative error u16.
    eps_p = u16 + 4 (d + 3) u32 smax + 8 u32;
  * the numerator carries eps_p and an fp32 accumulation error of at most T u32, the denominator (summed in fp32 from the UNROUNDED
    probabilities) the score part of eps_p and T u32, and the final reciprocal and product three more roundings:
    |O~ - O| <= 1.05 (2 eps_p + 4 T u32) A,  A[i][c] = sum_j softmax_j |v_jc|  (>= |O[i][c]|);
  * fp16 only: a probability below 2^-14 is subnormal in the storage format and rounds with an ABSOLUTE error of at most 2^-25.  The
    maximum is exact, so the largest probability is 1 and the denominator at least 1: at most T 2^-25 max|v| in the numerator;
  * the store: u16 |want| (+ half a subnormal step of fp16, 2^-25; 2^-24 is used).
  bound = u16 |want| + 1.05 (2 eps_p + 4 T u32) A + [fp16] T 2^-25 max|v| + 2^-24.
"""
import json

import numpy as np
import torch

from tests.helpers_clip_half import FACTOR, GUARD, _bands_untouched, _guarded, u16  # noqa: F401

ATTENTION_T = (1, 16, 17, 20, 64, 77, 128)
ATTENTION_BH = (2, 2)              # B x H = 4 workgroups
CAUSAL_SHAPE = (2, 3, 64, 77)
CAUSAL_T0 = (0, 15, 16, 31, 32, 63, 64, 75)


def hip_model(cfg, params, proj, dtype, with_projection=True):
    import difashion_amd as da
    from tests.helpers_clip_text_half import config_kwargs
    if with_projection:
        m = da.CLIPTextModelWithProjection(projection_dim=proj.shape[0], init_seed=None, torch_dtype=dtype, **config_kwargs(cfg))
        m.load_state_dict(dict(params, **{"text_projection.weight": proj}))
    else:
        m = da.CLIPTextModel(init_seed=None, torch_dtype=dtype, **config_kwargs(cfg))
        m.load_state_dict(params)
    return m.to("cuda").eval().requires_grad_(False)


def causal_attention(qkv, B, T, H, out=None):
    """dfh_causal_attention over qkv [B * T][3 * H * 64] in the storage dtype -> out [B * T][H * 64]."""
    from difashion_amd import _lib
    out = torch.empty((B * T, H * 64), dtype=qkv.dtype, device=qkv.device) if out is None else out
    _lib.call("dfh_causal_attention", _lib.ptr(qkv), _lib.ptr(out), B, T, H, 64, 64 ** -0.5, _lib.stream_ptr())
    return out


def parity(name):
    """One 16-bit encode of a case by both text classes -> {output: (hip distance from fp64, the real class's)}, census, structural facts."""
    from difashion_amd import _lib
    from tests.helpers_clip_text_half import (YARDSTICKS, case_inputs, checksum, eos_positions, load_fixture, max_one_minus_cos, output_keys, rel,
                                              yardstick)
    fmt, sd = _lib.storage(), _lib.storage_dtype()
    cfg, params, proj, ids = case_inputs(name)
    fx, ys = load_fixture(name), dict(np.load(YARDSTICKS))
    ok = bool(np.allclose(fx["checksum"], checksum(params, proj, ids), rtol=1e-12) and np.allclose(ys[f"{name}/checksum"], fx["checksum"], rtol=1e-12)
              and np.array_equal(fx["input_ids"], ids.numpy()))
    m = hip_model(cfg, params, proj, sd)
    plain = hip_model(cfg, params, proj, sd, with_projection=False)
    del params
    dids = ids.to("cuda")
    _lib.census_reset()
    out = m(dids, output_hidden_states=True)
    torch.cuda.synchronize()
    census = _lib.census()
    _lib.census_reset()
    pout = plain(ids, output_hidden_states=True)                                 # tokenizer output is a CPU tensor
    torch.cuda.synchronize()
    pcensus = _lib.census()
    B, T, D, L = ids.shape[0], ids.shape[1], cfg.hidden_size, cfg.num_hidden_layers
    tensors = (out.text_embeds, out.pooler_output, out.last_hidden_state) + tuple(out.hidden_states)
    eos = torch.tensor(eos_positions(cfg, ids))
    embeds_only = m.encode_text(dids)
    facts = {
        "checksum": ok,
        "shapes": out.last_hidden_state.shape == (B, T, D) and out.pooler_output.shape == (B, D) and out.text_embeds.shape == (B, proj.shape[0])
                  and len(out.hidden_states) == L + 1,
        "fp32_outputs": all(t.dtype == torch.float32 and t.device.type == "cuda" for t in tensors),
        "finite": all(bool(torch.isfinite(t).all()) for t in tensors),
        # the taps are exact upcasts of the 16-bit stream
        "exact_upcasts": all(torch.equal(t.to(sd).float(), t) for t in out.hidden_states),
        # pooler_output is the eos row of last_hidden_state (gather-then-normalise = normalise-then-gather: LayerNorm is row-local)
        "pooled_is_eos_row": torch.equal(out.pooler_output.cpu(), out.last_hidden_state.cpu()[torch.arange(B), eos]),
        "encode_text": torch.equal(embeds_only, out.text_embeds),
        # CLIPTextModel runs the same walk: the same bits
        "both_classes_agree": torch.equal(pout.last_hidden_state, out.last_hidden_state) and torch.equal(pout.pooler_output, out.pooler_output)
                              and all(torch.equal(a, b) for a, b in zip(pout.hidden_states, out.hidden_states)),
        "same_census": all(pcensus[k] == census[k] for k in ("cliph_attention", "cliph_embed", "layernorm")),
    }
    rows = torch.from_numpy(fx["rows"]).long()
    got = {"text_embeds": out.text_embeds.cpu(), "pooler_output": out.pooler_output.cpu(), "last_hidden_state": out.last_hidden_state.cpu()[:, rows]}
    for t in fx["taps"]:
        got[f"hidden_{int(t)}"] = out.hidden_states[int(t)].cpu()[:, rows]
    assert sorted(got) == sorted(output_keys(fx))
    dist = {k: (rel(got[k], torch.from_numpy(fx[k])), yardstick(ys, name, fmt, k)) for k in output_keys(fx)}
    dist["cos"] = (max_one_minus_cos(got["text_embeds"], torch.from_numpy(fx["text_embeds"])), yardstick(ys, name, fmt, "cos"))
    print(f"clipth parity {name} {fmt} " + " ".join(f"{k}: hip {e:.2e} real_{fmt} {r:.2e} ratio {e / r:.2f};" for k, (e, r) in dist.items()), flush=True)
    keys = ("cliph_attention", "cliph_embed", "attention_16", "attention_x32", "clipv_attention", "layernorm", "splitk_reduce")
    return {"dist": dist, "census": {k: census[k] for k in keys}, "layers": L, "facts": {k: bool(v) for k, v in facts.items()}}


def _qkv(B, H, T, seed, q_gain=1.5):
    from difashion_amd import _lib
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * T, 3 * H * 64, generator=g)
    qkv[:, :H * 64] *= q_gain                                                    # peaked, not one-hot, softmaxes
    return qkv.to(_lib.storage_dtype())


def attention_check(T):
    """dfh_causal_attention at (B, H, 64, T) against the fp64 causal softmax of the same rounded operands."""
    from difashion_amd import _lib
    B, H = ATTENTION_BH
    d, sd, u, u32 = 64, _lib.storage_dtype(), u16(), 2.0 ** -24
    qkv = _qkv(B, H, T, 7000 + T)
    split = lambda t: t.double().reshape(B, T, H, d).transpose(1, 2)            # [B][H][T][d]
    q64, k64, v64 = (split(qkv[:, i * H * d:(i + 1) * H * d]) for i in range(3))
    scale = d ** -0.5
    allowed = torch.ones(T, T, dtype=torch.bool).tril()
    p = torch.softmax((q64 @ k64.transpose(-1, -2) * scale).masked_fill(~allowed, float("-inf")), dim=-1)
    back = lambda t: t.transpose(1, 2).reshape(B * T, H * d)
    want, A = back(p @ v64), back(p @ v64.abs())
    smax = (scale * (q64.abs() @ k64.abs().transpose(-1, -2)).masked_fill(~allowed, 0.0).amax(-1))          # [B][H][T]
    smax = back(smax.unsqueeze(-1).expand(B, H, T, d))
    eps_p = u + 4.0 * (d + 3) * u32 * smax + 8.0 * u32
    sub = T * 2.0 ** -25 * float(v64.abs().max()) if _lib.storage() == "fp16" else 0.0
    bound = u * want.abs() + 1.05 * (2.0 * eps_p + 4.0 * T * u32) * A + sub + 2.0 ** -24
    sentinel = -1234.0
    dqkv = qkv.cuda()
    res, outs = {}, []
    for _ in range(2):
        buf, o = _guarded((B * T, H * d), sd, sentinel)
        _lib.census_reset()
        causal_attention(dqkv, B, T, H, out=o)
        torch.cuda.synchronize()
        res["bands_untouched"] = _bands_untouched(buf, sentinel) and res.get("bands_untouched", True)
        outs.append(o.clone())
    err = (outs[0].cpu().double() - want).abs()
    res.update(one_launch=_lib.census()["cliph_attention"] == 1, finite=bool(torch.isfinite(outs[0]).all()), rerun_identical=torch.equal(outs[0], outs[1]),
               worst_ratio=float((err / bound).max()), rel_l2=float(err.norm() / want.norm()))
    print(f"clipth attention {_lib.storage()} B={B} H={H} T={T}: max err/bound {res['worst_ratio']:.3f} rel L2 {res['rel_l2']:.2e}", flush=True)
    return res


def causality_check():
    """Bitwise: rows <= t0 of the output do not depend on rows > t0 of q, k and v (values up to 2^12 in magnitude, finite in both formats)."""
    from difashion_amd import _lib
    B, H, d, T = CAUSAL_SHAPE
    sd = _lib.storage_dtype()
    qkv = _qkv(B, H, T, 8100).cuda()
    base = causal_attention(qkv, B, T, H).view(B, T, H * d)
    res = {}
    for t0 in CAUSAL_T0:
        g = torch.Generator().manual_seed(8200 + t0)
        noise = ((torch.rand(B, T, 3 * H * d, generator=g) * 2 - 1) * 4096.0).to(sd).cuda()
        moved = qkv.view(B, T, 3 * H * d).clone()
        moved[:, t0 + 1:] = noise[:, t0 + 1:]
        out = causal_attention(moved.view(B * T, 3 * H * d), B, T, H).view(B, T, H * d)
        torch.cuda.synchronize()
        res[str(t0)] = {"prefix_identical": torch.equal(out[:, :t0 + 1], base[:, :t0 + 1]), "suffix_moved": not torch.equal(out[:, t0 + 1:], base[:, t0 + 1:]),
                        "finite": bool(torch.isfinite(out).all())}
    print(f"clipth causality {_lib.storage()} " + " ".join(f"t0={k}:{int(v['prefix_identical'])}" for k, v in res.items()), flush=True)
    return res


def model_causality_check(name="thalf_tiny_77", positions=(0, 15, 16, 40, 75)):
    """Bitwise at model level: other ids after position t (same batch and T, hence the same GEMM plan) leave hidden_states[*][:, :t + 1] as they were."""
    from difashion_amd import _lib
    from tests.helpers_clip_text_half import case_inputs
    cfg, params, proj, ids = case_inputs(name)
    m = hip_model(cfg, params, proj, _lib.storage_dtype(), with_projection=False)
    base = m(ids, output_hidden_states=True).hidden_states
    res = {}
    for t in positions:
        g = torch.Generator().manual_seed(8300 + t)
        other = ids.clone()
        other[:, t + 1:] = torch.randint(1, cfg.bos_token_id, other[:, t + 1:].shape, generator=g)
        hs = m(other, output_hidden_states=True).hidden_states
        res[str(t)] = {"prefix_identical": all(torch.equal(a[:, :t + 1], b[:, :t + 1]) for a, b in zip(hs, base)),
                       "suffix_moved": not torch.equal(hs[-1][:, t + 1:], base[-1][:, t + 1:])}
    print(f"clipth model causality {_lib.storage()} " + " ".join(f"t={k}:{int(v['prefix_identical'])}" for k, v in res.items()), flush=True)
    return res


def main():
    from difashion_amd import _lib
    from tests.helpers_clip_text_half import HALF_CASES
    res = {"storage": _lib.storage(), "build_info": _lib.raw().dfh_build_info().decode(), "parity": {}, "attention": {}}
    for name in HALF_CASES:
        res["parity"][name] = parity(name)
        torch.cuda.empty_cache()
    for T in ATTENTION_T:
        res["attention"][str(T)] = attention_check(T)
    res["causality"] = causality_check()
    res["model_causality"] = model_causality_check()
    print("CLIPTH_RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
