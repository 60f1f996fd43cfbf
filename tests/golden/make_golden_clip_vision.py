#!/usr/bin/env python3
"""Golden vectors for the CLIP image encoder from the REAL third-party class.  Build machine only (needs the
installed ``transformers``; nothing of it travels to the GPU box): the committed ``clipv_*.npz`` are what travels.

The reference's evaluation scripts call ``encode_image`` of an OpenCLIP ViT-H/14 (Evaluation/extract_hist_embs.py:83-100,
Evaluation/eval_utils.py:91-135, :503-535); ``transformers.CLIPVisionModelWithProjection`` is the same architecture.  For every case of
``tests/helpers_clip_vision.py`` this script builds that class (eager attention, eval), loads the seeded weights under the class's own
state-dict names and runs it on the seeded pixel inputs TWICE: in fp64 -- the recorded truth, stored as fp32 -- and in fp32.  The
distance of the fp32 run from the recorded truth, per output, is stored as ``ref_*``: the yardstick the GPU test holds the HIP encoder
to (at most 3 x that distance).  ``pooler_output`` is ``vision_model.post_layernorm(last_hidden_state[:, 0])``, the tensor
``visual_projection`` reads.  The full-size cases keep the token rows ``FULL_SIZE_ROWS`` of the [B, T, D] tensors.

The script asserts what the synthetic weights are meant to give: finite activations, and softmaxes that are neither one-hot nor
uniform in every layer.

    python tests/golden/make_golden_clip_vision.py [case ...]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import transformers  # noqa: E402
from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection  # noqa: E402

from helpers_clip_vision import CASES, FULL_SIZE_ROWS, case_inputs, checksum, fixture_path, rel  # noqa: E402


def real_model(cfg, params, dtype):
    hf_cfg = CLIPVisionConfig(attn_implementation="eager", **cfg.kwargs())
    model = CLIPVisionModelWithProjection(hf_cfg).eval().to(dtype)
    own = [k for k in model.state_dict() if not k.endswith("position_ids")]
    assert own == list(params), "state-dict names / order differ from tests/helpers_clip_vision.param_shapes"
    missing, unexpected = model.load_state_dict({k: v.to(dtype) for k, v in params.items()}, strict=False)
    assert not unexpected and all(m.endswith("position_ids") for m in missing), (missing, unexpected)
    return model


def run(cfg, params, pixels, dtype, attentions=False):
    model = real_model(cfg, params, dtype)
    out = model(pixel_values=pixels.to(dtype), output_hidden_states=True, output_attentions=attentions)
    hs = out.hidden_states
    assert len(hs) == cfg.num_hidden_layers + 1
    assert torch.equal(hs[-1], out.last_hidden_state)
    pooled = model.vision_model.post_layernorm(out.last_hidden_state[:, 0])
    assert torch.allclose(model.visual_projection(pooled), out.image_embeds, rtol=1e-5, atol=1e-6)
    return out, pooled


def main(names):
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    for name in names:
        cfg, params, pixels = case_inputs(name)
        full = CASES[name][3]
        out64, pooled64 = run(cfg, params, pixels, torch.float64)
        out32, pooled32 = run(cfg, params, pixels, torch.float32, attentions=True)
        # the synthetic weights exercise the tower: finite, and the softmax neither one-hot nor uniform in any layer
        assert all(torch.isfinite(h).all() for h in out64.hidden_states) and torch.isfinite(out64.image_embeds).all()
        T = cfg.num_tokens
        peak = [float(a.max(-1).values.mean()) for a in out32.attentions]
        assert all(2.0 / T < p < 0.8 for p in peak), peak
        L = cfg.num_hidden_layers
        taps = [0, L // 2, L] if full else list(range(L + 1))
        rows = torch.tensor(FULL_SIZE_ROWS) if full else None
        pick = (lambda t: t[:, rows]) if full else (lambda t: t)
        rec = {"taps": np.array(taps), "checksum": checksum(params, pixels), "transformers_version": np.array(transformers.__version__),
               "attention_peak": np.array(peak)}
        if full:
            rec["rows"] = rows.numpy()
        pairs = {"last_hidden_state": (pick(out64.last_hidden_state), pick(out32.last_hidden_state)), "pooler_output": (pooled64, pooled32),
                 "image_embeds": (out64.image_embeds, out32.image_embeds)}
        for t in taps:
            pairs[f"hidden_{t}"] = (pick(out64.hidden_states[t]), pick(out32.hidden_states[t]))
        for key, (t64, t32) in pairs.items():
            stored = t64.float()
            rec[key] = stored.numpy()
            rec["ref_" + key] = np.array(rel(t32, stored))          # ref_fp32_rel_l2: the real class in fp32 against the stored truth
        np.savez_compressed(fixture_path(name), **rec)
        print(f"wrote clipv_{name}.npz ({os.path.getsize(fixture_path(name)) / 1024:.0f} KiB): T = {T}, |image_embeds| = "
              f"{float(out64.image_embeds.norm()):.4f}, |last| = {float(out64.last_hidden_state.norm()):.2f}, attention peak "
              f"{min(peak):.3f} .. {max(peak):.3f}, ref_fp32_rel_l2 "
              + " ".join(f"{k}={float(rec['ref_' + k]):.2e}" for k in pairs))


if __name__ == "__main__":
    main(sys.argv[1:] or list(CASES))
