#!/usr/bin/env python3
"""Golden vectors for the CLIP text tower with projection from the REAL third-party class.  Build machine only (needs
the installed ``transformers``; nothing of it travels to the GPU box): the committed ``cliptp_*.npz`` are what travels.

The reference's evaluation calls ``encode_text`` of an OpenCLIP ViT-H/14 (Evaluation/eval_utils.py:101-114, :408-435);
``transformers.CLIPTextModelWithProjection`` is the same architecture.  For every case of ``tests/helpers_eval_scores.TEXT_CASES`` this
script builds that class (eager attention, eval), loads the seeded weights under the class's own state-dict names and runs it on the
seeded token ids TWICE: in fp64 -- the recorded truth, stored as fp32 -- and in fp32.  The distance of the fp32 run from the recorded
truth, per output, is stored as ``ref_*``: the yardstick the GPU test holds the HIP encoder to (at most 3 x that distance).  The eos
sits at a different index in every row, first and last position included, and the script asserts that the class pooled exactly there.
The full-size case keeps the token rows ``FULL_SIZE_ROWS`` of the [B, T, D] tensors.

    python tests/golden/make_golden_clip_text_proj.py [case ...]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import transformers  # noqa: E402
from transformers import CLIPTextConfig, CLIPTextModelWithProjection  # noqa: E402

from helpers_eval_scores import (FULL_SIZE_ROWS, TEXT_CASES, fixture_path, rel, text_case_inputs, text_checksum,  # noqa: E402
                                 text_kwargs)


def run(cfg, pd, params, ids, dtype):
    model = CLIPTextModelWithProjection(CLIPTextConfig(attn_implementation="eager", **text_kwargs(cfg, pd))).eval().to(dtype)
    own = [k for k in model.state_dict() if not k.endswith("position_ids")]
    assert own == list(params), "state-dict names / order differ from tests/helpers_eval_scores.text_params"
    missing, unexpected = model.load_state_dict({k: v.to(dtype) for k, v in params.items()}, strict=False)
    assert not unexpected and all(m.endswith("position_ids") for m in missing), (missing, unexpected)
    out = model(input_ids=ids, output_hidden_states=True)
    pooled = model.text_model(input_ids=ids).pooler_output
    assert len(out.hidden_states) == cfg.num_hidden_layers + 1
    assert torch.allclose(model.text_projection(pooled), out.text_embeds, rtol=1e-5, atol=1e-6)
    return out, pooled


def main(names):
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    for name in names:
        cfg, pd, params, ids = text_case_inputs(name)
        pos, full = TEXT_CASES[name][4], TEXT_CASES[name][5]
        out64, pooled64 = run(cfg, pd, params, ids, torch.float64)
        out32, pooled32 = run(cfg, pd, params, ids, torch.float32)
        assert torch.isfinite(out64.text_embeds).all() and all(torch.isfinite(h).all() for h in out64.hidden_states)
        # the class pooled at the planted eos index of every row, and no two rows share it
        assert len(set(pos)) == len(pos) and 0 in pos and ids.shape[1] - 1 in pos
        assert torch.equal(pooled64, out64.last_hidden_state[torch.arange(len(pos)), torch.tensor(pos)])
        L = cfg.num_hidden_layers
        taps = [0, L // 2, L] if full else list(range(L + 1))
        rows = torch.tensor(FULL_SIZE_ROWS) if full else None
        pick = (lambda t: t[:, rows]) if full else (lambda t: t)
        rec = {"taps": np.array(taps), "checksum": text_checksum(params, ids), "transformers_version": np.array(transformers.__version__),
               "input_ids": ids.numpy(), "eos_positions": np.array(pos), "param_names": np.array(list(params))}
        if full:
            rec["rows"] = rows.numpy()
        pairs = {"text_embeds": (out64.text_embeds, out32.text_embeds), "pooler_output": (pooled64, pooled32),
                 "last_hidden_state": (pick(out64.last_hidden_state), pick(out32.last_hidden_state))}
        for t in taps:
            pairs[f"hidden_{t}"] = (pick(out64.hidden_states[t]), pick(out32.hidden_states[t]))
        for key, (t64, t32) in pairs.items():
            stored = t64.float()
            rec[key] = stored.numpy()
            rec["ref_" + key] = np.array(rel(t32, stored))
        np.savez_compressed(fixture_path("cliptp_" + name), **rec)
        print(f"wrote cliptp_{name}.npz ({os.path.getsize(fixture_path('cliptp_' + name)) / 1024:.0f} KiB): |text_embeds| = "
              f"{float(out64.text_embeds.norm()):.4f}, ref_fp32_rel_l2 " + " ".join(f"{k}={float(rec['ref_' + k]):.2e}" for k in pairs))


if __name__ == "__main__":
    main(sys.argv[1:] or list(TEXT_CASES))
