#!/usr/bin/env python3
"""Golden vectors and yardsticks for the 16-bit CLIP text encoder from the REAL third-party classes.  Build
machine only (needs the installed ``transformers``, CPU): the committed ``clipt_half_*.npz`` are what travels.

For every case of ``tests/helpers_clip_text_half.py`` the real ``transformers.CLIPTextModel`` and ``CLIPTextModelWithProjection`` (eager
attention, eval, seeded weights under their own state-dict names) run in fp64 on the seeded ids, called as the reference calls them
(``input_ids`` only); ``last_hidden_state``, ``pooler_output``, ``text_embeds`` and the hidden states (all taps for the tiny cases; 0,
L / 2 and L at full size) go to ``clipt_half_<case>.npz``, stored as fp32 on the token rows ``kept_rows(cfg, ids)``.

Then the same classes run with ``.to(torch.bfloat16)`` and ``.to(torch.float16)``: their relative-L2 distance from the fp64 values per
output, and the maximum of 1 - cos over the sequences' ``text_embeds``, go to ``clipt_half_yardsticks.npz`` under
``<case>/<format>/<output>`` beside the case's input checksum.  They are what the HIP 16-bit path is held to (at most 3 x).  The script
asserts that every 16-bit run is finite.

    python tests/golden/make_golden_clip_text_half.py [case ...]      (cases not named keep their yardsticks)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import transformers  # noqa: E402
from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection  # noqa: E402

from tests.helpers_clip_text_half import (FORMATS, HALF_CASES, TORCH_DTYPE, YARDSTICKS, case_inputs, checksum, config_kwargs,  # noqa: E402
                                          fixture_path, kept_rows, kept_taps, load_fixture, max_one_minus_cos, output_keys, rel)


def real_model(cls, cfg, params, proj, dtype):
    hf_cfg = CLIPTextConfig(projection_dim=proj.shape[0], attn_implementation="eager", **config_kwargs(cfg))
    model = cls(hf_cfg).eval().to(dtype)
    # transformers 4.32.1 (the reference's pin) nests the tower under ``text_model.``; newer releases flattened it in CLIPTextModel
    sd = {}
    for k in model.state_dict():
        if k.endswith("position_ids"):
            continue
        sd[k] = (proj if k == "text_projection.weight" else params[k if k in params else "text_model." + k]).to(dtype)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(m.endswith("position_ids") for m in missing), (missing, unexpected)
    assert len(sd) == len(params) + (cls is CLIPTextModelWithProjection), (len(sd), len(params))
    return model


def run(cfg, params, proj, ids, dtype):
    """The real classes in ``dtype`` -> {output name: tensor in float64}."""
    L = cfg.num_hidden_layers
    out = real_model(CLIPTextModel, cfg, params, proj, dtype)(ids, output_hidden_states=True)
    assert len(out.hidden_states) == L + 1
    wp = real_model(CLIPTextModelWithProjection, cfg, params, proj, dtype)(ids)
    assert torch.equal(wp.last_hidden_state, out.last_hidden_state)
    res = {"text_embeds": wp.text_embeds, "pooler_output": out.pooler_output, "last_hidden_state": out.last_hidden_state}
    res.update({f"hidden_{i}": h for i, h in enumerate(out.hidden_states)})
    return {k: v.double() for k, v in res.items()}


def main(names):
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    ys = dict(np.load(YARDSTICKS)) if os.path.exists(YARDSTICKS) else {}
    ys["transformers_version"] = np.array(transformers.__version__)
    for name in names:
        cfg, params, proj, ids = case_inputs(name)
        rows = torch.tensor(kept_rows(cfg, ids))
        out64 = run(cfg, params, proj, ids, torch.float64)
        assert all(torch.isfinite(v).all() for v in out64.values())
        taps = kept_taps(name)
        rec = {"taps": np.array(taps), "rows": rows.numpy(), "input_ids": ids.numpy(), "checksum": checksum(params, proj, ids),
               "transformers_version": np.array(transformers.__version__)}
        for k in ["text_embeds", "pooler_output", "last_hidden_state"] + [f"hidden_{t}" for t in taps]:
            rec[k] = (out64[k][:, rows] if out64[k].dim() == 3 else out64[k]).float().numpy()
        np.savez_compressed(fixture_path(name), **rec)
        print(f"wrote {os.path.basename(fixture_path(name))} ({os.path.getsize(fixture_path(name)) / 1024:.0f} KiB): rows {rows.tolist()}")
        fx = load_fixture(name)
        ys[f"{name}/checksum"] = fx["checksum"]
        for fmt in FORMATS:
            got = run(cfg, params, proj, ids, TORCH_DTYPE[fmt])
            assert all(torch.isfinite(v).all() for v in got.values()), (name, fmt, "the real class is not finite in this format")
            line = []
            for k in output_keys(fx):
                want = torch.from_numpy(fx[k])
                ys[f"{name}/{fmt}/{k}"] = np.array(rel(got[k][:, rows] if got[k].dim() == 3 else got[k], want))
                line.append(f"{k}={float(ys[f'{name}/{fmt}/{k}']):.2e}")
            ys[f"{name}/{fmt}/cos"] = np.array(max_one_minus_cos(got["text_embeds"], torch.from_numpy(fx["text_embeds"])))
            ys[f"{name}/{fmt}/max_abs_last"] = np.array(float(got["last_hidden_state"].abs().max()))
            print(f"{name} {fmt}: 1-cos={float(ys[f'{name}/{fmt}/cos']):.2e} max|last|={float(ys[f'{name}/{fmt}/max_abs_last']):.1f} " + " ".join(line))
        np.savez_compressed(YARDSTICKS, **ys)
    print(f"wrote {os.path.basename(YARDSTICKS)} ({os.path.getsize(YARDSTICKS) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main(sys.argv[1:] or list(HALF_CASES))
