#!/usr/bin/env python3
"""Golden vectors and yardsticks for the 16-bit CLIP image encoder from the REAL third-party class.  Build machine
only (needs the installed ``transformers``, CPU): the committed ``clipv_half_*.npz`` are what travels.

For every new tiny case of ``tests/helpers_clip_vision_half.py`` the real ``transformers.CLIPVisionModelWithProjection`` (eager
attention, eval, seeded weights under its own state-dict names) runs in fp64 on the seeded pixels; ``image_embeds``, ``pooler_output``
(``post_layernorm(last_hidden_state[:, 0])``), ``last_hidden_state`` and every block's hidden state go to
``clipv_half_<case>.npz``, stored as fp32 on the token rows ``kept_rows(T)``.  The full-size cases reuse the committed fp64 fixtures
``clipv_vit_{l,h}_14.npz``.

Then, for EVERY case, the same class runs with ``.to(torch.bfloat16)`` and ``.to(torch.float16)``: its relative-L2 distance from the
fp64 values per output, and the maximum of 1 - cos over the images' ``image_embeds``, go to ``clipv_half_yardsticks.npz`` under
``<case>/<format>/<output>`` beside the case's input checksum.  They are what the HIP 16-bit path is held to (at most 3 x).  The
script asserts that every 16-bit run is finite.

    python tests/golden/make_golden_clip_vision_half.py [case ...]      (cases not named keep their yardsticks)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import transformers  # noqa: E402
from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection  # noqa: E402

from tests.helpers_clip_vision import checksum, rel  # noqa: E402
from tests.helpers_clip_vision_half import (FORMATS, HALF_CASES, NEW_CASES, TORCH_DTYPE, YARDSTICKS, case_inputs, fixture_path,  # noqa: E402
                                            kept_rows, load_fixture, max_one_minus_cos, output_keys)


def run(cfg, params, pixels, dtype):
    """The real class in ``dtype`` -> {output name: tensor in float64}."""
    model = CLIPVisionModelWithProjection(CLIPVisionConfig(attn_implementation="eager", **cfg.kwargs())).eval().to(dtype)
    own = [k for k in model.state_dict() if not k.endswith("position_ids")]
    assert own == list(params), "state-dict names / order differ from tests/helpers_clip_vision.param_shapes"
    missing, unexpected = model.load_state_dict({k: v.to(dtype) for k, v in params.items()}, strict=False)
    assert not unexpected and all(m.endswith("position_ids") for m in missing), (missing, unexpected)
    out = model(pixel_values=pixels.to(dtype), output_hidden_states=True)
    assert len(out.hidden_states) == cfg.num_hidden_layers + 1 and torch.equal(out.hidden_states[-1], out.last_hidden_state)
    pooled = model.vision_model.post_layernorm(out.last_hidden_state[:, 0])
    res = {"image_embeds": out.image_embeds, "pooler_output": pooled, "last_hidden_state": out.last_hidden_state}
    res.update({f"hidden_{i}": h for i, h in enumerate(out.hidden_states)})
    return {k: v.double() for k, v in res.items()}


def main(names):
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    ys = dict(np.load(YARDSTICKS)) if os.path.exists(YARDSTICKS) else {}
    ys["transformers_version"] = np.array(transformers.__version__)
    for name in names:
        cfg, params, pixels = case_inputs(name)
        T, L = cfg.num_tokens, cfg.num_hidden_layers
        if name in NEW_CASES:
            out64 = run(cfg, params, pixels, torch.float64)
            assert all(torch.isfinite(v).all() for v in out64.values())
            rows = torch.tensor(kept_rows(T))
            rec = {"taps": np.arange(L + 1), "rows": rows.numpy(), "checksum": checksum(params, pixels),
                   "transformers_version": np.array(transformers.__version__)}
            for k in ["image_embeds", "pooler_output", "last_hidden_state"] + [f"hidden_{t}" for t in range(L + 1)]:
                rec[k] = (out64[k][:, rows] if out64[k].dim() == 3 else out64[k]).float().numpy()
            np.savez_compressed(fixture_path(name), **rec)
            print(f"wrote {os.path.basename(fixture_path(name))} ({os.path.getsize(fixture_path(name)) / 1024:.0f} KiB): T = {T}")
        fx = load_fixture(name)
        np.testing.assert_allclose(fx["checksum"], checksum(params, pixels), rtol=1e-12)
        rows = torch.from_numpy(fx["rows"]).long()
        ys[f"{name}/checksum"] = fx["checksum"]
        for fmt in FORMATS:
            got = run(cfg, params, pixels, TORCH_DTYPE[fmt])
            assert all(torch.isfinite(v).all() for v in got.values()), (name, fmt, "the real class is not finite in this format")
            line = []
            for k in output_keys(fx):
                want = torch.from_numpy(fx[k])
                ys[f"{name}/{fmt}/{k}"] = np.array(rel(got[k][:, rows] if got[k].dim() == 3 else got[k], want))
                line.append(f"{k}={float(ys[f'{name}/{fmt}/{k}']):.2e}")
            ys[f"{name}/{fmt}/cos"] = np.array(max_one_minus_cos(got["image_embeds"], torch.from_numpy(fx["image_embeds"])))
            ys[f"{name}/{fmt}/max_abs_last"] = np.array(float(got["last_hidden_state"].abs().max()))
            print(f"{name} {fmt}: 1-cos={float(ys[f'{name}/{fmt}/cos']):.2e} max|last|={float(ys[f'{name}/{fmt}/max_abs_last']):.1f} " + " ".join(line))
        np.savez_compressed(YARDSTICKS, **ys)
    print(f"wrote {os.path.basename(YARDSTICKS)} ({os.path.getsize(YARDSTICKS) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main(sys.argv[1:] or list(HALF_CASES))
