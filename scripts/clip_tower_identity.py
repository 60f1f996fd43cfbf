#!/usr/bin/env python3
"""What the two CLIP towers compute on the GPU, as text: the SHA-256 of every output (last hidden state, pooled output, image
embeds, every hidden state) of every tiny case of the text tower (tests/helpers_clip.py) and of the vision tower
(tests/helpers_clip_vision.py).  The kernels are deterministic and free of atomics, so a host-only change of csrc/clip*.hip or of the
Python wrappers must leave this output bit-identical: run it on both commits on the same machine and diff.

``--half``: the same for the two 16-bit towers (csrc/clip_text_half.hip, clip_vision_half.hip) in the storage format of the library the
process runs (DFH_STORAGE), over the tiny cases of tests/helpers_clip_text_half.py and tests/helpers_clip_vision_half.py, with the
census counts of one encode."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import difashion_amd as da
from difashion_amd import _lib
from tests import helpers_clip
from tests.clip_vision_child import digests
from tests.helpers_clip_vision import TINY_CASES


def text_digests(name):
    cfg, params, ids = helpers_clip.case_inputs(name)
    m = da.CLIPTextModel(**{k: getattr(cfg, k) for k in ("vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers",
                                                          "num_attention_heads", "max_position_embeddings", "hidden_act", "layer_norm_eps",
                                                          "eos_token_id", "bos_token_id", "pad_token_id")}, init_seed=None)
    m.load_state_dict(params)
    out = m.to("cuda").eval().requires_grad_(False)(ids.to("cuda"), output_hidden_states=True)
    torch.cuda.synchronize()
    sha = lambda t: hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()
    rec = {"last_hidden_state": sha(out.last_hidden_state), "pooler_output": sha(out.pooler_output)}
    rec.update({f"hidden_{i}": sha(h) for i, h in enumerate(out.hidden_states)})
    return rec


def half_digests(tower, name):
    """One 16-bit encode (the library's storage format) of a tiny case of tests/helpers_clip_{vision,text}_half.py: the digests of every
    output and hidden state, and what the encode added to every census counter."""
    sd = _lib.storage_dtype()
    if tower == "vision_half":
        from tests.clip_vision_half_child import hip_model
        from tests.helpers_clip_vision_half import case_inputs
        cfg, params, x = case_inputs(name)
        m = hip_model(cfg, params, sd)
    else:
        from tests.clip_text_half_child import hip_model
        from tests.helpers_clip_text_half import case_inputs
        cfg, params, proj, x = case_inputs(name)
        m = hip_model(cfg, params, proj, sd)
    x = x.to("cuda")
    m(x)                                                     # the packed copy and the workspace are made by the first call
    torch.cuda.synchronize()
    _lib.census_reset()
    out = m(x, output_hidden_states=True)
    torch.cuda.synchronize()
    census = _lib.census()
    sha = lambda t: hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()
    rec = {f: sha(getattr(out, f)) for f in out._fields if torch.is_tensor(getattr(out, f))}
    rec.update({f"hidden_{i}": sha(h) for i, h in enumerate(out.hidden_states)})
    rec.update({f"census_{k}": v for k, v in census.items() if v})
    return rec


if __name__ == "__main__":
    print(_lib.raw().dfh_build_info().decode())
    if "--half" in sys.argv[1:]:
        from tests.helpers_clip_text_half import TINY_CASES as TEXT_HALF
        from tests.helpers_clip_vision_half import NEW_CASES as VISION_HALF
        for tower, names in (("text_half", TEXT_HALF), ("vision_half", VISION_HALF)):
            for name in names:
                for key, value in half_digests(tower, name).items():
                    print(f"{tower} {name} {key} {value}")
        sys.exit(0)
    for tower, names, fn in (("text", [n for n, c in helpers_clip.CASES.items() if c[4]], text_digests), ("vision", TINY_CASES, digests)):
        for name in names:
            for key, value in fn(name).items():
                print(f"{tower} {name} {key} {value}")
