"""Child process of tests/test_gpu_clip_vision.py: the tiny cases of the CLIP image encoder under the storage build that
``DFH_STORAGE`` selects (a process holds one storage format).  Prints one ``CLIPV_RESULT {json}`` line: build info and a SHA-256 of every
output tensor per case.

    DFH_STORAGE=fp16 python -m tests.clip_vision_child
"""
import hashlib
import json

import torch


def digests(name):
    import difashion_amd as da
    from tests.helpers_clip_vision import case_inputs
    cfg, params, pixels = case_inputs(name)
    m = da.CLIPVisionModelWithProjection(**cfg.kwargs(), init_seed=None)
    m.load_state_dict(params)
    m = m.to("cuda").eval().requires_grad_(False)
    out = m(pixels.to("cuda"), output_hidden_states=True)
    torch.cuda.synchronize()
    sha = lambda t: hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()
    rec = {"image_embeds": sha(out.image_embeds), "last_hidden_state": sha(out.last_hidden_state), "pooler_output": sha(out.pooler_output)}
    rec.update({f"hidden_{i}": sha(h) for i, h in enumerate(out.hidden_states)})
    return rec


def main():
    from difashion_amd import _lib
    from tests.helpers_clip_vision import TINY_CASES
    res = {"storage": _lib.storage(), "build_info": _lib.raw().dfh_build_info().decode()}
    for name in TINY_CASES:
        res[name] = digests(name)
    print("CLIPV_RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
