"""Host only, no GPU: every field, launch and region of dfh_clipvh_plan and dfh_cliph_plan, the size queries and every refusal message,
as text.  Two builds of the library plan the same walks exactly when their outputs are byte-identical:

    python scripts/clip_half_plans.py > here.txt
    DFH_LIB=<other checkout>/difashion_amd/csrc/libdifashion_hip.so python scripts/clip_half_plans.py > there.txt

Covers every case of tests/helpers_clip_vision_half.py and tests/helpers_clip_text_half.py at the batches (and lengths) their plan
tests use, the full-size towers (ViT-L/14 and ViT-H/14 at batch 1, 64 and 200; CLIP-L and OpenCLIP-H text at (51, 77)) and the configs the two
test_plan_refuses_what_the_walk_cannot_run tests hand in.  DFH_STORAGE=fp16 asks the other library."""
import ctypes as C
import dataclasses
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from difashion_amd import _lib  # noqa: E402
from oracle import clip_ref  # noqa: E402
from tests import helpers_clip_text_half as th  # noqa: E402
from tests import helpers_clip_vision_half as vh  # noqa: E402
from tests.helpers_clip_vision import TINY_GELU  # noqa: E402
from tests.test_clip_text_half_cpu import _ctx as text_ctx  # noqa: E402
from tests.test_clip_vision_half_cpu import _ctx as vision_ctx  # noqa: E402


def dump(s, indent="  "):
    """Every field of a ctypes struct, arrays of structs up to the count the struct itself reports."""
    for name, typ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Array) and isinstance(v[0], C.Structure):
            n = getattr(s, "num_" + name)
            for i in range(n):
                print(f"{indent}{name}[{i}]: " + " ".join(f"{f}={getattr(v[i], f).decode() if isinstance(getattr(v[i], f), bytes) else getattr(v[i], f)}"
                                                         for f, _ in v[i]._fields_))
        else:
            print(f"{indent}{name} = {v.decode() if isinstance(v, bytes) else v}")


def plan(fn, mirror, h, *args):
    p = mirror()
    try:
        _lib.call(fn, h, *args, C.byref(p))
    except _lib.DfhError as e:
        print(f"  refused: {e}")
        return
    dump(p)


def vision(label, cfg, batches):
    h, lib = vision_ctx(cfg), _lib.raw()
    try:
        print(f"dfh_clipvh {label}: packed_bytes {lib.dfh_clipvh_packed_bytes(h)}")
        for B in batches:
            print(f" batch {B}: workspace_bytes {lib.dfh_clipvh_workspace_bytes(h, B)}")
            plan("dfh_clipvh_plan", _lib.CLIPVHalfPlanC, h, B)
    finally:
        lib.dfh_clipv_destroy(h)


def text(label, cfg, shapes):
    h, lib = text_ctx(cfg), _lib.raw()
    try:
        print(f"dfh_cliph {label}: packed_bytes {lib.dfh_cliph_packed_bytes(h)}")
        for B, T in shapes:
            print(f" batch {B} tokens {T}: workspace_bytes {lib.dfh_cliph_workspace_bytes(h, B, T)}")
            plan("dfh_cliph_plan", _lib.CLIPTHalfPlanC, h, B, T)
    finally:
        lib.dfh_clip_destroy(h)


def main():
    print(f"storage {_lib.storage()}")
    for name, (cfg, _, batch, full) in vh.HALF_CASES.items():
        vision(name, cfg, (1, 64, 200) if full else (1, batch, 7))
    for name, (cfg, _, batch, T, _, full) in th.HALF_CASES.items():
        text(name, cfg, ((1, 1), (batch, T), (7, 33)) + (((51, 77),) if full else ()))
    # the refusals
    vision("fp32 tiny (head dim 16)", TINY_GELU, (2,))
    tiny_v = vh.HALF_CASES["half_tiny_d64"][0]
    vision("hidden 192 / 3 heads", dataclasses.replace(tiny_v, hidden_size=192, intermediate_size=768, num_attention_heads=3), (3,))
    vision("half_tiny_d64, bad batches", tiny_v, (0, -1, 65536))
    vision("half_tiny_d64, hidden 136 (head dim 68)", dataclasses.replace(tiny_v, hidden_size=136), (2,))
    vision("half_tiny_d64, intermediate 260", dataclasses.replace(tiny_v, intermediate_size=260), (2,))
    vision("vit_h_14, offsets", vh.HALF_CASES["vit_h_14"][0], (2000,))
    for cfg, d in ((clip_ref.TINY_CLIP, 16), (clip_ref.TINY_CLIP_GELU, 32)):
        text(f"fp32 tiny (head dim {d})", cfg, ((2, 20),))
    tiny_t = th.HALF_CASES["thalf_tiny_77"][0]
    text("128 positions", dataclasses.replace(tiny_t, max_position_embeddings=128), ((2, 128), (2, 129), (2, 0), (2, -1), (0, 77), (65536, 77)))
    text("77 positions", tiny_t, ((2, 78),))
    text("hidden 132", dataclasses.replace(tiny_t, hidden_size=132), ((2, 20),))
    text("intermediate 260", dataclasses.replace(tiny_t, intermediate_size=260), ((2, 20),))
    text("sd2_openclip_h, offsets", th.HALF_CASES["sd2_openclip_h"][0], ((60000, 77),))
    p = _lib.CLIPVHalfPlanC()
    for fn, args in (("dfh_clipvh_plan", (None, 1, C.byref(p))), ("dfh_cliph_plan", (None, 1, 1, C.byref(_lib.CLIPTHalfPlanC())))):
        try:
            _lib.call(fn, *args)
        except _lib.DfhError as e:
            print(f"{fn}(NULL): refused: {e}")


if __name__ == "__main__":
    main()
