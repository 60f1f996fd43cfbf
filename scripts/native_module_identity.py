#!/usr/bin/env python3
"""What the Python model wrappers build, as text: run it on two commits and diff the outputs (CPU; needs only the built library).

Per model (U-Net at SD-1.5 defaults and tiny, VAE at defaults and tiny, CLIP tiny and CLIP-L, two tiny CLIP vision towers, LPIPS and the
two Inception v3 variants), once with
``init_seed=0`` and once with ``init_seed=None``: the native ``param_table()``, the ``state_dict()`` key order and a SHA-256 over the
parameter bytes; the ViT-H/14 vision table without its weights.  Then the eight wrappers (MutualEncoder included) through
``save_pretrained`` / ``from_pretrained``: file names, sorted ``config.json`` keys, what the reloaded object keeps in ``.config``,
and whether the state dicts agree bit for bit.  ``--digest`` prints one SHA-256 line per table / key listing instead of the listing.

A refactor of difashion_amd/{_native,unet,vae,clip,clip_vision,mutual,lpips,inception}.py must leave this output unchanged
(profiles/native_module_identity.txt).
The hashes are NOT a test: they would pin torch's CPU generator, not this code."""
import hashlib
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import difashion_amd as da
from tests.helpers_clip_vision import TINY_GELU, TINY_QUICKGELU, VIT_H_14

TINY_UNET = dict(sample_size=16, in_channels=8, block_out_channels=(64, 128, 256, 256), cross_attention_dim=64, attention_head_dim=(2, 2, 2, 2))
TINY_VAE = dict(block_out_channels=(32, 64, 64, 64), sample_size=32)
TINY_CLIP = dict(vocab_size=1000, hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=4, bos_token_id=998,
                 pad_token_id=999)
MODELS = [("unet sd15", da.UNet2DConditionModel, {}), ("unet tiny", da.UNet2DConditionModel, TINY_UNET),
          ("vae default", da.AutoencoderKL, {}), ("vae tiny", da.AutoencoderKL, TINY_VAE),
          ("clip tiny", da.CLIPTextModel, TINY_CLIP), ("clip L", da.CLIPTextModel, {}),
          ("clip vision tiny quick_gelu", da.CLIPVisionModelWithProjection, TINY_QUICKGELU.kwargs()),
          ("clip vision tiny gelu", da.CLIPVisionModelWithProjection, TINY_GELU.kwargs()),
          ("lpips vgg16", da.LPIPS, {}), ("fid inception v3, four blocks", da.FIDInceptionV3, dict(output_blocks=(0, 1, 2, 3))),
          ("inception v3, 50 classes", da.InceptionV3, dict(num_classes=50))]


DIGEST = "--digest" in sys.argv      # one sha256 line per table / key listing instead of the listing: the form that is kept in profiles/


def listing(lines):
    lines = list(lines)
    if DIGEST:
        print(f"listing sha256 {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()} ({len(lines)} lines)")
    else:
        print("\n".join(lines))


def digest(sd):
    h = hashlib.sha256()
    for v in sd.values():
        h.update(v.detach().contiguous().numpy().tobytes())
    return h.hexdigest()


def describe(title, cls, kw):
    first = None
    for seed in (0, None):
        torch.manual_seed(1234)
        m = cls(init_seed=seed, **kw)
        table, keys, sd = m.param_table(), list(m.state_dict().keys()), m.state_dict()
        print(f"== {title}, init_seed={seed}: {len(table)} table entries, {len(keys)} state-dict keys, "
              f"{sum(v.numel() for v in sd.values())} values, dtypes {sorted({str(v.dtype) for v in sd.values()})}")
        if first is None or first != (table, keys):
            listing([f"table {name} {shape}" for name, shape in table] + [f"key {k} {tuple(sd[k].shape)}" for k in keys])
        else:
            print("table and key order: identical to the init_seed=0 build above")
        first = (table, keys)
        print(f"sha256 {digest(sd)}")
        print(f"config {json.dumps(dict(m.config), sort_keys=True)}")
        del m, sd


def round_trip(title, model, load, **load_kw):
    with tempfile.TemporaryDirectory() as d:
        model.save_pretrained(os.path.join(d, "sub"))
        files = sorted(os.listdir(os.path.join(d, "sub")))
        with open(os.path.join(d, "sub", "config.json")) as f:
            text = f.read()
        back = load(d, subfolder="sub", **load_kw)
        flat = load(os.path.join(d, "sub"))
    a, b, c = model.state_dict(), back.state_dict(), flat.state_dict()
    same = list(a) == list(b) == list(c) and all(torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) for k in a)
    print(f"== round trip {title}: files {files}")
    print(f"config.json keys {sorted(json.loads(text))}")
    print(f"config.json sha256 {hashlib.sha256(text.encode()).hexdigest()}")
    print(f"reloaded .config {json.dumps(dict(back.config), sort_keys=True)}")
    print(f"state dicts bit-identical after reload: {same}; sha256 {digest(b)}")
    return back


def main():
    print(f"torch {torch.__version__}")
    for title, cls, kw in MODELS:
        describe(title, cls, kw)
    vit = da.CLIPVisionModelWithProjection(init_seed=None, **TINY_GELU.kwargs())
    vit.register_to_config(**VIT_H_14.kwargs())                         # the full-size table from the library alone: no weights
    table = vit.param_table()
    print(f"== clip vision ViT-H/14: {len(table)} table entries, {sum(torch.Size(s).numel() for _, s in table)} values, no weights")
    listing(f"table {name} {shape}" for name, shape in table)
    unet = da.UNet2DConditionModel(init_seed=3, **TINY_UNET)
    unet.register_to_config(decay=0.9999, optimization_step=7)          # what diffusers' EMAModel.save_pretrained adds
    back = round_trip("unet tiny", unet, da.UNet2DConditionModel.from_pretrained, max_batch=3)
    print(f"max_batch {back.max_batch}")
    # the pipeline's 4 -> 8 channel conv_in replacement: in_channels is written from the module, not from the config
    unet4 = da.UNet2DConditionModel(init_seed=3, **dict(TINY_UNET, in_channels=4))
    unet4.conv_in = torch.nn.Conv2d(8, 64, 3, 1, 1)
    with torch.no_grad():
        unet4.conv_in.weight.copy_(torch.randn(unet4.conv_in.weight.shape, generator=torch.Generator().manual_seed(5)))
    back = round_trip("unet tiny, conv_in replaced", unet4, da.UNet2DConditionModel.from_pretrained)
    print(f"max_batch {back.max_batch}; conv_in {tuple(back.conv_in.weight.shape)}")
    round_trip("vae tiny", da.AutoencoderKL(init_seed=3, **TINY_VAE), da.AutoencoderKL.from_pretrained)
    round_trip("clip tiny", da.CLIPTextModel(init_seed=3, **TINY_CLIP), da.CLIPTextModel.from_pretrained)
    round_trip("clip vision tiny", da.CLIPVisionModelWithProjection(init_seed=3, **TINY_QUICKGELU.kwargs()),
               da.CLIPVisionModelWithProjection.from_pretrained)
    round_trip("lpips vgg16", da.LPIPS(init_seed=3), da.LPIPS.from_pretrained)
    round_trip("fid inception v3", da.FIDInceptionV3((1, 3), resize_input=False, init_seed=3), da.FIDInceptionV3.from_pretrained)
    back = round_trip("inception v3", da.InceptionV3(num_classes=50, init_seed=3), da.InceptionV3.from_pretrained, max_workspace_bytes=1 << 30)
    print(f"max_workspace_bytes {back.max_workspace_bytes}")
    torch.manual_seed(4)
    enc = da.MutualEncoder(cate_num=4, cate_emb_size=8, latent_channels=4, latent_size=16, hid_dim=32)
    enc.register_to_config(decay=0.9999)
    round_trip("mutual encoder", enc, da.MutualEncoder.from_pretrained)


if __name__ == "__main__":
    main()
