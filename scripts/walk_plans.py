"""Prints everything the host-side planning code decides, without a GPU: parameter tables, arena sizes and workspace sizes of the
U-Net (inference, fp8, run cache, training) and the VAE.  Two builds of the library plan the same way when their outputs are equal
as text:

    python scripts/walk_plans.py > new.txt
    DFH_LIB=<other build>/libdifashion_hip.so python scripts/walk_plans.py > old.txt
    diff old.txt new.txt

profiles/walk_common_plans.txt is this tree's output."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from difashion_amd import _lib  # noqa: E402

BATCHES = (1, 2, 4, 8, 16)
# name -> (sample_size, block_out_channels, cross_attention_dim, num_heads, use_linear_projection); oracle/unet_ref.py SD15, SD2BASE, TINY
# and tests/helpers.py GLUE_CFG
UNETS = {
    "sd15": (64, (320, 640, 1280, 1280), 768, (8, 8, 8, 8), 0),
    "sd2base": (64, (320, 640, 1280, 1280), 1024, (5, 10, 20, 20), 1),
    "tiny": (16, (64, 128, 256, 256), 64, (2, 2, 2, 2), 0),
    "glue": (16, (32, 64, 128, 128), 64, (1, 2, 2, 2), 0),
}
# name -> (block_out_channels, [(batch, image size)]): the shapes of tests/test_gpu_vae.py and bench.py --mode vae (latent size = image / 8)
VAES = {
    "sd_vae": ((128, 256, 512, 512), [(1, 512), (4, 512), (3, 64), (3, 32)]),
    "mid_vae": ((64, 128, 256, 256), [(3, 64)]),
    "tiny_vae": ((32, 64, 64, 64), [(3, 32), (3, 64)]),
}


def unet_ctx(spec):
    size, boc, xdim, heads, linproj = spec
    c = _lib.UNetConfigC()
    c.sample_size, c.in_channels, c.out_channels, c.num_blocks = size, 8, 4, 4
    for i in range(4):
        c.block_out_channels[i], c.num_heads[i], c.down_attn[i] = boc[i], heads[i], int(i < 3)
    c.layers_per_block, c.cross_attention_dim, c.use_linear_projection = 2, xdim, linproj
    c.norm_num_groups, c.norm_eps, c.text_len = 32, 1e-5, 77
    h = C.c_void_p()
    _lib.call("dfh_unet_create", C.byref(c), C.byref(h))
    return h


def table(lib, kind, h):
    f = lambda n: getattr(lib, f"dfh_{kind}_{n}")
    for i in range(f("num_params")(h)):
        shape = "x".join(str(f("param_dim")(h, i, d)) for d in range(f("param_ndim")(h, i)))
        print(f"  param {i} {f('param_name')(h, i).decode()} {shape}")
    print(f"  arena16_bytes {f('arena16_bytes')(h)}")
    print(f"  arena32_bytes {f('arena32_bytes')(h)}")


def main():
    lib = _lib.raw()
    for name, spec in UNETS.items():
        print(f"unet {name}")
        h = unet_ctx(spec)
        table(lib, "unet", h)
        for b in BATCHES:
            print(f"  workspace_bytes B={b} {lib.dfh_unet_workspace_bytes(h, b)}")
        for b in BATCHES:
            print(f"  run_cache_bytes B={b} n_t=50 {lib.dfh_unet_run_cache_bytes(h, b, 50)}")
        print(f"  arena16t_bytes {lib.dfh_unet_arena16t_bytes(h)}")
        print(f"  grad16_bytes {lib.dfh_unet_grad16_bytes(h)}")
        print(f"  grad32_bytes {lib.dfh_unet_grad32_bytes(h)}")
        for b in BATCHES:
            print(f"  train_workspace_bytes B={b} {lib.dfh_unet_train_workspace_bytes(h, b)}")
        lib.dfh_unet_destroy(h)
        for attn in (0, 1):
            h = unet_ctx(spec)
            _lib.call("dfh_unet_enable_fp8_attention", h, attn)
            _lib.call("dfh_unet_enable_fp8", h)
            print(f"  fp8 attention={attn} arena8_bytes {lib.dfh_unet_arena8_bytes(h)}")
            for b in BATCHES:
                print(f"  fp8 attention={attn} workspace_bytes B={b} {lib.dfh_unet_workspace_bytes(h, b)}")
                print(f"  fp8 attention={attn} run_cache_bytes B={b} n_t=50 {lib.dfh_unet_run_cache_bytes(h, b, 50)}")
            lib.dfh_unet_destroy(h)
    for name, (boc, shapes) in VAES.items():
        print(f"vae {name}")
        c = _lib.VAEConfigC(3, 3, 4, 4, (C.c_int * 4)(*boc), 2, 32)
        h = C.c_void_p()
        _lib.call("dfh_vae_create", C.byref(c), C.byref(h))
        table(lib, "vae", h)
        for b, s in shapes:
            print(f"  workspace_bytes encode B={b} size={s} {lib.dfh_vae_workspace_bytes(h, 1, b, s)}")
            print(f"  workspace_bytes decode B={b} size={s // 8} {lib.dfh_vae_workspace_bytes(h, 0, b, s // 8)}")
        lib.dfh_vae_destroy(h)


if __name__ == "__main__":
    main()
