"""No GPU: the fp16-storage build of the kernel library (csrc/Makefile, -DDFH_F16 -> libdifashion_hip_f16.so) and its per-process
selection (DFH_STORAGE / difashion_amd.set_storage)."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

from difashion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "difashion_amd", "csrc")
F16_LIB = os.path.join(CSRC, "libdifashion_hip_f16.so")
LLVM = "/opt/rocm/lib/llvm/bin"


def run_child(code, storage=None):
    env = {k: v for k, v in os.environ.items() if k not in ("DFH_STORAGE", "DFH_LIB")}
    if storage is not None:
        env["DFH_STORAGE"] = storage
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def exported(lib):
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--dyn-syms", "-W", lib], capture_output=True, text=True, check=True).stdout
    rows = [l.split() for l in out.splitlines()]
    return sorted(r[-1] for r in rows if len(r) >= 8 and r[3] == "FUNC" and r[6] != "UND" and r[-1].startswith("dfh_"))


def test_both_libraries_are_built_with_one_abi_and_one_symbol_set():
    _lib.build()
    assert os.path.exists(F16_LIB) and os.path.exists(os.path.join(CSRC, "libdifashion_hip.so"))
    a, b = exported(os.path.join(CSRC, "libdifashion_hip.so")), exported(F16_LIB)
    assert a == b and set(_lib.SIGNATURES) <= set(b)
    code = "from difashion_amd import _lib; l = _lib.raw(); print(l.dfh_abi_version(), _lib.ABI_VERSION, l.dfh_build_info().decode())"
    d, h = run_child(code), run_child(code, "fp16")
    assert d.split()[0] == d.split()[1] == h.split()[0] == h.split()[1] == str(_lib.ABI_VERSION)
    assert "storage=bf16" in d and "storage=fp16" in h and "gfx950" in h


def disassembly(obj):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", obj], check=True, capture_output=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True, capture_output=True)
        return subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout


FORWARD_OBJECTS = ("gemm.o", "gemm_wide.o", "mlp_fused2.o", "attention.o", "attention_x32.o", "winograd.o")


def test_fp16_code_objects_no_spills_and_fp16_mfma_only():
    """The zero-scratch rule of test_cabi_cpu.py::test_no_product_kernel_spills on the fp16 code objects, and the MFMA operand type of
    either library read from its disassembly; the pair conversion is the packed round-to-nearest-even one."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources
    from tests.test_cabi_cpu import _SPILL_ALLOWED
    _lib.build()
    tab = kernel_resources.kernel_table(os.path.join(CSRC, "obj_f16"))
    ref = kernel_resources.kernel_table()
    assert len(tab) > 100 and set(tab) == set(ref)
    bad = {k: (v.get("vgpr_spill_count", 0), v.get("private_segment_fixed_size", 0)) for k, v in tab.items()
           if (v.get("vgpr_spill_count", 0) or v.get("private_segment_fixed_size", 0)) and not any(a in v["mangled"] for a in _SPILL_ALLOWED)}
    assert not bad, bad
    for frag in ("gemm_bf16_kernelILi128ELi160ELi4ELi2ELi2ELb1", "gemm_bf16_kernelILi256ELi320", "gemm_wide_kernelILi256ELi160",
                 "attention_x32_kernelILi40ELi2ELi2", "gn_apply_kernel", "gn_stats_kernel"):
        hits = [k for k, v in tab.items() if frag in v["mangled"]]
        assert hits, frag
        for k in hits:
            assert tab[k].get("private_segment_fixed_size", 0) == 0, (k, tab[k])
    seen = set()
    objects = sorted(o for o in os.listdir(os.path.join(CSRC, "obj_f16")) if o.endswith(".o"))
    assert set(FORWARD_OBJECTS) <= set(objects) and len(objects) >= 20
    for o in objects:
        try:
            f16, bf = disassembly(os.path.join(CSRC, "obj_f16", o)), disassembly(os.path.join(CSRC, o))
        except subprocess.CalledProcessError:
            assert o not in FORWARD_OBJECTS, o                 # a host-only object has no device code
            continue
        assert not re.search(r"v_mfma_\w*_f16\b", bf) and "v_cvt_pk_f16_f32" not in bf, o       # the whole bf16 library: no fp16 MFMA
        assert "v_cvt_pkrtz" not in f16, o                     # round toward zero would cost half a bit
        if o not in FORWARD_OBJECTS:
            continue
        assert not re.search(r"v_mfma_\w*bf16", f16), o
        seen |= set(re.findall(r"v_mfma_f32_\w+_f16\b", f16))
        if o != "winograd.o":                                  # the Winograd transforms convert; their products run on the GEMM kernels
            assert re.search(r"v_mfma_f32_\w+_f16\b", f16), o
        assert "v_cvt_pk_f16_f32" in f16 and "v_med3_f32" in f16, o      # packed RNE convert behind the +-65504 clamp
    assert {"v_mfma_f32_32x32x16_f16", "v_mfma_f32_16x16x32_f16"} <= seen, seen


def test_fp16_conversion_saturates_and_keeps_nan(tmp_path):
    """The contract of f2bf / pack2bf under -DDFH_F16, read from what the compiler folds them to for gfx950: beyond the range (inf
    included) -> +-65504 (0x7bff / 0xfbff), NaN stays NaN, in-range values round to nearest even; under bf16 nothing is clamped."""
    src = tmp_path / "fold.hip"
    src.write_text('#include "dfh_common.h"\n'
                   "__global__ void fold(volatile uint32_t* o) {\n"      # volatile: one scalar store per value
                   
                   "  o[0] = f2bf(__builtin_nanf(\"\")); o[1] = pack2bf(__builtin_nanf(\"\"), 1.0f); o[2] = f2bf(1.0e6f); o[3] = f2bf(-__builtin_inff());\n"
                   "  o[4] = pack2bf(65520.0f, -70000.0f); o[5] = f2bf(65504.0f); o[6] = f2bf(1.00048828125f); o[7] = f2bf(1.00146484375f);\n"
                   "}\n")
    def fold(flags):
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-emit-llvm",
                            f"-I{CSRC}", *flags, str(src), "-o", "-"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        vals = [int(v) & 0xffffffff for v in re.findall(r"store volatile i32 (-?\d+),", r.stdout)]
        assert len(vals) == 8, r.stdout[-3000:]
        return vals
    v = fold(["-DDFH_F16"])
    is_nan16 = lambda h: (h & 0x7c00) == 0x7c00 and (h & 0x03ff) != 0
    assert is_nan16(v[0] & 0xffff), hex(v[0])
    assert is_nan16(v[1] & 0xffff) and v[1] >> 16 == 0x3c00, hex(v[1])
    assert v[2] == 0x7bff and v[3] == 0xfbff and v[4] == 0xfbff7bff and v[5] == 0x7bff, [hex(x) for x in v]
    assert v[6] == 0x3c00 and v[7] == 0x3c02, [hex(x) for x in v]          # ties to even: 1 + 2^-11 -> 1, 1 + 3 * 2^-11 -> 1 + 2^-9
    b = fold([])
    assert (b[0] & 0x7f80) == 0x7f80 and (b[0] & 0x7f) and b[3] == 0xff80 and b[2] == 0x4974, [hex(x) for x in b]


def test_storage_selection_per_process():
    probe = ("import difashion_amd as da, torch\n"
             "print('S0', da.storage())\n"
             "from oracle import unet_ref\n"
             "m = da.UNet2DConditionModel(sample_size=16, in_channels=8, block_out_channels=(64, 128, 256, 256), cross_attention_dim=64,\n"
             "                            attention_head_dim=(2, 2, 2, 2), init_seed=None)\n"
             "try:\n"
             "    m(torch.zeros(1, 8, 16, 16), 1, torch.zeros(1, 77, 64)); print('RAN')\n"
             "except da.DfhError as e:\n"
             "    print('CPU', 'no CPU fallback' in str(e))\n"
             "da._lib.raw()\n"
             "other = 'bf16' if da.storage() == 'fp16' else 'fp16'\n"
             "try:\n"
             "    da.set_storage(other); print('SWITCHED')\n"
             "except da.DfhError as e:\n"
             "    print('LATE', 'already loaded' in str(e))\n"
             "da.set_storage(da.storage())\n"
             "print('S1', da.storage(), da._lib.raw().dfh_build_info().decode())\n")
    for env, want in ((None, "bf16"), ("fp16", "fp16"), ("bf16", "bf16")):
        out = run_child(probe, env)
        assert f"S0 {want}" in out and f"S1 {want}" in out and f"storage={want}" in out, out
        assert "CPU True" in out and "LATE True" in out and "SWITCHED" not in out and "RAN" not in out, out
    out = run_child("import difashion_amd as da\nda.set_storage('fp16')\nprint(da.storage(), da._lib.raw().dfh_build_info().decode())")
    assert out.startswith("fp16") and "storage=fp16" in out
    env = dict(os.environ, DFH_STORAGE="fp32")
    r = subprocess.run([sys.executable, "-c", "import difashion_amd"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and "'bf16' (default) or 'fp16'" in r.stderr


def test_fp16_library_refuses_training_and_fp8_without_a_gpu():
    code = ("import difashion_amd as da, ctypes as C\nfrom difashion_amd import _lib\n"
            "for n, a in (('dfh_geglu_bwd', (None, None, None, 0, 0, None)), ('dfh_quantize_rows_fp8', (None, 0, None, None, 0, 0, None))):\n"
            "    try:\n        _lib.call(n, *a); print(n, 'RAN')\n"
            "    except da.DfhError as e:\n        print(n, 'REFUSED', e)\n"
            "m = da.UNet2DConditionModel(sample_size=16, in_channels=8, block_out_channels=(64, 128, 256, 256), cross_attention_dim=64,\n"
            "                            attention_head_dim=(2, 2, 2, 2), init_seed=None)\n"
            "try:\n    m.enable_fp8(); print('fp8 RAN')\nexcept da.DfhError as e:\n    print('fp8 REFUSED', e)\n")
    out = run_child(code, "fp16")
    assert "dfh_geglu_bwd REFUSED" in out and "dfh_quantize_rows_fp8 REFUSED" in out and "fp8 REFUSED" in out and "RAN" not in out, out
    assert "training" in out and "bf16 producers" in out
