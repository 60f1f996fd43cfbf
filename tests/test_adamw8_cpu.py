"""CPU (-m "not gpu"): the host side of the block-wise 8-bit optimizer states -- the tables the library owns (dfh_q8_table, no GPU
needed) against the formulas restated in tests/helpers_adamw8.py, the C-ABI prototypes, and the refusals of da.AdamW8bit."""
import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib, training
from tests import helpers_adamw8 as h8


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_q8_table_matches_the_restated_formula(signed):
    got, want = training.q8_table(signed), h8.table(signed)
    assert got.dtype == np.float32 and got.shape == (256,) and want.shape == (256,)
    assert np.all(np.diff(got.astype(np.float64)) > 0), "not strictly ascending"
    # within 1 ulp of fp32: neighbouring floats have neighbouring bit patterns (same sign), and 0 must be exact
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert int(ulps.max()) <= 1, int(ulps.max())
    assert got[h8.zero_code(signed)] == 0.0 and got[255] == 1.0
    assert np.count_nonzero(got == 0.0) == 1
    if signed:
        assert got[0] > -1.0 and got[0] == -got[254] and np.array_equal(got[:127], -got[254:127:-1])      # no -1; symmetric otherwise
    else:
        assert got[1] == np.float32(3.25e-7)          # the floor's code


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_q8_table_largest_distance_to_the_nearest_entry(signed):
    t = training.q8_table(signed).astype(np.float64)
    lo = -1.0 if signed else 0.0
    grid = np.linspace(lo, 1.0, 4_000_001)
    pos = np.clip(np.searchsorted(t, grid), 1, 255)
    dist = np.minimum(np.abs(grid - t[pos - 1]), np.abs(grid - t[pos]))
    # the exact figure is half the widest gap between neighbours inside the range (and the distance from -1 to the first entry)
    exact = max(float(np.diff(t).max()) / 2, float(t[0] - lo))
    assert abs(float(dist.max()) - h8.MAX_GAP[signed]) <= 1e-6, float(dist.max())
    assert abs(exact - h8.MAX_GAP[signed]) <= 1e-6, exact


def test_the_four_entry_points_have_prototypes():
    lib = _lib.raw()
    for name in ("dfh_q8_table", "dfh_q8_quantize", "dfh_q8_dequantize", "dfh_adamw8"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert len(_lib.SIGNATURES["dfh_adamw8"][1]) == 18
    assert lib.dfh_abi_version() == 8
    with pytest.raises(_lib.DfhError, match="null"):
        _lib.call("dfh_q8_table", 1, None)


def test_device_entry_points_refuse_bad_arguments_before_any_launch():
    """Null pointers, a length that is no multiple of the block and misaligned buffers fail with a message; nothing is launched (there
    is no GPU here)."""
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, None, 0.0, 0.0, None)
    if _lib.storage() != "bf16":          # the fp16-storage library refuses the optimizer outright, like dfh_adamw
        with pytest.raises(_lib.DfhError, match="fp16-storage"):
            _lib.call("dfh_adamw8", 64, 64, 64, 64, 64, 64, None, 64, *hyper)
        return
    with pytest.raises(_lib.DfhError, match="null"):
        _lib.call("dfh_adamw8", None, 64, 64, 64, 64, 64, None, 64, *hyper)
    with pytest.raises(_lib.DfhError, match="multiple of the 64-element block"):
        _lib.call("dfh_adamw8", 64, 64, 64, 64, 64, 64, None, 100, *hyper)
    with pytest.raises(_lib.DfhError, match="16-byte aligned"):
        _lib.call("dfh_adamw8", 72, 64, 64, 64, 64, 64, None, 64, *hyper)
    for name in ("dfh_q8_quantize", "dfh_q8_dequantize"):
        with pytest.raises(_lib.DfhError, match="null"):
            _lib.call(name, None, 64, 64, 64, 1, None)
        with pytest.raises(_lib.DfhError, match="multiple of the 64-element block"):
            _lib.call(name, 64, 64, 64, 96, 1, None)
    with pytest.raises(_lib.DfhError, match="16-byte aligned"):
        _lib.call("dfh_q8_quantize", 68, 64, 64, 64, 0, None)


def test_adamw8bit_is_exported_and_refuses_cpu_tensors_like_its_parent():
    assert issubclass(da.AdamW8bit, da.FusedAdamW) and "AdamW8bit" in da.__all__
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(da.DfhError, match="HIP path only"):
        da.AdamW8bit([p], lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8)      # the reference's call (train.py:586-593)
    with pytest.raises(da.DfhError, match="HIP path only"):
        da.FusedAdamW([p])


def test_min_8bit_size_is_refused_by_name():
    p = torch.nn.Parameter(torch.zeros(8))
    with pytest.raises(da.DfhError, match="min_8bit_size"):
        da.AdamW8bit([p], min_8bit_size=4096)


def test_restatement_quantiser_is_self_consistent():
    """The yardstick itself: a round trip stays inside the table's largest distance, the floor and the zero block hold."""
    for signed in (True, False):
        x = h8.hard_blocks(64 * 12, seed=1, signed=signed)
        codes, am = h8.quantize(x, signed)
        assert np.array_equal(am, h8.block_absmax(x))
        back = h8.dequantize(codes, am, signed).astype(np.float64)
        assert np.all(np.abs(back - x) <= h8.MAX_GAP[signed] * 1.0001 * np.repeat(am.astype(np.float64), 64) + 1e-45)
        assert np.all(codes[:64] == h8.zero_code(signed)) and np.all(back[:64] == 0.0) and am[0] == 0.0
        if not signed:
            assert np.all(codes[x > 0] >= 1) and np.any(h8.floor_applies(x, am, signed))
