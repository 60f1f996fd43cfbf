"""The item store without a GPU: the two entry points are declared, built into both libraries and bound with matching
argument counts; every host refusal fires, by message, on made-up aligned addresses; the HistoryTable's CSR arrays and lookups by int
and by 0-d tensor; save / load and from_latents on CPU-side metadata; and the pure-torch emulation the GPU tests compare against is
itself held to fp64 under the derived bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from tests import helpers_item_store as H
from tests.helpers_data import synthetic_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dfh_item_gather", "dfh_history_rows"]
P = C.c_void_p(256)              # a non-null, 16-byte aligned stand-in: every guard below fires before a pointer is followed
ODD = C.c_void_p(264)
NULL = C.c_void_p(0)


def test_new_symbols_in_header_both_libraries_and_binding():
    src = open(os.path.join(ROOT, "include", "difashion_hip.h")).read()
    assert "#define DFH_ABI_VERSION 8" in src                    # additive: the ABI number stays
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.raw()
    f16 = C.CDLL(os.path.join(_lib.CSRC, "libdifashion_hip_f16.so"))
    for n in NEW_SYMBOLS:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, decl, flags=re.S)
        assert m, n
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[n][1]), n
        assert hasattr(lib, n) and hasattr(f16, n), n
    assert lib.dfh_abi_version() == 8
    for name in ("ItemLatentStore", "HistoryTable"):
        assert name in da.__all__ and hasattr(da, name)
    assert hasattr(da.data, "build_item_store") and hasattr(da.data, "history_table")
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert len(re.findall(r"item_store\.o: item_store\.hip \$\(HDRS\)\n\t(?:@mkdir[^\n]*\n\t)?\$\(HIPCC\) \$\((?:CXX|F16)FLAGS\) -ffp-contract=off", mk)) == 2


def gather_call(**kw):
    a = dict(table=P, table_rows=10, row_stride=32, row_elems=16, iids=P, rows=3, eps=P, scale=1.0, out=P)
    a.update(kw)
    _lib.call("dfh_item_gather", a["table"], a["table_rows"], a["row_stride"], a["row_elems"], a["iids"], a["rows"], a["eps"], a["scale"], a["out"],
              NULL)


def history_call(**kw):
    a = dict(table=P, table_rows=10, row_stride=32, row_elems=16, seg_items=P, seg_offsets=P, row_seg=P, rows=3, null_row=P, scale=1.0, out=P)
    a.update(kw)
    _lib.call("dfh_history_rows", a["table"], a["table_rows"], a["row_stride"], a["row_elems"], a["seg_items"], a["seg_offsets"], a["row_seg"],
              a["rows"], a["null_row"], a["scale"], a["out"], NULL)


def test_gather_refusals_are_reached_without_a_device():
    for k in ("table", "iids", "out"):
        with pytest.raises(da.DfhError, match="null argument"):
            gather_call(**{k: NULL})
    for kw in (dict(row_elems=18, row_stride=36), dict(row_stride=34)):
        with pytest.raises(da.DfhError, match="multiples of 4"):
            gather_call(**kw)
    with pytest.raises(da.DfhError, match="row_stride smaller than row_elems"):
        gather_call(row_stride=12, eps=NULL)
    with pytest.raises(da.DfhError, match=r"row_stride smaller than 2 \* row_elems"):
        gather_call(row_stride=16)
    for k in ("table", "eps", "out"):
        with pytest.raises(da.DfhError, match="16-byte aligned"):
            gather_call(**{k: ODD})
    for kw in (dict(rows=-1), dict(table_rows=-1), dict(row_elems=0), dict(row_elems=-4)):
        with pytest.raises(da.DfhError, match="negative table_rows / rows, or row_elems not positive"):
            gather_call(**kw)
    # legal without a launch: a means-only table with eps absent and no rows
    gather_call(row_stride=16, eps=NULL, rows=0)


def test_history_refusals_are_reached_without_a_device():
    for k in ("table", "seg_items", "seg_offsets", "row_seg", "null_row", "out"):
        with pytest.raises(da.DfhError, match="null argument"):
            history_call(**{k: NULL})
    for kw in (dict(row_elems=18, row_stride=36), dict(row_stride=34)):
        with pytest.raises(da.DfhError, match="multiples of 4"):
            history_call(**kw)
    with pytest.raises(da.DfhError, match="row_stride smaller than row_elems"):
        history_call(row_stride=12)
    for k in ("table", "null_row", "out"):
        with pytest.raises(da.DfhError, match="16-byte aligned"):
            history_call(**{k: ODD})
    for kw in (dict(rows=-1), dict(table_rows=-1), dict(row_elems=0)):
        with pytest.raises(da.DfhError, match="negative table_rows / rows, or row_elems not positive"):
            history_call(**kw)
    history_call(row_stride=16, rows=0)                          # a means-only table is legal here


def test_history_table_csr_and_lookups():
    _, _, history, latents = synthetic_dataset()
    store = da.ItemLatentStore.from_latents(latents, 0.18215)
    ht = da.HistoryTable(history, store)
    assert len(ht) == 5
    assert ht.offsets == [0, 2, 3, 6, 10, 11] and ht.items == [1, 3, 5, 2, 8, 11, 4, 6, 9, 12, 10]
    assert ht.seg_offsets.tolist() == ht.offsets and ht.seg_items.tolist() == ht.items
    assert ht.seg_offsets.dtype == torch.int64 and ht.seg_items.dtype == torch.int64
    assert ht.segment_of == {(7, 1): 0, (7, 2): 1, (7, 5): 2, (9, 3): 3, (9, 4): 4}
    uids, cates = [7, 7, 9, 9, 7], [1, 5, 4, 3, 2]
    assert ht.segment_ids(uids, cates) == [0, 2, 4, 3, 1]
    # keys by integer value: 0-d tensors, tensors of another dtype, numpy integers
    assert ht.segment_ids([torch.tensor(u) for u in uids], [torch.tensor(c, dtype=torch.int32) for c in cates]) == [0, 2, 4, 3, 1]
    assert ht.segment_ids(torch.tensor(uids), list(torch.tensor(cates))) == [0, 2, 4, 3, 1]
    assert ht.segment_ids(np.array(uids), np.array(cates)) == [0, 2, 4, 3, 1]
    # a missing user, a missing category, use_history=False
    assert ht.segment_ids([8, 7, 9, torch.tensor(9)], [1, 3, 1, torch.tensor(5)]) == [-1, -1, -1, -1]
    assert ht.segment_ids(uids, cates, use_history=False) == [-1] * 5
    with pytest.raises(ValueError, match="2 uids for 1 categories"):
        ht.segment_ids([7, 7], [1])
    with pytest.raises(IndexError, match=r"history\[7\]\[1\]: item id out of range \[0, 13\): 13"):
        da.HistoryTable({7: {1: [1, 13]}}, store)
    empty = da.HistoryTable({}, store)
    assert len(empty) == 0 and empty.offsets == [0] and empty.segment_ids([7], [1]) == [-1]
    # data.history_latents' dict carries a "null" entry beside the users; the raw dict does not, and the entry is no user
    assert da.HistoryTable({**history, "null": latents[0]}, store).offsets == ht.offsets
    assert da.data.history_table(store, history).items == ht.items
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        ht.rows(uids, cates, latents[0])


def test_store_metadata_save_load_and_from_latents(tmp_path):
    _, _, _, latents = synthetic_dataset()
    st = da.ItemLatentStore.from_latents(latents.numpy(), 0.18215)
    assert len(st) == 13 and st.latent_shape == (4, 8, 8) and st.row_elems == 256 and st.nbytes == 13 * 256 * 4
    assert st.scale == 1.0 and st.scaling_factor == 0.18215 and not st.has_std and st.table.shape == (13, 256)
    assert torch.equal(st.table.reshape(13, 4, 8, 8), latents)
    with pytest.raises(ValueError, match="means only"):
        st.sample([1, 2])
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        st.modes([1, 2])
    for bad in ([13], [-1], torch.tensor([0, 99])):
        with pytest.raises(IndexError, match=r"out of range \[0, 13\)"):
            st.modes(bad)
    with pytest.raises(TypeError, match="integers"):
        st.modes(torch.tensor([0.5]))
    full = da.ItemLatentStore(H.make_table(6, 64, seed=2), (4, 4, 4), 0.18215, 0.18215, True)
    assert len(full) == 6 and full.nbytes == 6 * 128 * 4 and full.has_std
    for s in (st, full):
        path = str(tmp_path / ("store%d" % len(s)))
        s.save(path)
        assert sorted(os.listdir(tmp_path)) and os.path.exists(path + ".npy") and os.path.exists(path + ".json")
        back = da.ItemLatentStore.load(path, "cpu")
        assert torch.equal(back.table, s.table) and back.latent_shape == s.latent_shape and back.has_std == s.has_std
        assert back.scale == s.scale and back.scaling_factor == s.scaling_factor and len(back) == len(s)
    with pytest.raises(ValueError, match="needs 128"):
        da.ItemLatentStore(torch.zeros(3, 64), (4, 4, 4), 1.0, 1.0, True)
    with pytest.raises(ValueError, match="multiple of 4"):
        da.ItemLatentStore(torch.zeros(3, 6), (1, 2, 3), 1.0, 1.0, False)


def test_difashion_refuses_a_missing_null_image_without_a_store():
    m = da.DiFashion.__new__(da.DiFashion)
    with pytest.raises(ValueError, match="null_img=None needs an ItemLatentStore"):
        m._null_latent(None, None)


@pytest.mark.parametrize("row_elems", [16, 256])
def test_emulation_against_fp64_and_exact_data(row_elems):
    segs = H.make_segments(H.ITEMS, seed=5)
    row_seg = H.row_segments(33)
    assert sorted(len(s) for s in segs) == sorted(H.SEG_LENS) and {len(segs[s]) for s in row_seg if s >= 0} == set(H.SEG_LENS)
    assert row_seg[0] == -1 and row_seg[-1] == -1 and any(i == 0 for s in segs for i in s) and any(i == H.ITEMS - 1 for s in segs for i in s)
    table = H.make_table(H.ITEMS, row_elems, seed=3)
    null = torch.full((row_elems,), 0.25)
    got = H.emulate_history(table, row_elems, segs, row_seg, null, H.SCALE)
    ref, bound = H.history_ref64(table, row_elems, segs, row_seg, null, H.SCALE)
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all())
    live = bound > 0
    print(f"emulation vs fp64, row_elems {row_elems}: worst error / bound {float((err[live] / bound[live]).max()):.3f}")
    assert H.same_bits(got[0], null) and H.same_bits(got[3], null) and H.same_bits(got[-1], null)      # null first, empty segment, null last
    assert not H.exact_condition(table, row_elems, segs, H.SCALE)
    exact = H.make_table(H.ITEMS, row_elems, seed=4, exact=True)
    assert H.exact_condition(exact, row_elems, segs, 1.0) and not H.exact_condition(exact, row_elems, segs, H.SCALE)
    assert H.same_bits(H.emulate_history(exact, row_elems, segs, row_seg, null, 1.0), H.torch_mean_history(exact, row_elems, segs, row_seg, null))
    # the gather: its emulation is the torch expression of DiagonalGaussianDistribution.sample() * sf itself
    ids = H.gather_ids(5, H.ITEMS, seed=6)
    eps = torch.randn(5, row_elems, generator=torch.Generator().manual_seed(7))
    want = (table[ids, :row_elems] + table[ids, row_elems:] * eps) * H.SCALE
    assert H.same_bits(H.emulate_gather(table, row_elems, ids, eps, H.SCALE), want)
    assert H.same_bits(H.emulate_gather(table, row_elems, ids, None, H.SCALE), table[ids, :row_elems] * H.SCALE)
    bad = H.emulate_gather(table, row_elems, [1, H.ITEMS, 2, -1], None, 1.0)
    assert bool(bad[1].isnan().all()) and bool(bad[3].isnan().all()) and H.same_bits(bad[0], table[1, :row_elems]) and H.same_bits(bad[2], table[2, :row_elems])
