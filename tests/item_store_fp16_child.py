"""Child-process body of tests/test_gpu_item_store.py::test_fp16_storage_library_gives_the_same_bits: the storage format is a property
of the process (tests/fp16_child.py), so one gather and one history case run here under DFH_STORAGE=fp16
(``python -m tests.item_store_fp16_child``) and print their results' bits as one line ``ITEM_STORE_FP16_RESULT {...}``."""
import json

import torch

import difashion_amd as da
from tests import helpers_item_store as H
from tests.gpu_util import DEV


def case(device):
    """The shared case of parent and child: row_elems 256, 5 rows."""
    row_elems, rows = 256, 5
    table = H.make_table(H.ITEMS, row_elems, seed=3)
    ids = H.gather_ids(rows, H.ITEMS, seed=6)
    eps = torch.randn(rows, row_elems, generator=torch.Generator().manual_seed(7))
    segs, row_seg = H.make_segments(H.ITEMS, seed=5), H.row_segments(rows)
    null = torch.full((row_elems,), 0.25)
    d = lambda t: t.to(device)
    gathered = H.run_gather(d(table), row_elems, d(ids), d(eps), H.SCALE)
    hist = H.run_history(d(table), row_elems, *H.history_device_inputs(segs, row_seg, device), d(null), H.SCALE)
    torch.cuda.synchronize()
    return gathered, hist


def main():
    assert da.storage() == "fp16", "start this process with DFH_STORAGE=fp16"
    gathered, hist = case(DEV)
    print("ITEM_STORE_FP16_RESULT " + json.dumps({"storage": da.storage(), "build_info": da._lib.raw().dfh_build_info().decode(),
                                                  "gather": H.bits(gathered).flatten().tolist(), "history": H.bits(hist).flatten().tolist()}),
          flush=True)


if __name__ == "__main__":
    main()
