"""Child-process body of tests/test_gpu_lpips.py::test_fp16_storage_library_gives_the_same_bits: the storage format is a property of the
process (tests/fp16_child.py), so the LPIPS walk of one fixture case runs here under DFH_STORAGE=fp16
(``python -m tests.lpips_fp16_child <case>``) and prints its results' bits as one line ``LPIPS_FP16_RESULT {...}``."""
import json
import sys

import torch

import difashion_amd as da
from tests import helpers_lpips as H
from tests.gpu_util import DEV


def main(case):
    assert da.storage() == "fp16", "start this process with DFH_STORAGE=fp16"
    model = da.LPIPS(init_seed=None)
    model.load_state_dict(H.make_params())
    model = model.to(DEV)
    a, b = H.case_inputs(case)
    val, layers = model(a.to(DEV), b.to(DEV), retPerLayer=True)
    torch.cuda.synchronize()
    bits = lambda t: t.flatten().cpu().view(torch.int32).tolist()
    print("LPIPS_FP16_RESULT " + json.dumps({"storage": da.storage(), "build_info": da._lib.raw().dfh_build_info().decode(), "total": bits(val),
                                             "layers": [bits(t) for t in layers]}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
