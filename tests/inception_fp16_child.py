"""Child-process body of tests/test_gpu_inception.py::test_fp16_storage_library_gives_the_same_bits: the storage format is a property of
the process (tests/fp16_child.py), so the Inception walk of one fixture case runs here under DFH_STORAGE=fp16
(``python -m tests.inception_fp16_child <case>``) and prints its results' bits as one line ``INCEPTION_FP16_RESULT {...}``."""
import json
import sys

import torch

import difashion_amd as da
from tests import helpers_inception as H
from tests.gpu_util import DEV


def main(case):
    assert da.storage() == "fp16", "start this process with DFH_STORAGE=fp16"
    variant, params, x, _ = H.load_case(case)
    assert variant == "fid"
    model = da.FIDInceptionV3((0, 1, 2, 3), init_seed=None)
    model.load_state_dict(params)
    model = model.to(DEV)
    taps = model(x.to(DEV))
    torch.cuda.synchronize()
    bits = lambda t: t.flatten().cpu().view(torch.int32).tolist()
    print("INCEPTION_FP16_RESULT " + json.dumps({"storage": da.storage(), "build_info": da._lib.raw().dfh_build_info().decode(),
                                                 "taps": [bits(t) for t in taps]}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
