"""Child-process body of tests/test_gpu_grounding.py::test_fp16_storage_library_gives_the_same_bits: the storage format is a property of
the process (tests/fp16_child.py), so the ranking of one fixture case runs here under DFH_STORAGE=fp16
(``python -m tests.grounding_fp16_child <case>``) and prints its results' bits as one line ``GROUNDING_FP16_RESULT {...}``."""
import json
import sys

import torch

import difashion_amd as da
from tests import helpers_grounding as H
from tests.gpu_util import DEV


def main(case):
    assert da.storage() == "fp16", "start this process with DFH_STORAGE=fp16"
    inp = H.case_inputs(case)
    ranked = da.rank_candidates(inp["gen"].to(DEV), inp["table"].to(DEV), inp["candidates"], H.TOPN[-1])
    torch.cuda.synchronize()
    print("GROUNDING_FP16_RESULT " + json.dumps({"storage": da.storage(), "build_info": da._lib.raw().dfh_build_info().decode(),
                                                 "ids": ranked.ids.flatten().tolist(), "positions": ranked.positions.flatten().tolist(),
                                                 "sims": ranked.sims.flatten().cpu().view(torch.int32).tolist(),
                                                 "counts": ranked.counts.tolist()}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
