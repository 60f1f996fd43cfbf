"""Child-process body of tests/test_gpu_sched_multistep.py::test_fp16_storage_library_gives_the_same_bits: the storage format is a
property of the process (tests/fp16_child.py), so the two kernel cases run here under DFH_STORAGE=fp16
(``python -m tests.sched_multistep_fp16_child``) and print their results' bits as one line ``SCHED_MULTISTEP_FP16_RESULT {...}``."""
import json

import torch

import difashion_amd as da
from tests import helpers_sched_multistep as H

FP16_CASES = {"dpm2": ("full", (3, 4, 8, 8), H.CONV_X0_EPS, H.DPM2, 1), "plms4": ("cate_hist", (1, 4, 5, 5), H.CONV_NONE, H.PLMS, 4)}


def case_bits(name):
    mode, shape, conv, kind, terms = FP16_CASES[name]
    got = H.check_kernel_case(mode, shape, conv, kind, terms, seed=7)
    return {k: v.flatten().view(torch.int32).tolist() for k, v in got.items()}


def main():
    assert da.storage() == "fp16", "start this process with DFH_STORAGE=fp16"
    print("SCHED_MULTISTEP_FP16_RESULT " + json.dumps({"storage": da.storage(), "build_info": da._lib.raw().dfh_build_info().decode(),
                                                       "cases": {n: case_bits(n) for n in FP16_CASES}}), flush=True)


if __name__ == "__main__":
    main()
