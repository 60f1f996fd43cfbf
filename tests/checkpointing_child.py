"""Child of tests/test_gpu_checkpointing.py::test_side_stream_reads_of_recomputed_tensors_are_ordered: forward + backward of the GLUE_CFG
U-Net in checkpointing modes 0 / 1 / 2, twice each, every gradient saved to argv[1] as {(mode, repeat): {name: tensor}}.  The test starts it
with DFH_TRAIN_SIDE_MIN_FLOP=0 (read once per process by the library, hence a process): every weight-gradient launch then runs on the
side stream and reads tensors the recompute wrote on the main stream."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from oracle import unet_ref
from tests.gpu_util import DEV
from tests.helpers import GLUE_CFG
from tests.test_gpu_unet import hip_unet, inputs


def main():
    cfg = GLUE_CFG
    m = hip_unet(cfg, unet_ref.init_params(cfg, seed=5, w_std=0.05), max_batch=4).train()
    x, e = inputs(cfg, 4, 77)
    x, e = x.to(DEV), e.to(DEV)
    t = torch.tensor([3, 250, 750, 990], device=DEV)
    dout = (torch.randn(4, cfg.out_channels, cfg.sample_size, cfg.sample_size, generator=torch.Generator().manual_seed(1)) / 64).to(DEV)
    grads = {}
    for mode in (0, 1, 2):
        if mode:
            m.enable_gradient_checkpointing(keep_attention=mode == 2)
        for rep in range(2):
            for p in m.parameters():
                p.grad = None
            m(x, t, e).sample.backward(dout)
            torch.cuda.synchronize()
            grads[(mode, rep)] = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}
    torch.save(grads, sys.argv[1])


if __name__ == "__main__":
    main()
