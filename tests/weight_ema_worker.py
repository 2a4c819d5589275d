"""Worker for tests/test_weight_ema.py::test_two_ranks_keep_identical_shadows: one process per rank (gloo, CPU tensors, kernels through
the host emulator).  Launched with torch.distributed.run; two steps of the tiny model on different data per rank, with the generator's
weight EMA on; every rank writes its parameters and its shadow into $VQ_WEMA_OUT."""
import os
import sys
import warnings

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")
import vqgan_training_amd as vq  # noqa: E402
from vqgan_training_amd import ops  # noqa: E402
from oracle import weights as W  # noqa: E402

RES, CH, STEPS, DECAY = 16, 32, 2, 0.5


def main():
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    vq._lib._set_library_for_tests(vq._lib.VqLibrary(os.path.join(ROOT, "tests", "emu", "libvqhip_emu.so")))
    ops.set_default_precision("fp32x3")
    vae = vq.ae.VAE(RES, 3, CH, 3, [1, 2], 1, 4, False, False, False)
    vae.load_state_dict(W.randomize_state_dict(vae.state_dict(), 1 + rank))     # different weights per rank before the broadcast
    lp = vq.utils.LPIPS(pretrained_path=None)
    lp.load_state_dict(W.randomize_state_dict(lp.state_dict(), 2, relu_net=True))
    lp.eval()
    vq.distributed.broadcast_parameters(vae)            # BEFORE the step object: every rank's shadow starts from rank 0's bits
    step = vq.vae_trainer.VAETrainStep(vae, lp, None, learning_rate_vae=1e-2, vae_ch=CH, max_steps=10, warmup_steps=0,
                                       bucket_bytes=64 << 10, ema_decay=DECAY)
    start = [e.detach().clone() for e in step.optimizer_G.ema_parameters()]
    for it in range(STEPS):
        step(W.image_batch(1, RES, seed=60 + 10 * it + rank))
    torch.save({"rank": rank, "start": start, "ema": [e.detach().clone() for e in step.optimizer_G.ema_parameters()],
                "params": [p.detach().clone() for g in step.optimizer_G.param_groups for p in g["params"]]},
               os.path.join(os.environ["VQ_WEMA_OUT"], f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
