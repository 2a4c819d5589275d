"""Worker for tests/test_vq_ema.py::test_rank_split_independence: one process per rank (gloo, CPU tensors, kernels through the host
emulator).  Launched with torch.distributed.run; every rank holds its half of the batch and writes N, m and the codebook after every
step into $VQ_EMA_OUT.  `run_steps` is also what the test itself runs, in one process, on the whole batch."""
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")
import vqgan_training_amd as vq  # noqa: E402
from oracle import weights as W  # noqa: E402

K, D, STEPS = 48, 8, 4


def batches():
    """The global batches [4, D, 4, 8] (128 tokens): tokens spread over a few codes' neighbourhoods, magnitudes O(1)."""
    return [W.uniform_tensor((4, D, 4, 8), 500 + s, -1, 1) * (1.0 + 0.5 * s) for s in range(STEPS)]


def make_quantizer():
    # decay 0.7: an unused code's N is 0.49 after two updates, so the reseeding of step 1 (and 3) finds dead codes
    q = vq.quantizer.VectorQuantizer(K, D, beta=0.25, ema=True, decay=0.7, eps=1e-5, init_from_data=True, reseed_below=0.5,
                                     reseed_every=2, seed=11)
    with torch.no_grad():
        q.embedding.weight.copy_(W.uniform_tensor((K, D), 77, -1.5, 1.5))
        q.ema_embed_sum.copy_(q.embedding.weight)
    return q


def run_steps(q, rank, world):
    """-> per step (N, m, codebook, indices of this rank's tokens)"""
    out = []
    for z in batches():
        per = z.shape[0] // world
        zl = z[rank * per:(rank + 1) * per].clone().requires_grad_()
        _, loss, idx = q(zl)
        loss.backward()
        usage = q.ema_update()
        out.append({"N": q.ema_cluster_size.clone(), "m": q.ema_embed_sum.clone(), "cb": q.embedding.weight.detach().clone(),
                    "idx": idx.clone(), "usage": usage.clone()})
    return out


def main():
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    vq._lib._set_library_for_tests(vq._lib.VqLibrary(os.path.join(ROOT, "tests", "emu", "libvqhip_emu.so")))
    q = make_quantizer()
    if rank != 0:                                  # rank 0's state must reach everybody: codebook, N and m in ONE coalesced broadcast
        with torch.no_grad():
            q.embedding.weight.zero_(); q.ema_embed_sum.zero_(); q.ema_cluster_size.fill_(7.0)
    issued = vq.distributed.broadcast_parameters(q)
    res = {"steps": run_steps(q, rank, world), "broadcasts": issued, "rank": rank}
    torch.save(res, os.path.join(os.environ["VQ_EMA_OUT"], f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
