"""VQ codebook quantizer on the HIP path (BASELINE.json north_star / config 5).

Not part of the reference (no quantizer/codebook exists in cloneofsimo/vqgan-training; its
`reg` is the identity DiagonalGaussian).  Semantics are the standard VQGAN ones and are pinned by
oracle/vq_oracle.{c,py}: nearest code under |z|^2 - 2 z.e + |e|^2 in a fixed fp32 evaluation order
(bit-exact indices, lowest index on ties), straight-through output, commitment + codebook loss.

`VectorQuantizer(..., ema=True)` trains the codebook without an optimizer instead: exponential-moving-average cluster sizes and sums
from order-independent integer statistics, optional initialisation from encoder outputs and reseeding of dead codes (include/vqhip.h
"EMA codebook"; float64 restatement in tests/test_vq_ema.py).
"""
from __future__ import annotations

import logging
import math

import torch
import torch.distributed as dist
from torch import nn

from ._lib import VQ_F32, lib, ptr, stream_of, workspace


class _VQLookup(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tokens, codebook, beta, lookup_tokens=None, ema=False):
        tokens = tokens.contiguous().float()
        cb = codebook.contiguous().float()
        n, d = tokens.shape
        k = cb.shape[0]
        L = lib()
        ws = workspace(tokens.device, L.size("vq_vq_workspace", n, k))
        idx = torch.empty(n, dtype=torch.int64, device=tokens.device)
        zq = torch.empty_like(tokens)
        md = torch.empty(n, dtype=torch.float32, device=tokens.device)
        # `lookup_tokens`: the tokens the nearest-code search READS when they are not the ones the gradient flows through (policy
        # ref_vq: an fp32-class evaluation of the encoder for the integer work, the binary16 one for the gradients); zq = rows of the
        # codebook either way, the losses and the straight-through output are formed with `tokens`
        look = tokens if lookup_tokens is None else lookup_tokens.contiguous().float()
        L.call("vq_vq_nearest_fwd", ptr(look), ptr(cb), n, k, d, ptr(idx), ptr(zq), ptr(md), ptr(ws), ws.numel(),
               stream_of(tokens))
        ctx.save_for_backward(tokens, zq, idx)
        ctx.beta, ctx.k, ctx.ema = float(beta), k, bool(ema)
        ctx.mark_non_differentiable(idx)
        diff2 = (zq - tokens).pow(2).mean()                  # [n,D] glue on a few hundred KB
        # value of beta*|sg(zq)-z|^2 + |zq-sg(z)|^2; an EMA codebook has no codebook term (it is not trained by a gradient)
        loss = (beta if ema else 1.0 + beta) * diff2
        return zq, loss, idx                                 # zq doubles as the straight-through output

    @staticmethod
    def backward(ctx, g_out, g_loss, _):
        tokens, zq, idx = ctx.saved_tensors
        n, d = tokens.shape
        scale = 2.0 / (n * d)
        diff = zq - tokens
        # straight-through: d out / d z = I ; commitment: beta * 2 (z - zq) / N ; codebook: 2 (zq - z) / N
        gz = g_out - (ctx.beta * scale) * g_loss * diff
        if ctx.ema:                                          # no codebook gradient is built, none is scattered
            return gz, None, None, None, None
        gq = (scale * g_loss * diff).contiguous()
        dcb = torch.zeros(ctx.k, d, dtype=torch.float32, device=tokens.device)
        L = lib()
        ws = workspace(tokens.device, L.size("vq_vq_scatter_workspace", ctx.k, d), slot=2)   # (slot 1 belongs to the side stream)
        L.call("vq_vq_scatter_add", ptr(gq), ptr(idx), n, ctx.k, d, ptr(dcb), ptr(ws), ws.numel(), stream_of(tokens))
        return gz, dcb, None, None, None


def _world():
    return dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1


class VectorQuantizer(nn.Module):
    """forward(z [B,D,h,w]) -> (z_q with straight-through gradient, loss, indices [B,h,w]).

    ema=True: the codebook is a frozen parameter moved by `ema_update()` (call it once per training step, where the optimizer
    steps) from the statistics the training forward leaves behind:
        N_k <- decay N_k + (1 - decay) n_k ;  m_k <- decay m_k + (1 - decay) s_k ;  e_k = m_k / ((N_k + eps) / (sum N + K eps) sum N)
    with n_k / s_k the number / sum of the tokens on code k over ALL ranks (fp32 buffers `ema_cluster_size`, `ema_embed_sum`).  The
    loss is the commitment term alone.  init_from_data: the first training forward replaces every code by a token of its batch
    before the lookup; reseed_below > 0: after the update of every `reseed_every`-th step the codes with N_k < reseed_below are
    replaced by tokens of that step's batch (hash of seed, step and code: include/vqhip.h).  The statistics are integers, so N, m
    and the codebook do not depend on the order of the tokens nor on how a batch is split over ranks.  Nothing moves in eval(),
    under torch.no_grad() or while `frozen` is set (a calibration pass).
    Restrictions: tokens-per-forward * dim must be a multiple of 8 (ValueError otherwise), and with several ranks every rank must
    hold the same number of tokens (checked with one host readback the first time a token count is seen; RuntimeError otherwise).
    Checkpoints carry the codebook, N and m, not `ema_steps` — like the optimizer's step count and the LR schedule, which
    save_checkpoint does not write either: a resumed run restarts the reseeding cadence and the hash's step at 0."""

    def __init__(self, n_codes: int = 16384, dim: int = 32, beta: float = 0.25, *, ema: bool = False, decay: float = 0.99,
                 eps: float = 1e-5, init_from_data: bool = False, reseed_below: float = 0.0, reseed_every: int = 100, seed: int = 0):
        super().__init__()
        self.n_codes, self.dim, self.beta = n_codes, dim, beta
        self.embedding = nn.Embedding(n_codes, dim)
        self.embedding.weight.data.uniform_(-1.0 / n_codes, 1.0 / n_codes)
        self.ema = bool(ema)
        if not self.ema:
            assert not init_from_data and reseed_below == 0.0, "init_from_data / reseed_below belong to the EMA codebook (ema=True)"
            return
        assert 0.0 <= decay <= 1.0 and eps >= 0.0 and reseed_every >= 1 and reseed_below >= 0.0 and seed >= 0
        self.decay, self.eps = float(decay), float(eps)
        self.init_from_data, self.reseed_below, self.reseed_every, self.seed = bool(init_from_data), float(reseed_below), int(reseed_every), int(seed)
        self.embedding.weight.requires_grad_(False)
        # fp32 like the codebook: broadcast_parameters carries all three in one coalesced buffer
        self.register_buffer("ema_cluster_size", torch.ones(n_codes, dtype=torch.float32))
        self.register_buffer("ema_embed_sum", self.embedding.weight.detach().clone())
        self.frozen = False            # VAETrainStep sets it for a calibration pass: no statistics, no initialisation
        self.ema_steps = 0             # updates applied: the `step` of the reseeding cadence and hash
        self._data_init_done = False   # the first-forward flag of init_from_data
        self._pending = None           # (tokens, n_local, n_global, all-reduce handle) of the forward that awaits ema_update()
        self._scratch = None           # device scratch: accumulators + update scratch, max |token|, usage scalars, candidate rows
        self._checked_n = set()

    # ---- EMA state ---------------------------------------------------------------------------------------------------------
    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        if self.ema:
            ck, ek, wk = prefix + "ema_cluster_size", prefix + "ema_embed_sum", prefix + "embedding.weight"
            if ck not in state_dict and ek not in state_dict and wk in state_dict:
                # a codebook trained without the EMA statistics (a plain quantizer's checkpoint): N = 1, m = codebook, so m / N is it
                logging.getLogger(__name__).warning("EMA quantizer: checkpoint has no EMA statistics; starting them from the loaded "
                                                    "codebook (cluster sizes 1, sums = codebook)")
                state_dict = dict(state_dict)
                state_dict[ck] = torch.ones(self.n_codes, dtype=torch.float32)
                state_dict[ek] = state_dict[wk].detach().clone().float()
            if wk in state_dict:
                self._data_init_done = True          # a loaded codebook is not overwritten by init_from_data
            self._pending = None
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def ema_state(self) -> dict:
        """Everything `ema_update` and the first forward change (VAETrainStep.state_snapshot)."""
        return {"codebook": self.embedding.weight.detach().clone(), "cluster_size": self.ema_cluster_size.clone(),
                "embed_sum": self.ema_embed_sum.clone(), "steps": self.ema_steps, "data_init_done": self._data_init_done}

    @torch.no_grad()
    def ema_restore(self, st: dict) -> None:
        self.embedding.weight.copy_(st["codebook"])
        self.ema_cluster_size.copy_(st["cluster_size"])
        self.ema_embed_sum.copy_(st["embed_sum"])
        self.ema_steps, self._data_init_done, self._pending = st["steps"], st["data_init_done"], None

    def _buffers_for(self, dev):
        sc = self._scratch
        if sc is None or sc["ws"].device != dev:
            L = lib()
            sc = {"ws": torch.zeros(L.size("vq_vq_ema_workspace", self.n_codes, self.dim), dtype=torch.uint8, device=dev),
                  "amax": torch.zeros(1, dtype=torch.float32, device=dev),
                  "usage": torch.zeros(2, dtype=torch.float32, device=dev),
                  "cand": torch.zeros(self.n_codes, self.dim, dtype=torch.float32, device=dev)}
            # what the ranks all-reduce (int64 SUM): counts [K] and fixed-point sums [K, D]
            sc["acc"] = sc["ws"][:8 * self.n_codes * (self.dim + 1)].view(torch.int64)
            self._scratch = sc
        return sc

    def _check_equal_split(self, n_local, dev):
        """Global token g lives on rank g // n_local: every rank must hold the same number of tokens (checked once per size)."""
        if n_local in self._checked_n:
            return
        t = torch.tensor([n_local, -n_local], dtype=torch.int64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        lo_hi = t.tolist()                         # the one host readback of the EMA path: once per token count, multi-rank only
        if lo_hi[0] != n_local or -lo_hi[1] != n_local:
            raise RuntimeError(f"EMA quantizer: ranks hold different numbers of tokens ({-lo_hi[1]} .. {lo_hi[0]}); the statistics' "
                               "scale and the reseeding (global token g lives on rank g // n_local) need an equal split")
        self._checked_n.add(n_local)

    @torch.no_grad()
    def _reseed(self, tokens, threshold: float, step: int) -> None:
        """Codes with N < threshold take the tokens the hash picks from the global batch (this rank holds `tokens`)."""
        dev = tokens.device
        sc = self._buffers_for(dev)
        L, w = lib(), self.embedding.weight
        n, world = tokens.shape[0], _world()
        if world > 1:
            self._check_equal_split(n, dev)
        off = n * (dist.get_rank() if world > 1 else 0)
        args = (ptr(self.ema_cluster_size), float(threshold), int(step), int(self.seed), ptr(tokens), n, off, n * world, self.n_codes,
                self.dim, ptr(sc["cand"]), ptr(self.ema_embed_sum), ptr(w), stream_of(w))
        L.call("vq_vq_ema_reseed", 0, *args)
        if world > 1:
            dist.all_reduce(sc["cand"], op=dist.ReduceOp.SUM)      # one non-zero contributor per row: the rows arrive intact
        L.call("vq_vq_ema_reseed", 1, *args)

    @torch.no_grad()
    def _accumulate(self, tokens, idx) -> None:
        """Right behind the lookup: this rank's histogram and fixed-point sums, then their sum over ranks — enqueued here so that
        the pass and the two collectives run under the decoder; ema_update() picks the result up."""
        dev = tokens.device
        sc = self._buffers_for(dev)
        L = lib()
        n, world = tokens.shape[0], _world()
        if (n * self.dim) % 8 != 0:
            raise ValueError(f"EMA quantizer: n_tokens * dim = {n} * {self.dim} must be a multiple of 8 (vq_absmax, which measures "
                             "the fixed-point scale, reads 8 elements per lane)")
        if world > 1:
            self._check_equal_split(n, dev)
        s = stream_of(tokens)
        sc["amax"].zero_()
        L.call("vq_absmax", ptr(tokens), n * self.dim, VQ_F32, ptr(sc["amax"]), s)
        if world > 1:                                              # 4 bytes: the fixed-point scale must be the same everywhere
            dist.all_reduce(sc["amax"], op=dist.ReduceOp.MAX)
        L.call("vq_vq_ema_accumulate", ptr(tokens), ptr(idx), n, n * world, self.n_codes, self.dim, ptr(sc["amax"]), ptr(sc["ws"]),
               sc["ws"].numel(), s)
        handle = dist.all_reduce(sc["acc"], op=dist.ReduceOp.SUM, async_op=True) if world > 1 else None
        self._pending = (tokens, n, n * world, handle)

    @torch.no_grad()
    def ema_update(self):
        """Apply the update (and, on its cadence, the reseeding) from the statistics of the last training forward; once per step,
        where an optimizer would step.  -> device tensor [perplexity, codes used] of that forward's batch, or None when no forward
        left statistics (eval, no_grad, frozen)."""
        if not self.ema or self._pending is None:
            return None
        tokens, _n, n_global, handle = self._pending
        self._pending = None
        if handle is not None:
            handle.wait()
        sc = self._buffers_for(tokens.device)
        w = self.embedding.weight
        lib().call("vq_vq_ema_update", ptr(sc["ws"]), sc["ws"].numel(), n_global, ptr(sc["amax"]), self.n_codes, self.dim, self.decay,
                   self.eps, ptr(self.ema_cluster_size), ptr(self.ema_embed_sum), ptr(w), ptr(sc["usage"]), stream_of(w))
        step = self.ema_steps
        self.ema_steps += 1
        if self.reseed_below > 0.0 and (step + 1) % self.reseed_every == 0:
            self._reseed(tokens, self.reseed_below, step)
        return sc["usage"].clone()

    def forward(self, z, lookup_from=None):
        b, d, h, w = z.shape
        tokens = z.permute(0, 2, 3, 1).reshape(-1, d)
        look = None if lookup_from is None else lookup_from.detach().permute(0, 2, 3, 1).reshape(-1, d)
        if not self.ema:
            zq, loss, idx = _VQLookup.apply(tokens, self.embedding.weight, self.beta, look)
            return zq.reshape(b, h, w, d).permute(0, 3, 1, 2), loss, idx.reshape(b, h, w)
        moves = self.training and torch.is_grad_enabled() and not self.frozen
        # the tokens the search reads are the ones the statistics are made of
        src = (tokens if look is None else look).detach().contiguous().float()
        assert self.embedding.weight.device == src.device and not self.embedding.weight.requires_grad
        if moves and self.init_from_data and not self._data_init_done:
            self._reseed(src, math.inf, self.ema_steps)            # every code: N_k < +inf
            self._data_init_done = True
        zq, loss, idx = _VQLookup.apply(tokens, self.embedding.weight, self.beta, look, True)
        if moves:
            self._accumulate(src, idx)
        return zq.reshape(b, h, w, d).permute(0, 3, 1, 2), loss, idx.reshape(b, h, w)
