"""Train-step hot path + DDP entrypoint — drop-in for the reference's vae_trainer.py surface.

Kept: `gradnorm` / `GradNormFunction`, `avg_scalar_over_nodes`, `gan_disc_loss`, `vae_loss_function`,
the `train_ddp` click command with the reference's 31 options and torchrun environment
(RANK / LOCAL_RANK / WORLD_SIZE, vae_trainer.py:392-394).
Changed on purpose (each documented in DESIGN.md):
  * the loop body (vae_trainer.py:525-708) is `VAETrainStep`: no `.item()` / `.cpu()` inside the step —
    every scalar stays on the device and is read back only when logging;
  * VAE gradients ARE all-reduced (bucketed, overlapped; reference omits it);
    `--sync_vae_grads False` restores the reference behaviour;
  * the discriminator's weight gradients are not computed in the generator step (the reference
    computes and discards them, all-reducing 60 MB for nothing — SURVEY C4);
  * `lecam_loss_item` is initialised (reference NameError without --use_lecam);
  * `--synthetic` feeds seeded uniform [-1,1] images (no webdataset / network here).
"""
from __future__ import annotations

import logging
import math
import os
import random
import time

import torch
import torch.distributed as dist
import torch.nn.functional as F  # noqa: F401  (host-side glue on [B,256] logits only)

from . import ops
from ._lib import lib, ptr, stream_of
from .ae import VAE
from .distributed import BucketedGradReducer, broadcast_parameters
from .optim import FusedAdamW
from .utils import LPIPS, PatchDiscriminator, prepare_filter

GradNormFunction = ops._GradNorm


def gradnorm(x, weight=1.0):
    """vae_trainer.py:51-53.  Backward: g * weight / (mean over ranks of ||g||_2 + 1e-8), computed on
    the device (no .item(), a 4-byte all-reduce on the compute stream when world_size > 1)."""
    return ops.gradnorm(x, float(weight))


@torch.no_grad()
def avg_scalar_over_nodes(value: float, device):
    """vae_trainer.py:56-60 (kept for API compatibility; the step itself never calls it)."""
    t = torch.tensor(float(value), device=device)
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        t /= dist.get_world_size()
    return t.item()


class _GanDiscLoss(torch.autograd.Function):
    """One kernel produces loss, mean logits, accuracy count and dLoss/dlogits (vae_trainer.py:63-90)."""

    @staticmethod
    def forward(ctx, real, fake, disc_type):
        real, fake = real.contiguous().float(), fake.contiguous().float()
        out6 = torch.empty(6, dtype=torch.float32, device=real.device)
        d_real, d_fake = torch.empty_like(real), torch.empty_like(fake)
        lib().call("vq_gan_disc_loss", ptr(real), ptr(fake), real.numel(), 1 if disc_type == "hinge" else 0,
                   ptr(out6), ptr(d_real), ptr(d_fake), stream_of(real))
        ctx.save_for_backward(d_real, d_fake)
        loss = (out6[0] + out6[1]) * 0.5
        ctx.mark_non_differentiable(out6)
        return loss, out6

    @staticmethod
    def backward(ctx, g, _):
        d_real, d_fake = ctx.saved_tensors
        L = lib()
        gr, gf = torch.empty_like(d_real), torch.empty_like(d_fake)
        gc = g.contiguous().float()
        L.call("vq_scale", ptr(d_real), 1.0, ptr(gc), d_real.numel(), ptr(gr), stream_of(gc))
        L.call("vq_scale", ptr(d_fake), 1.0, ptr(gc), d_fake.numel(), ptr(gf), stream_of(gc))
        return gr, gf, None


def gan_disc_loss_device(real_preds, fake_preds, disc_type="bce"):
    """-> (loss, stats[6] = {loss_real, loss_fake, mean_real, mean_fake, n_correct, count}) on device."""
    assert disc_type in ("bce", "hinge")
    return _GanDiscLoss.apply(real_preds, fake_preds, disc_type)


def gan_disc_loss(real_preds, fake_preds, disc_type="bce"):
    """Reference signature and return types (vae_trainer.py:63-90): floats imply one host sync."""
    loss, st = gan_disc_loss_device(real_preds, fake_preds, disc_type)
    s = st.tolist()
    return loss, s[2], s[3], s[4] / s[5]


class _MeanSquare(torch.autograd.Function):
    """mean(z^2) (vae_trainer.py:202-203) with device-resident moments for the logged statistics."""

    @staticmethod
    def forward(ctx, z):
        z = z.contiguous().float()
        out4 = torch.empty(4, dtype=torch.float32, device=z.device)
        scratch = torch.empty(1024, dtype=torch.float32, device=z.device)
        lib().call("vq_moments", ptr(z), z.numel(), ptr(out4), ptr(scratch), stream_of(z))
        ctx.save_for_backward(z)
        ctx.mark_non_differentiable(out4)
        return out4[1] / z.numel(), out4

    @staticmethod
    def backward(ctx, g, _):
        (z,) = ctx.saved_tensors
        dz = torch.empty_like(z)
        gc = g.contiguous().float()
        lib().call("vq_scale", ptr(z), 2.0 / z.numel(), ptr(gc), z.numel(), ptr(dz), stream_of(z))
        return dz


def vae_loss_device(z):
    """-> (0.1 * mean(z^2), moments[4] = {sum (|z| - mean|z|)^2, sum z^2, sum |z|, n}); recon term: SURVEY F9 (x0.0)."""
    zloss, mom = _MeanSquare.apply(z)
    return zloss * 0.1, mom


def vae_loss_function(x, x_reconstructed, z, do_pool=True, do_recon=False):
    """Reference signature (vae_trainer.py:179-217).  `do_recon` is False at every reference call
    site and its term is multiplied by 0.0 (vae_trainer.py:209); it is not on the HIP path."""
    if do_recon:
        raise NotImplementedError("do_recon=True is dead in the reference (weight 0.0, vae_trainer.py:209)")
    loss, mom = vae_loss_device(z)
    m2, ss, sa, n = mom.tolist()
    mean_abs = sa / n
    var_abs = m2 / max(n - 1, 1)                                              # torch.std: unbiased
    return loss, {"recon_loss": 0, "kl_loss": ss / n, "average_of_abs_z": mean_abs,
                  "std_of_abs_z": math.sqrt(var_abs), "average_of_logvar": 0.0, "std_of_logvar": 0.0}


# Per-module arithmetic of a train step.  The reference's own step is MIXED: the encoder runs outside autocast
# in fp32 with TF32 matmuls allowed (vae_trainer.py:18-19,538), the decoder under bf16 autocast (:453,623-624), LPIPS and the
# PatchDiscriminator in fp32/TF32 (utils.py:70-71 promotes the bf16 reconstruction to fp32).  gfx950 has no TF32 MFMA, so:
#   ref     encoder / LPIPS / discriminator on fp16 operands — the 10-bit mantissa of TF32 — with fp32 accumulation, power-of-two
#           tensor scales keeping weights and gradients inside fp16's exponent range; decoder bf16 like the reference's autocast
#   ref3    the same split with the 3-term bf16 split (fp32-class products, ~3x the MFMA work) in place of fp16
#   ref_vq  the policy of the quantized workload (configs[4]): "ref", plus a SECOND, gradient-free evaluation of the encoder in the
#           fp32-class f16x3 arithmetic (round 5; rounds 3-4: the fp32x3 split on the generic kernel) whose output the nearest-code lookup reads (`lookup="f16x3"`).  The lookup is integer work (north_star:
#           "bit-exact for the VQ argmin indices") and with a binary16 encoder ~0.5 % of the tokens sit close enough to a Voronoi
#           boundary for the rounding to pick another code; gradients, losses and the straight-through output keep flowing through
#           the binary16 evaluation, so only a forward pass of the encoder is paid for in the slow arithmetic (round 4, first form:
#           the whole encoder, forward and backward, in the split: 29 img/s where this form runs ~47)
#   bf16    everything on bf16 operands (narrower than the reference outside the decoder: a throughput mode)
#   fp32x3  everything fp32-class (operands to 16 mantissa bits): the parity mode against the CPU fp32 oracle (1e-4)
#   fp32x6  everything in fp32-EXACT products (three bf16 pieces per operand, six MFMAs per product): the reference CPU path's own
#           arithmetic — what it takes to keep even the generator's GAN term, evaluated right after the discriminator's first
#           sign-like AdamW step, inside 1e-4 at the headline model
#   fp32    fp32 storage, single bf16 product
#   f16x3   everything as TWO binary16 pieces per value (hi + lo: 22 significand bits, include/vqhip.h VQ_F16X2) and three binary16
#           MFMAs per product, fp32 accumulate — the fp32-tolerance arithmetic on the TUNED kernels (LDS-DMA tiles, nine-tap and
#           patch-staged kernels, three-tap weight gradients), where fp32x3 / fp32x6 only exist on the generic register-staged
#           kernel.  Per-product error ~2^-21 (fp32x3: 2^-16, fp32x6: 2^-24).  Scaled like the binary16 stacks of "ref".
#   ref2    "ref" with the decoder, LPIPS and the discriminator in f16x3 (the encoder stays binary16: its share of the parity gap
#           is 3e-6, profiles/r4a_parity_attrib.txt)
PRECISION_POLICIES = {
    "ref": dict(encoder="fp16", decoder="bf16", lpips="fp16", disc="fp16"),
    "bf16": dict(encoder="bf16", decoder="bf16", lpips="bf16", disc="bf16"),
    "fp32": dict(encoder="fp32", decoder="fp32", lpips="fp32", disc="fp32"),
    "fp32x3": dict(encoder="fp32x3", decoder="fp32x3", lpips="fp32x3", disc="fp32x3"),
    "fp32x6": dict(encoder="fp32x6", decoder="fp32x6", lpips="fp32x6", disc="fp32x6"),
    "ref3": dict(encoder="fp32x3", decoder="bf16", lpips="fp32x3", disc="fp32x3"),
    "ref_vq": dict(encoder="fp16", decoder="bf16", lpips="fp16", disc="fp16", lookup="f16x3"),
    "f16x3": dict(encoder="f16x3", decoder="f16x3", lpips="f16x3", disc="f16x3"),
    "ref2": dict(encoder="fp16", decoder="f16x3", lpips="f16x3", disc="f16x3"),
}


def apply_precision_policy(policy: str, vae: VAE, lpips: LPIPS | None = None, disc: PatchDiscriminator | None = None) -> dict:
    """Pin every module of the step to the arithmetic `policy` names (see PRECISION_POLICIES); returns the module map."""
    if policy not in PRECISION_POLICIES:
        raise ValueError(f"unknown precision policy '{policy}' (known: {', '.join(PRECISION_POLICIES)})")
    pol = PRECISION_POLICIES[policy]

    def pick(name, role):       # every fp16 stack is its own loss-scale domain (ops.Precision.grad_scale)
        return ops.fp16_region(role) if name == "fp16" else (ops.f16x3_region(role) if name == "f16x3" else ops.resolve_precision(name))

    vae.encoder.precision = pick(pol["encoder"], "encoder")
    vae.encoder.lookup_precision = ops.resolve_precision(pol["lookup"]) if pol.get("lookup") else None   # VAETrainStep: exact code lookup
    vae.decoder.precision = pick(pol["decoder"], "decoder")
    if lpips is not None:
        lpips.precision = pick(pol["lpips"], "lpips")
    if disc is not None:
        disc.precision = pick(pol["disc"], "disc")
    return pol


def cosine_with_warmup(step: int, warmup: int, total: int) -> float:
    """transformers.get_cosine_schedule_with_warmup's multiplier (vae_trainer.py:486-490)."""
    if step < warmup:
        return step / max(1, warmup)
    prog = (step - warmup) / max(1, total - warmup)
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * 2.0 * 0.5 * prog)))


_DEFER_D_JOIN = os.environ.get("VQ_DEFER_D_JOIN", "1") != "0"         # A/B knob (tools/): see VAETrainStep.__call__
_LPIPS_PREFETCH = os.environ.get("VQ_LPIPS_PREFETCH", "1") != "0"     # A/B knob (tools/): LPIPS' target features on the side stream


class VAETrainStep:
    """One iteration of vae_trainer.py:525-708.

    Augmentations (flips, flip/crop invariance, pre-LPIPS flips) follow the reference's draw order on `rng`
    (default: the `random` module, seeded by train_ddp like vae_trainer.py:374-378).  rng=False disables every
    draw — including the unconditional 50 % horizontal flip of :534 — for fixed-input parity tests and bench.py.
    `enc_size` is the encoder input size of the area resize (:531-533; the reference hard-codes (256, 256)).

    Weight EMA (not in the reference): with `ema_decay` > 0 optimizer_G keeps an exponential moving average of every generator
    parameter, updated inside its AdamW launch (optim.FusedAdamW; `ema_warmup`: decay min(ema_decay, (1 + t) / (10 + t))), and
    `ema_weights()` swaps it in for evaluation and checkpoints.  A gradient-trained codebook sits in optimizer_G's main group and
    gets a shadow like every other generator parameter; the codebook of an `ema=True` quantizer is no optimizer parameter: it has
    no shadow and the swap leaves it alone.  The discriminator keeps no shadow."""

    def __init__(self, vae: VAE, lpips: LPIPS, discriminator: PatchDiscriminator | None = None, *,
                 do_ganloss=False, disc_type="bce", use_lecam=False, learning_rate_vae=1e-5, learning_rate_disc=2e-4,
                 vae_ch=256, max_steps=1000, warmup_steps=200, do_clamp=False, clamp_th=8.0, sync_vae_grads=True,
                 bucket_bytes=32 << 20, on_backward=None, rng=False, enc_size=None, flip_invariance=False,
                 crop_invariance=False, augment_before_perceptual_loss=False, decoder_also_perform_hr=False,
                 downscale_factor=16, quantizer=None, single_rank_collectives=False, on_d_backward=None, gradnorm_dp_chunks=1,
                 ema_decay=0.0, ema_warmup=False):
        self.vae, self.lpips, self.disc = vae, lpips, discriminator
        self.quantizer = quantizer                # config 5: VectorQuantizer in place of `vae.reg` (not in the reference, F1)
        self.rng = random if rng is None else rng
        self.enc_size = enc_size
        self.flip_invariance, self.crop_invariance = flip_invariance, crop_invariance
        self.augment_before_perceptual_loss = augment_before_perceptual_loss
        self.decoder_also_perform_hr, self.downscale_factor = decoder_also_perform_hr, downscale_factor
        self.do_ganloss, self.disc_type, self.use_lecam = do_ganloss, disc_type, use_lecam
        self.do_clamp, self.clamp_th = do_clamp, clamp_th
        self.max_steps, self.warmup_steps = max_steps, warmup_steps
        named = list(vae.named_parameters())
        self._ema_vq = quantizer is not None and getattr(quantizer, "ema", False)
        # an EMA codebook has no optimizer: not in optimizer_G (no AdamW, no weight decay), not in the gradient buckets; its update is
        # applied where optimizer_G steps (quantizer.ema_update)
        if quantizer is not None and not self._ema_vq:   # the codebook trains with the VAE's main group, its gradient rides in the VAE buckets
            # ... at the place its gradient becomes final in a backward pass: after the whole decoder, before the encoder.  Buckets are
            # cut in reverse parameter order and go on the wire strictly in index order (BucketedGradReducer): appended LAST, the
            # codebook would share bucket 0 with the decoder's last layers and hold every decoder bucket back until the decoder's
            # backward is over
            first_dec = next((i for i, (n, _) in enumerate(named) if n.startswith("decoder.")), len(named))
            named[first_dec:first_dec] = [("quantizer." + n, p) for n, p in quantizer.named_parameters()]
        # vae_trainer.py:455-468: everything but *conv_in* at lr_vae/ch, conv_in at 1e-4; wd 1e-3, betas (.9,.95)
        self.optimizer_G = FusedAdamW(
            [{"params": [p for n, p in named if "conv_in" not in n], "lr": learning_rate_vae / vae_ch},
             {"params": [p for n, p in named if "conv_in" in n], "lr": 1e-4}],
            weight_decay=1e-3, betas=(0.9, 0.95), ema_decay=ema_decay if ema_decay else None, ema_warmup=ema_warmup)
        self._base_lrs = [g["lr"] for g in self.optimizer_G.param_groups]
        self.reducer_G = BucketedGradReducer(self.optimizer_G._flat, bucket_bytes, enabled=sync_vae_grads,
                                             single_rank_ok=single_rank_collectives)
        self.optimizer_G.grad_scale = self.reducer_G.grad_scale()
        self.optimizer_D = self.reducer_D = None
        if do_ganloss:
            assert discriminator is not None
            self.optimizer_D = FusedAdamW(discriminator.parameters(), lr=learning_rate_disc, weight_decay=1e-3,
                                          betas=(0.9, 0.95))
            self.reducer_D = BucketedGradReducer(self.optimizer_D._flat, bucket_bytes, overlap=False,
                                                 single_rank_ok=single_rank_collectives)
            self.optimizer_D.grad_scale = self.reducer_D.grad_scale()
        self.global_step = 0
        self.on_backward = on_backward            # test hook: called after the G backward, before the optimizer step
        self.on_d_backward = on_d_backward        # test hook: after the discriminator's backward + exchange, before its step
        self.gradnorm_dp_chunks = gradnorm_dp_chunks   # test knob: GradNorm as k data-parallel ranks would compute it (ops._GradNorm)
        dev = named[0][1].device
        self.lecam_anchor = torch.zeros(2, dtype=torch.float32, device=dev)   # (real, fake) logits EMA
        self.lecam_beta, self.lecam_loss_weight = 0.9, 0.1
        self.comm_events = None                   # bench.py: list collecting (start, end) HIP events around the reducer waits
        self.event_factory = lambda: torch.cuda.Event(enable_timing=True)
        self._dry = False                         # calibrate_grad_scales: a step without parameter updates
        self.range_events = None                  # [stacks, EV_COLS] int32: see bind_range_events
        self._skipped = None
        self.bind_range_events()

    # ---- binary16 range events: the live overflow / underflow signal of the fp16 stacks ----------------------------------------
    # The reference's fp32 / TF32 path cannot overflow (vae_trainer.py:18-19,538); binary16 stores here saturate at +-65504.  Every
    # kernel that writes a tensor of an fp16 stack reports to the stack's device counters (include/vqhip.h "range events"):
    #   row = [saturated, flushed, headroom (>= 2^13) of this window | their totals]   of the GRADIENT stores (backward), then the same
    #         six for the FORWARD stores (ops._events picks the half by the pass that is running).
    # The optimizers read column 0 ON THE DEVICE (vq_adamw_multi skip_flags): a step whose GRADIENTS were clipped changes no
    # parameter — a re-calibrated loss scale fixes that.  Forward stores (activations, stored unscaled) never gate the optimizer:
    # no loss scale can help there, so they are logged and, when they persist, escalated (escalate_forward_saturation).
    # Nothing here syncs; run_training reads the totals at its logging cadence and re-calibrates the loss scales.
    EV_COLS = 12
    HOT_RESCALE_LOG2 = 3                      # a stack that reported headroom events gets its loss scale lowered by 2^3 at the next poll

    def bind_range_events(self):
        """(Re-)attach the counters to the current fp16 stacks — call again after apply_precision_policy replaced them."""
        stacks = self.fp16_stacks()
        self._fwd_sat_polls = {}                  # region -> consecutive polls that saw forward saturation
        if not stacks:
            self.range_events = self._skipped = None
            self.optimizer_G.skip_flags = None
            if self.optimizer_D is not None:
                self.optimizer_D.skip_flags = None
            return
        dev = next(self.vae.parameters()).device
        self.range_events = torch.zeros((len(stacks), self.EV_COLS), dtype=torch.int32, device=dev)
        self._skipped = torch.zeros(2, dtype=torch.int32, device=dev)            # optimizer steps dropped on the device: (G, D)
        for i, p in enumerate(stacks):
            p.events = self.range_events[i]
        self.optimizer_G.skip_flags = (self.range_events, len(stacks), self.EV_COLS)   # any stack: G's gradients cross all of them
        if self.optimizer_D is not None:
            row = self._disc_row()
            self.optimizer_D.skip_flags = (self.range_events[row], 1, self.EV_COLS) if row is not None else None

    def _close_window(self, which: int, row="all"):
        """After an optimizer step (which = 0: G, 1: D): fold the window counters of stack `row` ("all": every stack) into the
        totals and clear them; a non-zero GRADIENT saturation window means the step was dropped on the device.  `row=None` (the
        discriminator is not an fp16 stack, so optimizer_D has no skip flags and its step was applied) is a no-op: the other stacks'
        windows still belong to the generator step that follows.  Device-side glue on a handful of integers (views only: the
        counters the kernels and the optimizers point at must stay where they are)."""
        ev = self.range_events
        if ev is None or row is None:
            return
        if row != "all":
            ev = ev[row:row + 1]
        self._skipped[which] += (ev[:, 0].max() > 0).to(torch.int32)
        ev[:, 3:6] += ev[:, 0:3]
        ev[:, 0:3] = 0
        if which == 0:                           # the forward windows close once per iteration, with the generator step
            ev[:, 9:12] += ev[:, 6:9]
            ev[:, 6:9] = 0

    def _sync_window(self, reducer):
        """All ranks must take the same skip decision: the gradients are averaged, so one rank's clipped tensor reaches everybody.
        (Without a gradient exchange — `sync_vae_grads=False`, the reference's behaviour — every rank decides for itself.)"""
        if (self.range_events is not None and reducer is not None and reducer.enabled and dist.is_available() and dist.is_initialized()
                and dist.get_world_size() > 1):
            dist.all_reduce(self.range_events, op=dist.ReduceOp.MAX)

    def poll_range_events(self) -> dict:
        """ONE host sync: per stack the totals since the last poll (gradient stores and forward stores apart), and the optimizer
        steps dropped on the device (the Adam step counters are rewound by those).  Call at the logging cadence.
        COLLECTIVE when a process group is up: EVERY rank must call it at the same point (run_training and bench.py do) — the totals
        and the dropped-step counts are MAX-reduced so that all ranks rewind, re-calibrate and escalate alike, also when the
        gradients are not exchanged (`sync_vae_grads=False`: the windows are then per-rank).  The OPEN windows (columns 0:2, 4:6)
        are not touched: they belong to the step in flight and are synchronised by `_sync_window` where that is needed."""
        if self.range_events is None:
            return {"stacks": [], "skipped_G": 0, "skipped_D": 0}
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            ev_t = self.range_events
            tot = torch.cat([ev_t[:, 3:6].reshape(-1), ev_t[:, 9:12].reshape(-1), self._skipped.reshape(-1).to(ev_t.dtype)])
            dist.all_reduce(tot, op=dist.ReduceOp.MAX)
            n = ev_t.shape[0]
            ev_t[:, 3:6] = tot[:3 * n].view(n, 3)
            ev_t[:, 9:12] = tot[3 * n:6 * n].view(n, 3)
            self._skipped.copy_(tot[6 * n:].to(self._skipped.dtype))
        ev = self.range_events.tolist()
        sk = self._skipped.tolist()
        self.range_events[:, 3:6] = 0
        self.range_events[:, 9:12] = 0
        self._skipped.zero_()
        if sk[0]:
            self.optimizer_G.rewind(sk[0])
            self.global_step = max(0, self.global_step - sk[0])      # the LR schedule counts applied updates too
        if sk[1] and self.optimizer_D is not None:
            self.optimizer_D.rewind(sk[1])
        stacks = []
        for p, r in zip(self.fp16_stacks(), ev):
            self._fwd_sat_polls[p.region] = self._fwd_sat_polls.get(p.region, 0) + 1 if r[9] else 0
            stacks.append({"region": p.region, "grad_scale_log2": math.log2(p.grad_scale), "saturated": r[3], "flushed": r[4],
                           "headroom": r[5], "fwd_saturated": r[9], "fwd_flushed": r[10],
                           "fwd_saturated_polls": self._fwd_sat_polls[p.region]})
        return {"stacks": stacks, "skipped_G": sk[0], "skipped_D": sk[1]}

    def relax_hot_scales(self, polled: dict) -> list:
        """The cheap half of keeping binary16 gradients in range (the other: calibrate_grad_scales): every stack whose gradient stores
        reached 2^13 since the last poll — three bits under the limit, nothing clipped — has its loss scale lowered by
        2^HOT_RESCALE_LOG2, in place (the scale is a host float handed to every launch).  `polled` = poll_range_events()'s result, the
        same on every rank; no pass over the model, no state touched.  A run whose gradients grow (a GAN: 16x over 25 steps on
        configs[2]) is walked down ahead of the growth, so the device-side step drop stays what it is meant to be: the last resort.
        -> [(region, new log2 scale)]"""
        by_region = {e["region"]: e for e in polled["stacks"]}
        moved = []
        for p in self.fp16_stacks():
            e = by_region.get(p.region)
            if e is not None and e["headroom"] and not e["saturated"]:
                p.grad_scale = max(p.grad_scale / float(1 << self.HOT_RESCALE_LOG2), 2.0 ** -20)
                moved.append((p.region, math.log2(p.grad_scale)))
        return moved

    def escalate_forward_saturation(self, regions) -> list:
        """Forward activations of these binary16-range stacks keep reaching binary16's limit (+-65504): they are stored unscaled, so
        no loss-scale calibration can fix it.  Binary16 stacks move to bf16 storage + operands (8 exponent bits, the reference's
        autocast type); f16x3 stacks (two binary16 pieces: the same exponent range) move to fp32x6 — fp32 storage, the same
        tolerance class, no range limit — so that the tolerance policy stays a tolerance policy.  Weights are re-packed, the counters
        re-bound.  Returns [(region, new arithmetic)] of the stacks moved (the lookup arithmetic of `ref_vq` included)."""
        moved = []
        for m in (self.vae.encoder, self.vae.decoder, self.lpips, self.disc):
            for attr in ("precision", "lookup_precision"):
                p = getattr(m, attr, None)
                if isinstance(p, ops.Precision) and p.half_range() and p.region in regions:
                    to = "bf16" if p.dtype == torch.float16 else "fp32x6"
                    setattr(m, attr, ops.resolve_precision(to))
                    moved.append((p.region, to))
        if moved:
            ops.clear_caches()
            self.bind_range_events()
            for region, _ in moved:
                self._fwd_sat_polls.pop(region, None)
        return moved

    def ema_weights(self):
        """Context manager: the generator's parameters (and packed conv operands) hold the EMA shadow inside (FusedAdamW.ema_weights)."""
        return self.optimizer_G.ema_weights()

    def load_ema(self, path: str | None) -> bool:
        """The shadow from a checkpoint file `save_checkpoint` wrote inside `ema_weights()` — a strict load into the swapped-in
        parameters, which the exit of the context writes back to the shadow's place.  No file (None, or missing): the shadow
        starts from the current parameters, with a log line.  Returns whether a file was loaded."""
        opt = self.optimizer_G
        if path is None or not os.path.exists(path):
            with torch.no_grad():
                for f in opt._flat:
                    f.flat_ema.copy_(f.flat_p)
            logging.getLogger(__name__).info(f"no EMA checkpoint{'' if path is None else ' at ' + path}: the EMA weights start from the loaded weights")
            return False
        quantizer = self.quantizer if (self.quantizer is not None and not self._ema_vq) else None
        with opt.ema_weights():
            # (an EMA quantizer's codebook has no shadow: the `quantizer.*` keys of the file are dropped, its state stays as loaded)
            load_checkpoint(self.vae, path, quantizer=quantizer)
            with torch.no_grad():
                for f in opt._flat:
                    f.flat_ema.copy_(f.flat_p)
        return True

    def state_snapshot(self) -> dict:
        """Everything a step changes — parameters, AdamW moments and step counts of both optimizers (the weight EMA inside G's), the LR schedule's counter, the
        LeCam anchors, the random streams the step draws from — so that `state_restore` puts the run back exactly here (bench.py:
        the rehearsal that measures the loss scales the timed steps need)."""
        return {"G": self.optimizer_G.snapshot(moments=True),
                # an EMA codebook (with its cluster sizes, sums and first-forward flag) is no part of optimizer_G's flat buffers
                "vq_ema": self.quantizer.ema_state() if self._ema_vq else None,
                "D": self.optimizer_D.snapshot(moments=True) if self.optimizer_D is not None else None,
                "global_step": self.global_step, "lecam": self.lecam_anchor.clone(),
                "py_rng": self.rng.getstate() if (self.rng and hasattr(self.rng, "getstate")) else None,
                "torch_rng": torch.get_rng_state(),
                "cuda_rng": torch.cuda.get_rng_state(self.lecam_anchor.device) if self.lecam_anchor.is_cuda else None}

    def state_restore(self, snap: dict) -> None:
        self.optimizer_G.restore(snap["G"])
        if self._ema_vq and snap.get("vq_ema") is not None:
            self.quantizer.ema_restore(snap["vq_ema"])
        if self.optimizer_D is not None and snap["D"] is not None:
            self.optimizer_D.restore(snap["D"])
        self.global_step = snap["global_step"]
        self.lecam_anchor.copy_(snap["lecam"])
        if snap["py_rng"] is not None:
            self.rng.setstate(snap["py_rng"])
        torch.set_rng_state(snap["torch_rng"])
        if snap["cuda_rng"] is not None:
            torch.cuda.set_rng_state(snap["cuda_rng"], self.lecam_anchor.device)
        if self.range_events is not None:
            self.range_events.zero_()
            self._skipped.zero_()
        self._fwd_sat_polls.clear()

    def _disc_row(self):
        if self.range_events is None or self.disc is None:
            return None
        dp = getattr(self.disc, "precision", None)
        rows = [i for i, p in enumerate(self.fp16_stacks()) if p is dp]
        return rows[0] if rows else None

    def fp16_stacks(self):
        """The loss-scale domains of this step: one ops.Precision object per fp16 module stack (policy "ref")."""
        seen, out = set(), []
        for m in (self.vae.encoder, self.vae.decoder, self.lpips, self.disc):
            p = getattr(m, "precision", None)
            if isinstance(p, ops.Precision) and p.half_range() and id(p) not in seen:
                seen.add(id(p))
                out.append(p)
        return out

    def calibrate_grad_scales(self, real_images_hr: torch.Tensor, rounds: int = 3, target_log2=10) -> list:
        """Loss scales of the fp16 stacks from MEASURED gradient maxima: runs the step's forward + backward on this batch
        without updating anything (no optimizer step, no LR step, gradients zeroed afterwards) with a vq_absmax pass behind
        every gradient tensor the stacks produce, and sets each stack's power-of-two scale so that its largest tensor
        maximum sits at 2^target_log2 (binary16 tops out at 2^16: 6 bits of headroom — measured on configs[2]: with a random-VGG
        discriminator the gradients of the encoder stack grow 16x over the first 25 steps, profiles/r3a_*; the smallest per-tensor
        maximum of a stack then still sits ~2^15 above binary16's smallest normal number).  What the headroom does not cover is caught
        while training: the kernels count clipped stores (range events), the optimizers drop such a step on the device, and
        run_training re-calibrates at its next log line.
        Repeats while a scale moved (a saturated first pass under-reports).  One host sync per round; call it before
        training and, if losses change character, again every few thousand steps.  Returns the per-stack report of the
        last round: region, scale, largest / smallest non-zero tensor maximum in stored units."""
        stacks = self.fp16_stacks()
        report = []
        if not stacks:
            return report
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        for _ in range(rounds):
            self._dry = True
            # the dry pass must not move the run's random streams (augmentation draws, LPIPS dropout seeds)
            py_state = self.rng.getstate() if (self.rng and hasattr(self.rng, "getstate")) else None
            t_state = torch.get_rng_state()
            try:
                with ops.monitor_gradients() as mon:
                    self(real_images_hr)
                stats = mon.report()
            finally:
                self._dry = False
                torch.set_rng_state(t_state)
                if py_state is not None:
                    self.rng.setstate(py_state)
                if self.range_events is not None:      # what a calibration pass clipped is the calibration's business
                    self.range_events[:, 0:3] = 0
                    self.range_events[:, 6:9] = 0
            moved, report = False, []
            for p in stacks:
                st = stats.get(id(p))
                if st is None or st["max"] <= 0.0:
                    report.append({"region": p.region, "grad_scale": p.grad_scale, "tensors": 0})
                    continue
                tgt = target_log2.get(p.region, 10) if isinstance(target_log2, dict) else target_log2     # (per stack: {region: log2})
                shift = tgt - math.floor(math.log2(st["max"]))
                if st["max"] >= 65504.0:           # saturated: the true maximum is unknown, back off hard
                    shift = -8
                new = p.grad_scale * 2.0 ** shift
                new = min(max(new, 2.0 ** -40), 2.0 ** 60)
                report.append({"region": p.region, "grad_scale": new, "previous": p.grad_scale, "tensors": st["tensors"],
                               "max_stored": st["max"] * 2.0 ** shift, "min_nonzero_tensor_max_stored": st["min"] * 2.0 ** shift,
                               "all_zero_tensors": st["zero"]})
                if new != p.grad_scale:
                    p.grad_scale, moved = new, True
            if not moved and not multi:       # (every rank runs the same number of passes: they hold collectives)
                break
        return report

    def _finish(self, reducer):
        """reducer.finish() = the point where the compute stream waits for the bucket all-reduces: the time between the
        two events is the part of the exchange that was NOT hidden under backward kernels ("exposed")."""
        if self.comm_events is None or not reducer.enabled:
            return reducer.finish()
        s, e = self.event_factory(), self.event_factory()
        s.record()
        reducer.finish()
        e.record()
        self.comm_events.append((s, e))

    def _set_lr(self):
        mult = cosine_with_warmup(self.global_step, self.warmup_steps, self.max_steps)
        for g, base in zip(self.optimizer_G.param_groups, self._base_lrs):
            g["lr"] = base * mult

    def __call__(self, real_images_hr: torch.Tensor) -> dict:
        vae = self.vae
        out = {}
        self._set_lr()                                    # LambdaLR semantics: lr(step) used by this step
        rng = self.rng
        x_hr = real_images_hr
        x_enc = ops.area_downsample(x_hr, self.enc_size) if self.enc_size is not None else x_hr    # :531-533
        if rng and rng.random() < 0.5:                     # :534-536
            x_enc, x_hr = ops.flip_nchw(x_enc, flip_w=True), ops.flip_nchw(x_hr, flip_w=True)
        z_look = None
        look_prec = getattr(vae.encoder, "lookup_precision", None) if self.quantizer is not None else None
        if look_prec is not None:
            # policy ref_vq: the encoder once more, without autograd, in the fp32-class arithmetic — what the integer code lookup
            # reads.  On the side stream: it shares nothing with the gradient-carrying evaluation below but its input.
            def exact_encoder():
                grad_prec, vae.encoder.precision = vae.encoder.precision, look_prec
                try:
                    with torch.no_grad():
                        return vae.encoder(x_enc)
                finally:
                    vae.encoder.precision = grad_prec
            z_look = ops.run_on_side_stream(exact_encoder, x_enc)
        z = vae.encoder(x_enc)                             # :538
        if self.do_clamp:
            z = z.clamp(-self.clamp_th, self.clamp_th)     # :561-562
        vq_loss = None
        if self.quantizer is not None:
            if z_look is not None:
                z_look = z_look.wait()
                if self.do_clamp:
                    z_look = z_look.clamp(-self.clamp_th, self.clamp_th)
            if self._ema_vq:
                self.quantizer.frozen = self._dry          # a calibration pass leaves no statistics and initialises nothing
            z_s, vq_loss, indices = self.quantizer(z, lookup_from=z_look) if z_look is not None else self.quantizer(z)
            out["indices"] = indices
        else:
            z_s = vae.reg(z)                               # :563
        if rng:
            nz = z_s.shape[1]
            if rng.random() < 0.5 and self.flip_invariance:            # :567-570
                z_s = ops.flip_nchw(z_s, flip_w=True, negate_channels=(nz - 4, nz - 2))
                x_hr = ops.flip_nchw(x_hr, flip_w=True)
            if rng.random() < 0.5 and self.flip_invariance:            # :572-575
                z_s = ops.flip_nchw(z_s, flip_h=True, negate_channels=(nz - 2, nz))
                x_hr = ops.flip_nchw(x_hr, flip_h=True)
            if rng.random() < 0.5 and self.crop_invariance:            # :577-621
                z_h, z_w = z.shape[-2:]
                new_z_h, new_z_w = rng.randint(12, z_h - 1), rng.randint(12, z_w - 1)
                off_z_h, off_z_w = rng.randint(0, z_h - new_z_h - 1), rng.randint(0, z_w - new_z_w - 1)
                f = self.downscale_factor * (2 if self.decoder_also_perform_hr else 1)
                x_hr = x_hr[:, :, off_z_h * f:(off_z_h + new_z_h) * f, off_z_w * f:(off_z_w + new_z_w) * f].contiguous()
                z_s = z_s[:, :, off_z_h:off_z_h + new_z_h, off_z_w:off_z_w + new_z_w]
        x = x_hr                                           # what the discriminator and LPIPS compare against
        # LPIPS' features of the target depend on the batch alone (once the augmentation draws that touch it are made): requested
        # here on the side stream, they run under the decoder's GroupNorm passes and the discriminator step instead of after them
        tg_feats = None
        if (x.is_cuda and _LPIPS_PREFETCH and not (rng and self.augment_before_perceptual_loss)
                and hasattr(self.lpips, "target_features")):
            tg_feats = ops.run_on_side_stream(lambda: self.lpips.target_features(x), x)
        reconstructed = vae.decoder(z_s)                   # :623-624
        if self.do_ganloss:                                # :629-659 — discriminator step
            disc = self.disc
            # one pass over [real; fake] instead of two (utils.py:187-203 has no cross-sample op): twice the pixels per
            # GEMM for the small 16x16 / 32x32 layers and one weight-gradient launch per layer instead of two
            both = disc(torch.cat([x, reconstructed.detach()], 0))
            real_preds, fake_preds = both[:x.shape[0]], both[x.shape[0]:]
            d_loss, st = gan_disc_loss_device(real_preds, fake_preds, self.disc_type)
            avg = st[2:4].clone()
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                dist.all_reduce(avg)
                avg /= dist.get_world_size()
            if not self._dry:                              # (a calibration pass moves no state: not the EMA either)
                self.lecam_anchor.mul_(self.lecam_beta).add_(avg, alpha=1 - self.lecam_beta)
            total_d_loss = d_loss
            out["lecam_loss"] = torch.zeros((), device=x.device)
            if self.use_lecam:
                lecam = (real_preds - self.lecam_anchor[1]).pow(2).mean() + (fake_preds - self.lecam_anchor[0]).pow(2).mean()
                out["lecam_loss"] = lecam.detach()
                total_d_loss = total_d_loss + lecam * self.lecam_loss_weight
            # (the discriminator's last weight gradients, on ops' side stream, are not waited for here but in front of its optimizer
            # step: they run under the LPIPS forward below.  _DEFER_D_JOIN: tools' A/B knob)
            if _DEFER_D_JOIN:
                with ops.deferred_side_join():
                    total_d_loss.backward()
            else:
                total_d_loss.backward()
            self.reducer_D.start()                         # D's gradient all-reduce flies under the LPIPS forward below
            out.update(d_loss=d_loss.detach(), disc_stats=st)
        recon_p = ops.gradnorm(reconstructed, 1.0, None, self.gradnorm_dp_chunks)      # :662
        x_aug = x
        if rng and self.augment_before_perceptual_loss:    # :663-671
            if rng.random() < 0.5:
                recon_p, x_aug = ops.flip_nchw(recon_p, flip_w=True), ops.flip_nchw(x_aug, flip_w=True)
            if rng.random() < 0.5:
                recon_p, x_aug = ops.flip_nchw(recon_p, flip_h=True), ops.flip_nchw(x_aug, flip_h=True)
        percep = (self.lpips(recon_p, x_aug, target_feats=tg_feats) if tg_feats is not None else self.lpips(recon_p, x_aug)).mean()   # :676
        vae_loss, mom = vae_loss_device(z)                 # :680 (recon term: weight 0)
        overall = percep + vae_loss
        if self.do_ganloss:                                # :658-659 — D is updated before the generator term uses it
            ops.join_side_stream()                         # (D's weight gradients: see deferred_side_join above)
            self._finish(self.reducer_D)
            if self.on_d_backward is not None and not self._dry:
                self.on_d_backward(self)
            if not self._dry:
                self._sync_window(self.reducer_D)
                self.optimizer_D.step()                    # (dropped on the device if the D backward clipped a binary16 gradient)
                self._close_window(1, row=self._disc_row())
            self.optimizer_D.zero_grad()
        if vq_loss is not None:
            overall = overall + vq_loss
            out["vq_loss"] = vq_loss.detach()
        if self.do_ganloss:                                # :682-696 — generator GAN term with the updated D
            params = [p for p in self.disc.parameters()]
            for p in params:
                p.requires_grad_(False)                    # skip the wasted D-wgrad of the G step
            fake2 = self.disc(ops.gradnorm(reconstructed, 1.0, None, self.gradnorm_dp_chunks))
            g_gan = -fake2.mean() if self.disc_type == "hinge" else F.softplus(-fake2).mean()
            overall = overall + g_gan
            out["g_gan_loss"] = g_gan.detach()
        overall.backward()                                 # :701
        if self.do_ganloss:
            for p in params:
                p.requires_grad_(True)
        self._finish(self.reducer_G)
        if self.on_backward is not None and not self._dry:
            self.on_backward(self)
        if not self._dry:
            self._sync_window(self.reducer_G)
            self.optimizer_G.step()                        # :702 (dropped on the device if a binary16 gradient was clipped)
            self._close_window(0)
            if self._ema_vq:                               # the codebook's step: EMA update (+ reseeding on its cadence), no host sync
                usage = self.quantizer.ema_update()
                if usage is not None:
                    out["vq_perplexity"], out["vq_codes_used"] = usage[0], usage[1]
        self.optimizer_G.zero_grad()                       # :703
        if not self._dry:
            self.global_step += 1                          # lr_scheduler.step() (:704) == recompute next call
        out.update(overall_vae_loss=overall.detach(), perceptual_loss=percep.detach(), vae_loss=vae_loss.detach(),
                   z_moments=mom, reconstructed=reconstructed.detach(), z=z.detach(), target=x)
        return out


# ----------------------------------------------------------------------------- eval / checkpoints
def strip_checkpoint_prefixes(state_dict: dict) -> dict:
    """vae_trainer.py:505-513 and 903-907: checkpoints are written from the DDP wrapper (`module.` prefix).  With --do_compile
    the reference compiles `vae.module.encoder` / `.decoder` (vae_trainer.py:443-448), so its keys read
    `module.encoder._orig_mod.conv_in.weight` — `_orig_mod.` in the MIDDLE — and its loader removes it with
    `k.replace("_orig_mod.", "")` (vae_trainer.py:511).  Same here: leading `module.` prefixes go, `_orig_mod.` goes anywhere."""
    out = {}
    for k, v in state_dict.items():
        k = k.replace("_orig_mod.", "")
        while k.startswith("module."):
            k = k[len("module."):]
        out[k] = v
    return out


QUANTIZER_PREFIX = "quantizer."     # checkpoint namespace of the VQ codebook (config 5; not in the reference: SURVEY F1)


def save_checkpoint(vae: VAE, path: str, ddp_prefix: bool = True, quantizer=None) -> None:
    """torch.save of the VAE state dict in the reference's on-disk format (vae_trainer.py:903-907 saves the DDP
    wrapper's state dict, hence the `module.` prefix; fp32 OIHW conv weights).  With a VectorQuantizer (config 5) its
    state rides along under `quantizer.*` (un-prefixed: it is not part of the reference's wrapper) so that a resumed run does
    not restart from a fresh codebook; a reference loader reads the file after dropping those keys.
    Like the reference, no optimizer moments / step / LR-schedule state are saved: --load_path restarts AdamW's bias
    correction and the warm-up (vae_trainer.py:505-513)."""
    sd = {("module." + k if ddp_prefix else k): v.detach().cpu() for k, v in vae.state_dict().items()}
    if quantizer is not None:
        sd.update({QUANTIZER_PREFIX + k: v.detach().cpu() for k, v in quantizer.state_dict().items()})
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(sd, path)


def ema_checkpoint_path(path: str) -> str:
    """`<name>_ema<ext>`: the sibling file that holds the EMA weights of checkpoint `path`."""
    root, ext = os.path.splitext(path)
    return root + "_ema" + ext


def export_bf16_safetensors(vae: VAE, path: str) -> None:
    """The release format of README.hf.md:38-40 / tester_upload.sh (fal/AuraEquiVAE `*_bf16.pt`): a safetensors file of
    bf16 tensors with un-prefixed keys, loadable by `VAE(...).bfloat16().load_state_dict(load_file(path))`."""
    from safetensors.torch import save_file
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    save_file({k: v.detach().cpu().to(torch.bfloat16).contiguous() for k, v in vae.state_dict().items()}, path)


def load_checkpoint(vae: VAE, path: str, quantizer=None) -> None:
    """--load_path (vae_trainer.py:505-513): a torch.save'd state dict (any of the prefixes) or a safetensors export.
    The fp32 master weights are overwritten in place (bf16 files are widened), strict=True like the reference.
    `quantizer.*` keys (save_checkpoint with a VectorQuantizer) go to `quantizer` when one is given — strict as well: a
    codebook checkpoint must match the configured codebook — and are dropped otherwise.  An EMA quantizer's cluster sizes and
    sums ride under the same prefix; loading a file without them into an EMA quantizer starts them from the loaded codebook
    (sizes 1, sums = codebook) and says so in the log (VectorQuantizer._load_from_state_dict)."""
    with open(path, "rb") as f:
        head = f.read(8)
    is_zip_or_pickle = head[:2] == b"PK" or head[:1] == b"\x80"
    if is_zip_or_pickle:
        sd = torch.load(path, map_location="cpu")
    else:
        from safetensors.torch import load_file
        sd = load_file(path)
    sd = strip_checkpoint_prefixes(sd)
    qsd = {k[len(QUANTIZER_PREFIX):]: v for k, v in sd.items() if k.startswith(QUANTIZER_PREFIX)}
    vae.load_state_dict({k: v for k, v in sd.items() if not k.startswith(QUANTIZER_PREFIX)}, strict=True)
    if quantizer is not None and qsd:
        quantizer.load_state_dict(qsd, strict=True)
    ops.clear_pack_cache()


@torch.no_grad()
def evaluate(vae: VAE, test_batches, *, do_clamp=False, clamp_th=8.0, flip_invariance=False,
             decoder_also_perform_hr=False, enc_size=None, quantizer=None):
    """vae_trainer.py:811-886: reconstruct the first two test batches, un-normalise, clamp, and tile the first 8 images
    into the 2 x 4 grids the reference logs (each [3, 4D, 4D], only the top 2D rows are filled, as in the reference).
    With flip_invariance the latent is flipped on both axes with channels [-4:] negated and the output flipped back
    (:838-855) — the equivariance check of README.hf.md.  `quantizer`: the VectorQuantizer that takes `vae.reg`'s place in
    the train step (config 5) does so here too.  Returns (test_grid, recon_grid) on the CPU."""
    originals, recons = [], []
    for batch in test_batches:
        ori = batch[0] if isinstance(batch, (tuple, list)) else batch
        x = ops.area_downsample(ori, enc_size) if enc_size is not None else ori          # :818-820
        z = vae.encoder(x)
        if do_clamp:
            z = z.clamp(-clamp_th, clamp_th)
        z_look = None
        look_prec = getattr(vae.encoder, "lookup_precision", None) if quantizer is not None else None
        if look_prec is not None:                # policy ref_vq: the indices come from the fp32-class evaluation, as in the train step
            grad_prec, vae.encoder.precision = vae.encoder.precision, look_prec
            try:
                with torch.no_grad():
                    z_look = vae.encoder(x)
            finally:
                vae.encoder.precision = grad_prec
            if do_clamp:
                z_look = z_look.clamp(-clamp_th, clamp_th)
        z_s = (quantizer(z, lookup_from=z_look)[0] if z_look is not None else quantizer(z)[0]) if quantizer is not None else vae.reg(z)
        if flip_invariance:
            nz = z_s.shape[1]
            z_s = ops.flip_nchw(z_s, flip_h=True, flip_w=True, negate_channels=(nz - 4, nz))
        rec = vae.decoder(z_s)
        ori, rec = (ori * 0.5 + 0.5).clamp(0, 1), (rec * 0.5 + 0.5).clamp(0, 1)           # host-side image glue
        if flip_invariance:
            rec = ops.flip_nchw(rec, flip_h=True, flip_w=True)
        originals.append(ori)
        recons.append(rec)
        if len(originals) >= 2:
            break
    test, rec = torch.cat(originals, 0), torch.cat(recons, 0)
    D = 512 if decoder_also_perform_hr else 256
    D = min(D, test.shape[-1], rec.shape[-1])            # (the reference assumes >= D pixels; smaller test images tile as-is)
    test, rec = test[:, :, :D, :D].cpu(), rec[:, :, :D, :D].cpu()
    recon_grid, test_grid = torch.zeros((3, D * 4, D * 4)), torch.zeros((3, D * 4, D * 4))
    for i in range(2):
        for j in range(4):
            if i * 4 + j < test.shape[0]:
                recon_grid[:, i * D:(i + 1) * D, j * D:(j + 1) * D] = rec[i * 4 + j]
                test_grid[:, i * D:(i + 1) * D, j * D:(j + 1) * D] = test[i * 4 + j]
    return test_grid, recon_grid


def cleanup():
    if dist.is_initialized():
        dist.destroy_process_group()


def synthetic_batch(batch_size, resolution, device, generator=None):
    """x = rand(B,3,R,R)*2-1 (images are normalised to [-1,1]: vae_trainer.py:98,108)."""
    return torch.rand(batch_size, 3, resolution, resolution, device=device, generator=generator) * 2 - 1


def _build_cli():
    import click

    @click.command()
    @click.option("--dataset_url", type=str, default="", help="URL for the training dataset")
    @click.option("--test_dataset_url", type=str, default="", help="URL for the test dataset")
    @click.option("--num_epochs", type=int, default=2)
    @click.option("--batch_size", type=int, default=8, help="per rank (vae_trainer.py:479-481)")
    @click.option("--do_ganloss", is_flag=True)
    @click.option("--learning_rate_vae", type=float, default=1e-5)
    @click.option("--learning_rate_disc", type=float, default=2e-4)
    @click.option("--vae_resolution", type=int, default=256)
    @click.option("--vae_in_channels", type=int, default=3)
    @click.option("--vae_ch", type=int, default=256)
    @click.option("--vae_ch_mult", type=str, default="1,2,4,4")
    @click.option("--vae_num_res_blocks", type=int, default=2)
    @click.option("--vae_z_channels", type=int, default=16)
    @click.option("--run_name", type=str, default="run")
    @click.option("--max_steps", type=int, default=1000)
    @click.option("--evaluate_every_n_steps", type=int, default=250)
    @click.option("--load_path", type=str, default=None)
    @click.option("--do_clamp", is_flag=True)
    @click.option("--clamp_th", type=float, default=8.0)
    @click.option("--max_spatial_dim", type=int, default=256)
    @click.option("--do_attn", type=bool, default=False)
    @click.option("--decoder_also_perform_hr", type=bool, default=False)
    @click.option("--project_name", type=str, default="vae_sweep_attn_lr_width")
    @click.option("--crop_invariance", type=bool, default=False)
    @click.option("--flip_invariance", type=bool, default=False)
    @click.option("--do_compile", type=bool, default=False)
    @click.option("--use_wavelet", type=bool, default=False)
    @click.option("--augment_before_perceptual_loss", type=bool, default=False)
    @click.option("--downscale_factor", type=int, default=16)
    @click.option("--use_lecam", type=bool, default=False)
    @click.option("--disc_type", type=str, default="bce")
    # additive flags (not in the reference)
    @click.option("--synthetic", type=bool, default=True, help="seeded uniform [-1,1] images instead of webdataset")
    @click.option("--precision", type=str, default=None, help="default: ref (ref_vq with a quantizer); ref | ref2 | ref3 | ref_vq | bf16 | fp32 | fp32x3 | fp32x6 | f16x3 (PRECISION_POLICIES)")
    @click.option("--sync_vae_grads", type=bool, default=True, help="False = reference behaviour (SURVEY F2)")
    @click.option("--backend", type=str, default="nccl", help="torch.distributed backend (nccl == RCCL on ROCm)")
    @click.option("--ema_decay", type=float, default=0.0, help="decay of the generator's weight EMA (0 = off); evaluation and <ckpt>_ema files use it")
    @click.option("--ema_warmup", is_flag=True, help="EMA decay min(ema_decay, (1 + t) / (10 + t)) over the applied updates t")
    @click.option("--vgg_backbone_path", type=str, default=None,
                  help="torchvision vgg16 state dict (vgg16-397923af.pth) for LPIPS / PatchDiscriminator; default: $VQ_VGG16_WEIGHTS or ./vgg16*.pth")
    def train_ddp(**kw):
        return run_training(**kw)

    return train_ddp


def run_training(*, dataset_url="", test_dataset_url="", num_epochs=2, batch_size=8, do_ganloss=False,
                 learning_rate_vae=1e-5, learning_rate_disc=2e-4, vae_resolution=256, vae_in_channels=3, vae_ch=256,
                 vae_ch_mult="1,2,4,4", vae_num_res_blocks=2, vae_z_channels=16, run_name="run", max_steps=1000,
                 evaluate_every_n_steps=250, load_path=None, do_clamp=False, clamp_th=8.0, max_spatial_dim=256,
                 do_attn=False, decoder_also_perform_hr=False, project_name="", crop_invariance=False,
                 flip_invariance=False, do_compile=False, use_wavelet=False, augment_before_perceptual_loss=False,
                 downscale_factor=16, use_lecam=False, disc_type="bce", synthetic=True, precision=None,
                 sync_vae_grads=True, backend="nccl", log_every=5, vgg_backbone_path=None, train_batches=None,
                 test_batches=None, quantizer=None, ema_decay=0.0, ema_warmup=False):
    """train_ddp body (vae_trainer.py:339-912) for the hot path: setup, step loop, device-side logging.
    Input: `train_batches` / `test_batches` = any iterable (list, generator, DataLoader, a webdataset pipeline built by the
    caller) of [-1, 1] NCHW float batches, or (batch, label) pairs as the reference's loader yields (vae_trainer.py:530:
    `real_images_hr[0]`); host tensors are moved to the rank's device.  The train iterable is walked `num_epochs` times or
    until `max_steps`; every rank must be handed its own shard (the reference splits by node and worker inside webdataset,
    vae_trainer.py:119-140 — that I/O layer is out of scope here).  Without iterables: `--synthetic True` (default)
    feeds uniform-noise batches resident in HBM; `--synthetic False` needs the iterables.
    `quantizer`: a VectorQuantizer in place of `vae.reg` (config 5): trained, evaluated and checkpointed with the VAE.
    `ema_decay` > 0 (`--ema_decay`, `--ema_warmup`): the generator's weight EMA (VAETrainStep) — the logged reconstructions are the
    EMA model's, every checkpoint `X.pt` is followed by `X_ema.pt` in the same format (save_checkpoint inside `ema_weights()`), and
    `--load_path X.pt` resumes the shadow from `X_ema.pt` when that file exists."""
    if not synthetic and train_batches is None:
        raise NotImplementedError("no input: pass train_batches=<iterable of [-1,1] NCHW batches> to run_training (the reference's "
                                  "webdataset pipeline, vae_trainer.py:119-140, is out of scope) or use --synthetic True")
    if do_compile:
        logging.warning("--do_compile is accepted and ignored: no tracing compiler on the HIP path")
    torch.manual_seed(42)                                  # vae_trainer.py:374-378
    random.seed(42)
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    use_cuda = torch.cuda.is_available() and backend == "nccl"
    device = torch.device(f"cuda:{local_rank}") if use_cuda else torch.device("cpu")
    if use_cuda:
        torch.cuda.set_device(device)
        torch.cuda.manual_seed_all(42)
    own_group = (world > 1 or "RANK" in os.environ) and not dist.is_initialized()
    if own_group:
        dist.init_process_group(backend=backend)
    precision_given = precision is not None      # an explicit --precision is taken at its word (also `ref` with a quantizer)
    if precision is None:
        precision = "ref"
    if precision not in PRECISION_POLICIES:
        raise ValueError(f"--precision {precision}: expected one of {', '.join(PRECISION_POLICIES)}")
    vae = VAE(resolution=vae_resolution, in_channels=vae_in_channels, ch=vae_ch, out_ch=vae_in_channels,
              ch_mult=[int(x) for x in vae_ch_mult.split(",")], num_res_blocks=vae_num_res_blocks,
              z_channels=vae_z_channels, use_attn=do_attn, decoder_also_perform_hr=decoder_also_perform_hr,
              use_wavelet=use_wavelet).to(device)
    discriminator = PatchDiscriminator(backbone_path=vgg_backbone_path).to(device) if do_ganloss else None
    prepare_filter(device)
    if quantizer is not None:
        quantizer = quantizer.to(device)
    if load_path is not None:                              # vae_trainer.py:505-513 (DDP 'module.' / '_orig_mod.' prefixes)
        load_checkpoint(vae, load_path, quantizer=quantizer)
    broadcast_parameters(vae)
    if quantizer is not None:
        broadcast_parameters(quantizer)
    if discriminator is not None:
        broadcast_parameters(discriminator)
    lpips = LPIPS(backbone_path=vgg_backbone_path).to(device)      # train mode => Dropout live
    if rank == 0 and not lpips.backbone_loaded:
        logging.warning("LPIPS / PatchDiscriminator run on a randomly initialised VGG16 (no ImageNet weights found): "
                        "pass --vgg_backbone_path or set VQ_VGG16_WEIGHTS")
    if quantizer is not None and not precision_given:      # the code lookup is integer work: keep its input fp32-class (PRECISION_POLICIES)
        precision = "ref_vq"
        if rank == 0:
            logging.info("quantizer in place of `reg`: precision policy ref -> ref_vq (encoder in the fp32-class split, indices bit-exact)")
    apply_precision_policy(precision, vae, lpips, discriminator)
    step = VAETrainStep(vae, lpips, discriminator, do_ganloss=do_ganloss, disc_type=disc_type, use_lecam=use_lecam,
                        learning_rate_vae=learning_rate_vae, learning_rate_disc=learning_rate_disc, vae_ch=vae_ch,
                        max_steps=max_steps, do_clamp=do_clamp, clamp_th=clamp_th, sync_vae_grads=sync_vae_grads,
                        rng=None, enc_size=(vae_resolution, vae_resolution), flip_invariance=flip_invariance, crop_invariance=crop_invariance,
                        augment_before_perceptual_loss=augment_before_perceptual_loss,
                        decoder_also_perform_hr=decoder_also_perform_hr, downscale_factor=downscale_factor, quantizer=quantizer,
                        ema_decay=ema_decay, ema_warmup=ema_warmup)
    logger = logging.getLogger(__name__)
    logger.setLevel(logging.INFO)
    if rank == 0 and not logger.handlers:
        logger.addHandler(logging.StreamHandler())
    use_ema = bool(ema_decay)
    if use_ema and load_path is not None:                  # every rank reads the same file (or none): the shadows start from the same bits
        step.load_ema(ema_checkpoint_path(load_path))
    gen = torch.Generator(device=device).manual_seed(42 + rank)
    img_res = vae_resolution * (2 if decoder_also_perform_hr else 1)
    test_gen = torch.Generator(device=device).manual_seed(4242)
    def on_device(batch):                                  # (batch, label) pairs as in vae_trainer.py:530; host tensors -> HBM
        x = batch[0] if isinstance(batch, (tuple, list)) else batch
        return x.to(device=device, dtype=torch.float32, non_blocking=True)

    if rank != 0:
        eval_batches = []
    elif test_batches is not None:                         # vae_trainer.py:811-816: the first two test batches
        eval_batches = [on_device(b) for _, b in zip(range(2), test_batches)]
    else:
        eval_batches = [synthetic_batch(4, img_res, device, test_gen) for _ in range(2)]

    def batches():
        if train_batches is None:
            while True:
                yield synthetic_batch(batch_size, img_res, device, gen)
        for _ in range(num_epochs):                        # vae_trainer.py:520-523
            for b in train_batches:
                yield on_device(b)

    t0 = time.time()
    history = []
    for global_step, x in zip(range(max_steps), batches()):
        if step.fp16_stacks() and global_step % max(evaluate_every_n_steps, 250) == 0:
            rep = step.calibrate_grad_scales(x)            # loss scales of the fp16 stacks from measured gradient maxima
            if rank == 0:
                logger.info("fp16 loss scales: " + ", ".join(f"{r['region']}=2^{math.log2(r['grad_scale']):.0f}" for r in rep))
        res = step(x)
        # vae_trainer.py:805-910: the reference tests `global_step % n == 1` AFTER incrementing the counter
        if evaluate_every_n_steps > 0 and (global_step + 1) % evaluate_every_n_steps == 1 and rank == 0:
            eval_kw = dict(do_clamp=do_clamp, clamp_th=clamp_th, flip_invariance=flip_invariance,
                           decoder_also_perform_hr=decoder_also_perform_hr, enc_size=(vae_resolution, vae_resolution), quantizer=quantizer)
            ckpt = f"./ckpt/{run_name}/vae_epoch_0_step_{global_step + 1}.pt"
            if not use_ema:
                evaluate(vae, eval_batches, **eval_kw)
            save_checkpoint(vae, ckpt, quantizer=quantizer)
            logger.info(f"Saved checkpoint to {ckpt}")
            if use_ema:                                    # ONE swap: the logged grids are the EMA model's, and so is the second file —
                with step.ema_weights():                   # the same writer, the same keys and layout: any loader of `ckpt` reads it
                    evaluate(vae, eval_batches, **eval_kw)
                    save_checkpoint(vae, ema_checkpoint_path(ckpt), quantizer=quantizer)
                logger.info(f"Saved EMA checkpoint to {ema_checkpoint_path(ckpt)}")
        if global_step % log_every == 0:                   # the only host syncs: every `log_every` steps (every rank: the poll may re-calibrate)
            rec = logged_scalars(res, step, do_ganloss) if rank == 0 else {}
            rec["time_taken_till_step"] = time.time() - t0
            ev = step.poll_range_events()                  # binary16 overflow / underflow signal of the fp16 stacks (same sync)
            relaxed = step.relax_hot_scales(ev)            # gradients within three bits of the limit: lower those scales now
            if relaxed and rank == 0:
                logger.info(f"step {global_step}: binary16 gradient stores reached 2^13 in " + ", ".join(r for r, _ in relaxed) +
                            "; loss scales lowered ahead of a clip: " + ", ".join(f"{r}=2^{s:.0f}" for r, s in relaxed))
            bad = [e for e in ev["stacks"] if e["saturated"]]
            if bad or ev["skipped_G"] or ev["skipped_D"]:
                rep = step.calibrate_grad_scales(x)        # collective-safe: every rank polls and sees the all-reduced windows
                if rank == 0:
                    logger.warning(f"step {global_step}: binary16 stores saturated in " + ", ".join(f"{e['region']} ({e['saturated']} waves)" for e in bad) +
                                   f"; {ev['skipped_G']} G / {ev['skipped_D']} D optimizer steps were dropped on the device; loss scales now " +
                                   ", ".join(f"{r['region']}=2^{math.log2(r['grad_scale']):.0f}" for r in rep))
            stuck = [e["region"] for e in ev["stacks"] if e["fwd_saturated_polls"] >= 2]
            if stuck:                                      # forward activations at binary16's limit for two log lines in a row
                moved = step.escalate_forward_saturation(stuck)
                if rank == 0 and moved:
                    logger.warning(f"step {global_step}: forward activations keep saturating binary16 (stored unscaled: no loss scale "
                                   "can help); " + ", ".join(f"{r} now runs in {to}" for r, to in moved))
                elif rank == 0:
                    logger.warning(f"step {global_step}: forward activations of {', '.join(stuck)} keep saturating binary16 and no "
                                   "stack could be moved to a wider type")
            if rank == 0:
                rec["fp16/fwd_saturated_waves"] = sum(e["fwd_saturated"] for e in ev["stacks"])
                rec["fp16/saturated_waves"] = sum(e["saturated"] for e in ev["stacks"])
                rec["fp16/flushed_waves"] = sum(e["flushed"] for e in ev["stacks"])
                rec["fp16/skipped_steps"] = ev["skipped_G"] + ev["skipped_D"]
                history.append(rec)
                logger.info(f"step {global_step} " + " ".join(f"{k}={v:.5f}" for k, v in rec.items() if isinstance(v, (int, float))))
        t0 = time.time()
    if own_group:                       # vae_trainer.py:911 `cleanup()`: only the group this call brought up (an embedding program's stays)
        cleanup()
    return history


def logged_scalars(res: dict, step: VAETrainStep, do_ganloss: bool) -> dict:
    """The scalars the reference sends to wandb every 5 steps (vae_trainer.py:713-748), under its names, from what the step left on
    the device: one host sync here instead of ~10 `.item()` / `.cpu()` calls inside every step (vae_trainer.py:541,640-652,688-693).
    `mse_loss` is the reference's `recon_loss` = 0 (its term is multiplied by 0.0, :209); the logvar entries are 0 as there (:212-216)."""
    m2, ss, sa, n = res["z_moments"].tolist()
    mean_abs = sa / n
    var_abs = m2 / max(n - 1, 1)
    rec = {"overall_vae_loss": float(res["overall_vae_loss"]), "mse_loss": 0.0, "kl_loss": ss / n,
           "perceptual_loss": float(res["perceptual_loss"]), "vae_loss": float(res["vae_loss"]),
           "z_quantiles/abs_z": mean_abs, "z_quantiles/std_z": math.sqrt(var_abs), "z_quantiles/logvar": 0.0}
    z = res["z"].detach().float().reshape(-1).cpu()                       # vae_trainer.py:541-557 (there: every step)
    qs = {f"{q:.1f}": float(z.quantile(q)) if z.numel() <= 16_000_000 else float("nan") for q in (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)}
    zc = z - z.mean()
    sd = float(z.std())
    qs["kurtosis"] = float((zc ** 4).mean()) / max(sd ** 4, 1e-30)
    qs["skewness"] = float((zc ** 3).mean()) / max(sd ** 3, 1e-30)
    rec["z_quantiles/qs"] = qs
    if "vq_loss" in res:
        rec["vq_loss"] = float(res["vq_loss"])
    if "vq_perplexity" in res:                # EMA codebook: usage of the step's batch (quantizer.ema_update)
        rec["vq_perplexity"], rec["vq_codes_used"] = float(res["vq_perplexity"]), float(res["vq_codes_used"])
    if do_ganloss:
        st = res["disc_stats"].tolist()       # {loss_real, loss_fake, mean_real, mean_fake, n_correct, count}
        anchor = step.lecam_anchor.tolist()
        rec.update({"gan/generator_gan_loss": float(res["g_gan_loss"]), "gan/avg_real_logits": st[2], "gan/avg_fake_logits": st[3],
                    "gan/discriminator_loss": float(res["d_loss"]), "gan/discriminator_accuracy": st[4] / max(st[5], 1.0),
                    "gan/lecam_loss": float(res["lecam_loss"]), "gan/lecam_anchor_real_logits": anchor[0],
                    "gan/lecam_anchor_fake_logits": anchor[1]})
    return rec


train_ddp = _build_cli()


def main():
    train_ddp()


if __name__ == "__main__":
    main()
