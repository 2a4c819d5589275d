"""bench.py — whole-job throughput of the VAE train step on MI355X (driver contract in the task).

A "step" is one full iteration of the reference's loop body (vae_trainer.py:525-708) on one synthetic
batch already resident in HBM: encoder -> reg -> decoder -> [D(real), D(fake), D loss bwd, D AdamW]
-> GradNorm -> LPIPS -> z-regulariser -> G GAN term -> backward -> bucketed gradient all-reduce ->
fused AdamW (both param groups) -> LR schedule.  Nothing is skipped inside the timed region.

Workload (BASELINE.json): metric "images/sec full train step (enc+dec+LPIPS+disc+bwd), 256x256 f=8";
default = configs[2] "vae_ch=128 ch_mult=1,2,4,4 f=8, batch=16 256x256, LPIPS + PatchDiscriminator +
GradNorm" per GPU (the configuration the metric's "disc" names; `--workload c2` drops the GAN branch =
configs[1]).  N>1: one process per GPU over RCCL, the batch dimension shards data-parallel, weak scaling;
`python bench.py --gpus N` without a torchrun environment re-launches itself under torch.distributed.run
(the reference's launcher.sh:3-9 is a torchrun line too).

Precision (`--precision`, vae_trainer.PRECISION_POLICIES): the default mirrors the reference's own mixed step
(encoder / LPIPS / discriminator at TF32-class operand precision or better, decoder bf16 as under its autocast);
`bf16` is the all-bf16 throughput mode, reported beside it on the same line (`bf16_mode`).

A plain run (`--gpus 1 --steps N --warmup W`) does only what the headline needs: set-up (model, resident batches, loss-scale
calibration and the rehearsal of the timed steps), W warm-up steps, the N timed steps, then the JSON line (`value`, `ms_per_step`, ...).
`--dump-outputs DIR` also writes what the LAST timed step returned to its caller (VAETrainStep.__call__'s dictionary: losses,
reconstruction, latents, ...) as DIR/<name>.npy — the inputs are seeded, so two builds can be compared output for output.
Everything else this file measures or checks runs only with `--full`, and is then unchanged.

Extra objects on the JSON line (`--full`):
  roofline     — dominant kernel family (implicit-GEMM conv fwd/dgrad on MFMA): algorithmic FLOPs of every launch in the
                 timed region / their HIP-event durations, vs the dense MFMA peak; `wgrad` = the weight-gradient family,
                 `conv3x3` = the 3x3 conv GEMMs with >= 64 channels on both sides in all three passes (the north-star's 40 %
                 sub-metric); `traffic` = HBM bytes per launch of the family from the PMC passes of tools/gpu_traffic.sh
                 (read from profiles/<round>_traffic.json when present: PMC counters cannot be collected from inside).
  hbm          — the HBM-bound families (GroupNorm passes, LPIPS tail, max-pool, GradNorm, AdamW, weight re-pack, layout):
                 algorithmic bytes / HIP-event time of every call in a short instrumented pass AFTER the timed region.
  parity       — the timed precision against the CPU fp32 oracle on the batch the cpu_baseline leg runs (same weights).
  comm         — N > 1: un-overlapped duration of the step's gradient all-reduces and the part the compute stream waited for.
  cpu_baseline — the oracle's restated reference step (oracle/model_ref.py, plain PyTorch CPU fp32) timed on this box's
                 host cores: configs[0] in full, and the benchmark's model at batch 2 (rank 0, N=1 only).
"""
from __future__ import annotations

import argparse
import glob
import math
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

# TEST-ONLY device switch (tests/test_bench_multirank.py): "emu" runs main() on host cores through the fiber emulator build of the
# kernel sources (tests/emu) with gloo collectives and a toy configuration ($VQ_BENCH_TEST_CFG), so that every rank-gated branch of
# this file — the `comm` block, calibration rounds, the instrumented pass, the secondary leg — is executed with 2 ranks before the
# first multi-GPU run on hardware.  Nothing it prints is a measurement; the driver never sets it.
TEST_DEVICE = os.environ.get("VQ_BENCH_TEST_DEVICE", "")


class _HostEvent:
    """torch.cuda.Event stand-in of the test device: wall clock at record()."""

    def record(self):
        self.t = time.perf_counter()

    def elapsed_time(self, other):
        return (other.t - self.t) * 1e3


def _event():
    return _HostEvent() if TEST_DEVICE else torch.cuda.Event(enable_timing=True)


def _sync():
    if not TEST_DEVICE:
        torch.cuda.synchronize()


def _empty_cache():
    if not TEST_DEVICE:
        torch.cuda.empty_cache()


PEAK_MFMA_TFLOPS = 2500.0     # MI355X dense bf16 / fp16 MFMA (MI355X_MICROARCH.md: 2.5 PF spec, 2495 TF measured)
PEAK_FP32_VECTOR_TFLOPS = 157.3   # MI355X fp32 vector / fp32-MFMA peak (same guide): the bound of the nearest-code search's fixed-order fp32 FMA chains
PEAK_HBM_GBS = 8000.0         # HBM3E spec; 6290 GB/s is what a float4 copy reaches (same guide)
DEFAULT_PRECISION = "ref"          # c5 (the quantized workload): "ref_vq" — the code lookup is integer work, its input stays fp32-class

DTYPE_NAMES = {
    "bf16": "bf16",
    "fp32": "bf16 MFMA operands / fp32 storage",
    "fp32x3": "bf16x3-split (fp32-class)",
    "fp32x6": "bf16x6-split (fp32-exact products: three bf16 pieces per operand)",
    "ref3": "mixed like the reference: encoder+LPIPS+discriminator bf16x3-split (fp32-class, >= TF32), decoder bf16",
    "ref_vq": "ref (encoder+LPIPS+discriminator fp16 operands, decoder bf16) + a gradient-free bf16x3-split (fp32-class) evaluation of the encoder that the integer code lookup reads: indices bit-exact",
    "f16x3": "binary16 hi+lo pairs (22 significand bits per value), three binary16 MFMAs per product, fp32 accumulate (fp32-class: meets the 1e-4 gate)",
    "ref2": "encoder fp16 operands; decoder+LPIPS+discriminator binary16 hi+lo pairs, three MFMAs per product (fp32-class)",
    "ref": "mixed like the reference: encoder+LPIPS+discriminator fp16 operands (TF32's 10-bit mantissa) / fp32 accumulate, decoder bf16",
}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="c3", choices=["c2", "c3", "c5", "l1", "l2"],
                    help="BASELINE.json configs[1] / configs[2] (default: the one the metric is quoted on) / configs[4] per-GPU share; "
                         "l1 / l2 = the reference's own launch lines (launcher.sh:7-21: vae_ch=64, batch 12, bce GAN, HR decoder 256 -> 512; "
                         "scripts/launch_hdr.sh:9-30: vae_ch=128 1,2,4,4,4 z=64, wavelet front-end, HR decoder, batch 4, hinge + lecam) — "
                         "per-GPU shapes the dispatch rules were NOT fitted on")
    ap.add_argument("--batch", type=int, default=0, help="per GPU (default: 16; 8 for c5)")
    ap.add_argument("--precision", default="", choices=[""] + list(DTYPE_NAMES), help="default: ref (c2 / c3), ref_vq (c5)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline: instrumented + serial passes (roofline), HBM-family pass, fp16 report, comm, "
                         "the other precisions, the configs[4] leg, CPU baseline and parity against the oracle (minutes); the --no-* options "
                         "below trim that set")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the tensors the last timed step returned as DIR/<name>.npy (float32; integers as float64; at most 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-calibrate", action="store_true",
                    help="keep the default loss scales of the fp16 stacks (PMC passes under rocprofv3: traffic only, no timing claims)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the all-bf16 secondary measurement and the HBM-family pass")
    ap.add_argument("--conv-table", default="", help="write the per-layer-shape conv timing table to this path")
    ap.add_argument("--cpu-baseline-res", type=int, default=256)
    ap.add_argument("--parity-steps", type=int, default=5, help="optimizer steps of the HIP-vs-oracle trajectory in `parity_randomized`")
    ap.add_argument("--no-serial-pass", action="store_true", help="skip the one-stream pass the per-kernel roofline fractions are timed in")
    ap.add_argument("--no-c5-leg", action="store_true", help="skip the configs[4] (VQ, 512x512) leg of the default line")
    ap.add_argument("--parity-mode-steps", type=int, default=5, help="timed steps of each `parity_mode` leg (fp32x6 / fp32x3 / ref3)")
    args = ap.parse_args(argv)
    if not args.full:
        if args.conv_table:
            ap.error("--conv-table needs --full (the per-layer table is timed in the serial pass)")
        args.no_cpu_baseline = args.no_secondary = args.no_c5_leg = True
    if not args.precision:
        args.precision = "ref_vq" if args.workload == "c5" else DEFAULT_PRECISION
    return args


class ConvTimer:
    """HIP-event timing of library calls on the stream they are launched on (torch's current stream): the conv GEMM
    launches (kinds conv_igemm / conv_wgrad, work = algorithmic FLOPs) and, when `hbm` is on, the HBM-bound families
    (kind "hbm:<family>", work = algorithmic bytes)."""

    def __init__(self):
        self.records = []     # (kind, work, start_event, end_event, tag)
        self.enabled = False
        self.hbm = False

    def launch(self, kind, work, fn, tag=""):
        if kind.startswith("hbm:"):
            if not self.hbm:
                return fn()
        elif not self.enabled:
            return fn()
        s, e = _event(), _event()
        s.record()
        fn()
        e.record()
        self.records.append((kind, work, s, e, tag))

    def table(self, steps):
        """Per layer-shape rows: launches/step, ms/step, achieved TFLOP/s — sorted by time."""
        agg = {}
        for kind, flops, s, e, tag in self.records:
            if kind.startswith("hbm:"):
                continue
            d = agg.setdefault(tag, [0, 0.0, 0.0])
            d[0] += 1
            d[1] += flops
            d[2] += s.elapsed_time(e)
        rows = sorted(agg.items(), key=lambda kv: -kv[1][2])
        tot = sum(v[2] for _, v in rows) or 1.0
        lines = [f"{'layer':46s} {'n/step':>6s} {'ms/step':>8s} {'share':>6s} {'TFLOP/s':>8s}"]
        for tag, (n, fl, ms) in rows:
            lines.append(f"{tag:46s} {n / steps:6.1f} {ms / steps:8.3f} {ms / tot:6.1%} {fl / ms / 1e9:8.1f}")
        return "\n".join(lines)

    def family(self, pred):
        """(launches, FLOPs, seconds) over the records whose (what, cin, cout, k, stride) parsed from the layer tag satisfy
        pred — e.g. the 3x3 convolution GEMMs the north-star target is stated on."""
        import re
        pat = re.compile(r"^(\w+) (\d+)->(\d+) in \d+x\d+x\d+ k(\d+) s(\d+) up")
        n, fl, sec = 0, 0.0, 0.0
        for _kind, flops, s, e, tag in self.records:
            m = pat.match(tag)
            if m and pred(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5))):
                n += 1
                fl += flops
                sec += s.elapsed_time(e) * 1e-3
        return n, fl, sec

    def conv_bytes(self, kind="conv_igemm"):
        """Algorithmic HBM bytes of the recorded launches of `kind` (16-bit storage): one read of the input tensor and of the
        weights, one write of the output — what the layer moves if nothing is read twice; residual / bias /
        mask operands are left out, so the PMC traffic of a fused epilogue may legitimately exceed it by the residual read."""
        import re
        pat = re.compile(r"^\w+ (\d+)->(\d+) in (\d+)x(\d+)x(\d+) k(\d+) s(\d+) up(\d+)")
        n, tot = 0, 0.0
        for k, _w, _s, _e, tag in self.records:
            m = pat.match(tag) if k == kind else None
            if not m:
                continue
            ci, co, N, H, W, r, st, up = (int(g) for g in m.groups())
            ho, wo = H * up // st, W * up // st
            tot += 2.0 * (N * H * W * ci + N * ho * wo * co + r * r * ci * co)
            n += 1
        return n, tot

    def summary(self):
        out = {}
        for kind, work, s, e, _tag in self.records:
            d = out.setdefault(kind, [0, 0.0, 0.0])
            d[0] += 1
            d[1] += work
            d[2] += s.elapsed_time(e) * 1e-3
        return out

    def hbm_rows(self, steps):
        """[{kernel, calls_per_step, ms_per_step, GB/s, frac_of_8TBps}] of the HBM-bound families, slowest first."""
        rows = []
        for kind, (n, nbytes, sec) in self.summary().items():
            if not kind.startswith("hbm:") or sec <= 0:
                continue
            gbs = nbytes / sec / 1e9
            rows.append({"kernel": kind[4:], "calls_per_step": round(n / steps, 1), "ms_per_step": round(sec / steps * 1e3, 3),
                         "algorithmic_MB_per_step": round(nbytes / steps / 1e6, 1), "GB/s": round(gbs, 1),
                         "frac_of_8TBps": round(gbs / PEAK_HBM_GBS, 3)})
        return sorted(rows, key=lambda r: -r["ms_per_step"])


def _median_time(fn, n):
    ts = []
    for _ in range(n):
        t0 = time.time()
        fn()
        ts.append(time.time() - t0)
    return statistics.median(ts)


# What the restated loop that is timed here (`kind: "port"`) was pinned against — to 2e-5 over three optimizer steps, same ATen ops:
# tests/test_oracle.py::test_train_step_restatement_matches_reference_modules against the steps recorded from the reference's own
# modules (tests/golden/train_step_ref_*.npz; like every tests/golden/*.npz an output of those modules, tests/golden/make_golden.py)
REFERENCE_PIN = ("cloneofsimo/vqgan-training (a snapshot without .git, files dated 2026-09-26; sha256[:16] ae.py 80e614adf9414229, "
                 "utils.py 80d49ec4f8d5f97b, vae_trainer.py 266616fb3991bbe2): three training steps of its own modules recorded in "
                 "tests/golden/train_step_ref_*.npz; pinned by tests/test_oracle.py::test_train_step_restatement_matches_reference_modules")


def cpu_baseline(args, cfg, configs0=True):
    """Oracle = restated reference step on CPU fp32 (kind 'port'), SURVEY §8(d): 1 warm-up + 3 timed steps, median;
    configs[0] (ch=64, 1,2, B=4, 128x128, no GAN) in full, then the benchmark's model at batch 2.  Returns the bench-line
    object and what the parity leg needs: (state dicts, batch, first-step outputs of the oracle from those weights)."""
    from oracle import model_ref as M
    import vqgan_training_amd as vq
    ncpu = os.cpu_count() or 1

    def fresh_state(ch, mult, z, res, gan, seed=42):
        torch.manual_seed(seed)
        vae = vq.ae.VAE(res, 3, ch, 3, list(mult), 2, z, False, False, False)
        lp = vq.utils.LPIPS(pretrained_path=None)
        disc = vq.utils.PatchDiscriminator() if gan else None
        sds = (vae.state_dict(), lp.state_dict(), None if disc is None else disc.state_dict())
        return sds

    # ---- configs[0] in full; also picks the intra-op thread count (PyTorch's CPU convolutions stop scaling, and collapse
    # when oversubscribed, long before the 256 hardware threads of the GPU box)
    kw1 = dict(do_ganloss=False, learning_rate_vae=1e-5, vae_ch=64, max_steps=1000)
    sds1 = fresh_state(64, (1, 2), 16, 128, False)
    g = torch.Generator().manual_seed(1)
    x1 = torch.rand(4, 3, 128, 128, generator=g) * 2 - 1
    best = None
    for thr in (sorted({t for t in (8, 16, 32, 64) if t <= ncpu} or {ncpu}) if configs0 else []):
        torch.set_num_threads(thr)
        st = M.RefState(*sds1)
        M.train_step_ref(st, x1, **kw1)                                  # warm-up (thread pool, allocator)
        dt = _median_time(lambda: M.train_step_ref(st, x1, **kw1), 3)
        if best is None or dt < best[0]:
            best = (dt, thr)
    dt1, thr = best if best is not None else (float("nan"), torch.get_num_threads())
    torch.set_num_threads(thr)
    # ---- the benchmark's model at batch 2: the first step (from the initial weights) is the warm-up AND the parity reference
    res = args.cpu_baseline_res
    kw = dict(do_ganloss=cfg["gan"], disc_type="hinge", learning_rate_vae=1e-5, vae_ch=cfg["ch"], max_steps=1000)
    sds = fresh_state(cfg["ch"], cfg["ch_mult"], cfg["z"], res, cfg["gan"])
    st = M.RefState(*sds)
    x = torch.rand(2, 3, res, res, generator=g) * 2 - 1
    t0 = time.time()
    first = M.train_step_ref(st, x, **kw)
    t_first = time.time() - t0
    n_timed = 3 if t_first < 15 else 1
    dt = _median_time(lambda: M.train_step_ref(st, x, **kw), n_timed)
    line = {"value": round(2.0 / dt, 4), "unit": "images/sec", "cores": thr, "kind": "port", "pinned_against": REFERENCE_PIN,
            "sample": f"restated reference loop (oracle/model_ref.py), CPU fp32, {thr} intra-op threads (best of 8..64 on configs[0]; "
                      f"{ncpu} logical CPUs on the box): the benchmark's model at batch 2, {res}x{res}: 1 warm-up + {n_timed} timed "
                      f"steps, median {dt:.2f} s/step",
            "configs0": {"value": round(4.0 / dt1, 3), "unit": "images/sec", "ms_per_step": round(dt1 * 1e3, 1),
                         "sample": "configs[0] in full: vae_ch=64 ch_mult=1,2, batch 4, 128x128, LPIPS only, 1 warm-up + 3 timed steps, median"}}
    return line, (sds, x, first, kw)


def _hip_step_from(sds, res, kw, policy, device, on_backward=None, codebook=None):
    """Fresh HIP modules holding the oracle's weights, pinned to `policy`, wrapped in a VAETrainStep (LPIPS in eval mode like the
    oracle: the reference's Dropout draws are not reproducible across libraries)."""
    import warnings
    import vqgan_training_amd as vq
    vae_sd, lp_sd, disc_sd = sds
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ch = vae_sd["encoder.conv_in.weight"].shape[0]
        mult, lvl = [], 0
        while f"encoder.down.{lvl}.block.0.conv1.weight" in vae_sd:
            mult.append(vae_sd[f"encoder.down.{lvl}.block.0.conv1.weight"].shape[0] // ch)
            lvl += 1
        z = vae_sd["encoder.conv_out.weight"].shape[0]
        vae = vq.ae.VAE(res, 3, ch, 3, mult, 2, z, False, False, False)
        vae.load_state_dict(vae_sd)
        lp = vq.utils.LPIPS(pretrained_path=None)
        lp.load_state_dict(lp_sd)
        disc = None
        if disc_sd is not None:
            disc = vq.utils.PatchDiscriminator()
            disc.load_state_dict(disc_sd)
    vae, lp = vae.to(device), lp.to(device).eval()
    disc = disc.to(device) if disc is not None else None
    vq.vae_trainer.apply_precision_policy(policy, vae, lp, disc)
    quant = None
    if codebook is not None:     # configs[4]: the quantizer in `reg`'s place
        quant = vq.quantizer.VectorQuantizer(codebook.shape[0], codebook.shape[1], beta=kw.get("vq_beta", 0.25))
        with torch.no_grad():
            quant.embedding.weight.copy_(codebook)
        quant = quant.to(device)
    step = vq.vae_trainer.VAETrainStep(vae, lp, disc, do_ganloss=kw["do_ganloss"], disc_type=kw.get("disc_type", "hinge"),
                                       learning_rate_vae=kw["learning_rate_vae"], vae_ch=kw["vae_ch"], max_steps=kw["max_steps"],
                                       warmup_steps=kw.get("warmup_steps", 200), on_backward=on_backward, quantizer=quant)
    return step, vae


# the policies meant to MEET north_star's 1e-4 against the CPU fp32 oracle, cheapest first
TOLERANCE_POLICIES = ("f16x3", "fp32x6", "fp32x3")


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-30)


def _sig(v):
    return float(f"{v:.3e}")


def _deviation(got, want, grads=None):
    """Relative deviations of one step's logged scalars (+ reconstruction, + the global L2 error of the VAE gradients) from the
    fp32 oracle step `want`."""
    out = {"perceptual_loss_rel": _sig(_rel(got["perceptual_loss"], want["perceptual_loss"])),
           "overall_vae_loss_rel": _sig(_rel(got["overall_vae_loss"], want["overall_vae_loss"]))}
    for k in ("d_loss", "g_gan_loss"):
        if k in want and k in got:
            out[k + "_rel"] = _sig(_rel(got[k], want[k]))
    rec_g, rec_w = got["reconstructed"].float().cpu(), want["reconstructed"]
    out["recon_rel"] = _sig(((rec_g - rec_w).abs().max() / rec_w.abs().max()).item())
    out["recon_rel_l2"] = _sig(((rec_g - rec_w).norm() / rec_w.norm()).item())
    if grads is not None:
        num = sum(((grads[k].float().cpu() - v) ** 2).sum().item() for k, v in want["grads"].items())
        den = sum((v ** 2).sum().item() for v in want["grads"].values())
        out["vae_grad_l2_rel"] = _sig((num / max(den, 1e-300)) ** 0.5)
    return out


def parity_vs_oracle(policy, ref, device):
    """The HIP step at the timed precision on the oracle's batch and CONSTRUCTOR-INITIALISED weights -> relative deviations of the
    logged scalars.  (Weak on its own — every ResnetBlock conv2 is ~1e-4/out_ch and the discriminator heads are zero at init,
    ae.py:119-121, utils.py:161-185: SURVEY F11 — see parity_randomized for the weights that exercise the kernels.)"""
    import vqgan_training_amd as vq
    sds, x, first, kw = ref
    step, _vae = _hip_step_from(sds, x.shape[-1], kw, policy, device)
    step.calibrate_grad_scales(x.to(device))
    got = step(x.to(device))
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    out = {"vs": "oracle/model_ref.py (CPU fp32), constructor-initialised weights, batch 2, LPIPS eval mode", "precision": policy}
    out.update(_deviation(got, first))
    del step, _vae
    vq.ops.clear_caches()
    if torch.device(device).type == "cuda":
        torch.cuda.empty_cache()
    return out


def parity_randomized(policy, cfg, res, device, n_traj=5):
    """Parity at the benchmark's model on weights that EXERCISE the kernels (oracle/weights.randomize_state_dict: SURVEY F11), batch 2:
      * first step: losses (perceptual / overall / d_loss / g_gan), reconstruction and the global L2 error of the VAE gradients of
        the timed policy against the fp32 oracle — next to the SAME quantities for the oracle's emulation of the reference's own GPU
        arithmetic (TF32 convolutions outside autocast, bf16 autocast in the decoder: oracle.model_ref.REFERENCE_GPU_ARITH), so the
        line says "ours X, the reference's own CUDA path Y";
      * trajectory: n_traj optimizer steps (AdamW, cosine schedule without warm-up so that every step moves the weights, the GAN
        branch with D at its real 2e-4) HIP vs fp32 oracle, per-step relative loss deviations, and beside each the deviation of the
        SAME trajectory run in the reference's emulated GPU arithmetic (`*_rel_reference_gpu_arithmetic`): a GAN trajectory amplifies
        round-off (AdamW's first updates are +-lr per element whatever the gradient's size), so "how far after n steps" only means
        something next to how far the reference's own arithmetic drifts."""
    from oracle import model_ref as M
    from oracle import weights as W
    import vqgan_training_amd as vq
    torch.manual_seed(7)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vae0 = vq.ae.VAE(res, 3, cfg["ch"], 3, list(cfg["ch_mult"]), 2, cfg["z"], False, False, False)
        lp0 = vq.utils.LPIPS(pretrained_path=None)
        disc0 = vq.utils.PatchDiscriminator() if cfg["gan"] else None
    sds = (W.randomize_state_dict(vae0.state_dict(), 1), W.randomize_state_dict(lp0.state_dict(), 2, relu_net=True),
           None if disc0 is None else W.randomize_state_dict(disc0.state_dict(), 4, relu_net=True))
    del vae0, lp0, disc0
    kw = dict(do_ganloss=cfg["gan"], disc_type="hinge", learning_rate_vae=1e-5, vae_ch=cfg["ch"], max_steps=1000, warmup_steps=0)
    x = W.image_batch(2, res, seed=11)
    t0 = time.time()
    st = M.RefState(*sds)
    exact = [M.train_step_ref(st, x, **kw) for _ in range(n_traj)]
    st_emu = M.RefState(*sds)
    emus = [M.train_step_ref(st_emu, x, arith=M.REFERENCE_GPU_ARITH, **kw) for _ in range(n_traj)]
    emu = emus[0]
    t_cpu = time.time() - t0
    grads = {}
    step, vae = _hip_step_from(sds, res, kw, policy, device,
                               on_backward=lambda s_: grads.update({n: p.grad.detach().clone() for n, p in vae.named_parameters()}) if not grads else None)
    scales = step.calibrate_grad_scales(x.to(device))
    traj = []
    first = None
    for it in range(n_traj):
        got = step(x.to(device))
        if it == 0:
            first = _deviation(got, exact[0], grads)
        row = {"step": it}
        for k in ("perceptual_loss", "overall_vae_loss", "d_loss", "g_gan_loss"):
            if k in got and k in exact[it]:
                row[k + "_rel"] = _sig(_rel(got[k], exact[it][k]))
                row[k + "_rel_reference_gpu_arithmetic"] = _sig(_rel(emus[it][k], exact[it][k]))
                row[k] = round(float(exact[it][k]), 5)
        traj.append(row)
    events = step.poll_range_events()
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    del step, vae
    vq.ops.clear_caches()
    _empty_cache()
    # the same first step in the policies that are meant to MEET north_star's 1e-4 (their throughput: `parity_mode` on this line)
    conformant = {}
    for pol in TOLERANCE_POLICIES + ("ref3",):
        if pol == policy:
            continue
        g2 = {}
        step, vae = _hip_step_from(sds, res, kw, pol, device,
                                   on_backward=lambda s_: g2.update({n: p.grad.detach().clone() for n, p in vae.named_parameters()}) if not g2 else None)
        step.calibrate_grad_scales(x.to(device))       # (loss scales of binary16-range stacks: f16x3; nothing for fp32 storage)
        conformant[pol] = _deviation(step(x.to(device)), exact[0], g2)
        del step, vae, g2
        vq.ops.clear_caches()
        _empty_cache()
    # the oracle's OWN sensitivity: the same first step evaluated in float64 against its float32 evaluation — what "agreement with
    # the fp32 reference" can mean for the ill-conditioned quantities (the gradients behind ReLU / max-pool ties, the GAN term
    # behind the discriminator's sign-like first AdamW step)
    own64 = None
    try:
        w64 = M.train_step_ref(M.RefState(*sds, dtype=torch.float64), x.double(), **kw)
        own64 = _deviation({k: (v.float() if torch.is_tensor(v) else v) for k, v in w64.items() if k != "grads"}, exact[0],
                           {k: v.float() for k, v in w64["grads"].items()})
        del w64
    except Exception as exc:      # an auxiliary yardstick must never cost the parity object
        own64 = {"error": repr(exc)}
    out = {"vs": f"oracle/model_ref.py (CPU fp32), re-randomised weights (oracle/weights.py, SURVEY F11), batch 2, {res}x{res}, LPIPS eval "
                 f"mode, warm-up 0; oracle CPU time {t_cpu:.0f} s", "precision": policy,
           "first_step": first,
           "first_step_in_the_parity_modes": conformant,
           "float64_oracle_vs_float32_oracle_first_step": own64,
           "reference_gpu_arithmetic_first_step": _deviation(emu, exact[0], emu["grads"]),
           "yardstick": "reference_gpu_arithmetic_* = the same fp32 oracle steps recomputed in the reference's own CUDA arithmetic "
                        "(oracle.ops_ref.arith: TF32 conv operands in encoder / LPIPS / discriminator, bf16 autocast decoder)",
           "trajectory": traj,
           "fp16_loss_scales_log2": [{"region": r["region"], "grad_scale": round(math.log2(r["grad_scale"]), 1)} for r in scales if r.get("grad_scale", 0) > 0],
           "range_events": events}
    return out


def c5_leg(vq, ops, device, world, steps=6, warmup=2):
    """configs[4] (one GPU's share: VQ 16384 x 32, ch_mult 1,2,4,4,4, 512x512, batch 8, full loss) under its policy `ref_vq` on the line
    the driver runs: throughput, how many tokens a binary16 encoder would send to ANOTHER code than the fp32-class evaluation the
    lookup reads (both on the device: no CPU oracle in this leg — parity of the lookup itself: `python bench.py --workload c5`,
    tests/test_vq.py), and the nearest-code kernel alone against the fp32 vector peak."""
    cfg = {"ch": 128, "ch_mult": (1, 2, 4, 4, 4), "z": 32, "res": 512, "gan": True, "vq": (16384, 32)}
    B = 8
    st = build_step(vq, cfg, device, "ref_vq", B)
    gen = torch.Generator(device=device).manual_seed(4242)
    batches = [vq.vae_trainer.synthetic_batch(B, cfg["res"], device, gen) for _ in range(2)]
    calibrate(st, batches[0])
    e, out = timed_run(st, batches, steps, warmup, world, recalibrate=st.poll_range_events)     # (counters: timed steps only)
    ev5 = st.poll_range_events()
    row = {"optimizer_steps_dropped_in_timed_region": {"G": ev5["skipped_G"], "D": ev5["skipped_D"]},
           "workload": "configs[4] (one GPU's share): VQ 16384x32, vae_ch=128 ch_mult=1,2,4,4,4 f=16 z=32, 512x512, batch 8, LPIPS + "
                       "PatchDiscriminator(hinge) + GradNorm, full step incl. AdamW", "precision": "ref_vq",
           "value": round(steps * B * world / e, 3), "unit": "images/sec", "ms_per_step": round(e / steps * 1e3, 3), "steps": steps,
           "warmup": warmup, "final_loss": round(float(out["overall_vae_loss"]), 5)}
    enc, q = st.vae.encoder, st.quantizer
    with torch.no_grad():
        z16 = enc(batches[0])
        keep, enc.precision = enc.precision, enc.lookup_precision
        try:
            z_ex = enc(batches[0])
        finally:
            enc.precision = keep
        idx16, idx_ex = q(z16)[2], q(z_ex)[2]
        row["tokens"] = int(idx_ex.numel())
        row["tokens_with_another_code_under_a_binary16_encoder"] = int((idx16 != idx_ex).sum().item())
        row["codes_in_use"] = int(idx_ex.unique().numel())
        # vq_nearest_kernel alone: 2 n K D flops of fixed-order fp32 FMAs (bit-exact against oracle/vq_oracle.c)
        tokens = z_ex.permute(0, 2, 3, 1).reshape(-1, z_ex.shape[1]).contiguous().float()
        cb = q.embedding.weight.detach().contiguous().float()
        n, d = tokens.shape
        k = cb.shape[0]
        L = vq._lib.lib()
        ws = vq._lib.workspace(device, L.size("vq_vq_workspace", n, k))
        idx = torch.empty(n, dtype=torch.int64, device=device)
        zq, md = torch.empty_like(tokens), torch.empty(n, dtype=torch.float32, device=device)
        call = lambda: L.call("vq_vq_nearest_fwd", vq._lib.ptr(tokens), vq._lib.ptr(cb), n, k, d, vq._lib.ptr(idx), vq._lib.ptr(zq),
                              vq._lib.ptr(md), vq._lib.ptr(ws), ws.numel(), vq._lib.stream_of(tokens))
        for _ in range(3):
            call()
        if torch.device(device).type == "cuda":
            reps = 20
            e0, e1 = _event(), _event()
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            _sync()
            us = e0.elapsed_time(e1) * 1e3 / reps
            tf = 2.0 * n * k * d / (us * 1e-6) / 1e12
            row["vq_nearest"] = {"kernel": "vq_code_norms_kernel + vq_nearest_mfma_kernel<32> + vq_finalize_kernel (one lookup)", "tokens": n, "codes": k, "dim": d, "us_per_launch": round(us, 1),
                                 "TFLOP/s": round(tf, 2), "bound": "fp32 FMA (v_mfma_f32_32x32x2_f32: exact fp32, the oracle's chain order)", "peak": PEAK_FP32_VECTOR_TFLOPS,
                                 "frac": round(tf / PEAK_FP32_VECTOR_TFLOPS, 4), "timing": f"HIP events around {reps} back-to-back launches"}
            row["vq_nearest_us"], row["vq_nearest_frac_of_fp32_vector_peak"] = round(us, 1), round(tf / PEAK_FP32_VECTOR_TFLOPS, 4)
        assert torch.equal(idx, idx_ex.reshape(-1))      # (the timed launches computed the lookup the step used)
    del st, out, batches
    ops.clear_caches()
    _empty_cache()
    return row


def tolerance_summary(line, timed_policy):
    """-> top-level scalars naming the FASTEST policy on this line whose every `*_loss_rel` — constructor-initialised weights
    (`parity`) AND the re-randomised first step (`parity_randomized`) — is <= 1e-4, with its throughput on the same workload."""
    cands = {}
    def worst(*objs):
        vals = [v for o in objs if isinstance(o, dict) for k, v in o.items() if k.endswith("_loss_rel") and isinstance(v, float)]
        return max(vals) if vals else None
    pr = line.get("parity_randomized") or {}
    cands[timed_policy] = (line.get("value"), worst(line.get("parity"), pr.get("first_step")))
    for pol, row in (line.get("parity_mode") or {}).items():
        if isinstance(row, dict) and "value" in row:
            cands[pol] = (row["value"], worst(row.get("parity"), (pr.get("first_step_in_the_parity_modes") or {}).get(pol)))
    ok = {pol: v for pol, v in cands.items() if v[1] is not None and v[1] <= 1e-4}
    out = {"tolerance_bound": 1e-4,
           "worst_loss_rel_by_policy": {pol: v[1] for pol, v in cands.items()}}
    if ok:
        best = max(ok, key=lambda pol: ok[pol][0])
        out.update({"tolerance_policy": best, "tolerance_policy_images_per_sec": ok[best][0], "tolerance_policy_worst_loss_rel": ok[best][1],
                    "tolerance_policy_vs_timed_policy": round(ok[best][0] / max(line.get("value") or 1e-30, 1e-30), 4)})
    else:
        out["tolerance_policy"] = None
    return out


def parity_quantized(policy, cfg, res, device):
    """configs[4] (the VQ workload): ONE image through the full step — encoder, nearest-code lookup against the K x D codebook,
    straight-through decoder, LPIPS, discriminator, commitment / codebook loss — on re-randomised weights against the fp32 oracle
    (oracle/model_ref.py + oracle/vq_oracle.c, pinned by tests/test_vq_oracle_pin.py):
      * in the parity mode (fp32x3): the code indices must be IDENTICAL (integer work: bit-exact) and the losses agree to 1e-4;
      * at the timed policy: how many tokens pick another code (their latents differ by the policy's rounding, so near-ties flip)
        and what that does to the losses."""
    from oracle import model_ref as M
    from oracle import weights as W
    import vqgan_training_amd as vq
    import warnings
    torch.manual_seed(7)
    K, D = cfg["vq"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vae0 = vq.ae.VAE(res, 3, cfg["ch"], 3, list(cfg["ch_mult"]), 2, cfg["z"], False, False, False)
        lp0 = vq.utils.LPIPS(pretrained_path=None)
        disc0 = vq.utils.PatchDiscriminator() if cfg["gan"] else None
    sds = (W.randomize_state_dict(vae0.state_dict(), 1), W.randomize_state_dict(lp0.state_dict(), 2, relu_net=True),
           None if disc0 is None else W.randomize_state_dict(disc0.state_dict(), 4, relu_net=True))
    del vae0, lp0, disc0
    kw = dict(do_ganloss=cfg["gan"], disc_type="hinge", learning_rate_vae=1e-5, vae_ch=cfg["ch"], max_steps=1000, warmup_steps=0)
    x = W.image_batch(1, res, seed=13)
    # a codebook that the encoder's latents actually spread over: K rows drawn around the latents' own scale
    with torch.no_grad():
        z0 = M.encoder({k: v for k, v in sds[0].items()}, x)
    book = W.uniform_tensor((K, D), 77, -1.0, 1.0) * (2.0 * z0.std().item())
    del z0
    sd = dict(sds[0])
    sd[M.VQ_KEY] = book.clone()
    t0 = time.time()
    want = M.train_step_ref(M.RefState(sd, sds[1], sds[2]), x, **kw)
    t_cpu = time.time() - t0
    out = {"vs": f"oracle/model_ref.py + oracle/vq_oracle.c (CPU fp32), re-randomised weights, codebook {K} x {D}, batch 1, {res}x{res}, "
                 f"oracle CPU time {t_cpu:.0f} s", "tokens": int(want["indices"].numel()), "codes_used_by_the_oracle": len(set(want["indices"].flatten().tolist()))}
    rows = [("parity_mode", "fp32x6"), ("fp32x3", "fp32x3"), ("timed_policy", policy)] + ([("ref_policy", "ref")] if policy != "ref" else [])
    for name, pol in rows:
        step, vae = _hip_step_from(sds, res, kw, pol, device, codebook=book)
        if step.fp16_stacks():
            step.calibrate_grad_scales(x.to(device), rounds=int(_TEST_SHRINK.get("calibrate_rounds", 3)))
        got = step(x.to(device))
        idx = got["indices"].cpu()
        row = {"precision": pol, "indices_identical": bool(torch.equal(idx, want["indices"])),
               "tokens_with_another_code": int((idx != want["indices"]).sum())}
        for k in ("perceptual_loss", "overall_vae_loss", "vq_loss", "d_loss", "g_gan_loss"):
            if k in got and k in want:
                row[k + "_rel"] = _sig(_rel(got[k], want[k]))
        rec_g, rec_w = got["reconstructed"].float().cpu(), want["reconstructed"]
        row["recon_rel_l2"] = _sig(((rec_g - rec_w).norm() / rec_w.norm()).item())
        out[name] = row
        del step, vae, got
        vq.ops.clear_caches()
        _empty_cache()
    return out


def scales_after_run(step, batch):
    """The fp16 stacks after the timed steps, under the loss scales those steps actually used: what the kernels reported while they
    ran (range events: clipped / vanished binary16 stores, optimizer steps dropped on the device) and one monitored dry step
    (ops.monitor_gradients: a vq_absmax pass behind every gradient tensor) -> per stack the largest and the smallest non-zero
    per-tensor maximum in stored units."""
    from vqgan_training_amd import ops
    events = step.poll_range_events()
    stacks = step.fp16_stacks()
    if not stacks:
        return None
    step._dry = True
    t_state = torch.get_rng_state()
    try:
        with ops.monitor_gradients() as mon:
            step(batch)
        stats = mon.report()
    finally:
        step._dry = False
        torch.set_rng_state(t_state)
        if step.range_events is not None:
            step.range_events[:, 0:3] = 0
            step.range_events[:, 6:9] = 0
    rows = []
    for p in stacks:
        st = stats.get(id(p))
        ev = next((e for e in events["stacks"] if e["region"] == p.region), {})
        row = {"region": p.region, "grad_scale_log2": round(math.log2(p.grad_scale), 1), "saturated_waves_in_run": ev.get("saturated"),
               "flushed_waves_in_run": ev.get("flushed")}
        if st is not None and st["max"] > 0:
            row.update(max_stored_log2=round(math.log2(st["max"]), 1), min_nonzero_log2=round(math.log2(st["min"]), 1),
                       tensors=st["tensors"], all_zero_tensors=st["zero"],
                       saturated_tensors=int(st["max"] >= 65504.0))
        rows.append(row)
    return {"stacks": rows, "optimizer_steps_dropped": {"G": events["skipped_G"], "D": events["skipped_D"]}}


DUMP_BUDGET_BYTES = 64 * 10 ** 6


def dump_outputs(out, path, budget=DUMP_BUDGET_BYTES):
    """Every tensor of a step's output dictionary -> path/<name>.npy (float32; integer tensors float64), `budget` bytes at most in
    all: when the whole would be larger, every tensor above 1 MB is cut down to a fixed sample (elements at sorted indices drawn
    from numpy's default_rng(0), the same from run to run).  -> {name: [stored elements, elements]}"""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrs = {}
    for k in sorted(out):
        v = out[k]
        if not torch.is_tensor(v):
            continue
        v = v.detach().cpu()
        arrs[k] = v.to(torch.float32 if v.dtype.is_floating_point else torch.float64).contiguous().numpy()
    total = sum(a.nbytes for a in arrs.values())
    small = sum(a.nbytes for a in arrs.values() if a.nbytes <= 10 ** 6)
    keep = 1.0 if total <= budget else max(budget - small, 0) / max(total - small, 1)
    stored = {}
    for k, a in arrs.items():
        n = a.size
        if keep < 1.0 and a.nbytes > 10 ** 6:
            idx = np.sort(np.random.default_rng(0).integers(0, n, size=int(n * keep)))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, k + ".npy"), a)
        stored[k] = [int(a.size), int(n)]
    return stored


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _self_launch(args):
    """`python bench.py --gpus N` with no torchrun environment: start N ranks of this file, one per GPU (reference:
    launcher.sh:3-9 `torchrun --nproc_per_node=8 vae_trainer.py ...`), and hand its single JSON line through."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC only on this driver (RCCL needs it across processes)
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.call(cmd, env=env)


def build_step(vq, cfg, device, policy, B):
    import warnings
    torch.manual_seed(42)                                 # vae_trainer.py:374-378: same seed on every rank
    vae = vq.ae.VAE(cfg["res"], 3, cfg["ch"], 3, list(cfg["ch_mult"]), 2, cfg["z"], False, bool(cfg.get("hr")), bool(cfg.get("wavelet"))).to(device)
    disc = vq.utils.PatchDiscriminator().to(device) if cfg["gan"] else None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lpips = vq.utils.LPIPS().to(device)               # train mode: Dropout(0.5) live, as in the reference (F3)
    vq.vae_trainer.apply_precision_policy(policy, vae, lpips, disc)
    vq.distributed.broadcast_parameters(vae)
    if disc is not None:
        vq.distributed.broadcast_parameters(disc)
    quant = None
    if cfg["vq"]:
        quant = vq.quantizer.VectorQuantizer(cfg["vq"][0], cfg["vq"][1]).to(device)
        vq.distributed.broadcast_parameters(quant)
    extra = {}
    if cfg.get("hr"):          # the reference's HR-decoder runs: 512 x 512 batches, area-resized to 256 x 256 for the encoder (vae_trainer.py:531-533)
        extra = dict(decoder_also_perform_hr=True, enc_size=(cfg["res"], cfg["res"]), do_clamp=True, use_lecam=bool(cfg.get("lecam")))
    return vq.vae_trainer.VAETrainStep(vae, lpips, disc, do_ganloss=cfg["gan"], disc_type=cfg.get("disc_type", "hinge"),
                                       learning_rate_vae=1e-5, vae_ch=cfg["ch"], max_steps=1000, quantizer=quant, **extra)


_TEST_SHRINK = {}     # test device only ($VQ_BENCH_TEST_CFG): calibrate_rounds / hbm_steps / secondary_steps — emulator minutes, not behaviour


def calibrate(step, batch):
    """Loss scales of the fp16 stacks from measured gradient maxima (VAETrainStep.calibrate_grad_scales): part of set-up, like
    the reference's GradScaler-free fp32/TF32 path needs none — outside the timed region, no parameter is touched."""
    rep = step.calibrate_grad_scales(batch, rounds=int(_TEST_SHRINK.get("calibrate_rounds", 3)))
    return [{k: (round(math.log2(v), 1) if k in ("grad_scale", "max_stored", "min_nonzero_tensor_max_stored") and v > 0 else v)
             for k, v in r.items() if k != "previous"} for r in rep]


def timed_run(step, batches, steps, warmup, world, timer=None, recalibrate=None, trace=None, trace_key="d_loss"):
    """-> (seconds for exactly `steps` steps: barrier + synchronize on both sides, max over ranks; last step's outputs).
    `recalibrate` (set-up, outside the timed region): called after the warm-up steps — with a randomly initialised discriminator the
    first optimizer steps change the gradient magnitudes by an order of magnitude, and the fp16 loss scales the timed steps run under
    should be measured on the model they run on."""
    def barrier():
        if world > 1:
            dist.barrier()
        _sync()

    for i in range(warmup):
        step(batches[i % len(batches)])
    if recalibrate is not None:
        recalibrate()
    barrier()
    if timer is not None:
        timer.enabled = True
    t0 = time.perf_counter()
    last = None
    kept = []
    for i in range(steps):
        last = step(batches[i % len(batches)])
        if trace is not None and (trace_key in last or "overall_vae_loss" in last):
            kept.append(last.get(trace_key, last["overall_vae_loss"]))      # (device scalars: read after the timed region)
    barrier()
    elapsed = time.perf_counter() - t0
    if trace is not None:
        trace[:] = [round(float(v), 5) for v in kept]
    if timer is not None:
        timer.enabled = False
    if world > 1:
        t = torch.tensor([elapsed], device=batches[0].device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    return elapsed, last


def kernel_sources_sha():
    """sha256 over the kernel sources and the ABI header (sorted by path): what a PMC traffic file must have been measured on."""
    import hashlib
    h = hashlib.sha256()
    base = os.path.join(ROOT, "vqgan-training_amd", "csrc")
    files = sorted(glob.glob(os.path.join(base, "*.hip")) + glob.glob(os.path.join(base, "*.h")) + glob.glob(os.path.join(base, "*.cpp")) +
                   [os.path.join(ROOT, "include", "vqhip.h")])
    for f in files:
        h.update(os.path.relpath(f, ROOT).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def load_traffic(precision, workload="c3"):
    """HBM bytes per launch of the implicit-GEMM family from the committed PMC passes (tools/gpu_traffic.sh writes
    profiles/<round>_traffic.json; PMC counters need rocprofv3 around the process and cannot be read from inside).  Only a file
    measured on THESE kernel sources (its `sources_sha` == kernel_sources_sha()) and at this precision is used: a kernel change
    without a new PMC pass reports `traffic: null` with the reason, never stale bytes.  -> (info | None, source | None, reason | None)"""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")))
    if not files:
        return None, None, "no profiles/r*_traffic.json"
    want = kernel_sources_sha()
    reason = None
    for path in reversed(files):
        try:
            with open(path) as f:
                t = json.load(f)
        except Exception as exc:
            reason = f"{os.path.basename(path)}: {exc!r}"
            continue
        if t.get("sources_sha") != want:
            reason = reason or (f"{os.path.basename(path)} was measured on other kernel sources (sources_sha {t.get('sources_sha')} != {want}): "
                                "re-run tools/gpu_traffic.sh")
            continue
        if t.get("precision", precision) != precision:
            reason = reason or f"{os.path.basename(path)} holds precision {t.get('precision')}, not {precision}"
            continue
        if t.get("workload", "c3") != workload:      # (tools/gpu_traffic.sh profiles the default workload)
            reason = reason or f"{os.path.basename(path)} was measured on workload {t.get('workload', 'c3')}, not {workload}"
            continue
        return t, os.path.relpath(path, ROOT), None
    return None, None, reason


def build_roofline(timer, elapsed, args):
    """The `roofline` object from the conv launches `timer` recorded over `elapsed` seconds of args.steps steps."""
    summ = timer.summary()
    if "conv_igemm" not in summ:
        return None
    n, fl, sec = summ["conv_igemm"]
    ach = fl / sec / 1e12
    tinfo, traffic_src, traffic_why = load_traffic(args.precision, args.workload)
    traffic = tinfo.get("igemm_family_bytes_per_launch") if tinfo else None
    nb, alg_bytes = timer.conv_bytes("conv_igemm")
    roof = {"bound": "mfma", "kernel": "conv_igemm_* (implicit-GEMM conv fwd + dgrad)",
            "achieved": round(ach, 2), "peak": PEAK_MFMA_TFLOPS, "unit": "TFLOP/s",
            "frac": round(ach / PEAK_MFMA_TFLOPS, 4), "traffic": traffic, "traffic_source": traffic_src if tinfo else None,
            "traffic_null_reason": traffic_why,
            "algorithmic_bytes_per_launch": round(alg_bytes / max(nb, 1)),
            "traffic_vs_algorithmic": round(traffic / (alg_bytes / max(nb, 1)), 3) if traffic and nb else None,
            "launches": n, "avg_launch_ms": round(sec / n * 1e3, 4),
            "algorithmic_gflop_per_launch": round(fl / n / 1e9, 2),
            "share_of_step_time": round(sec / elapsed, 3),
            "timing": "two HIP events around every conv launch on the launch stream, INSIDE the timed region "
                      f"({(len(timer.records)) // max(args.steps, 1)} launches per step)",
            "_tinfo": tinfo}
    if "conv_wgrad" in summ:
        n2, fl2, sec2 = summ["conv_wgrad"]
        roof["wgrad"] = {"achieved": round(fl2 / sec2 / 1e12, 2), "launches": n2,
                         "frac": round(fl2 / sec2 / 1e12 / PEAK_MFMA_TFLOPS, 4),
                         "share_of_step_time": round(sec2 / elapsed, 3)}
    try:   # the sub-metric BASELINE.json's north_star names: the 3x3 conv GEMMs (>= 64 channels both sides), all three passes
        n3, fl3, sec3 = timer.family(lambda what, ci, co, k, st: k == 3 and ci >= 64 and co >= 64)
        if n3 and sec3 > 0:
            roof["conv3x3"] = {"achieved": round(fl3 / sec3 / 1e12, 2), "frac": round(fl3 / sec3 / 1e12 / PEAK_MFMA_TFLOPS, 4),
                               "launches": n3, "share_of_step_time": round(sec3 / elapsed, 3)}
    except Exception as exc:   # an auxiliary field must never cost the bench line
        roof["conv3x3"] = {"error": repr(exc)}
    return roof


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(_self_launch(args))
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    import vqgan_training_amd as vq
    from vqgan_training_amd import ops
    if TEST_DEVICE:                                       # test-only: host cores + emulator build + gloo (see TEST_DEVICE above)
        assert TEST_DEVICE == "emu", TEST_DEVICE
        device = torch.device("cpu")
        vq._lib._set_library_for_tests(vq._lib.VqLibrary(os.path.join(ROOT, "tests", "emu", "libvqhip_emu.so")))
        if world > 1:
            dist.init_process_group("gloo")
    else:
        assert torch.cuda.is_available(), "bench.py needs MI355X GPUs"
        device = torch.device(f"cuda:{local_rank}")
        torch.cuda.set_device(device)
        if world > 1:
            dist.init_process_group("nccl", device_id=device)
    if os.environ.get("VQ_BENCH_AB_LIB"):                 # tools/ A/B runs only (another BUILD of the library); never set by the driver
        vq._lib._set_library_for_tests(vq._lib.VqLibrary(os.environ["VQ_BENCH_AB_LIB"]))
    vq._lib.lib()                                         # fail loudly if libvqhip.so is missing
    # A/B knobs for kernel experiments (tools/): VqConvDesc.kernel_hint of every descriptor; never set by the driver
    ops._hint_conv, ops._hint_wgrad = int(os.environ.get("VQ_TILE", "0")), int(os.environ.get("VQ_WGTILE", "0"))
    cfg = {"ch": 128, "ch_mult": (1, 2, 4, 4), "z": 16, "res": 256, "gan": args.workload == "c3", "vq": None}
    if args.workload == "c5":   # configs[4]: VQ codebook 16384 x 32, 512x512, f=16 (ch=128 assumed), full loss
        cfg = {"ch": 128, "ch_mult": (1, 2, 4, 4, 4), "z": 32, "res": 512, "gan": True, "vq": (16384, 32)}
    if args.workload == "l1":   # launcher.sh:7-21 (options it does not pass: the CLI defaults 1,2,4,4 / z=16 / 256 / bce)
        cfg = {"ch": 64, "ch_mult": (1, 2, 4, 4), "z": 16, "res": 256, "gan": True, "vq": None, "hr": True, "disc_type": "bce"}
    if args.workload == "l2":   # scripts/launch_hdr.sh:9-30
        cfg = {"ch": 128, "ch_mult": (1, 2, 4, 4, 4), "z": 64, "res": 256, "gan": True, "vq": None, "hr": True, "wavelet": True, "lecam": True}
    if not args.batch:
        args.batch = {"c5": 8, "l1": 12, "l2": 4}.get(args.workload, 16)
    if TEST_DEVICE and os.environ.get("VQ_BENCH_TEST_CFG"):
        over = json.loads(os.environ["VQ_BENCH_TEST_CFG"])
        args.batch = int(over.pop("batch", args.batch))
        for k in ("calibrate_rounds", "hbm_steps", "secondary_steps"):
            if k in over:
                _TEST_SHRINK[k] = int(over.pop(k))
        cfg.update({k: (tuple(v) if isinstance(v, list) else v) for k, v in over.items()})
    B = args.batch

    step = build_step(vq, cfg, device, args.precision, B)
    timer = ConvTimer()
    ops.set_launch_hook(timer.launch)
    gen = torch.Generator(device=device).manual_seed(42 + rank)
    in_res = cfg["res"] * (2 if cfg.get("hr") else 1)        # HR-decoder runs are fed 2x the encoder's resolution (vae_trainer.py:530-533)
    batches = [vq.vae_trainer.synthetic_batch(B, in_res, device, gen) for _ in range(4)]   # resident in HBM
    scales = [] if args.no_calibrate else calibrate(step, batches[0])      # [] unless the policy has fp16 stacks
    step.event_factory = _event
    if world > 1 and args.full:
        step.comm_events = []
    recal = []
    # The discriminator learns to tell uniform noise from reconstructions within a few steps (random-init VGG trunk, lr 2e-4): after the
    # warm-up its hinge terms are exactly zero and its backward would stream zeros / flushed binary16 values through the timed region
    # (round 4: d_loss = 0.0, 5304 flushed waves).  Set-up, outside the timed region: D goes back to its initial parameters with fresh
    # AdamW state after the warm-up, so the timed steps are D's FIRST steps — live gradients, the range machinery on meaningful data.
    # With D learning from scratch the generator's GAN gradient grows by orders of magnitude inside the timed steps (g_gan 0.5 -> 14 in 20
    # steps): a loss scale measured on the first of them clips binary16 stores later, and the optimizers DROP such a step on the device
    # (20 timed + 21 serial + 2 instrumented steps: 8 dropped generator steps in this round's first closing run).  A dropped step is
    # skipped work, so — set-up as well — the timed steps are REHEARSED: from a snapshot of the whole training state (parameters, AdamW
    # moments, counters, random streams) run steps + 1 steps, lower the loss scale of every stack that reported a clipped gradient store
    # by 2^4, restore, repeat until a rehearsal is clean; the timed region then starts from the restored snapshot under those scales
    # and repeats the clean rehearsal (same state, same scales, deterministic kernels).  `optimizer_steps_dropped_in_timed_region` on the
    # line is what the timed steps themselves reported.  The serial and the instrumented pass below start from the same snapshot.
    disc_snap = step.optimizer_D.snapshot() if step.optimizer_D is not None else None
    d_trace = []
    state = {}
    rehearsal = {"attempts": 0, "lowered": []}

    def after_warmup():
        if disc_snap is not None:
            step.optimizer_D.restore(disc_snap)
        if not args.no_calibrate:
            recal.append(calibrate(step, batches[0]))
        step.poll_range_events()
        if not args.no_calibrate and step.fp16_stacks():
            state["snap"] = step.state_snapshot()
            for _ in range(6):
                rehearsal["attempts"] += 1
                r_trace = []
                for i in range(args.steps + 1):
                    out = step(batches[i % len(batches)])
                    r_trace.append(out.get("d_loss", out["overall_vae_loss"]))      # (device scalars: read after the rehearsal)
                state["rehearsed"] = [round(float(v), 5) for v in r_trace[:args.steps]]
                ev = step.poll_range_events()             # (one host sync per rehearsal; every rank sees the MAX over ranks)
                step.state_restore(state["snap"])
                bad = {e["region"] for e in ev["stacks"] if e["saturated"]}
                if not bad and not ev["skipped_G"] and not ev["skipped_D"]:
                    break
                for p in step.fp16_stacks():
                    if p.region in bad or not bad:
                        p.grad_scale = max(p.grad_scale * 2.0 ** -4, 2.0 ** -40)
                        rehearsal["lowered"].append({"region": p.region, "grad_scale_log2": round(math.log2(p.grad_scale), 1)})
            for r in (recal[0] if recal else []):         # the scales the timed steps run under
                p = next((q for q in step.fp16_stacks() if q.region == r.get("region")), None)
                if p is not None and "grad_scale" in r:
                    r["grad_scale"] = round(math.log2(p.grad_scale), 1)
        step.poll_range_events()                          # (counters: timed steps only)

    # The timed region carries NO per-launch instrumentation (round 6): two HIP events around each of the ~330 GEMM launches of a step,
    # on two streams, cost the step 2.9 % (60.2 vs 58.5 ms, same box, alternating: profiles/r6k_ab_timed_events.txt) — the rounds 1-5
    # lines were timed WITH them.  The per-kernel durations "as timed" (both streams live) come from an instrumented repeat of the
    # same steps from the same state snapshot right after; the serial pass (one stream) follows that.  VQ_BENCH_TIMED_EVENTS=1 (tools'
    # A/B only) puts the brackets back into the timed region.
    # (--no-serial-pass, the profiler stages' short form, skips both extra passes: its roofline then comes from brackets in the timed region)
    # A plain run (no --full) has neither the brackets nor the extra passes: `roofline` is null on its line.
    events_in_timed_region = os.environ.get("VQ_BENCH_TIMED_EVENTS", "0") == "1" or (args.full and args.no_serial_pass)
    if not events_in_timed_region:
        ops.set_launch_hook(None)
    elapsed, last = timed_run(step, batches, args.steps, args.warmup, world, timer if events_in_timed_region else None,
                              recalibrate=after_warmup, trace=d_trace)
    dumped = dump_outputs(last, args.dump_outputs) if args.dump_outputs and rank == 0 else None
    if args.full:
        ops.set_launch_hook(timer.launch)
    timed_events = step.poll_range_events()               # (after the closing barrier of the timed region)
    if "rehearsed" in state:                              # the timed steps repeated the clean rehearsal (same state, scales, kernels)?
        rehearsal["repeated_by_the_timed_steps"] = state["rehearsed"] == d_trace
    dropped_timed = {"G": timed_events["skipped_G"], "D": timed_events["skipped_D"]}
    if recal and recal[0]:
        scales = recal[0]                                 # the scales the timed steps ran under
    instr_elapsed = elapsed if events_in_timed_region else None
    if args.full and not events_in_timed_region and not args.no_serial_pass:
        # the instrumented repeat: same steps, same state, both streams live, every GEMM launch between two events
        timed_comm_events, step.comm_events = step.comm_events, None
        try:
            if "snap" in state:
                step.state_restore(state["snap"])
            instr_elapsed, _ = timed_run(step, batches, args.steps, 0 if "snap" in state else 1, world, timer)
        finally:
            step.comm_events = timed_comm_events
    serial_timer, serial_elapsed = None, None
    if args.full and not TEST_DEVICE and ops._wgrad_overlap and not args.no_serial_pass:
        # per-kernel durations need every kernel alone on the chip: the same steps once more on ONE stream (see `roofline.timing`)
        ops.set_wgrad_overlap(False)
        serial_timer = ConvTimer()
        ops.set_launch_hook(serial_timer.launch)
        timed_comm_events, step.comm_events = step.comm_events, None     # (`comm.exposed_ms` is about the timed region: not these steps)
        try:
            if "snap" in state:
                step.state_restore(state["snap"])         # literally the same steps: the state the timed region started from
            serial_elapsed, _ = timed_run(step, batches, args.steps, 0 if "snap" in state else 1, world, serial_timer)
        finally:
            ops.set_wgrad_overlap(True)
            ops.set_launch_hook(timer.launch)
            step.comm_events = timed_comm_events
    loss = float(last["overall_vae_loss"])
    assert loss == loss, "non-finite loss"
    comm = None
    if world > 1 and args.full:
        # `exposed`: what the compute stream waited for inside reducer.finish() over the timed steps (the warm-up's events
        # are dropped); `allreduce`: the same buckets reduced back to back with nothing to hide under.
        ev = step.comm_events[-2 * args.steps:] if cfg["gan"] else step.comm_events[-args.steps:]
        step.comm_events = None
        exposed = sum(s.elapsed_time(e) for s, e in ev) / args.steps
        bufs = [b for r in (step.reducer_G, step.reducer_D) if r is not None and r.enabled for (b, _) in r.buckets]
        _sync()
        t0 = time.perf_counter()
        for _ in range(3):
            hs = [dist.all_reduce(b, async_op=True) for b in bufs]
            for h in hs:
                h.wait()
            _sync()
        alone = (time.perf_counter() - t0) / 3
        for r in (step.reducer_G, step.reducer_D):        # the buffers were summed in place: clear them again
            if r is not None:
                for (b, _) in r.buckets:
                    b.zero_()
        nbytes = int(sum(b.numel() * 4 for b in bufs))
        comm = {"world_seen_by_rccl": dist.get_world_size(), "backend": dist.get_backend(), "buckets": len(bufs),
                "bytes_per_step": nbytes, "allreduce_ms": round(alone * 1e3, 3), "exposed_ms": round(exposed, 3),
                # SURVEY section 5's link model, to read the two measured fields against: a ring all-reduce moves 2 (N - 1) / N of the
                # buffer through every link direction (xGMI: ~76.8 GB/s per direction and link); exposed_ms should stay near the LAST
                # bucket's share of that (everything earlier flies under backward)
                "link_model": {"ring_allreduce_ms_expected": round(2.0 * (world - 1) / world * nbytes / 76.8e9 * 1e3, 3),
                               "last_bucket_ms_expected": round(2.0 * (world - 1) / world * (bufs[-1].numel() * 4 if bufs else 0) / 76.8e9 * 1e3, 3),
                               "link_GBps_per_direction_assumed": 76.8}}

    hbm = None
    if not args.no_secondary:                             # instrumented pass (every rank: the steps hold collectives): 2 steps
        timer.hbm = True                                  # with every HBM-bound call bracketed by events
        mark = len(timer.records)
        n_hbm = int(_TEST_SHRINK.get("hbm_steps", 2))
        overlap = ops._wgrad_overlap
        ops.set_wgrad_overlap(False)                      # (one stream: an HBM-bound call is timed alone on the chip)
        try:
            if "snap" in state:
                step.state_restore(state["snap"])
            for i in range(n_hbm):
                step(batches[i % len(batches)])
            _sync()
        finally:
            ops.set_wgrad_overlap(overlap)
        timer.hbm = False
        t2 = ConvTimer()
        t2.records = [r for r in timer.records[mark:] if r[0].startswith("hbm:")]
        hbm = t2.hbm_rows(n_hbm)
        timer.records = timer.records[:mark]
    fp16_after = None
    try:                                                  # (every rank: the dry step holds the same collectives as a real one)
        fp16_after = None if args.no_calibrate or not args.full else scales_after_run(step, batches[0])   # (PMC passes: exactly steps + warmup steps)
    except Exception as exc:   # an auxiliary object must never cost the bench line
        fp16_after = {"error": repr(exc)}
    if world > 1:
        dist.barrier()

    line = None
    if rank == 0:
        if args.conv_table:
            with open(args.conv_table, "w") as f:
                f.write((serial_timer or timer).table(args.steps) + "\n")
        roof = build_roofline(serial_timer or timer, serial_elapsed or instr_elapsed or elapsed, args)
        if roof is not None and serial_timer is not None:
            # the timed region runs the weight-gradient GEMMs on a second stream, UNDER the HBM-bound kernels of the backward chain
            # (ops._on_side_stream): a launch's event-bracketed duration there includes whatever shared the chip with it, so the
            # per-kernel fractions come from a serial pass of the same steps right after the timed region (one stream: every kernel
            # alone on the chip, as rocprofv3 --kernel-trace reports it under VQ_WGRAD_OVERLAP=0)
            co = build_roofline(timer, instr_elapsed, args) if (timer.records and instr_elapsed) else None
            roof["timing"] = ("two HIP events around every conv launch on the launch stream, in a SERIAL pass of the same "
                              f"{args.steps} steps right after the timed region (weight-gradient stream overlap off: "
                              f"{round(serial_elapsed / args.steps * 1e3, 3)} ms/step); `*_as_timed` / in_timed_region_with_overlap: the "
                              "same brackets in an instrumented repeat of the timed steps from the same state with both streams live"
                              + (f" ({round(instr_elapsed / args.steps * 1e3, 3)} ms/step with the brackets" if instr_elapsed else " (not run")
                              + f"; the timed region itself carries no per-launch events: {round(elapsed / args.steps * 1e3, 3)} ms/step)")
            roof["serial_ms_per_step"] = round(serial_elapsed / args.steps * 1e3, 3)
            if instr_elapsed:
                roof["instrumented_ms_per_step_with_overlap"] = round(instr_elapsed / args.steps * 1e3, 3)
            roof["in_timed_region_with_overlap"] = {
                k: (co[k] if not isinstance(co.get(k), dict) else {kk: co[k][kk] for kk in ("achieved", "frac") if kk in co[k]})
                for k in ("achieved", "frac", "wgrad", "conv3x3") if co and k in co}
        tinfo = roof.pop("_tinfo", None) if roof else None
        if roof:      # scalars beside the nested objects (a parser that keeps only top-level scalars of `roofline` still sees them)
            for k in ("conv3x3", "wgrad"):
                if isinstance(roof.get(k), dict) and "frac" in roof[k]:
                    roof[k + "_frac"] = roof[k]["frac"]
                ov = (roof.get("in_timed_region_with_overlap") or {}).get(k)
                if isinstance(ov, dict) and "frac" in ov:
                    roof[k + "_frac_as_timed"] = ov["frac"]
        summ = (serial_timer or timer).summary()
        ips = args.steps * B * world / elapsed
        line = {
            "metric": ("images/sec full train step (enc+VQ+dec+LPIPS+disc+bwd), 512x512 f=16" if cfg["vq"] else
                       f"images/sec full train step (area-resize+enc+HR-dec+LPIPS+disc+bwd), {in_res}x{in_res} batches, {cfg['res']}x{cfg['res']} encoder" if cfg.get("hr") else
                       "images/sec full train step (enc+dec+LPIPS+disc+bwd), 256x256 f=8"),
            "value": round(ips, 3), "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "full": args.full,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": DTYPE_NAMES[args.precision],
            "data": f"synthetic uniform [-1,1] {in_res}x{in_res} RGB resident in HBM; random-init VAE (seed 42); random-init VGG16 "
                    "weights for LPIPS / PatchDiscriminator (no network for ImageNet weights)",
            "config": {"workload": (f"the reference's launch line {'launcher.sh:7-21' if args.workload == 'l1' else 'scripts/launch_hdr.sh:9-30'}: vae_ch={cfg['ch']} ch_mult={','.join(map(str, cfg['ch_mult']))} z={cfg['z']}"
                                    f"{' wavelet' if cfg.get('wavelet') else ''}, HR decoder 256 -> 512, {cfg.get('disc_type', 'hinge')} GAN{' + lecam' if cfg.get('lecam') else ''}, do_clamp, full step incl. AdamW "
                                    "(augmentation draws off)" if cfg.get("hr") else
                                    "configs[4] (one GPU's share): VQ 16384x32, vae_ch=128 ch_mult=1,2,4,4,4 f=16 z=32, 512x512, LPIPS + PatchDiscriminator(hinge) + GradNorm, full step incl. AdamW"
                                    if cfg["vq"] else "configs[2]: vae_ch=128 ch_mult=1,2,4,4 f=8 z=16, 256x256, LPIPS + PatchDiscriminator(hinge) + GradNorm, full step incl. AdamW"
                                    if cfg["gan"] else
                                    "configs[1]: vae_ch=128 ch_mult=1,2,4,4 f=8 z=16, 256x256, LPIPS only, full step incl. AdamW"),
                       "per_gpu_batch": B, "global_batch": B * world, "parallelism": f"dp{world}", "precision": args.precision,
                       "precision_policy": vq.vae_trainer.PRECISION_POLICIES[args.precision], "final_loss": round(loss, 5), "final_losses": {k: round(float(last[k]), 5) for k in ("perceptual_loss", "vae_loss", "d_loss", "g_gan_loss", "vq_loss") if k in last},
                       "fp16_loss_scales_log2": scales, "fp16_after_run": fp16_after,
                       "disc_reset_after_warmup": disc_snap is not None, ("d_loss_by_timed_step" if cfg["gan"] else "loss_by_timed_step"): d_trace,
                       "loss_scale_rehearsal": (dict(rehearsal, steps=args.steps + 1, note="set-up, outside the timed region: the timed steps "
                                                     "rehearsed from a snapshot of the training state until no gradient store clips; see bench.py main()")
                                                if rehearsal["attempts"] else None),
                       "range_events_in_timed_region": timed_events["stacks"],
                       "peak_hbm_allocated_GB": (round(torch.cuda.max_memory_allocated(device) / 1e9, 2) if device.type == "cuda" else None)},
            "roofline": roof,
            # optimizer steps the device-side range check dropped INSIDE the timed region (a clipped binary16 gradient store): must be 0
            "optimizer_steps_dropped_in_timed_region": dropped_timed,
        }
        if hbm is not None:
            fam = (tinfo or {}).get("families") if "conv_igemm" in summ else None
            for row in hbm or []:                         # PMC bytes of the family's kernels per step / its algorithmic bytes
                f = (fam or {}).get(row["kernel"])
                if f and row["algorithmic_MB_per_step"] > 0:
                    row["hbm_MB_per_step"] = round(f["bytes_per_step"] / 1e6, 1)
                    row["bytes_vs_algorithmic"] = round(f["bytes_per_step"] / 1e6 / row["algorithmic_MB_per_step"], 2)
            seen = {row["kernel"] for row in hbm or []}
            for k, f in sorted((fam or {}).items()):      # families without a call of their own (the split-K reduction runs inside
                if k not in seen:                         # vq_conv2d_wgrad): PMC bytes only, their time is in profiles/*kernel_stats*
                    hbm.append({"kernel": k, "calls_per_step": f["launches_per_step"], "hbm_MB_per_step": round(f["bytes_per_step"] / 1e6, 1),
                                "note": "no call of its own on the host side: bytes from the PMC passes, time in the rocprofv3 kernel stats"})
            line["hbm"] = hbm
        if comm is not None:
            line["comm"] = comm
        if dumped is not None:
            line["dumped_outputs"] = {"dir": args.dump_outputs, "elements_stored_of": dumped}

    # ---- secondary legs on the same workload (fresh modules each; the primary step is released first):
    #   bf16_mode    the all-bf16 throughput mode
    #   parity_mode  what north_star's 1e-4 tolerance COSTS: the policies that meet it against the CPU fp32 oracle (fp32x6: every
    #                logged loss at the headline model, tests/test_model.py::test_headline_model_step...; fp32x3: everything but
    #                the GAN term behind the discriminator's first AdamW step) and ref3 (fp32-class outside the bf16 decoder)
    #   ref_policy   c5 only: the plain `ref` policy (binary16 encoder) whose rounding lets ~0.5 % of the tokens pick another code
    if not args.no_secondary:
        ops.set_launch_hook(None)
        del step, last
        ops.clear_caches()
        _empty_cache()
        shrink = "secondary_steps" in _TEST_SHRINK

        def leg(policy, n, w):
            st = build_step(vq, cfg, device, policy, B)
            if st.fp16_stacks() and not args.no_calibrate:
                calibrate(st, batches[0])
            st.poll_range_events()
            e, out = timed_run(st, batches, n, w, world, recalibrate=st.poll_range_events)    # (counters: timed steps only)
            ev = st.poll_range_events()
            row = {"value": round(n * B * world / e, 3), "unit": "images/sec", "ms_per_step": round(e / n * 1e3, 3), "steps": n, "warmup": w,
                   "dtype": DTYPE_NAMES[policy], "final_loss": round(float(out["overall_vae_loss"]), 5),
                   "optimizer_steps_dropped_in_timed_region": {"G": ev["skipped_G"], "D": ev["skipped_D"]}}
            del st, out
            ops.clear_caches()
            _empty_cache()
            return row

        if args.precision != "bf16":
            n2 = int(_TEST_SHRINK.get("secondary_steps", max(3, args.steps // 2)))
            row = leg("bf16", n2, 1 if shrink else 2)
            if rank == 0:
                row["note"] = "every module on bf16 operands: narrower than the reference's own arithmetic outside the decoder"
                line["bf16_mode"] = row
        if cfg["vq"] and args.precision != "ref":
            n2 = int(_TEST_SHRINK.get("secondary_steps", max(3, args.steps // 2)))
            row = leg("ref", n2, 1 if shrink else 2)
            if rank == 0:
                row["note"] = "binary16 encoder in front of the code lookup: see parity.ref_policy.tokens_with_another_code"
                line["ref_policy"] = row
        if not cfg["vq"] and not shrink:
            pm = {}
            for pol in TOLERANCE_POLICIES + ("ref3",):
                if pol != args.precision:
                    # f16x3 is the tolerance-grade policy the line is judged on: as many steps as the bf16 leg; the generic-kernel splits fewer
                    n_pm = max(3, args.steps // 2) if pol == "f16x3" else max(1, min(3, args.parity_mode_steps) if pol == "fp32x6" else args.parity_mode_steps)
                    pm[pol] = leg(pol, n_pm, 2 if pol == "f16x3" else 1)
            if rank == 0:
                pm["note"] = ("throughput of the policies that meet north_star's 1e-4 against the CPU fp32 oracle — f16x3 (two binary16 pieces "
                              "per value, three MFMAs per product, on the TUNED kernels) and fp32x6 (generic kernel): every logged loss at "
                              "this model, tests/test_model.py::test_headline_model_step_matches_oracle_in_the_parity_mode; fp32x3: all but "
                              "the GAN term behind the discriminator's first AdamW step — and of ref3; same workload, each leg's `steps`")
                line["parity_mode"] = pm
        if args.workload == "c3" and not shrink and not args.no_c5_leg and not TEST_DEVICE and world == 1:      # (N = 1 only, like the parity legs)
            try:
                row = c5_leg(vq, ops, device, world)
                if rank == 0:
                    line["c5"] = row
            except Exception as exc:       # a secondary leg must never cost the bench line
                if rank == 0:
                    line["c5"] = {"error": repr(exc)}

    if rank == 0:
        if world == 1 and not args.no_cpu_baseline and not cfg["vq"] and not cfg.get("hr"):
            cpu_line, ref = cpu_baseline(args, cfg)
            line["cpu_baseline"] = cpu_line
            try:
                line["parity"] = parity_vs_oracle(args.precision, ref, device)
                if not args.no_secondary and args.precision != "bf16":
                    line["bf16_mode"]["parity"] = parity_vs_oracle("bf16", ref, device)
                if not args.no_secondary and "parity_mode" in line:
                    for pol in TOLERANCE_POLICIES + ("ref3",):
                        if pol in line["parity_mode"]:
                            line["parity_mode"][pol]["parity"] = parity_vs_oracle(pol, ref, device)
            except Exception as exc:   # never lose the bench line to the checker
                line["parity"] = {"error": repr(exc)}
            try:
                line["parity_randomized"] = parity_randomized(args.precision, cfg, args.cpu_baseline_res, device, n_traj=args.parity_steps)
            except Exception as exc:
                line["parity_randomized"] = {"error": repr(exc)}
            try:      # top-level scalars: the cheapest policy whose EVERY logged loss is within 1e-4 of the CPU fp32 oracle on this line
                ts = tolerance_summary(line, args.precision)
                line.update(ts)
                # ... and INSIDE `config` (the key a reader of the bare contract keeps): the headline is never read without the deviation
                # of the arithmetic it was timed in, nor without the throughput of the arithmetic that meets the 1e-4 bar
                line["config"]["parity_of_the_timed_policy"] = {
                    "policy": args.precision, "worst_loss_rel_vs_cpu_fp32_oracle": (ts.get("worst_loss_rel_by_policy") or {}).get(args.precision),
                    "bound": ts.get("tolerance_bound"), "tolerance_policy": ts.get("tolerance_policy"),
                    "tolerance_policy_images_per_sec": ts.get("tolerance_policy_images_per_sec"),
                    "tolerance_policy_worst_loss_rel": ts.get("tolerance_policy_worst_loss_rel")}
            except Exception as exc:
                line["tolerance_policy_error"] = repr(exc)
            if isinstance(line.get("c5"), dict) and "value" in line["c5"]:
                line["config"]["configs4_share_images_per_sec"] = line["c5"]["value"]
        if world == 1 and not args.no_cpu_baseline and cfg["vq"]:
            try:
                line["parity"] = parity_quantized(args.precision, cfg, cfg["res"] if not TEST_DEVICE else args.cpu_baseline_res, device)
            except Exception as exc:
                line["parity"] = {"error": repr(exc)}
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
