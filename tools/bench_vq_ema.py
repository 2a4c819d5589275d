"""EMA codebook at configs[4]'s per-GPU size (8192 tokens x 16384 codes x 32 dims).
(a) the three kernels alone: vq_vq_ema_accumulate (2 MB of 64-bit integer atomics + 64 KB of counts), vq_vq_ema_update, and
    vq_vq_ema_reseed (both phases, every code: the initialisation-from-data case);
(b) the whole configs[4] train step with VectorQuantizer(ema=True) against ema=False (the gradient-trained codebook: scatter-add,
    AdamW share, bucket traffic), same process, alternating, three repetitions each; the spread of the ema=False repetitions is the
    noise margin.
usage: python tools/bench_vq_ema.py [--out profiles/vq_ema_c5.txt] [--steps 8] [--warmup 2] [--reps 3] [--kernels-only]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import vqgan_training_amd as vq  # noqa: E402
from vqgan_training_amd._lib import VQ_F32, lib, ptr, stream_of  # noqa: E402


def time_us(call, reps=50, warm=3):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        call()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def kernels(dev, n=8192, K=16384, D=32):
    L = lib()
    g = torch.Generator(device=dev).manual_seed(1)
    tok = torch.randn(n, D, device=dev, generator=g)
    rows = []
    for name, idx in (("uniform codes", torch.randint(0, K, (n,), device=dev, generator=g)),
                      ("skewed codes (a third of the tokens on one code)", (torch.rand(n, device=dev, generator=g) ** 3 * K).long().clamp(0, K - 1))):
        ws = torch.zeros(L.size("vq_vq_ema_workspace", K, D), dtype=torch.uint8, device=dev)
        amax = torch.zeros(1, device=dev)
        L.call("vq_absmax", ptr(tok), tok.numel(), VQ_F32, ptr(amax), stream_of(tok))
        N, m, cb = torch.ones(K, device=dev), torch.randn(K, D, device=dev, generator=g), torch.zeros(K, D, device=dev)
        usage, cand = torch.zeros(2, device=dev), torch.zeros(K, D, device=dev)
        s = stream_of(tok)
        acc = lambda: L.call("vq_vq_ema_accumulate", ptr(tok), ptr(idx), n, n, K, D, ptr(amax), ptr(ws), ws.numel(), s)
        upd = lambda: L.call("vq_vq_ema_update", ptr(ws), ws.numel(), n, ptr(amax), K, D, 0.99, 1e-5, ptr(N), ptr(m), ptr(cb), ptr(usage), s)
        rs = lambda ph: L.call("vq_vq_ema_reseed", ph, ptr(N), float("inf"), 0, 0, ptr(tok), n, 0, n, K, D, ptr(cand), ptr(m), ptr(cb), s)
        t_acc = time_us(acc)
        atomic_bytes = 8.0 * n * (D + 1)
        rows.append(f"{name}: vq_vq_ema_accumulate (memset of {8 * K * (D + 1) / 1e6:.2f} MB + one pass) {t_acc:.1f} us = "
                    f"{atomic_bytes / t_acc / 1e6:.3f} TB/s of 64-bit integer atomics ({atomic_bytes / 1e6:.2f} MB added)")
        rows.append(f"{name}: vq_vq_ema_update (sizes + apply, {K} x {D}) {time_us(upd):.1f} us")
        rows.append(f"{name}: vq_vq_ema_reseed pick {time_us(lambda: rs(0)):.1f} us, install {time_us(lambda: rs(1)):.1f} us (every code)")
    return rows


def build_step(cfg, dev, ema):
    """bench.build_step's configs[4] step (policy ref_vq), with the quantizer of either kind."""
    import warnings
    torch.manual_seed(42)
    vae = vq.ae.VAE(cfg["res"], 3, cfg["ch"], 3, list(cfg["ch_mult"]), 2, cfg["z"], False, False, False).to(dev)
    disc = vq.utils.PatchDiscriminator().to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lpips = vq.utils.LPIPS().to(dev)
    vq.vae_trainer.apply_precision_policy("ref_vq", vae, lpips, disc)
    kw = dict(ema=True, init_from_data=True, reseed_below=0.05, reseed_every=100) if ema else {}
    quant = vq.quantizer.VectorQuantizer(cfg["vq"][0], cfg["vq"][1], **kw).to(dev)
    return vq.vae_trainer.VAETrainStep(vae, lpips, disc, do_ganloss=True, disc_type="hinge", learning_rate_vae=1e-5, vae_ch=cfg["ch"],
                                       max_steps=1000, quantizer=quant)


def whole_step(dev, steps, warmup, reps):
    import bench
    from vqgan_training_amd import ops
    cfg = {"ch": 128, "ch_mult": (1, 2, 4, 4, 4), "z": 32, "res": 512, "gan": True, "vq": (16384, 32)}
    B = 8
    gen = torch.Generator(device=dev).manual_seed(4242)
    batches = [vq.vae_trainer.synthetic_batch(B, cfg["res"], dev, gen) for _ in range(2)]
    ms = {False: [], True: []}
    usage = None
    for rep in range(reps):
        for ema in (False, True):
            st = build_step(cfg, dev, ema)
            bench.calibrate(st, batches[0])
            e, out = bench.timed_run(st, batches, steps, warmup, 1, recalibrate=st.poll_range_events)
            ms[ema].append(e / steps * 1e3)
            if ema:
                usage = (float(out["vq_perplexity"]), float(out["vq_codes_used"]))
            del st, out
            ops.clear_caches()
            torch.cuda.empty_cache()
    p, e = ms[False], ms[True]
    spread = max(p) - min(p)
    med = lambda v: sorted(v)[len(v) // 2]
    rows = [f"configs[4] step, batch {B}, policy ref_vq, {steps} timed steps after {warmup} warm-up steps, {reps} repetitions each, alternating:",
            "  ema=False ms/step: " + ", ".join(f"{v:.2f}" for v in p) + f"   (median {med(p):.2f}, spread {spread:.2f})",
            "  ema=True  ms/step: " + ", ".join(f"{v:.2f}" for v in e) + f"   (median {med(e):.2f})",
            f"  median difference ema=True - ema=False: {med(e) - med(p):+.2f} ms/step ({(med(e) / med(p) - 1) * 100:+.2f} %); noise margin "
            f"(spread of ema=False): {spread:.2f} ms -> " + ("within the noise margin or faster" if med(e) - med(p) <= spread else "SLOWER beyond the noise margin"),
            f"  last EMA step: perplexity {usage[0]:.1f}, codes used {usage[1]:.0f} of 16384 (8192 tokens; random-weight encoder on noise images)"]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vq_ema_c5.txt"))
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = [f"EMA codebook on {torch.cuda.get_device_name(0)} (tools/bench_vq_ema.py); HIP events around 50 back-to-back launches", "(a) kernels"]
    rows += ["  " + r for r in kernels(dev)]
    if not a.kernels_only:
        rows.append("(b) whole step")
        rows += whole_step(dev, a.steps, a.warmup, a.reps)
    text = "\n".join(rows) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
