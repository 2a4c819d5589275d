"""vq_adamw_multi alone, with and without the EMA shadow (VqAdamTensor::ema), on flat buffers of the headline generator's parameter
count (BASELINE.json configs[2]: VAE ch 128, ch_mult 1,2,4,4, z 16 — the count is taken from the model).
Per launch: HIP events around every single launch after a warm-up, the median of `--launches` of them; `--reps` repetitions of the
whole measurement, alternating the variants, give the run-to-run spread.  The byte model is 28 B/param without a shadow and 36 with
one (ratio 1.286); the separate pass the fused form replaces, `ema.lerp_(p, 1 - d)` (12 B/param and a launch of its own), is timed
on the same buffers.
usage: python tools/adamw_ema_ab.py [--out profiles/pr_weight_ema_adamw_tool.txt] [--launches 200] [--reps 5]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import vqgan_training_amd as vq  # noqa: E402
from vqgan_training_amd._lib import VqAdamTensor, lib, ptr, stream_of  # noqa: E402

CHUNK = 65536


def generator_numel():
    vae = vq.ae.VAE(256, 3, 128, 3, [1, 2, 4, 4], 2, 16, False, False, False)
    return sum(p.numel() for p in vae.parameters())


def median_us(call, launches, warm=10):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for s, e in evs:
        s.record()
        call()
        e.record()
    torch.cuda.synchronize()
    t = sorted(s.elapsed_time(e) * 1e3 for s, e in evs)
    return t[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pr_weight_ema_adamw_tool.txt"))
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = generator_numel()
    g = torch.Generator(device=dev).manual_seed(1)
    p, grad, m, e = (torch.randn(n, device=dev, generator=g) * 0.05 for _ in range(4))
    v = torch.rand(n, device=dev, generator=g) * 1e-3
    d = torch.full((1,), 0.999, device=dev)
    chunks = (n + CHUNK - 1) // CHUNK
    offs = torch.tensor([0, chunks], dtype=torch.int64, device=dev)

    def table(shadow):
        ent = VqAdamTensor(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, e.data_ptr() if shadow else None,
                           d.data_ptr() if shadow else None)
        return torch.frombuffer(bytearray(bytes(memoryview(ent))), dtype=torch.uint8).to(dev)
    tabs = {False: table(False), True: table(True)}
    L, s = lib(), stream_of(p)

    def adamw(shadow):
        return lambda: L.call("vq_adamw_multi", ptr(tabs[shadow]), ptr(offs), 1, chunks, CHUNK, 1e-5, 1e-3, 0.9, 0.95, 1e-8, 0.5, 0.5,
                              1.0, None, 0, 1, s)
    lerp = lambda: e.lerp_(p, 0.001)            # noqa: E731
    plain, fused, sep = [], [], []
    for _ in range(a.reps):
        plain.append(median_us(adamw(False), a.launches))
        fused.append(median_us(adamw(True), a.launches))
        sep.append(median_us(lerp, a.launches))
    med = lambda t: sorted(t)[len(t) // 2]      # noqa: E731
    fmt = lambda t: ", ".join(f"{x:.1f}" for x in t)   # noqa: E731
    mp, mf, ms = med(plain), med(fused), med(sep)
    ratios = sorted(f / q for f, q in zip(fused, plain))
    rows = [f"vq_adamw_multi on {torch.cuda.get_device_name(0)} (tools/adamw_ema_ab.py): {n} parameters (headline generator), one table "
            f"entry, chunk {CHUNK}; median of {a.launches} single launches between HIP events, {a.reps} repetitions, alternating",
            f"  no shadow  (28 B/param): us {fmt(plain)}   median {mp:.1f} us = {28.0 * n / mp / 1e6:.3f} TB/s",
            f"  shadow     (36 B/param): us {fmt(fused)}   median {mf:.1f} us = {36.0 * n / mf / 1e6:.3f} TB/s",
            f"  ratio shadow / no shadow per repetition: {', '.join(f'{r:.3f}' for r in ratios)}   (byte model 36 / 28 = 1.286)",
            f"  separate pass ema.lerp_(p, 1 - d) (12 B/param): us {fmt(sep)}   median {ms:.1f} us = {12.0 * n / ms / 1e6:.3f} TB/s",
            f"  fused {mf:.1f} us against no shadow + separate pass {mp + ms:.1f} us: " +
            ("the fused form is faster" if mf < mp + ms else "the fused form is NOT faster")]
    text = "\n".join(rows) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
