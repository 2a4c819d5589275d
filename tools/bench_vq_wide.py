"""Nearest-code search (vq_vq_nearest_fwd: code norms + search + split merge, one lookup) at the wide code dimensions:
8192 tokens x 16384 codes x {32, 128, 256} and 8192 x 1024 x 256, beside two yardsticks — the fit of the narrow kernel at
8192 x 16384 (36 us + 5.3 us * D / 2) and torch's fp32 `z @ codebook.T` of the same shape (the tool may call it; the
product never does).  HIP events around batches of back-to-back launches after a warm-up; a row is the median over the batches, with
their range.  The D = 32 row is the no-regression check of the narrow kernel: `--compare-lib` times the same row through a second
library (the parent commit's), the two alternating batch by batch in one process.
usage: python tools/bench_vq_wide.py [--out profiles/vq_wide_dims.txt] [--batches 9] [--launches 20] [--compare-lib PATH]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import vqgan_training_amd as vq  # noqa: E402
from vqgan_training_amd._lib import ptr, stream_of  # noqa: E402

PEAK_TF = 157.3                                   # fp32 matrix peak of the MI355X
SHAPES = [(8192, 16384, 32), (8192, 16384, 128), (8192, 16384, 256), (8192, 1024, 256)]


def batch_us(call, launches):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(launches):
        call()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / launches


def measure(calls, batches, launches, warm=5):
    """calls: {name: callable}; the callables alternate batch by batch, in rotating order -> {name: (median, min, max)} in us per launch."""
    for c in calls.values():
        for _ in range(warm):
            c()
    torch.cuda.synchronize()
    got = {k: [] for k in calls}
    names = list(calls)
    for b in range(batches):
        for k in names[b % len(names):] + names[:b % len(names)]:      # rotate: nobody always runs behind the same neighbour
            got[k].append(batch_us(calls[k], launches))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def lookup_call(L, z, cb):
    n, d = z.shape
    k = cb.shape[0]
    ws = torch.empty(L.size("vq_vq_workspace", n, k), dtype=torch.uint8, device=z.device)
    idx = torch.empty(n, dtype=torch.int64, device=z.device)
    zq, md = torch.empty_like(z), torch.empty(n, device=z.device)
    keep = (ws, idx, zq, md)
    return lambda: L.call("vq_vq_nearest_fwd", ptr(z), ptr(cb), n, k, d, ptr(idx), ptr(zq), ptr(md), ptr(ws), ws.numel(), stream_of(z)), keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vq_wide_dims.txt"))
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--compare-lib", default=None, help="a second libvqhip.so (the parent commit's) for the D = 32 row")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L = vq._lib.lib()
    other = vq._lib.VqLibrary(a.compare_lib) if a.compare_lib else None
    torch.backends.cuda.matmul.allow_tf32 = False
    rows = [f"vq_vq_nearest_fwd at wide code dimensions on {torch.cuda.get_device_name(0)} (tools/bench_vq_wide.py): HIP events around "
            f"{a.launches} back-to-back launches, median [min .. max] of {a.batches} such batches after 5 warm-up launches; "
            f"TF = 2 n K D / time, against the {PEAK_TF} TF fp32-matrix peak",
            "fit = 36 us + 5.3 us * D / 2, the narrow kernel's line at 8192 x 16384 (DESIGN.md §3); torch = fp32 z @ codebook.T alone "
            "(no norms, no argmin), same shapes, same process"]
    g = torch.Generator(device=dev).manual_seed(1)
    for n, k, d in SHAPES:
        z = torch.randn(n, d, device=dev, generator=g)
        cb = torch.randn(k, d, device=dev, generator=g) * 0.5
        ours, keep = lookup_call(L, z, cb)
        out = torch.empty(n, k, device=dev)
        calls = {"lookup": ours, "torch": lambda: torch.matmul(z, cb.t(), out=out)}
        if other is not None and d == 32:
            calls["other"], keep2 = lookup_call(other, z, cb)
        r = measure(calls, a.batches, a.launches)
        flop = 2.0 * n * k * d
        us, lo, hi = r["lookup"]
        tus = r["torch"][0]
        line = (f"{n} x {k} x {d}: lookup {us:.1f} us [{lo:.1f} .. {hi:.1f}] = {flop / us / 1e6:.1f} TF = {flop / us / 1e6 / PEAK_TF:.3f} of peak"
                f" | torch matmul {tus:.1f} us = {flop / tus / 1e6:.1f} TF (lookup / torch = {us / tus:.2f})")
        if k == 16384:
            fit = 36.0 + 5.3 * d / 2
            line += f" | fit {fit:.0f} us (lookup / fit = {us / fit:.2f})"
        rows.append(line)
        if "other" in r:
            ous, olo, ohi = r["other"]
            rows.append(f"    the same row through {os.path.basename(a.compare_lib)}: {ous:.1f} us [{olo:.1f} .. {ohi:.1f}]; this library / that one = "
                        f"{us / ous:.4f} (no-regression box: within 3 %: {'yes' if abs(us / ous - 1) <= 0.03 else 'NO'})")
        # the timed launches' answer against a torch fp32 argmin (near-ties may differ: the bit-exact check is tests/test_vq_wide.py)
        ref = ((z * z).sum(1, keepdim=True) - 2 * z @ cb.t() + (cb * cb).sum(1)).argmin(1)
        rows.append(f"    indices equal to a torch fp32 argmin on {(keep[1] == ref).float().mean().item() * 100:.2f} % of the tokens")
    text = "\n".join(rows) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
