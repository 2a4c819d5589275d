"""Per-kernel parity: HIP path (through the C ABI) vs the CPU oracle (oracle/ops_ref.py).

Each test runs on the host emulator (`-m "not gpu"`: same kernel sources, fibers) and on a real
MI355X (`-m gpu`).  Tolerances are relative to max|reference|:
  fp32x3 (fp32 storage, 3-term bf16 split, fp32 accumulate)  : 5e-5   ("fp32 tolerance")
  bf16 / fp32 (operands rounded to bf16, fp32 accumulate)     : 2e-2
  fp16 (binary16 storage + operands = TF32's mantissa, scaled weights / gradients, fp32 accumulate) : 2.5e-3
"""
import contextlib
import os
import zlib

import pytest
import torch
import torch.nn.functional as F

import vqgan_training_amd as vq
from vqgan_training_amd import ops
from oracle import ops_ref
from oracle import weights as W

# >= 2x the worst error over 200 seeds x 6 cancellation-prone / ragged / tile-kernel cases per precision on the emulator and on the
# MI355X (tools/tol_sweep.py -> profiles/r4_tol_sweep_{emu,gpu}.txt; the two agree to 3 digits): fp32x6 3.7e-6, fp32x3 1.8e-5, fp32 6.8e-3,
# bf16 8.8e-3, fp16 1.02e-3 — margins x2.3 ... x2.9
TOL = {"fp32x3": 5e-5, "fp32x6": 1e-5, "fp32": 2e-2, "bf16": 2e-2, "fp16": 2.5e-3, "f16x3": 1e-5}


def leaf(t, dev="cpu"):
    return t.detach().clone().to(dev).requires_grad_()


def rel_err(a, b, floor=0.0):
    """max|a - b| / max(max|b|, floor).  `floor` is the NATURAL scale of a reduction output (`reduction_scale`): a bias / dgamma /
    dbeta gradient is a sum of n terms whose storage rounding is ~eps * sqrt(n) * rms(term) whatever the sum comes to, so on an
    output of 1-3 elements a draw whose sums happen to cancel must not inflate the ratio (round 3: the driver's GPU suite went red on
    a 3-element bias gradient of -0.80, -0.34, 1.87 where sigma = 16)."""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).abs().max() / max(b.abs().max().item(), floor, 1e-12)).item()


def reduction_scale(terms, n):
    """sqrt(n) * rms(terms): one standard deviation of a sum of n of them."""
    return (float(n) ** 0.5) * terms.detach().float().pow(2).mean().sqrt().item()


def case_seed(*case):
    """A seed that is the same in every process and on every box (hash() of a tuple holding a str depends on PYTHONHASHSEED)."""
    return zlib.crc32(repr(case).encode()) & 0x7FFFFFFF


CONV_CASES = [
    # prec, N, H, W, Cin, Cout, R, stride, pad, up, relu, out_hw
    ("bf16", 1, 8, 8, 16, 32, 3, 1, 1, 1, False, None),
    ("fp32x3", 1, 8, 8, 16, 32, 3, 1, 1, 1, False, None),
    ("fp32", 2, 6, 10, 24, 136, 3, 1, 1, 1, False, None),        # ragged M, two cout tiles
    ("fp32x3", 1, 8, 8, 8, 24, 3, 2, 0, 1, False, (4, 4)),       # Downsample ae.py:150-154
    ("fp32x3", 1, 4, 4, 16, 16, 3, 1, 1, 2, False, None),        # Upsample ae.py:164-166
    ("fp32x3", 1, 8, 8, 72, 8, 1, 1, 0, 1, False, None),         # nin_shortcut 1x1
    ("fp32x3", 1, 8, 8, 16, 8, 4, 4, 0, 1, False, None),         # disc head k4s4 utils.py:156-160
    ("fp32x3", 1, 4, 4, 24, 1, 2, 2, 0, 1, False, None),         # disc head k2s2 -> 1 channel
    ("bf16", 1, 8, 8, 3, 64, 3, 1, 1, 1, True, None),            # VGG conv1_1 + ReLU
    ("fp32x3", 2, 8, 8, 64, 64, 3, 1, 1, 1, True, None),
    # bf16 with Cin % 64 == 0 -> LDS-DMA (global_load_lds) kernel, fwd and dgrad
    ("bf16", 1, 8, 8, 64, 64, 3, 1, 1, 1, False, None),
    ("bf16", 2, 6, 6, 128, 72, 3, 1, 1, 1, True, None),
    ("bf16", 1, 4, 4, 64, 64, 3, 1, 1, 2, False, None),
    ("bf16", 1, 8, 8, 64, 128, 3, 2, 0, 1, False, (4, 4)),
    ("bf16", 1, 8, 8, 64, 64, 4, 4, 0, 1, False, None),         # patch conv: dgrad = 1x1 conv + depth-to-space store
    ("bf16", 2, 8, 8, 16, 32, 4, 4, 0, 1, False, None),         #   ... K = 32 (generic kernel), 2 images
    ("fp32", 1, 4, 8, 24, 1, 2, 2, 0, 1, False, None),          #   ... k2s2 -> 1 channel, fp32 storage, non-square
    ("bf16", 1, 8, 8, 192, 64, 1, 1, 0, 1, False, None),
    ("bf16", 1, 8, 8, 128, 128, 3, 1, 1, 1, False, None),       # three-tap wgrad, 8-pixel rows: 8 segments per chunk (80 halo slots)
    ("bf16", 1, 8, 8, 256, 256, 3, 1, 1, 1, False, None),       # wgrad LDS-DMA tile 256 (8 waves)
    ("bf16", 2, 4, 8, 256, 512, 1, 1, 0, 1, False, None),
    ("bf16", 1, 16, 16, 128, 128, 3, 1, 1, 1, False, None),     # three-tap wgrad: 4 image-row segments per 64-pixel chunk (72 halo slots)
    ("bf16", 1, 2, 128, 128, 256, 3, 1, 1, 1, False, None),     #   ... rows longer than a chunk (one segment), two cout tiles
    ("bf16", 2, 4, 32, 256, 128, 3, 1, 1, 1, False, None),      #   ... two segments, two cin tiles, chunks that cross images
    ("bf16", 1, 8, 8, 128, 128, 3, 1, 1, 2, False, None),       #   ... behind the nearest-2x upsample (ae.py:164-166)
    ("bf16", 1, 4, 48, 128, 128, 3, 1, 1, 1, False, None),      #   ... rows of 48 pixels (crop-invariance sizes): division decode, 16-pixel segments
    ("bf16", 2, 6, 160, 128, 256, 3, 1, 1, 1, False, None),     #   ... rows of 160 = 5 x 32 pixels, 6 rows
    ("bf16", 4, 4, 68, 128, 128, 3, 1, 1, 1, False, None),      #   ... rows of 68 = 17 x 4 pixels: 4-pixel segments (96 halo slots)
    ("bf16", 1, 4, 16, 64, 96, 3, 1, 1, 1, True, None),         # three-tap igemm: half-empty pixel tile, ragged cout tile, ReLU
    ("bf16", 3, 2, 64, 192, 72, 3, 1, 1, 1, False, None),       #   ... 64-pixel rows (two segments per tile), 3 channel chunks
    # 3-channel image layers -> conv_small.hip (direct-to-register fwd, one-pass wgrad)
    ("bf16", 2, 8, 64, 3, 64, 3, 1, 1, 1, True, None),          # VGG conv1_1
    ("bf16", 1, 4, 128, 3, 128, 3, 1, 1, 1, False, None),       # encoder.conv_in
    ("bf16", 1, 5, 7, 3, 96, 3, 1, 1, 1, False, None),          # ragged: fwd kernel only, generic wgrad
    ("bf16", 1, 4, 64, 128, 3, 3, 1, 1, 1, False, None),        # decoder.conv_out: one-pass wgrad with the roles swapped
    ("bf16", 2, 3, 128, 64, 3, 3, 1, 1, 1, False, None),        #   ... 64 channels, 2 images, several runs per block row
    ("bf16", 1, 4, 64, 256, 3, 3, 1, 1, 1, False, None),        #   ... 256 channels (wavelet / HR-decoder models: two 128-channel tiles, blockIdx.y)
    ("bf16", 1, 2, 64, 3, 384, 3, 1, 1, 1, True, None),         #   ... 3 -> 384: the un-swapped form over three channel tiles, ReLU
    # phase-decomposed resampling convs (VqConvDesc.subpix): Upsample fwd = four 2x2 convs of the low-res input + its dgrad
    # as a 4x4/s2 conv (Cout % 32 == 0), Downsample dgrad = four 2x2 convs over dy (Cin % 32 == 0, even H and W)
    ("fp32x3", 2, 3, 5, 24, 96, 3, 1, 1, 2, False, None),       # phase blocks of 96 rows -> 32-row tiles, generic kernel
    ("fp32x3", 1, 4, 6, 8, 128, 3, 1, 1, 2, True, None),        #   ... 128-row tiles, ReLU epilogue
    ("bf16", 2, 5, 3, 64, 32, 3, 1, 1, 2, False, None),         #   ... LDS-DMA kernel, 32-row tiles (weights through LDS)
    ("bf16", 1, 4, 4, 64, 256, 3, 1, 1, 2, False, None),        #   ... 128-row tiles, register weights
    ("fp32x3", 2, 6, 10, 96, 96, 3, 2, 0, 1, False, (3, 5)),    # Downsample dgrad, non-square, two images
    ("bf16", 2, 4, 12, 128, 64, 3, 2, 0, 1, False, (2, 6)),
    ("fp32x3", 1, 7, 9, 32, 32, 3, 2, 0, 1, False, (3, 4)),     # odd extents: stays on the zero-dilated form
    # split 6 (fp32-exact products: three bf16 pieces per operand, six MFMAs; policy fp32x6): generic kernel, every tile height,
    # ragged M / Cout, Downsample, the sub-pixel Upsample, 1x1, a patch head
    ("fp32x6", 2, 6, 10, 24, 136, 3, 1, 1, 1, False, None),
    ("fp32x6", 1, 8, 8, 8, 24, 3, 2, 0, 1, False, (4, 4)),
    ("fp32x6", 1, 4, 6, 8, 128, 3, 1, 1, 2, True, None),
    ("fp32x6", 1, 8, 8, 72, 8, 1, 1, 0, 1, False, None),
    ("fp32x6", 1, 8, 8, 16, 8, 4, 4, 0, 1, False, None),
    ("fp32x6", 2, 8, 8, 64, 64, 3, 1, 1, 1, True, None),
]
GPU_ONLY_CONV_CASES = [
    ("bf16", 2, 32, 32, 128, 128, 3, 1, 1, 1, False, None),
    ("fp32x3", 2, 16, 16, 256, 512, 3, 1, 1, 1, False, None),
    ("bf16", 4, 16, 16, 512, 512, 3, 1, 1, 2, False, None),
    ("fp32x3", 2, 32, 32, 128, 128, 3, 2, 0, 1, False, (16, 16)),
    ("bf16", 2, 64, 64, 128, 3, 3, 1, 1, 1, False, None),
    ("fp32x3", 3, 16, 16, 16, 512, 3, 1, 1, 1, False, None),
    ("fp32x6", 2, 16, 16, 256, 512, 3, 1, 1, 1, False, None),
    ("fp32x6", 2, 32, 32, 128, 128, 3, 1, 1, 2, False, None),
]


@contextlib.contextmanager
def hinted(conv=0, wgrad=0):
    """VqConvDesc.kernel_hint for every descriptor built inside (include/vqhip.h): forces one of the shipped kernels at a small
    shape, or — values a release library refuses — one of the compile-time ablation knobs of `make ABLATE=1` builds: those
    cases are skipped unless the library under test was built that way."""
    vq.ops.clear_caches()
    try:
        with ops.kernel_hints(conv=conv, wgrad=wgrad):
            yield
    except RuntimeError as exc:
        if "ABLATE=1" in str(exc):
            pytest.skip("knob only exists in `make ABLATE=1` builds (compile-time ablations)")
        raise
    finally:
        vq.ops.clear_caches()


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_ONLY_CONV_CASES, ids=lambda c: "-".join(map(str, c)))
def test_conv_cases_too_large_for_the_emulator(hip_library, case):
    """Mid-size layer shapes (32x32 / 16x16 images at 128-512 channels, the sub-pixel Upsample at 512 channels, a strided Downsample,
    the 3-channel and 16-channel stems) against F.conv2d + autograd: forward, data, weight and bias gradients."""
    from conftest import Backend
    vq._lib._set_library_for_tests(hip_library)
    vq.ops.clear_caches()
    try:
        _conv_case(Backend("gpu", "cuda:0", hip_library), case)
    finally:
        vq._lib._set_library_for_tests(None)
        vq.ops.clear_caches()


def _conv_case(backend, case, seed=None, report=None):
    prec, N, H, W, Ci, Co, R, stride, pad, up, relu, out_hw = case
    P = ops._PRECISIONS[prec]
    g = torch.Generator().manual_seed(case_seed(*case) if seed is None else seed)
    x = torch.randn(N, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, R, R, generator=g) / (Ci * R * R) ** 0.5
    b = torch.randn(Co, generator=g)
    dev = backend.device
    xd, wd, bd = (leaf(t, dev) for t in (x, w, b))
    y = ops.to_nchw(ops.conv2d(ops.to_nhwc(xd, P), wd, bd, stride=stride, pad=(pad, pad), up=up, relu=relu,
                               split=P.split, out_hw=out_hw), Co)
    xr, wr, br = (leaf(t) for t in (x, w, b))
    if up == 2:
        yr = ops_ref.upsample(xr, wr, br)
    elif out_hw is not None:
        yr = ops_ref.downsample(xr, wr, br)
    else:
        yr = ops_ref.conv2d(xr, wr, br, stride=stride, padding=pad)
    if relu:
        yr = yr.relu()
    gy = torch.randn(yr.shape, generator=g)
    if relu:
        gy = gy * (yr > 0)  # consumer contract: dy arrives masked
    y.backward(gy.to(dev))
    yr.backward(gy)
    tol = TOL[prec]
    assert y.shape == yr.shape
    # every output is a sum of products: its natural scale (one standard deviation) floors the normalisation, so that outputs of a
    # handful of elements (Cout = 1 with a 2 x 2 image: four values of y; a 1-3 element bias gradient) cannot pass or fail by the
    # luck of a cancelling draw
    rms = lambda t: t.detach().float().pow(2).mean().sqrt().item()   # noqa: E731
    errs = {"y": rel_err(y, yr, floor=(Ci * R * R) ** 0.5 * rms(x) * rms(w)),
            "dx": rel_err(xd.grad, xr.grad, floor=(Co * R * R) ** 0.5 / stride * rms(gy) * rms(w)),
            "dw": rel_err(wd.grad, wr.grad, floor=(gy.numel() // Co) ** 0.5 * rms(gy) * rms(x)),
            "db": rel_err(bd.grad, br.grad, floor=reduction_scale(gy, gy.numel() // Co))}
    if report is not None:       # tools/tol_sweep.py: the sweep the tolerances are derived from
        report.update(errs)
        return
    for name, err in errs.items():
        assert err < tol, (name, err, tol)


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "-".join(map(str, c)))
def test_conv_fwd_dgrad_wgrad(backend, case):
    _conv_case(backend, case)


# The binary16 instantiations of the 16-bit kernels (same sources, `DT` template parameter): every bf16 case again with fp16
# storage, on both backends (generic / LDS-DMA with LDS and register weights / patch data gradient / three-tap and LDS-DMA weight
# gradients / the 8-channel image kernels / phase-decomposed forms).
FP16_CONV_CASES = [("fp16",) + c[1:] for c in CONV_CASES if c[0] == "bf16"]


@pytest.mark.parametrize("case", FP16_CONV_CASES, ids=lambda c: "-".join(map(str, c)))
def test_conv_fp16_storage(backend, case):
    _conv_case(backend, case)


# The VQ_F16X2 instantiations (two binary16 pieces per value, three MFMAs per product; policy "f16x3"): every 16-bit and fp32x3 case
# again in that storage, on both backends — same kernels, `DT` template parameter; the weight gradients of the three-tap shapes in the native
# three-product form (round 6), the others through the virtual-channel form and wgrad_reduce_x2_kernel.
F16X3_CONV_CASES = sorted({("f16x3",) + c[1:] for c in CONV_CASES if c[0] in ("bf16", "fp32x3")}, key=repr)


@pytest.mark.parametrize("case", F16X3_CONV_CASES, ids=lambda c: "-".join(map(str, c)))
def test_conv_f16x3_storage(backend, case):
    _conv_case(backend, case)


@pytest.mark.parametrize("mode", [1, 3, 5, 6, 7, 9, 3 + (512 << 4)])
@pytest.mark.parametrize("case", [("f16x3", 2, 16, 16, 32, 128, 3, 1, 1, 1, False, None), ("f16x3", 1, 16, 32, 64, 256, 3, 1, 1, 1, True, None),
                                  ("f16x3", 1, 8, 16, 64, 256, 3, 1, 1, 2, False, None), ("f16x3", 3, 8, 8, 32, 128, 1, 1, 0, 1, False, None)],
                         ids=lambda c: "-".join(map(str, c)))
def test_conv_f16x3_forced_kernels(backend, case, mode):
    """Every implicit-GEMM kernel family in its VQ_F16X2 form (VqConvDesc.kernel_hint as in test_conv_tile_modes: 1 = 128 x 128 register-
    weight tiles, 3 = the 256 x 256 tile — patch-staged where the shape allows, + 512 << 4 its one-tap ping-pong form —, 5 = nine-tap,
    6 = one-tap only, 7 = three-tap, 9 = weights through LDS): 32 real channels = one virtual chunk, 64 = two; ReLU, the sub-pixel
    Upsample (S = 2 patch kernel), a 1x1; forward + both gradients."""
    with hinted(conv=mode):
        _conv_case(backend, case)


@pytest.mark.parametrize("wgrad_hint", [0, 8], ids=["native", "virtual"])
@pytest.mark.parametrize("case", [("f16x3", 1, 8, 8, 128, 128, 3, 1, 1, 1, False, None),      # 2 x 2 tiles of 64 real channels, rows of 8 (general form)
                                  ("f16x3", 1, 16, 16, 64, 128, 3, 1, 1, 1, True, None),      # rows of 16: the power-of-two form, ReLU-masked dy
                                  ("f16x3", 2, 8, 20, 64, 64, 3, 1, 1, 1, False, None),       # rows of 20 pixels: division decode, two images
                                  ("f16x3", 1, 4, 8, 64, 64, 3, 1, 1, 2, False, None),        # behind the nearest-2x gather (Upsample)
                                  ("f16x3", 1, 32, 32, 64, 64, 3, 1, 1, 1, False, None),      # rows of 32, several pixel splits
                                  # the one-tap LDS-DMA kernel in the same form: 1x1 and strided layers, tiles of 128 virtual channels ...
                                  ("f16x3", 1, 8, 8, 128, 128, 1, 1, 0, 1, False, None), ("f16x3", 1, 16, 16, 128, 128, 3, 2, 0, 1, True, (8, 8)),
                                  ("f16x3", 2, 256, 256, 128, 128, 1, 1, 0, 1, False, None)], # ... and of 256 (long reductions only)
                         ids=lambda c: "-".join(map(str, c)))
def test_wgrad_f16x3_native_three_product(backend, case, wgrad_hint):
    """Round 6: the three-tap weight-gradient kernel forms hi*hi + hi*lo + lo*hi itself on VQ_F16X2 operands (conv_wgrad3_kernel<..., X3 = 1>:
    four waves, fragments = the hi / lo piece of 32 real channels, one accumulator per tap, real-channel slabs, the ordinary split
    reduction) instead of running on the virtual 2C x 2C problem with the quadrant sum behind it (kernel_hint bit 3 = 8 keeps that form
    for the A/B); so does the one-tap LDS-DMA kernel on its 128- and 256-wide tiles (conv_wgrad_glds_kernel<..., X3 = 1>).  Both forms against the fp32 oracle at the f16x3 tolerance: dw, the fused bias gradient, and — same launches — y / dx."""
    if backend.name == "emu" and case[2] * case[3] > 1024:
        # (run there once, 45-55 s each: dw / y / dx within tolerance, the fused bias gradient — an fp32 sum over 131072 pixels in the
        # emulator's block order — at 1.03e-5 against the 1e-5 bound the GPU meets; needs the device's reduction order)
        pytest.skip("256 x 256 images: needs the GPU")
    with hinted(wgrad=wgrad_hint):
        _conv_case(backend, case)


@pytest.mark.parametrize("wmag,gmag", [(1e-6, 1.0), (3e2, 1e-3), (1.0, 3e-6)])
def test_fp16_scales_keep_tiny_weights_and_gradients(backend, wmag, gmag):
    """binary16 has 5 exponent bits: weights of magnitude 1e-6 (the reference initialises ResnetBlock.conv2 with std
    1e-4 / out_ch, ae.py:119-121) or gradients of 1e-6 would flush without the per-tensor weight scale measured by the pack
    kernels and the loss scale of the stack — with them the relative accuracy of the three passes does not depend on the
    magnitudes.  (Activations are stored unscaled: the conv output joins an O(1) residual in the epilogue, as in the block.)"""
    g = torch.Generator().manual_seed(7)
    N, H, W, Ci, Co = 2, 8, 8, 64, 64
    x = torch.randn(N, Ci, H, W, generator=g)
    res = torch.randn(N, Co, H, W, generator=g) * max(1.0, 20 * wmag)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / 24 * wmag
    b = torch.randn(Co, generator=g) * wmag
    dev = backend.device
    # the stack's loss scale must hold its LARGEST gradient tensor (calibrate_grad_scales measures it): here dx ~ gy * 24 * wmag
    P = ops.fp16_region("test", grad_scale=2.0 ** round(torch.log2(torch.tensor(512.0 / (gmag * max(1.0, wmag)))).item()))
    xd, wd, bd = (leaf(t, dev) for t in (x, w, b))
    with ops.region(P):
        y = ops.to_nchw(ops.conv2d(ops.to_nhwc(xd, P), wd, bd, residual=ops.to_nhwc(res.to(dev), P), stride=1, pad=(1, 1), split=1), Co)
    xr, wr, br = (leaf(t) for t in (x, w, b))
    yr = ops_ref.conv2d(xr, wr, br, padding=1) + res
    gy = torch.randn(yr.shape, generator=g) * gmag
    y.backward(gy.to(dev)); yr.backward(gy)
    for got, want in ((y, yr), (xd.grad, xr.grad), (wd.grad, wr.grad), (bd.grad, br.grad)):
        assert rel_err(got, want) < TOL["fp16"]


@pytest.mark.parametrize("case", [("bf16", 2, 16, 16, 64, 128, 3, 1, 1, 1, False, None),
                                  ("bf16", 1, 8, 8, 128, 256, 3, 1, 1, 2, True, None),
                                  ("bf16", 3, 8, 8, 64, 128, 1, 1, 0, 1, False, None)],
                         ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("mode", [1, 3, 4, 5, 6, 8, 9])
def test_conv_tile_modes(backend, case, mode):
    """Force each implicit-GEMM tile (VqConvDesc.kernel_hint): 1 = 128x128 (4 waves x 32c x 128p, weights straight
    to registers), 3 = 256x256 (8 waves, 128 KiB LDS), 4 = the same without the ping-pong schedule (ABLATE builds), 5 = the
    nine-tap kernel (8 x 16 pixel patches with a halo, all nine taps from one staged tile); +8 = weights staged through LDS in
    every kernel."""
    with hinted(conv=mode):
        _conv_case(backend, case)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("dbg", [0, 72, 128, 256])
def test_nine_tap_kernel_variants(backend, dbg, prec):
    """conv_igemm_tap9_kernel (kernel_hint bits 4..): 0 = adopted form (tile DMA issued from inline asm so that hipcc
    does not drain the queue behind an LDS-DMA, unconditional weight requests, fragment addresses in registers, 32-KiB buffer
    stride, conflict-free lane -> pixel map); ABLATE builds only: 128 = the round-1 form, 256 (64-row tile only) = round-1 form of
    that tile; round 6: 72 = a one-chunk launch (Cin = 64) with BOTH halo buffers (the shipped form allocates one: four blocks per CU).
    Two channel chunks, two images, ReLU epilogue, forward + both gradients (the data gradient runs the same kernel)."""
    with hinted(conv=5 + (dbg << 4)):
        _conv_case(backend, (prec, 2, 16, 32, 128, 128, 3, 1, 1, 1, True, None))
        _conv_case(backend, (prec, 2, 16, 32, 64, 64, 3, 1, 1, 1, True, None))       # the 64-row tile (VGG conv1_2)


@pytest.mark.parametrize("mode,case", [(5, ("bf16", 2, 16, 32, 128, 64, 3, 1, 1, 1, True, None)),
                                       (5, ("bf16", 1, 4, 8, 64, 64, 3, 1, 1, 2, False, None)),
                                       (1 + (32 << 4), ("bf16", 2, 6, 10, 128, 192, 3, 1, 1, 1, True, None)),
                                       (1 + (32 << 4), ("bf16", 1, 8, 8, 64, 256, 3, 2, 0, 1, False, (4, 4)))],
                         ids=lambda v: str(v) if isinstance(v, int) else "-".join(map(str, v)))
def test_conv_ab_candidates_on_emulator(emu_library, mode, case):
    """Kernel instantiations kept behind knobs for the next A/B on hardware ("cheap follow-ups"): the nine-tap
    kernel as a 64-row tile and the register-weight one-tap tile as 2 x 2 waves.  Host emulator only: they have not run on an
    MI355X yet, so the `-m gpu` suite does not depend on them."""
    from conftest import Backend
    vq._lib._set_library_for_tests(emu_library)
    ops.set_subpixel(False)
    try:
        with hinted(conv=mode):
            _conv_case(Backend("emu", "cpu", emu_library), case)
    finally:
        ops.set_subpixel(True)
        vq._lib._set_library_for_tests(None)
        vq.ops.clear_caches()


@pytest.mark.parametrize("hint", [0, 16 << 4])
@pytest.mark.parametrize("case", [("bf16", 1, 4, 16, 64, 96, 3, 1, 1, 1, True, None), ("fp16", 2, 16, 16, 128, 512, 3, 1, 1, 1, True, None),
                                  ("bf16", 3, 2, 64, 192, 72, 3, 1, 1, 1, False, None), ("bf16", 1, 8, 32, 64, 64, 3, 1, 1, 2, False, None)],
                         ids=lambda c: "-".join(map(str, c)))
def test_three_tap_kernel_short_m_tiles(backend, case, hint):
    """conv_igemm_tap3_kernel on short-M layers (VGG conv5_x: 16 x 16 images): hint 0 = 64 x 64 tiles (4 waves x 32c x 32p: two blocks
    per CU where 64 x 128 tiles leave one wave per SIMD), 16 << 4 = the 64 x 128 tiles of rounds 1-2.  Half-empty and ragged tiles,
    1-3 channel chunks, rows of 16 / 32 / 64 pixels, ReLU, the nearest-2x gather; forward + both gradients."""
    with hinted(conv=hint):
        _conv_case(backend, case)


@pytest.mark.parametrize("case", [("bf16", 2, 16, 32, 128, 3, 3, 1, 1, 1, False, None), ("fp16", 1, 24, 16, 64, 3, 3, 1, 1, 1, False, None),
                                  ("bf16", 1, 8, 16, 192, 24, 3, 1, 1, 1, True, None), ("fp16", 2, 16, 16, 3, 64, 3, 1, 1, 1, True, None)],
                         ids=lambda c: "-".join(map(str, c)))
def test_nine_tap_kernel_with_32_row_tiles(backend, case):
    """Layers with <= 32 output channels (decoder.conv_out 128 -> 3; as a data gradient: VGG conv1_1) on the nine-tap kernel as 4 waves x
    32c x 32p with register weights (fragment-ordered layout, rows padded to 32): hint 5 = at any size (by itself from 512 tiles).
    One to three channel chunks, 3 / 24 real rows of the 32, bias / ReLU, both gradients; the last case reaches it as the data
    gradient of a 3 -> 64 layer (ReLU mask in the epilogue)."""
    with hinted(conv=5):
        _conv_case(backend, case)


@pytest.mark.parametrize("case", [("bf16", 2, 64, 64, 64, 32, 4, 4, 0, 1, False, None), ("fp16", 1, 32, 64, 128, 64, 4, 4, 0, 1, False, None),
                                  ("bf16", 4, 16, 32, 64, 64, 2, 2, 0, 1, False, None), ("fp16", 6, 32, 16, 32, 32, 2, 2, 0, 1, False, None)],
                         ids=lambda c: "-".join(map(str, c)))
def test_persistent_patch_data_gradient(backend, case):
    """conv_patch_dgrad_kernel: the data gradient of a patch conv (kernel == stride: PatchDiscriminator heads) with 32 channels of dy,
    register-resident weight fragments, dy fragments straight from global memory, blocks walking pixel-tile ranges (hint 56 << 4 =
    at any size; by itself from 64 pixel tiles).  4 x 4 and 2 x 2 patches, 8 row tiles / one, ranges of 4 and 6 pixel tiles; the two
    cases with 64 channels of dy stay on the tile kernels under the same hint (measured slower there, profiles/r3e_*).
    (Forward and weight gradient of the same layers run on the ordinary kernels.)"""
    with hinted(conv=56 << 4):
        _conv_case(backend, case)


def test_nine_tap_kernel_is_chosen_automatically(backend):
    """A layer with 256 tiles of 128 x 128 (the smallest the automatic rule hands to conv_igemm_tap9_kernel): same result as the
    one-tap kernel (knob 6) within bf16 rounding, but not bit-identical — the K order differs (chunk-major vs tap-major) — which is
    how the test knows the nine-tap kernel really ran."""
    g = torch.Generator().manual_seed(5)
    N, H, W, Ci, Co = 2, 128, 128, 128, 128
    x = torch.randn(N, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) / 34
    b = torch.randn(Co, generator=g)
    dev = backend.device
    xh = ops.to_nhwc(x.to(dev), ops.BF16)
    outs = []
    for mode in (0, 6):
        with hinted(conv=mode):
            outs.append(ops.to_nchw(ops.conv_fwd_raw(xh, w.to(dev), b.to(dev), None, 1, 1, 1, 1, False, 1, None), Co).cpu())
    ref = F.conv2d(x, w, b, padding=1)
    assert rel_err(outs[0], ref) < 2e-2 and rel_err(outs[1], ref) < 2e-2
    assert rel_err(outs[0], outs[1]) < 1e-2 and not torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("bt", [0, 16, 64, 128, 256, 1])
def test_wgrad_lds_dma_tiles(backend, bt, prec):
    """Weight-gradient kernels by hint (VqConvDesc.kernel_hint of vq_conv2d_wgrad): 0 = the plan's choice — the three-tap kernel (segment
    shift as a template parameter: rows of 16 / 32 / >= 64 pixels = SEG 4 / 5 / 6) with the two waves of a SIMD staging the next
    chunk half a chunk apart; 16 = every wave stages right after the chunk barrier; 64 / 128 / 256 = each one-tap LDS-DMA tile
    (4 / 4 / 8 waves); 1 = the 4 B/lane split reduction."""
    if backend.name == "gpu" and prec == "fp16" and bt not in (0, 16):
        pytest.skip("binary16 twins of the two forms of the three-tap kernel only (the other hints: on the emulator)")
    with hinted(wgrad=bt):
        _conv_case(backend, (prec, 1, 8, 16, 256, 256, 3, 1, 1, 1, False, None))      # rows of 16 pixels (SEG 4), two cin tiles
        _conv_case(backend, (prec, 3, 8, 16, 128, 128, 3, 1, 1, 1, False, None))      # 6 chunks in one split
        if bt in (0, 16):
            _conv_case(backend, (prec, 1, 4, 32, 128, 128, 3, 1, 1, 1, False, None))  # rows of 32 (SEG 5): the bias blocks are 2 of 3
            _conv_case(backend, (prec, 1, 2, 64, 128, 256, 3, 1, 1, 1, False, None))  # rows of 64 (SEG 6)


def test_subpixel_weights_and_equivalence(backend):
    """vq_subpixel_weights against its definition (include/vqhip.h), and the phase-decomposed Upsample / Downsample paths
    against the single-conv forms they replace (ae.py:150-154, 164-166) on the same inputs, incl. `add` + ReLU mask."""
    g = torch.Generator().manual_seed(11)
    dev = backend.device
    O, I = 40, 24
    w = torch.randn(O, I, 3, 3, generator=g)
    up = torch.tensor([[[1., 0, 0], [0, 1, 1]], [[1, 1, 0], [0, 0, 1]]])        # R_a(u) as 0/1 rows over r
    dn = torch.tensor([[[0., 0, 1], [1, 0, 0]], [[0, 1, 0], [0, 0, 0]]])        # D_a(u)
    t4 = torch.tensor([[0., 0, 1], [0, 1, 1], [1, 1, 0], [1, 0, 0]])            # T(ky)
    want = (torch.einsum("aur,oirs,bvs->aboiuv", up, w, up).reshape(4 * O, I, 2, 2),
            torch.einsum("kr,oirs,ls->iokl", t4, w, t4),
            torch.einsum("aur,oirs,bvs->abiouv", dn, w, dn).reshape(4 * I, O, 2, 2))
    for mode in range(3):
        got = ops._derived_weight(w.to(dev), mode)
        assert got.shape == want[mode].shape and rel_err(got, want[mode]) < 1e-6
    with pytest.raises(RuntimeError):
        backend.library.call("vq_subpixel_weights", vq._lib.ptr(w.to(dev)), vq._lib.ptr(w.to(dev)), O, I, 3, None)
    # same tensors through both forms
    P = ops.FP32X3
    x = ops.to_nhwc(torch.randn(2, 32, 6, 4, generator=g).relu().to(dev), P)
    wu = (torch.randn(32, 32, 3, 3, generator=g) / 17).to(dev)
    b = torch.randn(32, generator=g).to(dev)
    gy = ops.to_nhwc(torch.randn(2, 32, 12, 8, generator=g).to(dev), P)
    gd = ops.to_nhwc(torch.randn(2, 32, 3, 2, generator=g).to(dev), P)
    add = ops.to_nhwc(torch.randn(2, 32, 6, 4, generator=g).to(dev), P)
    res = {}
    for on in (True, False):
        ops.set_subpixel(on)
        ops.clear_caches()
        try:
            res[on] = (ops.conv_fwd_raw(x, wu, b, None, 1, 1, 1, 2, False, 3, None),
                       ops.conv_dgrad_raw(gy, x, wu, 1, 1, 1, 2, 3, False),
                       ops.conv_dgrad_raw(gd, x, wu, 2, 0, 0, 1, 3, True, add=add))
        finally:
            ops.set_subpixel(True)
    for a, c in zip(res[True], res[False]):
        assert a.shape == c.shape and rel_err(a, c) < 2e-5
    # a sub-pixel descriptor the kernels cannot run is refused, not mis-computed
    d = ops._desc(1, 4, 4, 32, 4, 4, 64, 32, 64, 2, 2, 1, 1, 1, 1, 1, vq._lib.VQ_F32, 3, False, subpix=2)    # 16 rows per phase
    with pytest.raises(RuntimeError):
        backend.library.call("vq_conv2d_fwd", vq._lib.C.byref(d), vq._lib.ptr(x), vq._lib.ptr(x), None, None, None, vq._lib.ptr(x), None, 0, None)


def test_conv_mask_input_grad_and_residual(backend):
    """x + h in the epilogue (ae.py:140) and the ReLU consumer contract."""
    P = ops.FP32X3
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 16, 6, 6, generator=g).relu()
    w = torch.randn(16, 16, 3, 3, generator=g) / 12
    r = torch.randn(1, 16, 6, 6, generator=g)
    dev = backend.device
    xd, wd, rd = (leaf(t, dev) for t in (x, w, r))
    y = ops.to_nchw(ops.conv2d(ops.to_nhwc(xd, P), wd, None, residual=ops.to_nhwc(rd, P), pad=(1, 1),
                               mask_input_grad=True, split=3), 16)
    xr, wr, rr = (leaf(t) for t in (x, w, r))
    yr = F.conv2d(xr.relu(), wr, padding=1) + rr   # x is a ReLU output: relu() re-applied is identity, grads get masked
    gy = torch.randn(yr.shape, generator=g)
    y.backward(gy.to(dev)); yr.backward(gy)
    assert rel_err(y, yr) < 5e-5
    assert rel_err(xd.grad, xr.grad) < 5e-5
    assert rel_err(rd.grad, rr.grad) < 1e-6
    assert rel_err(wd.grad, wr.grad) < 5e-5


@pytest.mark.parametrize("prec,C,H,W,silu", [("fp32x3", 32, 8, 8, True), ("fp32x3", 128, 40, 40, True),
                                             ("fp32x3", 64, 5, 7, False), ("bf16", 256, 8, 8, True),
                                             ("fp32x3", 512, 3, 3, True), ("fp32x3", 512, 16, 9, True),
                                             ("fp32x3", 1024, 6, 6, True),      # several reduction blocks; vae_ch=256 widths
                                             ("fp32x3", 96, 9, 5, True), ("bf16", 192, 7, 6, True),    # vae_ch=96: 3 / 6 channels per group
                                             # block-size boundaries of the reductions (32 / 64 / 128 / 256 pixels per block)
                                             ("fp32x3", 64, 33, 31, True), ("fp32x3", 160, 1, 1, False), ("fp32x3", 256, 2, 129, True),
                                             ("fp32x3", 32, 64, 65, True), ("fp32x3", 384, 11, 3, False), ("fp32x3", 640, 4, 8, True),
                                             ("fp32x3", 32, 150, 150, False),      # > 512 partials per sample: wave-wide finalize
                                             # > 64 partials per sample with 8 / 16 channels per group: the backward finalize runs 32 / 16
                                             # lanes per channel so that whole groups stay inside one block (coefficients in the same launch)
                                             ("bf16", 256, 96, 96, True), ("fp32x3", 512, 50, 50, True),
                                             ("fp16", 256, 8, 8, True), ("fp16", 96, 9, 5, False),
                                             ("f16x3", 256, 8, 8, True), ("f16x3", 96, 9, 5, False), ("f16x3", 128, 40, 40, True)])
def test_groupnorm_silu(backend, prec, C, H, W, silu):
    """ae.py:41-53 + ae.py:13-14, forward and backward incl. dgamma/dbeta."""
    P = ops._PRECISIONS[prec]
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(2, C, H, W, generator=g) * 2 + 0.5
    ga = torch.rand(C, generator=g) + 0.5
    be = torch.randn(C, generator=g) * 0.1
    dev = backend.device
    xd, gd, bd = (leaf(t, dev) for t in (x, ga, be))
    y = ops.to_nchw(ops.group_norm_silu(ops.to_nhwc(xd, P), gd, bd, 32, 1e-6, silu), C)
    xr, gr, br = (leaf(t) for t in (x, ga, be))
    yr = ops_ref.group_norm_fp32(xr, gr, br)
    if silu:
        yr = ops_ref.swish(yr)
    gy = torch.randn(yr.shape, generator=g)
    y.backward(gy.to(dev)); yr.backward(gy)
    tol = {"fp32x3": 2e-5, "fp16": 2.5e-3, "f16x3": 2e-5}.get(prec, 2e-2)
    assert rel_err(y, yr) < tol
    assert rel_err(xd.grad, xr.grad) < tol
    n_sum = 2 * H * W                                   # terms per channel of dgamma = sum dy * xhat, dbeta = sum dy
    assert rel_err(gd.grad, gr.grad, floor=reduction_scale(gy, n_sum)) < tol
    assert rel_err(bd.grad, br.grad, floor=reduction_scale(gy, n_sum)) < tol


def test_groupnorm_refuses_one_value_per_group_like_torch(backend):
    """F.group_norm (behind FP32GroupNorm, ae.py:41-53) raises ValueError when a group holds ONE value over the whole batch (N = 1,
    one channel per group, a 1 x 1 image: width-32 models on images as small as their downsampling factor); so does the op, with torch's
    message — two values (N = 2) are served."""
    dev = backend.device
    ga, be = torch.ones(32, device=dev), torch.zeros(32, device=dev)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        ops.group_norm_silu(torch.randn(1, 1, 1, 32, device=dev), ga, be, 32, 1e-6, True)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        F.group_norm(torch.randn(1, 32, 1, 1), 32)
    y = ops.group_norm_silu(torch.randn(2, 1, 1, 32, device=dev), ga, be, 32, 1e-6, False)
    # (x - x) * rstd + beta with rstd = 1 / sqrt(eps) = 1000: zero up to the rounding of x * 1000 in the kernel's fused multiply-add
    assert tuple(y.shape) == (2, 1, 1, 32) and float(y.abs().max()) < 1e-3


@pytest.mark.parametrize("prec", ["fp32x3", "f16x3", "fp16", "bf16"])
@pytest.mark.parametrize("offset", [30.0, 100.0, 300.0, -1000.0])
def test_groupnorm_on_offset_activations(backend, prec, offset):
    """ae.py:41-53 runs F.group_norm in fp32, whose moments keep their accuracy when |mean| >> std (biased conv layers, smooth images:
    a large DC per group).  A one-pass `E[x^2] - E[x]^2` on fp32 sums does not (round-5 verdict: 1.7e-4 / 1.8e-3 at |mean|/std = 100 /
    300 against 4.6e-6 / 1.1e-5 for F.group_norm).  Truth = fp64; the yardstick is F.group_norm in fp32 ON THE TENSOR THE KERNEL READ
    (the storage rounding of an offset input is the input's, not the statistics'): forward and dx within 3x of it (+ the storage
    type's own output rounding), per-channel offsets inside a group included."""
    P = ops._PRECISIONS[prec]
    g = torch.Generator().manual_seed(int(abs(offset)))
    C, H, W = 128, 24, 24
    x = torch.randn(2, C, H, W, generator=g) + offset + torch.randn(1, C, 1, 1, generator=g) * 0.5
    ga = torch.rand(C, generator=g) + 0.5
    be = torch.randn(C, generator=g) * 0.1
    dev = backend.device
    x_stored = ops.to_nchw(ops.to_nhwc(x.to(dev), P), C).detach().float().cpu()    # what the kernels see (re-stored exactly below)
    xd, gd, bd = leaf(x_stored, dev), leaf(ga, dev), leaf(be, dev)
    y = ops.to_nchw(ops.group_norm_silu(ops.to_nhwc(xd, P), gd, bd, 32, 1e-6, True), C)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy.to(dev))
    dx = xd.grad
    out = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        xr, gr, br = (leaf(t.to(dt)) for t in (x_stored, ga, be))
        yr = ops_ref.swish(torch.nn.functional.group_norm(xr, 32, gr, br, 1e-6))
        yr.backward(gy.to(dt))
        out[name] = (yr.detach(), xr.grad, gr.grad, br.grad)
    def err(a, b):
        return ((a.detach().double().cpu() - b.double()).abs().max() / b.abs().max()).item()
    floor = {"fp32x3": 2e-6, "f16x3": 2e-6, "fp16": 1.5e-3, "bf16": 1.2e-2}[prec]      # output rounding of the storage type
    for i, (got, what) in enumerate(((y, "y"), (dx, "dx"), (gd.grad, "dgamma"), (bd.grad, "dbeta"))):
        ours, ref32 = err(got, out["f64"][i]), err(out["f32"][i], out["f64"][i])
        assert ours <= 3.0 * ref32 + floor, (what, prec, offset, ours, ref32)


@pytest.mark.parametrize("prec,N,H,W,Ci,Co,silu", [("bf16", 2, 16, 16, 128, 64, True), ("fp16", 1, 32, 16, 64, 128, True),
                                                   ("bf16", 1, 16, 32, 256, 256, False), ("fp16", 3, 16, 16, 96, 64, True)])
def test_groupnorm_backward_sums_from_the_data_gradient_conv(backend, prec, N, H, W, Ci, Co, silu):
    """VqGnBwdFuse (include/vqhip.h; compiled into `make ABLATE=1` libraries and the emulator only — measured 0.9 % slower in the step,
    and its mere presence in the shared epilogue cost the default step 1.5 %): the data-gradient conv that produces the dy of a
    GroupNorm(+SiLU) forms that GroupNorm's backward sums in its epilogue (x read like a residual operand, one partial row per wave), and vq_gn_silu_bwd(part_in) skips its
    reduction pass.  Against the unfused pair of launches on the same tensors: the same dy bit for bit, dx / dgamma / dbeta to the
    rounding of dy (the fused sums see dy before it is rounded to 16 bits); 128- and 256-pixel tiles, 1-3 images, groups of 2-8
    channels, one and several channel tiles."""
    P = ops._PRECISIONS[prec]
    g = torch.Generator().manual_seed(N * 1000 + Ci)
    dev = backend.device
    xg = ops.to_nhwc((torch.randn(N, Ci, H, W, generator=g) * 1.5 + 0.3).to(dev), P)       # the GroupNorm's input (Ci channels)
    gamma = (torch.rand(Ci, generator=g) + 0.5).to(dev)
    beta = (torch.randn(Ci, generator=g) * 0.2).to(dev)
    a, stats = ops.gn_fwd_raw(xg, gamma, beta, 32, 1e-6, silu)
    w = (torch.randn(Co, Ci, 3, 3, generator=g) / (Ci * 9) ** 0.5).to(dev)                  # the conv that consumes the activation
    dout = ops.to_nhwc(torch.randn(N, Co, H, W, generator=g).to(dev), P)
    outs = {}
    for fused in (False, True):
        ops.set_gn_bwd_fusion(fused)
        try:
            da, part = ops.conv_dgrad_raw(dout, a, w, 1, 1, 1, 1, P.split, False, gn_bwd=(xg, stats, gamma, beta, 32, silu))
            if fused and part is None:
                pytest.skip("a release library does not carry the fused path (slower in the step: `make ABLATE=1` builds and the emulator only)")
            assert part is None or fused
            dx, dga, dbe = ops.gn_bwd_raw(xg, da, stats, gamma, beta, 32, silu, part=part)
        finally:
            ops.set_gn_bwd_fusion(False)
        outs[fused] = (da.float().cpu(), dx.float().cpu(), dga.cpu(), dbe.cpu())
    assert torch.equal(outs[False][0], outs[True][0])
    tol = 1e-2 if prec == "bf16" else 2e-3
    for i in (1, 2, 3):
        assert rel_err(outs[True][i], outs[False][i]) < tol, (i, rel_err(outs[True][i], outs[False][i]))


def test_maxpool_and_scaling_layer(backend):
    P = ops.FP32X3
    g = torch.Generator().manual_seed(5)
    dev = backend.device
    x = torch.randn(2, 16, 8, 12, generator=g).relu()
    xd = leaf(x, dev)
    y = ops.to_nchw(ops.max_pool2(ops.to_nhwc(xd, P)), 16)
    xr = leaf(x)
    yr = F.max_pool2d(xr, 2, 2)
    gy = torch.randn(yr.shape, generator=g)
    y.backward(gy.to(dev)); yr.backward(gy)
    assert torch.equal(y.cpu(), yr)
    assert torch.equal(xd.grad.cpu(), xr.grad)      # first-max tie rule incl. all-zero windows
    shift = torch.tensor([-.030, -.088, -.188]); scale = torch.tensor([.458, .448, .450])
    x = torch.randn(2, 3, 4, 4, generator=g)
    xd = leaf(x, dev)
    y = ops.to_nchw(ops.to_nhwc(xd, P, shift.to(dev), scale.to(dev)), 3)
    xr = leaf(x)
    yr = ops_ref.scaling_layer(xr, shift, scale)
    gy = torch.randn(yr.shape, generator=g)
    y.backward(gy.to(dev)); yr.backward(gy)
    assert rel_err(y, yr) < 1e-6 and rel_err(xd.grad, xr.grad) < 1e-6


@pytest.mark.parametrize("prec,H,W", [("fp32x3", 8, 12), ("fp32x3", 7, 9), ("bf16", 6, 6), ("fp16", 5, 8), ("f16x3", 7, 9), ("f16x3", 8, 12)])
def test_pool_with_tap_sums_both_gradients_in_the_pool_backward(backend, prec, H, W):
    """ops.pool_with_tap: a VGG slice output with two consumers (its tap and, through the 2x2 max-pool, the next slice:
    utils.py:116-131,187-203) as ONE autograd node — dx = route(d_pooled) + d_tap in vq_maxpool2_bwd, no separate elementwise add.
    Against F.max_pool2d + autograd's own fan-in sum, incl. odd extents (the dropped last row / column gets the tap gradient alone)."""
    P = ops._PRECISIONS[prec]
    g = torch.Generator().manual_seed(7)
    dev, N, C = backend.device, 2, 16
    x = torch.randn(N, C, H, W, generator=g).relu().bfloat16().float()    # exact in every storage type: the arg-max decisions agree
    xd, xr = leaf(x, dev), leaf(x)
    tap, pooled = ops.pool_with_tap(ops.to_nhwc(xd, P))
    t_ref, p_ref = xr * 1.0, F.max_pool2d(xr, 2, 2)
    gt, gp = torch.randn(t_ref.shape, generator=g), torch.randn(p_ref.shape, generator=g)
    (ops.to_nchw(tap, C) * gt.to(dev)).sum().backward(retain_graph=True)
    only_tap = xd.grad.clone(); xd.grad = None
    ((ops.to_nchw(tap, C) * gt.to(dev)).sum() + (ops.to_nchw(pooled, C) * gp.to(dev)).sum()).backward()
    ((t_ref * gt).sum() + (p_ref * gp).sum()).backward()
    tol = TOL[prec] if prec not in ("fp32x3", "f16x3") else 1e-6
    assert rel_err(ops.to_nchw(pooled, C), p_ref) < tol and rel_err(ops.to_nchw(tap, C), t_ref) < tol
    assert rel_err(xd.grad, xr.grad) < tol
    assert rel_err(only_tap, gt) < tol                 # the pooled output unused: the tap gradient passes through


def test_range_events_count_saturated_and_vanished_binary16_stores(backend):
    """include/vqhip.h "range events": kernels that write a binary16 tensor of a loss-scaled stack report clipped stores (counter 0)
    and fully flushed waves (counter 1) to the stack's device counters; a healthy launch writes nothing.  Through the layout entry
    (where a gradient enters a stack times its loss scale), the conv epilogue, the GroupNorm backward and the LPIPS tap backward."""
    dev = backend.device
    prec = ops.fp16_region("probe", 2.0 ** 12)
    prec.events = torch.zeros(4, dtype=torch.int32, device=dev)

    hot_seen = []

    def counts():
        c = prec.events.tolist()
        prec.events.zero_()
        hot_seen.append(c[2])
        return c[0], c[1]

    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 8, 8, generator=g)
    w = (torch.randn(64, 64, 3, 3, generator=g) / 24).to(dev)
    with ops.region(prec):
        xh = ops.to_nhwc(x.to(dev), prec)
        y = ops.conv_fwd_raw(xh, w, None, None, 1, 1, 1, 1, False, 1, None)
        assert counts() == (0, 0), "a healthy forward must not touch the counters"
        big = ops.conv_fwd_raw((xh * 2000).to(torch.float16), (w * 100).contiguous(), None, None, 1, 1, 1, 1, False, 1, None)   # |y| ~ 2e5
        sat, fl = counts()
        assert sat > 0 and fl == 0 and float(big.float().abs().max()) == 65504.0
        assert hot_seen[0] == 0 and hot_seen[1] > 0, "counter 2 (headroom): silent on a healthy launch, set by a clipped one"
        warm = ops.conv_fwd_raw((xh * 40).to(torch.float16), (w * 100).contiguous(), None, None, 1, 1, 1, 1, False, 1, None)   # |y| up to ~1.6e4: in range, 2^13 passed
        sat, fl = counts()
        assert sat == 0 and fl == 0 and hot_seen[-1] > 0 and 8192.0 <= float(warm.float().abs().max()) < 65504.0
        tiny = ops.conv_fwd_raw(xh, (w * 1e-9).contiguous(), None, None, 1, 1, 1, 1, False, 1, None)                          # |y| ~ 1e-9 < 2^-24
        sat, fl = counts()
        assert sat == 0 and fl > 0 and float(tiny.float().abs().max()) == 0.0
    # a gradient entering the stack times a loss scale that is far too large
    hot = ops.fp16_region("hot", 2.0 ** 30)
    hot.events = torch.zeros(4, dtype=torch.int32, device=dev)
    xd = leaf(torch.randn(1, 16, 4, 4, generator=g), dev)
    with ops.region(hot):
        out = ops.to_nchw(ops.to_nhwc(xd, hot), 16)
    out.sum().backward()
    assert hot.events[0].item() > 0
    # GroupNorm backward and LPIPS tap backward report through the node's own stack
    gam, bet = leaf(torch.ones(64), dev), leaf(torch.zeros(64), dev)
    with ops.region(prec):
        h = ops.group_norm_silu(ops.to_nhwc(leaf(x, dev), prec), gam, bet)
    (h.float() * 3e4).sum().backward()                 # dy = 3e4 per element: dx beyond binary16's range after the 1/sigma gain? no: count both ways
    sat_gn, _ = counts()
    f = torch.randn(2, 64, 4, 4, generator=g).relu()
    fd = leaf(f, dev)
    with ops.region(prec):
        fh = ops.to_nhwc(fd, prec)
        v = ops.lpips_tap(fh[:1], fh[1:], torch.rand(64, generator=g).to(dev))
    prec.grad_scale = 2.0 ** 40
    v.sum().backward()
    sat_lp, _ = counts()
    assert sat_lp > 0, "a 2^40 loss scale must clip the tap gradient"
    assert sat_gn >= 0


@pytest.mark.parametrize("prec,C,H", [("fp32x3", 64, 8), ("fp32x3", 512, 4), ("fp32x3", 128, 5), ("bf16", 256, 8), ("fp16", 128, 6),
                                      ("f16x3", 128, 6), ("f16x3", 512, 4), ("f16x3", 64, 5)])
def test_lpips_tap(backend, prec, C, H):
    """utils.py:44-57,134-140 with an injected dropout mask."""
    P = ops._PRECISIONS[prec]
    N = 2
    g = torch.Generator().manual_seed(C)
    f = torch.randn(2 * N, C, H, H, generator=g).relu()
    w = torch.rand(C, generator=g)
    mask = (torch.rand(N, C, H, H, generator=g) < 0.5).float() * 2
    dev = backend.device
    fd = leaf(f, dev)
    fh = ops.to_nhwc(fd, P)
    val = ops.lpips_tap(fh[:N], fh[N:].detach(), w.to(dev), mask.permute(0, 2, 3, 1).contiguous().to(dev), 0)
    fr = leaf(f)
    vr = ops_ref.lpips_tap(fr[:N], fr[N:].detach(), w, mask).reshape(-1)
    gy = torch.randn(N, generator=g)
    val.backward(gy.to(dev)); vr.backward(gy)
    gref = fr.grad.clone()
    gref = gref * (f > 0)          # ReLU consumer contract: the tap masks its own gradient
    tol = {"fp32x3": 1e-5, "fp16": 2.5e-3, "f16x3": 1e-5}.get(prec, 2e-2)
    assert rel_err(val, vr) < tol
    assert rel_err(fd.grad, gref) < tol
    assert fd.grad[N:].abs().max().item() == 0.0


def _dropout_keep_mask(seed, N, H, W, C):
    """The tap kernels' counter-based Dropout(0.5) mask (csrc/loss_ops.hip dropout_bits8): one splitmix64 round per group of 8
    consecutive channels of the NHWC tensor, bit e of the result's high half = channel e of the group.  -> [N,H,W,C] of {0, 2}."""
    import numpy as np
    groups = np.arange(N * H * W * C // 8, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + groups * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    hi = (z >> np.uint64(32)).astype(np.uint32)
    bits = (hi[:, None] >> np.arange(8, dtype=np.uint32)[None, :]) & np.uint32(1)
    return torch.from_numpy((bits.astype(np.float32) * 2.0).reshape(N, H, W, C))


@pytest.mark.parametrize("prec,C,H", [("fp32x3", 64, 8), ("fp16", 256, 6), ("bf16", 512, 4)])
def test_lpips_tap_dropout_from_the_seed(backend, prec, C, H):
    """LPIPS in train mode (the reference's default, SURVEY F3: nn.Dropout(0.5) in front of every lin layer, utils.py:76-89):
    the kernels draw the keep mask themselves from (seed, element index).  The mask is Bernoulli(0.5), and forward AND backward
    equal the explicit-mask path fed with the same mask (the hash restated in numpy above) — bit for bit."""
    P = ops._PRECISIONS[prec]
    N, seed = 2, 0x1234567890ABCDEF
    g = torch.Generator().manual_seed(C + 1)
    f = torch.randn(2 * N, C, H, H, generator=g).relu()
    w = torch.rand(C, generator=g)
    dev = backend.device
    mask = _dropout_keep_mask(seed, N, H, H, C)              # NHWC; C is a multiple of 8: no channel padding
    assert abs(mask.mean().item() - 1.0) < 0.05 and set(mask.unique().tolist()) == {0.0, 2.0}
    outs = []
    for use_seed in (True, False):
        fd = leaf(f, dev)
        fh = ops.to_nhwc(fd, P)
        val = ops.lpips_tap(fh[:N], fh[N:].detach(), w.to(dev), None if use_seed else mask.to(dev), seed if use_seed else 0)
        val.backward(torch.ones(N, device=dev))
        outs.append((val.detach().cpu(), fd.grad.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # and dropout really drops: the value differs from the mask-free one
    fd = leaf(f, dev)
    fh = ops.to_nhwc(fd, P)
    plain = ops.lpips_tap(fh[:N], fh[N:].detach(), w.to(dev), None, 0)
    assert not torch.allclose(plain.detach().cpu(), outs[0][0], rtol=1e-3)


def test_gradnorm(backend):
    """vae_trainer.py:27-53 at world_size 1."""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 3, 8, 8, generator=g)
    xd = leaf(x, backend.device)
    y = ops.gradnorm(xd, 0.5)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy.to(backend.device))
    assert torch.equal(y.detach().cpu(), x)
    assert rel_err(xd.grad, ops_ref.gradnorm_backward(gy, 0.5)) < 1e-6


# ----------------------------------------------------------------------------- input preparation
@pytest.mark.parametrize("prec", ["bf16", "fp32", "fp16", "f16x3"])
def test_wavelet_front_end(backend, prec):
    """utils.py:229-247 vs the oracle restatement: NHWC (padded to 16 channels) and NCHW outputs."""
    from oracle import ops_ref as R
    x = W.image_batch(2, 16, seed=31)
    x[:, :, :, 8:] *= 0.25                                            # not symmetric
    want = R.wavelet_transform(x)
    got = vq.ops.wavelet_nchw(x.to(backend.device))
    assert rel_err(got, want) < 1e-6
    y = vq.ops.wavelet_to_nhwc(x.to(backend.device), prec)
    assert tuple(y.shape) == (2, 8, 8, 16)
    if prec == "f16x3":                     # (torch cannot read the carrier dtype: through the layout kernel, all 16 channels)
        y = vq.ops.to_nchw(y, 16).permute(0, 2, 3, 1)
    assert float(y[..., 12:].abs().max()) == 0.0
    assert rel_err(y[..., :12].float().permute(0, 3, 1, 2), want) < {"bf16": 1e-2, "fp16": 1.5e-3}.get(prec, 1e-6)
    with pytest.raises(RuntimeError):
        vq.ops.wavelet_nchw(torch.zeros(1, 3, 5, 6, device=backend.device))


def test_flip_and_area_resize(backend):
    """torch.flip + latent sign flips (vae_trainer.py:567-575), its backward, and the integer-ratio area resize."""
    from oracle import ops_ref as R
    z = W.uniform_tensor((2, 6, 5, 7), 41)
    zd = z.to(backend.device).requires_grad_()
    y = vq.ops.flip_nchw(zd, flip_w=True, negate_channels=(2, 4))
    want = torch.flip(z, [-1]).clone(); want[:, 2:4] = -want[:, 2:4]
    assert torch.equal(y.detach().cpu(), want)
    g = W.uniform_tensor((2, 6, 5, 7), 42)
    y.backward(g.to(backend.device))
    gw = torch.flip(g, [-1]).clone(); gw[:, 2:4] = -gw[:, 2:4]
    assert torch.equal(zd.grad.cpu(), gw)
    y2 = vq.ops.flip_nchw(z.to(backend.device), flip_h=True, flip_w=True)
    assert torch.equal(y2.cpu(), torch.flip(z, [-2, -1]))
    img = W.image_batch(2, 32, seed=43)
    for size in ((16, 16), (8, 8), (32, 32)):
        assert rel_err(vq.ops.area_downsample(img.to(backend.device), size), R.area_resize(img, size)) < 1e-6
    with pytest.raises(NotImplementedError):
        vq.ops.area_downsample(img.to(backend.device), (24, 24))


@pytest.mark.parametrize("prec,n,t_hw,c,hd", [("fp32", 2, (6, 5), 128, 64), ("bf16", 1, (20, 17), 64, 64), ("fp32", 1, (1, 1), 64, 64),
                                              ("fp32", 1, (7, 6), 64, 8), ("bf16", 2, (9, 4), 128, 16), ("fp32", 1, (5, 8), 256, 32)])
def test_attention_kernels(backend, prec, n, t_hw, c, hd):
    """vq_attention_fwd/_bwd vs F.scaled_dot_product_attention with the head split of ae.py:79-90 (64 channels per head) and of
    tae.py:17-53 (8 heads of C/8 channels); T = 340 spans two query blocks and a ragged last key tile."""
    h, w = t_hw
    dt = torch.bfloat16 if prec == "bf16" else torch.float32
    qkv = (W.uniform_tensor((n, h, w, 3 * c), 71, -2, 2)).to(dt)
    g = W.uniform_tensor((n, h, w, c), 72)
    qd = qkv.clone().to(backend.device).requires_grad_()
    out = vq.ops.attention(qd, hd)
    out.backward(g.to(backend.device).to(dt))
    qr = qkv.float().clone().requires_grad_()
    q, k, v = (t.reshape(n, h * w, c // hd, hd).transpose(1, 2) for t in qr.split(c, dim=-1))
    ref = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(n, h, w, c)
    ref.backward(g.to(dt).float())
    tol = 2e-2 if prec == "bf16" else 2e-5
    assert rel_err(out, ref) < tol
    assert rel_err(qd.grad, qr.grad) < tol
    with pytest.raises(RuntimeError):
        vq.ops.attention(torch.zeros(1, 2, 2, 96, device=backend.device))      # 32 channels per q/k/v: not a multiple of 64
    with pytest.raises(RuntimeError):
        vq.ops.attention(torch.zeros(1, 2, 2, 3 * 48, device=backend.device), 24)   # unsupported head width


# ----------------------------------------------------------------------------- full-size, size-independent properties
FULL_SIZE_LAYERS = [   # (Cin, Cout, H_in, k, stride, up) at the per-GPU batch of BASELINE configs[1..3] (B = 16, 256x256 images)
    (128, 128, 256, 3, 1, 1),      # encoder level 0 / decoder level 0 ResnetBlock convs
    (256, 256, 128, 3, 1, 1),
    (512, 512, 64, 3, 1, 1),
    (512, 512, 32, 3, 1, 1),
    (256, 256, 128, 3, 1, 2),      # decoder Upsample conv (256 -> 256 @ 256x256 output): the most expensive layer
    (128, 128, 256, 3, 2, 1),      # encoder Downsample
    (256, 128, 256, 1, 1, 1),      # nin_shortcut
    (3, 128, 256, 3, 1, 1), (128, 3, 256, 3, 1, 1), (64, 32, 256, 4, 4, 1),    # image layers, discriminator patch head
    (64, 64, 256, 3, 1, 1),        # VGG conv1_2: the 64-row nine-tap tile (utils.py:102-111)
    (512, 512, 16, 3, 1, 1),       # VGG conv5_x: 16 x 16 images, the small-M tiles
    (512, 512, 64, 3, 1, 2),       # decoder Upsample conv 512 -> 512 @ 128x128: sub-pixel forward over the staged patch
]


@pytest.mark.gpu
@pytest.mark.parametrize("layer", FULL_SIZE_LAYERS, ids=lambda c: "-".join(map(str, c)))
def test_conv_layers_at_full_size_match_the_oracle(hip_library, layer):
    """The benchmark's real layer shapes (B = 16, 256x256 images) against the CPU fp32 oracle — F.conv2d and its autograd on
    the GPU box's host cores, a few seconds per layer — in the two timed arithmetics: bf16 operands (decoder) and binary16
    operands (encoder / LPIPS / discriminator of the "ref" policy).  Forward, data, weight and bias gradients."""
    from conftest import Backend
    vq._lib._set_library_for_tests(hip_library)
    vq.ops.clear_caches()
    try:
        ci, co, h, k, stride, up = layer
        B = 16 if ci * co * h * h <= 128 * 128 * 256 * 256 else 8
        dev = torch.device("cuda:0")
        g = torch.Generator().manual_seed(ci * 7 + co)
        x = torch.randn(B, ci, h, h, generator=g)
        w = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
        b = torch.randn(co, generator=g)
        pad = k // 2 if stride == 1 else 0
        torch.set_num_threads(min(64, os.cpu_count() or 8))
        xr, wr, br = (leaf(t) for t in (x, w, b))
        if up == 2:
            yr = ops_ref.upsample(xr, wr, br)
        elif stride == 2 and k == 3:
            yr = ops_ref.downsample(xr, wr, br)
        else:
            yr = ops_ref.conv2d(xr, wr, br, stride=stride, padding=pad)
        gy = torch.randn(yr.shape, generator=g)
        yr.backward(gy)
        out_hw = (h // 2, h // 2) if (stride == 2 and k == 3) else None
        for prec in ("bf16", "fp16", "f16x3"):
            P = ops._PRECISIONS[prec]
            xd, wd, bd = (leaf(t, dev) for t in (x, w, b))
            y = ops.to_nchw(ops.conv2d(ops.to_nhwc(xd, P), wd, bd, stride=stride, pad=(pad, pad), up=up, split=1, out_hw=out_hw), co)
            y.backward(gy.to(dev))
            tol = TOL[prec]
            errs = [rel_err(y, yr), rel_err(xd.grad, xr.grad), rel_err(wd.grad, wr.grad), rel_err(bd.grad, br.grad)]
            # the weight / bias gradients sum B * H * W products: their rounding errors average out further
            assert all(e < tol for e in errs), (prec, errs)
            del xd, wd, bd, y
    finally:
        vq._lib._set_library_for_tests(None)
        vq.ops.clear_caches()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["bf16", "fp16", "f16x3"])
@pytest.mark.parametrize("ci,co,h", [(128, 128, 256), (256, 256, 128), (512, 256, 128)])
def test_conv_epilogue_bias_residual_and_groupnorm_partials_at_full_size(hip_library, prec, ci, co, h):
    """A ResnetBlock's conv2 at the benchmark's size with EVERYTHING its epilogue carries at once — bias, the block's residual
    (ae.py:140), and the GroupNorm statistics of the sum for the next block's norm1 (ae.py:131) — against the fp32 oracle:
    y = conv(x) + b + res, and mean / rstd of y per (image, group) as F.group_norm would compute them."""
    vq._lib._set_library_for_tests(hip_library)
    vq.ops.clear_caches()
    try:
        B, dev, G, eps = 8, torch.device("cuda:0"), 32, 1e-6
        g = torch.Generator().manual_seed(ci + co)
        x = torch.randn(B, ci, h, h, generator=g)
        w = torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5
        b = torch.randn(co, generator=g)
        res = torch.randn(B, co, h, h, generator=g)
        torch.set_num_threads(min(64, os.cpu_count() or 8))
        want = F.conv2d(x, w, b, padding=1) + res
        P = ops._PRECISIONS[prec]
        xh, rh = ops.to_nhwc(x.to(dev), P), ops.to_nhwc(res.to(dev), P)
        y = ops.conv_fwd_raw(xh, w.to(dev), b.to(dev), rh, 1, 1, 1, 1, False, 1, None, gn=(G, eps))
        assert rel_err(ops.to_nchw(y, co), want) < TOL[prec]
        stats = getattr(y, "_vq_gn", None)
        assert stats is not None, "this layer's kernel must deliver the GroupNorm partials"
        yg = want.reshape(B, G, -1).double()
        mean, var = yg.mean(-1), yg.var(-1, unbiased=False)
        assert rel_err(stats[0][0].reshape(B, G), mean.float()) < 2e-3 + TOL[prec] * 0.1
        assert rel_err(stats[0][1].reshape(B, G), (1.0 / (var + eps).sqrt()).float()) < 2e-3
    finally:
        vq._lib._set_library_for_tests(None)
        vq.ops.clear_caches()


@pytest.mark.gpu
@pytest.mark.parametrize("layer", FULL_SIZE_LAYERS, ids=lambda c: "-".join(map(str, c)))
def test_conv_adjoint_identities_at_full_size(hip_library, layer):
    """At the benchmark's real layer sizes the CPU oracle is out of reach; the three convolution kernels of a layer are
    instead tied together by the adjoint identities  <conv(x), g> = <x, dgrad(g)> = <w, wgrad(x, g)>  (+ <b, dbias>),
    and wgrad by batch additivity — properties that hold at any size.  bf16 storage, fp32 dot products."""
    from conftest import Backend
    vq._lib._set_library_for_tests(hip_library)
    vq.ops.clear_caches()
    try:
        ci, co, h, k, stride, up = layer
        B, dev = 16, torch.device("cuda:0")
        gen = torch.Generator(device=dev).manual_seed(7)
        cin_p, pad = vq.ops.pad8(ci), (k // 2 if stride == 1 else 0)
        x = torch.zeros(B, h, h, cin_p, device=dev)
        x[..., :ci] = torch.rand(B, h, h, ci, device=dev, generator=gen) * 2 - 1
        x = x.to(torch.bfloat16)
        w = (torch.rand(co, ci, k, k, device=dev, generator=gen) * 2 - 1) / (ci * k * k) ** 0.5
        w = w.to(torch.bfloat16).float()                      # bf16-representable: forward and gradients see the same operand
        bias = torch.rand(co, device=dev, generator=gen) - 0.5
        out_hw = ((h - 2) // 2 + 1,) * 2 if (stride == 2 and k == 3) else None      # Downsample's asymmetric pad
        y = vq.ops.conv_fwd_raw(x, w, bias, None, stride, pad, pad, up, False, 1, out_hw)
        y0 = vq.ops.conv_fwd_raw(x, w, None, None, stride, pad, pad, up, False, 1, out_hw)
        g = torch.zeros_like(y)
        g[..., :co] = (torch.rand(y.shape[:3] + (co,), device=dev, generator=gen) * 2 - 1).to(torch.bfloat16)
        dx = vq.ops.conv_dgrad_raw(g, x, w, stride, pad, pad, up, 1, False)
        dw, db = vq.ops.conv_wgrad_raw(x, g, w, bias, stride, pad, pad, up, 1)
        dot = lambda a, b: (a.double() * b.double()).sum().item()      # noqa: E731
        lhs = dot(y0, g)                                       # y0 carries one bf16 rounding per element (zero-mean)
        scale = (dot(y0, y0) * dot(g, g)) ** 0.5
        assert abs(lhs - dot(x, dx)) < 2e-3 * scale, (lhs, dot(x, dx), scale)
        assert abs(lhs - dot(w, dw)) < 2e-3 * scale, (lhs, dot(w, dw), scale)
        assert abs((dot(y, g) - lhs) - dot(bias, db)) < 2e-3 * scale
        # batch additivity of the weight gradient (different split-K plans, same sum)
        dwa, dba = vq.ops.conv_wgrad_raw(x[:8].contiguous(), g[:8].contiguous(), w, bias, stride, pad, pad, up, 1)
        dwb, dbb = vq.ops.conv_wgrad_raw(x[8:].contiguous(), g[8:].contiguous(), w, bias, stride, pad, pad, up, 1)
        assert rel_err(dwa + dwb, dw) < 1e-3 and rel_err(dba + dbb, db) < 1e-3
    finally:
        vq._lib._set_library_for_tests(None)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(16, 256, 256, 128), (16, 128, 128, 256), (16, 32, 32, 512),
                                   (1, 48 * 256, 256, 64)], ids=str)      # last: one TVAE video sample (T*H = 12288 rows, tae.py:303)
def test_groupnorm_properties_at_full_size(hip_library, shape):
    """GroupNorm at the benchmark's tensor sizes: with gamma = 1, beta = 0 every (image, group) of the output has mean 0 and
    variance 1, and the input gradient is orthogonal to both 1 and x-hat inside every group (the two projections the
    backward removes) — checked in fp64 on the fp32-storage path."""
    vq._lib._set_library_for_tests(hip_library)
    try:
        n, h, w, c = shape
        dev = torch.device("cuda:0")
        gen = torch.Generator(device=dev).manual_seed(3)
        x = torch.randn(n, h, w, c, device=dev, generator=gen) * 1.7 + 0.3
        dy = torch.randn(n, h, w, c, device=dev, generator=gen)
        gamma, beta = torch.ones(c, device=dev), torch.zeros(c, device=dev)
        y, stats = vq.ops.gn_fwd_raw(x, gamma, beta, 32, 1e-6, False)
        yg = y.double().reshape(n, h * w, 32, c // 32)
        assert yg.mean(dim=(1, 3)).abs().max().item() < 1e-4
        assert (yg.var(dim=(1, 3), unbiased=False) - 1).abs().max().item() < 1e-3
        dx, dg, db = vq.ops.gn_bwd_raw(x, dy, stats, gamma, beta, 32, False)
        dxg = dx.double().reshape(n, h * w, 32, c // 32)
        scale = dxg.abs().mean().item() * h * w * (c // 32)
        assert dxg.sum(dim=(1, 3)).abs().max().item() < 1e-4 * scale
        assert (dxg * yg).sum(dim=(1, 3)).abs().max().item() < 1e-4 * scale
        assert rel_err(db, dy.double().sum(dim=(0, 1, 2)).float()) < 1e-4
        assert rel_err(dg, (dy.double() * y.double()).sum(dim=(0, 1, 2)).float()) < 1e-4
    finally:
        vq._lib._set_library_for_tests(None)


def _random_conv_cases(n, seed):
    """Seeded shape fuzz across every dispatch boundary of the bf16 conv kernels: channel counts on both sides of 8 / 32 / 64 /
    128 / 256, image rows of 1..40 pixels (powers of two and not), 1x1 / 3x3 / patch kernels, stride 2, the 2x upsample."""
    import random
    rng = random.Random(seed)
    cases = []
    chans = [3, 8, 16, 24, 32, 40, 64, 72, 96, 128, 136, 192, 256, 264]
    while len(cases) < n:
        kind = rng.choice(["k3", "k3", "k3", "k1", "down", "up", "patch"])
        ci, co = rng.choice(chans), rng.choice(chans)
        nimg = rng.choice([1, 1, 2, 3])
        h, w = rng.choice([1, 2, 3, 4, 5, 8, 9, 16]), rng.choice([1, 2, 4, 7, 8, 16, 17, 32, 40])
        if ci * co * h * w * nimg > 2_500_000:         # keep the emulated MFMA work small
            continue
        relu = rng.random() < 0.3
        if kind == "k3":
            cases.append(("bf16", nimg, h, w, ci, co, 3, 1, 1, 1, relu, None))
        elif kind == "k1":
            cases.append(("bf16", nimg, h, w, ci, co, 1, 1, 0, 1, relu, None))
        elif kind == "down" and h >= 2 and w >= 2:
            cases.append(("bf16", nimg, h, w, ci, co, 3, 2, 0, 1, False, ((h - 2) // 2 + 1, (w - 2) // 2 + 1)))
        elif kind == "up" and h * w <= 160:
            cases.append(("bf16", nimg, h, w, ci, co, 3, 1, 1, 2, False, None))
        elif kind == "patch":
            k = rng.choice([2, 4])
            if h % k == 0 and w % k == 0:
                cases.append(("bf16", nimg, h, w, ci, co, k, k, 0, 1, False, None))
    return cases


@pytest.mark.parametrize("case", _random_conv_cases(36, seed=20260925), ids=lambda c: "-".join(map(str, c)))
def test_conv_shape_fuzz(backend, case):
    _conv_case(backend, case)


@pytest.mark.parametrize("prec_name,Ci,Co,hw,k", [("bf16", 64, 128, 16, 3), ("fp16", 128, 128, 16, 3), ("bf16", 64, 256, 16, 1),
                                                 ("bf16", 64, 512, 16, 1), ("bf16", 128, 128, 32, 3), ("bf16", 256, 512, 32, 3),
                                                 ("bf16", 64, 256, 16, 3),      # the 8-wave 256-pixel tiles (knob 3)
                                                 ("f16x3", 64, 128, 16, 3), ("f16x3", 32, 256, 16, 3), ("f16x3", 16, 128, 16, 1)])
def test_groupnorm_statistics_from_the_conv_epilogue(backend, prec_name, Ci, Co, hw, k):
    """The epilogue of a convolution that feeds an FP32GroupNorm reduces that norm's statistics from its fp32 accumulators
    (vq_conv2d_fwd gn_partials + vq_gn_stats_finalize); they must equal the separate statistics pass over the stored tensor up
    to the storage rounding, the normalised output must match, and with the knob off nothing rides on the tensor."""
    big_tile = (Ci, Co, hw, k) in ((64, 256, 16, 3), (32, 256, 16, 3))
    with hinted(conv=3 if big_tile else 0):             # 3: the patch-staged 256 x 256 tile at a small shape, 8 partial rows per tile
        _gn_epilogue_case(backend, prec_name, Ci, Co, hw, k)


@pytest.mark.parametrize("Ci,Co,k,offset", [(64, 128, 3, 100.0), (32, 256, 3, 300.0), (16, 128, 1, -300.0), (64, 1024, 1, 1000.0)])
def test_groupnorm_statistics_from_the_conv_epilogue_on_offset_outputs(backend, Ci, Co, k, offset):
    """The same statistics when the conv's bias puts a large DC on its output (|mean| / std of 40 ... 400 per group): the epilogue's
    partial rows are moments about one of the row's own values, merged Chan-style (gn_silu.hip header) — rstd to 2e-5 of the fp64
    definition on the stored tensor (a one-pass sum of squares: 1e-3 ... 1e-1 here).  4 / 8 / 32 channels per group, both epilogue tiles."""
    with hinted(conv=3 if Co == 256 else 0):
        _gn_epilogue_case(backend, "f16x3", Ci, Co, 16, k, offset=offset, rstd_tol=2e-5)


def _gn_epilogue_case(backend, prec_name, Ci, Co, hw, k, offset=0.0, rstd_tol=2e-3):
    g = torch.Generator().manual_seed(11)
    N, G, eps = 2, 32, 1e-6
    P = ops.BF16 if prec_name == "bf16" else (ops.f16x3_region("test", grad_scale=256.0) if prec_name == "f16x3" else
                                              ops.fp16_region("test", grad_scale=256.0))
    dev = backend.device
    x = torch.randn(N, Ci, hw, hw, generator=g).to(dev)
    res = (torch.randn(N, Co, hw, hw, generator=g) * 2 + 0.5).to(dev)
    w = (torch.randn(Co, Ci, k, k, generator=g) / (Ci * k * k) ** 0.5).to(dev)
    b = (torch.randn(Co, generator=g) + offset).to(dev)
    gw, gb = torch.randn(Co, generator=g).to(dev), torch.randn(Co, generator=g).to(dev)
    outs = {}
    for fused in (True, False):
        ops.set_gn_fusion(fused)
        try:
            with ops.region(P), torch.no_grad():
                y = ops.conv2d(ops.to_nhwc(x, P), w, b, residual=ops.to_nhwc(res, P), stride=1, pad=(k // 2, k // 2), split=1,
                               gn=(G, eps))
                riding = getattr(y, "_vq_gn", None)
                a, st = ops.gn_fwd_raw(y, gw, gb, G, eps, True)
        finally:
            ops.set_gn_fusion(True)
        assert (riding is not None) == fused, "the statistics ride on the tensor exactly when the fusion is on"
        if fused:
            assert st is riding[0] or st.data_ptr() == riding[0].data_ptr()
        if prec_name == "f16x3":           # (torch cannot read the carrier dtype: through the layout kernel)
            y, a = ops.to_nchw(y, Co).permute(0, 2, 3, 1), ops.to_nchw(a, Co).permute(0, 2, 3, 1)
        outs[fused] = (y.float().cpu(), st.float().cpu(), a.float().cpu())
    assert torch.equal(outs[True][0], outs[False][0])
    mean_f, rstd_f = outs[True][1]
    mean_s, rstd_s = outs[False][1]
    # storage rounding of y (2^-9 relative for bf16, 2^-11 for fp16) averages out over the Cg*HW elements of a group
    assert (mean_f - mean_s).abs().max() < 2e-3 * outs[True][0].abs().max()
    assert ((rstd_f - rstd_s).abs() / rstd_s).max() < rstd_tol
    assert rel_err(outs[True][2], outs[False][2]) < (8e-3 if prec_name == "bf16" else 2e-3)   # one storage ulp where a rounding flips
    # and against the definition, in fp64 on the stored tensor
    yv = outs[True][0].double().reshape(N, hw * hw, G, Co // G)
    mean = yv.mean(dim=(1, 3)).reshape(-1)
    rstd = (yv.var(dim=(1, 3), unbiased=False) + eps).rsqrt().reshape(-1)
    assert (mean_f.double() - mean).abs().max() < 2e-3 * outs[True][0].abs().max()
    assert ((rstd_f.double() - rstd).abs() / rstd).max() < rstd_tol
    assert ((rstd_s.double() - rstd).abs() / rstd).max() < rstd_tol


@pytest.mark.parametrize("Co,Ci,k", [(512, 512, 3), (128, 128, 3), (128, 64, 1)])
def test_wgrad_split_reduction_accumulates_in_place(backend, Co, Ci, k):
    """The three split-K reductions (nine taps per thread for large 3x3 weights, 16 B/lane per tap, 4 B/lane) write
    dw = alpha * sum(splits) or add it to what dw holds (gradient sinks): both forms, same partial sums."""
    import ctypes as C
    from vqgan_training_amd._lib import ptr, stream_of, dtype_code, workspace
    g = torch.Generator().manual_seed(5)
    dev, N, H = backend.device, 2, (8 if Co == 512 else 16)
    x = torch.randn(N, H, H, Ci, generator=g).to(torch.bfloat16).to(dev)
    dy = torch.randn(N, H, H, Co, generator=g).to(torch.bfloat16).to(dev)
    L = backend.library
    d = ops._desc(N, H, H, Ci, H, H, Co, Ci, Co, k, k, 1, 1, 1, k // 2, k // 2, dtype_code(x), 1, False)
    ws = workspace(dev, L.size("vq_conv2d_wgrad_workspace", C.byref(d)))
    dw = torch.empty(Co, Ci, k, k, device=dev)
    db = torch.empty(Co, device=dev)
    L.call("vq_conv2d_wgrad", C.byref(d), ptr(x), ptr(dy), ptr(dw), ptr(db), 0, ptr(ws), ws.numel(), stream_of(x))
    want = torch.einsum("nhwo,nhwkli->oikl", dy.float().cpu(),
                        F.pad(x.float().cpu(), (0, 0, k // 2, k // 2, k // 2, k // 2)).unfold(1, k, 1).unfold(2, k, 1).permute(0, 1, 2, 4, 5, 3))
    assert rel_err(dw, want) < 1e-4
    base = torch.randn(Co, Ci, k, k, generator=g).to(dev)
    acc, accb = base.clone(), torch.ones(Co, device=dev)
    L.call("vq_conv2d_wgrad", C.byref(d), ptr(x), ptr(dy), ptr(acc), ptr(accb), 1, ptr(ws), ws.numel(), stream_of(x))
    assert torch.allclose(acc.cpu(), (base + dw).cpu(), rtol=0, atol=1e-5 * float(dw.abs().max()))
    assert torch.allclose(accb.cpu(), (1 + db).cpu(), rtol=0, atol=1e-5 * float(db.abs().max()))


@pytest.mark.parametrize("case", [("bf16", 2, 16, 32, 128, 256, 3, 1, 1, 1, True, None), ("fp16", 1, 32, 16, 64, 256, 3, 1, 1, 1, False, None),
                                  ("bf16", 3, 16, 16, 192, 512, 3, 1, 1, 1, False, None), ("bf16", 1, 8, 16, 128, 256, 3, 1, 1, 2, False, None),
                                  # the sub-pixel Upsample forward over the staged patch (S = 2: four 2x2 taps moved by the block's phase,
                                  # two patch pieces per tap slot, depth-to-space store): low resolution 16 x 32, 2 chunks, ReLU / plain
                                  ("bf16", 2, 16, 32, 128, 256, 3, 1, 1, 2, True, None), ("fp16", 1, 16, 16, 64, 512, 3, 1, 1, 2, False, None),
                                  ("f16x3", 1, 32, 16, 64, 256, 3, 1, 1, 1, True, None), ("f16x3", 1, 16, 16, 32, 512, 3, 1, 1, 2, False, None)],
                         ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("dbg", [0, 512])
def test_patch_staged_256_tile(backend, case, dbg):
    """conv_igemm_p9_kernel: the 256 x 256 tile with its pixels staged as a 16 x 16 patch + halo once per 64-channel chunk for all
    nine taps (weights per (chunk, tap) through LDS, ping-pong schedule); dbg 512 = the one-tap form it replaces.  Forced with
    tile knob 3 at emulator-sized shapes: several patches per image, 1-3 channel chunks, image borders on every side of a patch,
    ReLU / residual-free epilogues, the nearest-2x gather, forward + both gradients (the data gradient of the first three cases
    runs the same kernel with Cout = Cin of the layer: a partial 256-row tile)."""
    with hinted(conv=3 + (dbg << 4)):
        _conv_case(backend, case)


def test_wgrad_three_tap_kernel_with_tile_owning_xcds(backend):
    """conv_wgrad3_kernel's second block -> (tile, split) map: with a multiple of 8 tiles an XCD can own tiles / 8 tiles and ALL
    their pixel splits, so split counts that are not multiples of 8 still load the XCDs evenly (the plan picks 5 splits for the
    512-channel 32x32 layers: 240 blocks in one round instead of 384 in one and a half).  Forced here at emulator size: 256 x 512
    channels = 24 tiles, 2 and 3 splits, against the default map and the fp32 reference."""
    import ctypes as C
    from vqgan_training_amd._lib import ptr, stream_of, dtype_code, workspace
    g = torch.Generator().manual_seed(21)
    dev, N, H, Co, Ci = backend.device, 3, 16, 256, 512
    x = torch.randn(N, H, H, Ci, generator=g).to(torch.bfloat16).to(dev)
    dy = torch.randn(N, H, H, Co, generator=g).to(torch.bfloat16).to(dev)
    L = backend.library
    want = torch.einsum("nhwo,nhwkli->oikl", dy.float().cpu(),
                        F.pad(x.float().cpu(), (0, 0, 1, 1, 1, 1)).unfold(1, 3, 1).unfold(2, 3, 1).permute(0, 1, 2, 4, 5, 3))
    outs = []
    for forced in (0, 2, 3):                       # 768 pixels: at most 2 splits of >= 512 pixels -> 3 is clamped to 2
        with ops.kernel_hints(wgrad=forced << 16):     # bits 16.. of the hint: forced split-K count
            d = ops._desc(N, H, H, Ci, H, H, Co, Ci, Co, 3, 3, 1, 1, 1, 1, 1, dtype_code(x), 1, False, wgrad=True)
        ws = workspace(dev, L.size("vq_conv2d_wgrad_workspace", C.byref(d)))
        dw, db = torch.empty(Co, Ci, 3, 3, device=dev), torch.empty(Co, device=dev)
        L.call("vq_conv2d_wgrad", C.byref(d), ptr(x), ptr(dy), ptr(dw), ptr(db), 0, ptr(ws), ws.numel(), stream_of(x))
        assert rel_err(dw, want) < 1e-4 and rel_err(db, dy.float().sum(dim=(0, 1, 2)).cpu()) < 1e-5, forced
        outs.append(dw.cpu())
    assert torch.allclose(outs[0], outs[1], rtol=0, atol=1e-4 * float(want.abs().max()))
