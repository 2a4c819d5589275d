"""The nine-tap 128-channel x 256-pixel tile (one 16 x 16 patch, 2 x 2 waves of 64c x 128p, one halo buffer): forced through
kernel_hint dbg 80 at the smallest shapes at which it can go wrong, against oracle/ops_ref.py in float64 at test_kernels.py's
bf16 / fp16 tolerances, and — the K walk is the 128 x 128 tile's — bit for bit against that tile (dbg 88).

Runs on the host emulator and on a real MI355X like tests/test_kernels.py.
"""
import ctypes as C

import pytest
import torch

import vqgan_training_amd as vq
from vqgan_training_amd import ops
from oracle import ops_ref

TOL = {"bf16": 2e-2, "fp16": 2.5e-3}          # tests/test_kernels.py::TOL
WIDE = (80 << 4) | 5                           # the 128 x 256 tile wherever the shape admits it
NARROW = (88 << 4) | 5                         # the 128 x 128 nine-tap tile in the same places


def _prec(name):
    return ops.BF16 if name == "bf16" else ops.fp16_region("tap9_wide", grad_scale=256.0)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / max(b.abs().max().item(), 1e-12)).item()


def _nhwc(t, P, dev):
    with torch.no_grad():
        return ops.to_nhwc(t.to(dev), P)


def _fwd(hint, P, x, w, bias=None, residual=None, mask=None, up=1):
    """vq_conv2d_fwd of a 3x3 / stride 1 / pad 1 conv (behind the nearest-2x gather for up = 2) with every epilogue operand the
    entry point takes; x / residual / mask are NHWC storage tensors.  Returns the NHWC output."""
    n, h, wd, cin = x.shape
    co_w, ci_w = w.shape[:2]
    cout = ops.pad8(co_w)
    ho, wo = h * up, wd * up
    y = torch.empty((n, ho, wo, cout), dtype=x.dtype, device=x.device)
    with ops.kernel_hints(conv=hint), ops.region(P):
        d = ops._desc(n, h, wd, cin, ho, wo, cout, ci_w, co_w, 3, 3, 1, 1, up, 1, 1, ops.dtype_code(x), 1, False)
        wp, sc = ops._packed(w, "fwd", cout, cin, 1, d, ops._op(x))
        d.alpha_dev = ops._adev(sc)
        vq._lib.lib().call("vq_conv2d_fwd", C.byref(d), ops.ptr(x), ops.ptr(wp), ops.ptr(bias), ops.ptr(residual), ops.ptr(mask),
                           ops.ptr(y), None, 0, ops.stream_of(x))
    return y


def _case(seed, n, h, w, ci, co):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, ci, h, w, generator=g)
    wt = torch.randn(co, ci, 3, 3, generator=g) / (ci * 9) ** 0.5
    return g, x, wt


FORWARD = [
    # N, H, W, Cin, Cout, up
    (1, 16, 16, 128, 128, 1),      # one patch: every halo edge is an image border
    (1, 32, 16, 64, 128, 1),       # a single 64-channel chunk: no buffer hand-over
    (1, 32, 16, 192, 128, 1),      # three chunks: an odd count through the hand-over
    (1, 16, 16, 128, 256, 1),      # two channel tiles
    (1, 8, 8, 128, 128, 2),        # the nearest-2x gather in the halo addresses
]


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", FORWARD, ids=lambda s: "x".join(map(str, s)))
def test_forward_matches_the_oracle_and_the_128_pixel_tile(backend, prec, shape):
    n, h, w, ci, co, up = shape
    P, dev = _prec(prec), backend.device
    _, x, wt = _case(sum(shape), n, h, w, ci, co)
    xh, wd = _nhwc(x, P, dev), wt.to(dev)
    y = _fwd(WIDE, P, xh, wd, up=up)
    y0 = _fwd(NARROW, P, xh, wd, up=up)
    ref = (ops_ref.upsample if up == 2 else lambda a, b, c: ops_ref.conv2d(a, b, c, stride=1, padding=1))(x.double(), wt.double(), None)
    err = _rel(ops.to_nchw(y, co), ref)
    print(f"tap9 wide forward {prec} {shape}: rel err {err:.3e} (bound {TOL[prec]:.1e})")
    assert err < TOL[prec]
    assert torch.equal(y, y0), "same K walk as the 128 x 128 tile: bit-identical outputs"


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_forward_with_bias_residual_and_relu_mask(backend, prec):
    """2 x 16 x 32: an interior patch edge (the halo's right / left columns hold the neighbour patch) and a patch that starts a new
    image (its top halo row is padding, not the previous image's last row)."""
    n, h, w, ci, co = 2, 16, 32, 128, 128
    P, dev = _prec(prec), backend.device
    g, x, wt = _case(7, n, h, w, ci, co)
    b = torch.randn(co, generator=g)
    res = torch.randn(n, co, h, w, generator=g)
    mask = torch.randn(n, co, h, w, generator=g).relu()
    xh, rh, mh = (_nhwc(t, P, dev) for t in (x, res, mask))
    y = _fwd(WIDE, P, xh, wt.to(dev), b.to(dev), rh, mh)
    y0 = _fwd(NARROW, P, xh, wt.to(dev), b.to(dev), rh, mh)
    ref = ops_ref.conv2d(x.double(), wt.double(), b.double(), stride=1, padding=1) + res.double()
    ref = torch.where(mask > 0, ref, torch.zeros_like(ref))
    err = _rel(ops.to_nchw(y, co), ref)
    print(f"tap9 wide bias + residual + mask {prec}: rel err {err:.3e} (bound {TOL[prec]:.1e})")
    assert err < TOL[prec]
    assert torch.equal(y, y0)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_data_gradient(backend, prec):
    n, h, w, ci, co = 1, 16, 32, 128, 128
    P, dev = _prec(prec), backend.device
    g, x, wt = _case(11, n, h, w, ci, co)
    gy = torch.randn(n, co, h, w, generator=g)
    xh, gh, wd = _nhwc(x, P, dev), _nhwc(gy, P, dev), wt.to(dev)
    out = {}
    for hint in (WIDE, NARROW):
        with ops.kernel_hints(conv=hint), ops.region(P, backward=True), torch.no_grad():
            out[hint] = ops.conv_dgrad_raw(gh, xh, wd, 1, 1, 1, 1, 1, False)
    xr = x.double().requires_grad_()
    ops_ref.conv2d(xr, wt.double(), None, stride=1, padding=1).backward(gy.double())
    err = _rel(ops.to_nchw(out[WIDE], ci), xr.grad)
    print(f"tap9 wide data gradient {prec}: rel err {err:.3e} (bound {TOL[prec]:.1e})")
    assert err < TOL[prec]
    assert torch.equal(out[WIDE], out[NARROW])


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("nhw", [(1, 16, 32), (2, 32, 16)], ids=str)      # second shape: a lower patch row, a second image
def test_groupnorm_partials(backend, prec, nhw):
    """The tile writes the partial rows of the two 8 x 16 patches it covers (32 pixels per row, like the 128-pixel tile): mean / rstd
    after vq_gn_stats_finalize against vq_gn_stats on the same stored output, at the bounds of test_kernels.py::_gn_epilogue_case
    (mean 2e-3 of max|y|, rstd 2e-3 relative) — and bit for bit the statistics the 128-pixel tile delivers."""
    (n, h, w), ci, co, G, eps = nhw, 128, 128, 32, 1e-6
    P, dev = _prec(prec), backend.device
    g, x, wt = _case(13, n, h, w, ci, co)
    b = torch.randn(co, generator=g).to(dev)
    xh, wd = _nhwc(x, P, dev), wt.to(dev)
    gam, bet = torch.ones(co, device=dev), torch.zeros(co, device=dev)
    outs = {}
    for fused in (True, False):
        ops.set_gn_fusion(fused)
        try:
            with ops.kernel_hints(conv=WIDE), ops.region(P), torch.no_grad():
                y = ops.conv_fwd_raw(xh, wd, b, None, 1, 1, 1, 1, False, 1, None, gn=(G, eps))
                riding = getattr(y, "_vq_gn", None)
                _, st = ops.gn_fwd_raw(y, gam, bet, G, eps, False)
        finally:
            ops.set_gn_fusion(True)
        assert (riding is not None) == fused, "the forced tile must deliver the partials"
        outs[fused] = (y.float().cpu(), st.float().cpu())
    assert torch.equal(outs[True][0], outs[False][0])
    (mean_f, rstd_f), (mean_s, rstd_s) = outs[True][1], outs[False][1]
    dm = ((mean_f - mean_s).abs().max() / outs[True][0].abs().max()).item()
    dr = ((rstd_f - rstd_s).abs() / rstd_s).max().item()
    print(f"tap9 wide GroupNorm partials {prec}: mean {dm:.3e}, rstd {dr:.3e} (bounds 2e-3)")
    assert dm < 2e-3 and dr < 2e-3
    yv = outs[True][0].double().reshape(n, h * w, G, co // G)
    rstd = (yv.var(dim=(1, 3), unbiased=False) + eps).rsqrt().reshape(-1)
    assert ((rstd_f.double() - rstd).abs() / rstd).max() < 2e-3
    with ops.kernel_hints(conv=NARROW), ops.region(P), torch.no_grad():
        y0 = ops.conv_fwd_raw(xh, wd, b, None, 1, 1, 1, 1, False, 1, None, gn=(G, eps))
    assert torch.equal(y0.float().cpu(), outs[True][0]) and torch.equal(y0._vq_gn[0].float().cpu(), outs[True][1])


def _desc(n, hw, ci, co, hint=0):
    with ops.kernel_hints(conv=hint):
        return ops._desc(n, hw, hw, ci, hw, hw, co, ci, co, 3, 3, 1, 1, 1, 1, 1, ops.VQ_BF16, 1, False)


def test_gn_tile_follows_the_dispatch_rule(backend):
    """vq_conv2d_gn_tile is what Python sizes the partial buffer from.  The 4-wave 256-pixel tile writes the 32-pixel rows of the
    two 128-pixel tiles it covers, so that the statistics stay bit for bit what the 128-pixel tile gives: the answer is 32 where it
    runs (128 -> 128 @256^2 at B = 16, unhinted or forced), and unchanged where it does not (512 -> 512 @32^2)."""
    dll = vq._lib.lib().dll
    assert dll.vq_conv2d_gn_tile(C.byref(_desc(16, 256, 128, 128)), 32) == 32
    assert dll.vq_conv2d_gn_tile(C.byref(_desc(16, 256, 128, 128, WIDE)), 32) == 32
    assert dll.vq_conv2d_gn_tile(C.byref(_desc(16, 256, 128, 128, NARROW)), 32) == 32
    assert dll.vq_conv2d_gn_tile(C.byref(_desc(16, 32, 512, 512)), 32) == 32
    assert dll.vq_conv_weight_layout(C.byref(_desc(16, 256, 128, 128))) == 1


def test_fp16_range_events_of_a_loss_scaled_region(backend):
    """The epilogue's range-event counters (include/vqhip.h) through the 256-pixel tile: silent on a healthy launch, clipped
    stores and fully flushed waves counted."""
    dev = backend.device
    P = ops.fp16_region("tap9_wide_probe", 2.0 ** 12)
    P.events = torch.zeros(4, dtype=torch.int32, device=dev)

    def counts():
        c = P.events.tolist()
        P.events.zero_()
        return c[0], c[1]

    _, x, wt = _case(3, 1, 16, 16, 128, 128)
    xh, wd = _nhwc(x, P, dev), wt.to(dev)
    y = _fwd(WIDE, P, xh, wd)
    assert counts() == (0, 0), "a healthy forward must not touch the counters"
    ref = ops_ref.conv2d(x.double(), wt.double(), None, stride=1, padding=1)
    assert _rel(ops.to_nchw(y, 128), ref) < TOL["fp16"]
    big = _fwd(WIDE, P, (xh * 2000).to(torch.float16), (wd * 100).contiguous())            # |y| ~ 2e5
    sat, fl = counts()
    assert sat > 0 and fl == 0 and float(big.float().abs().max()) == 65504.0
    tiny = _fwd(WIDE, P, xh, (wd * 1e-9).contiguous())                                     # |y| ~ 1e-9 < 2^-24
    sat, fl = counts()
    assert sat == 0 and fl > 0 and float(tiny.float().abs().max()) == 0.0
