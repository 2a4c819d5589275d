"""Direct float64 checks of the non-convolution entry points of include/vqhip.h, through the C ABI, at the sizes where their launches
change shape: one block / two blocks / the block cap and the first grid-stride trip / a ragged tail, slot counts that do not divide a
block, tiles exactly full and one past, every storage type.  The whole-model tests bound a loss at 1e-4: one element dropped out of
three million, a partial row read twice or an fp64 finalize turned into fp32 moves none of them.

Two data regimes for every reduction:
  EXACT  small integers (exact in all four storage types, every fp32 partial sum below 2^24): any correct summation order gives the
         same bits, so the result must EQUAL the float64 result rounded once to fp32 (1 ulp where the kernel ends in an fp32 division).
         Fails when an element is dropped, read twice or taken from a neighbour.
  RANDOM torch.randn with a fixed seed against float64, under a bound DERIVED from the kernel's accumulation structure (stated at
         each test; u = 2^-24).  Fails on a precision regression.
Each test prints the worst error it measured; the figures in the docstrings are from one run of the emulator build and one run on an
MI355X.  `DIRECT` (below) maps every entry point of the header to the test that calls it by name.
"""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vqgan_training_amd import ops
from vqgan_training_amd._lib import VQ_BF16, VQ_F16, VQ_F16X2, VqAdamTensor, VqPackJob, dtype_code, lib, ptr, stream_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
VQ_ERR_INVALID, VQ_ERR_WORKSPACE = -1, -4
STORAGE = ["fp32", "f16x3", "fp16", "bf16"]                       # names of ops._PRECISIONS
HALF_ULP = {"fp32": 2.0 ** -24, "f16x3": 2.0 ** -22, "fp16": 2.0 ** -11, "bf16": 2.0 ** -8}

_E, _K, _M, _O, _Q, _H = ("tests/test_entry_points.py::", "tests/test_kernels.py::", "tests/test_model.py::", "tests/test_vq.py::",
                          "tests/test_vq_ema.py::", "tests/test_hw_layout.py::")
# entry point -> the test(s) that call it by name (or through a one-line ops wrapper); a pure query function may name the test of the
# call it sizes.  test_every_entry_point_names_its_direct_test keeps the keys equal to the header's declarations.
DIRECT = {
    "vq_last_error": ["tests/test_abi.py::test_error_contract_without_a_gpu"],
    "vq_abi_version": ["tests/test_abi.py::test_header_binding_and_library_agree"],
    "vq_conv_weight_layout": [_K + "test_conv_fwd_dgrad_wgrad"],
    "vq_packed_weight_elems": [_E + "test_repack_in_one_launch_equals_the_single_calls"],
    "vq_pack_weight_fwd": [_E + "test_repack_in_one_launch_equals_the_single_calls"],
    "vq_pack_weight_dgrad": [_E + "test_repack_in_one_launch_equals_the_single_calls"],
    "vq_pack_job": [_E + "test_repack_in_one_launch_equals_the_single_calls"],
    "vq_pack_job_blocks": [_E + "test_repack_in_one_launch_equals_the_single_calls"],
    "vq_pack_weights_multi": [_E + "test_repack_in_one_launch_equals_the_single_calls"],
    "vq_subpixel_weights": [_K + "test_subpixel_weights_and_equivalence"],
    "vq_subpixel_wgrad_fold": [_K + "test_subpixel_weights_and_equivalence"],
    "vq_attention_fwd": [_E + "test_attention_at_tile_and_block_boundaries", _K + "test_attention_kernels"],
    "vq_attention_workspace": [_E + "test_attention_at_tile_and_block_boundaries"],
    "vq_attention_bwd": [_E + "test_attention_at_tile_and_block_boundaries", _K + "test_attention_kernels"],
    "vq_wavelet_fwd": [_E + "test_wavelet_on_a_non_square_image", _K + "test_wavelet_front_end"],
    "vq_flip_nchw": [_E + "test_flip_at_size", _K + "test_flip_and_area_resize"],
    "vq_area_downsample_nchw": [_E + "test_area_downsample_at_size", _K + "test_flip_and_area_resize"],
    "vq_conv2d_fwd": [_K + "test_conv_fwd_dgrad_wgrad"],
    "vq_conv2d_gn_tile": [_K + "test_groupnorm_statistics_from_the_conv_epilogue"],
    "vq_conv2d_gnb_rows": [_K + "test_groupnorm_backward_sums_from_the_data_gradient_conv"],
    "vq_gn_stats_finalize": [_K + "test_groupnorm_statistics_from_the_conv_epilogue"],
    "vq_conv2d_wgrad_workspace": [_K + "test_conv_fwd_dgrad_wgrad"],
    "vq_conv2d_wgrad": [_K + "test_conv_fwd_dgrad_wgrad"],
    "vq_colsum_workspace": [_E + "test_colsum"],
    "vq_colsum": [_E + "test_colsum"],
    "vq_nchw_to_nhwc": [_E + "test_layout_round_trip_with_channel_padding"],
    "vq_nhwc_to_nchw": [_E + "test_layout_round_trip_with_channel_padding"],
    "vq_absmax": [_E + "test_absmax"],
    "vq_gn_workspace": [_K + "test_groupnorm_silu"],
    "vq_gn_stats": [_K + "test_groupnorm_silu", _K + "test_groupnorm_on_offset_activations"],
    "vq_gn_silu_fwd": [_K + "test_groupnorm_silu", _K + "test_groupnorm_on_offset_activations"],
    "vq_gn_silu_bwd": [_K + "test_groupnorm_silu", _K + "test_groupnorm_on_offset_activations"],
    "vq_maxpool2_fwd": [_E + "test_maxpool_on_odd_extents"],
    "vq_maxpool2_bwd": [_E + "test_maxpool_on_odd_extents"],
    "vq_sumpool2": [_E + "test_sumpool"],
    "vq_lpips_workspace": [_K + "test_lpips_tap"],
    "vq_lpips_tap_fwd": [_K + "test_lpips_tap", _K + "test_lpips_tap_dropout_from_the_seed"],
    "vq_lpips_tap_bwd": [_K + "test_lpips_tap", _K + "test_lpips_tap_dropout_from_the_seed"],
    "vq_moments": [_E + "test_moments"],
    "vq_l2norm": [_E + "test_l2norm_and_scale_by_norm"],
    "vq_scale_by_norm": [_E + "test_l2norm_and_scale_by_norm"],
    "vq_gan_disc_loss": [_E + "test_gan_disc_loss"],
    "vq_adamw_multi": [_E + "test_adamw_multi_through_the_abi"],
    "vq_scale": [_E + "test_scale"],
    "vq_vq_workspace": [_O + "test_indices_bit_exact_random"],
    "vq_vq_nearest_fwd": [_O + "test_indices_bit_exact_random", _O + "test_indices_ties_and_near_ties"],
    "vq_vq_scatter_workspace": [_O + "test_codebook_scatter_add_is_order_independent"],
    "vq_vq_scatter_add": [_O + "test_codebook_scatter_add_is_order_independent"],
    "vq_vq_ema_workspace": [_Q + "test_one_update_matches_the_restatement"],
    "vq_vq_ema_accumulate": [_Q + "test_one_update_matches_the_restatement"],
    "vq_vq_ema_update": [_Q + "test_one_update_matches_the_restatement"],
    "vq_vq_ema_reseed": [_Q + "test_reseeding_replaces_exactly_the_dead_codes_by_the_hashed_tokens"],
    "vq_debug_probe": [_H + "test_mfma_layout_matches_silicon", _H + "test_emulator_mfma_matches_matrix_product"],
}


def test_every_entry_point_names_its_direct_test():
    """A new declaration in include/vqhip.h fails here until someone says where it is tested; every named test must exist."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_abi import _header_functions
    assert sorted(DIRECT) == _header_functions(), (sorted(set(_header_functions()) - set(DIRECT)), sorted(set(DIRECT) - set(_header_functions())))
    sources = {}
    for name, ids in DIRECT.items():
        assert ids, name
        for nid in ids:
            path, test = nid.split("::")
            if path not in sources:
                sources[path] = open(os.path.join(ROOT, path)).read()
            assert re.search(rf"^def {test}\(", sources[path], flags=re.M), (name, nid)


# ----------------------------------------------------------------------------------------------- helpers
def f32(v):
    """A Python float (or a float64 tensor) rounded once to fp32."""
    if torch.is_tensor(v):
        return v.double().float()
    return float(np.float32(v))


def small_ints(shape, seed, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def store(x_nchw, prec, dev):
    """fp32 NCHW (CPU) -> the NHWC tensor of the storage type on `dev`, written by the project's own layout kernel."""
    return ops.to_nhwc(x_nchw.to(dev), ops._PRECISIONS[prec])


def load(y, c):
    """NHWC storage tensor -> fp32 NCHW on the CPU: the values a kernel reads from `y` (every storage type converts exactly)."""
    return ops.to_nchw(y, c).cpu()


def rows_to_nchw(x2d):
    """[pixels][C] -> the NCHW tensor whose NHWC form is that matrix."""
    p, c = x2d.shape
    return x2d.t().reshape(1, c, p, 1)


def max_rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


# ----------------------------------------------------------------------------------------------- 1. vq_l2norm, vq_scale_by_norm
def _gradnorm(dev, g, weight):
    L = lib()
    gd = g.to(dev)
    norm = torch.full((1,), -1.0, device=dev)
    scratch = torch.zeros(1024, device=dev)
    dx = torch.full_like(gd, float("nan"))
    s = stream_of(gd)
    L.call("vq_l2norm", ptr(gd), gd.numel(), ptr(norm), ptr(scratch), s)
    L.call("vq_scale_by_norm", ptr(gd), ptr(norm), weight, gd.numel(), ptr(dx), s)
    return norm.cpu().item(), dx.cpu()


@pytest.mark.parametrize("n", [1, 255, 2049, 524288 + 77, 1100003])
def test_l2norm_and_scale_by_norm(backend, n):
    """GradNorm's two kernels at one block, two blocks, the 256-block cap plus the first grid-stride trip, several trips with a ragged
    tail.  Structure: a lane adds k = ceil(n / (256 blocks)) squares in fp32, 6 shuffle levels and 3 adds join a block (~10 more
    roundings, all terms positive), the block partials are added and rooted in fp64:  |norm - ref| <= (k + 10) u |ref|.
    dx = g * (weight / (norm + 1e-8)): three more fp32 roundings, elementwise.
    Measured worst (norm, dx) relative error: emulator 6.0e-8, 1.2e-7; MI355X 6.0e-8, 1.2e-7 (bounds 6.6e-7 .. 1.6e-6, + 3 u for dx)."""
    blocks = max(1, min(256, -(-n // 2048)))
    k = -(-n // (256 * blocks))
    weight = 0.75
    # exact
    g = small_ints((n,), 100 + n)
    g[-1] = 8.0                                                    # the last element counts, and the norm is never zero
    norm, dx = _gradnorm(backend.device, g, weight)
    total = int((g.long() ** 2).sum())
    assert norm == f32(math.sqrt(total)), (n, norm, math.sqrt(total))
    # random
    g = randn((n,), 200 + n)
    norm, dx = _gradnorm(backend.device, g, weight)
    ref = g.double().pow(2).sum().sqrt().item()
    e_norm = abs(norm - ref) / ref
    want = weight * g.double() / (ref + 1e-8)
    e_dx = ((dx.double() - want).abs() / want.abs().clamp_min(1e-300)).max().item()
    print(f"l2norm n={n} blocks={blocks} k={k}: norm rel err {e_norm:.3e} (bound {(k + 10) * U:.3e}), dx rel err {e_dx:.3e}")
    assert e_norm <= (k + 10) * U
    assert e_dx <= (k + 10) * U + 3 * U
    # a zero gradient: 0 / 1e-8, not 0 / 0
    norm, dx = _gradnorm(backend.device, torch.zeros(n), weight)
    assert norm == 0.0 and torch.isfinite(dx).all() and (dx == 0).all()


# ----------------------------------------------------------------------------------------------- 2. vq_moments
def _moments(dev, x):
    xd = x.to(dev)
    out4 = torch.full((4,), float("nan"), device=dev)
    scratch = torch.zeros(1024 + 2, device=dev)
    rc = lib().dll.vq_moments(ptr(xd), xd.numel(), ptr(out4), C.c_void_p(scratch.data_ptr() + 4), stream_of(xd))
    assert rc == VQ_ERR_INVALID and "aligned" in lib().last_error()      # fp64 partial rows: a 4-byte offset is refused
    lib().call("vq_moments", ptr(xd), xd.numel(), ptr(out4), ptr(scratch), stream_of(xd))
    return out4.cpu()


@pytest.mark.parametrize("n,offset", [(1, 0), (2, 5), (2049, 0), (262144 + 5, 0), (600001, 1000)])
def test_moments(backend, n, offset):
    """out4 = {sum (|x| - mean|x|)^2, sum x^2, sum |x|, n}: one element, two, two blocks, the 128-block cap plus one grid-stride trip,
    and |mean| / std = 1000 over several trips.  Everything is accumulated in fp64, so each output is ONE fp32 rounding of an fp64 sum:
    within 2^-23 relative (a factor 2 on the rounding), out4[3] == n, and a single element has zero spread exactly.
    Measured worst relative error: emulator 4.8e-8; MI355X 4.8e-8."""
    # exact: integer data, integer sums; m2 = S2 - S1^2 / n as a rational, rounded once
    x = small_ints((n,), 300 + n) + offset
    out = _moments(backend.device, x)
    s1, s2 = int(x.long().abs().sum()), int((x.long() ** 2).sum())
    want = [f32(float(Fraction(s2) - Fraction(s1 * s1, n))), f32(s2), f32(s1), f32(n)]
    assert out.tolist() == want, (out.tolist(), want)
    # random
    x = randn((n,), 400 + n) + offset
    out = _moments(backend.device, x)
    a = x.double().abs()
    ref = [((a - a.mean()) ** 2).sum().item(), (a * a).sum().item(), a.sum().item()]
    errs = [abs(out[i].item() - ref[i]) / ref[i] if ref[i] else abs(out[i].item()) for i in range(3)]
    print(f"moments n={n} offset={offset}: rel err {errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e} (bound {2 * U:.3e})")
    assert max(errs) <= 2 * U
    assert out[3].item() == n
    if n == 1:
        assert out[0].item() == 0.0


# ----------------------------------------------------------------------------------------------- 3. vq_gan_disc_loss
SPECIAL_LOGITS = [0.0, -0.0, 1.0, -1.0, 30.0, -30.0, 100.0, -100.0, 1e4, -1e4]


def _disc_loss(dev, real, fake, disc_type, grads=True):
    r, f = real.to(dev), fake.to(dev)
    out6 = torch.full((6,), float("nan"), device=dev)
    dr = torch.full_like(r, float("nan")) if grads else None
    df = torch.full_like(f, float("nan")) if grads else None
    lib().call("vq_gan_disc_loss", ptr(r), ptr(f), r.numel(), disc_type, ptr(out6), ptr(dr), ptr(df), stream_of(r))
    return out6.cpu(), (dr.cpu() if grads else None), (df.cpu() if grads else None)


def _disc_loss_ref(real, fake, disc_type):
    r, f = real.double().requires_grad_(), fake.double().requires_grad_()
    if disc_type == 1:
        tr, tf = F.relu(1.0 - r), F.relu(1.0 + f)
    else:
        tr = F.binary_cross_entropy_with_logits(r, torch.ones_like(r), reduction="none")
        tf = F.binary_cross_entropy_with_logits(f, torch.zeros_like(f), reduction="none")
    (0.5 * (tr.mean() + tf.mean())).backward()
    correct = int((real > 0).sum()) + int((fake < 0).sum())
    return tr.detach(), tf.detach(), r.grad, f.grad, correct


@pytest.mark.parametrize("n", [1, 24, 257, 1000, 16384])
@pytest.mark.parametrize("disc_type", [0, 1], ids=["bce", "hinge"])
def test_gan_disc_loss(backend, disc_type, n):
    """vae_trainer.py:63-90 in one block: a lane walks ceil(n / 256) logits, 10 more roundings join the block, one fp32 division ends
    each mean:  |mean - ref| <= (ceil(n / 256) + 10) u mean|term|.  The first logits sit on the hinge kink, at +-0 (the strict > 0 /
    < 0 of the accuracy count) and far into the BCE tails, where exp under- / overflows and the sigmoid must still be 0 or 1.
    Hinge gradients are -+0.5 / n or 0 bit for bit; BCE gradients n |d - d_ref| <= 2e-6 (four ulp of the unit-range sigmoid: room
    for a one-ulp hardware exp2 and rcp).  Measured worst n |d - d_ref|: emulator 7.5e-8; MI355X 8.0e-8; worst mean error over its
    bound: emulator 0.19; MI355X 0.19."""
    if disc_type == 1:
        # exact: integer logits make every hinge term and every sum an integer; the mean is one fp32 division (1 ulp)
        real, fake = small_ints((n,), 700 + n), small_ints((n,), 800 + n)
        out6, _, _ = _disc_loss(backend.device, real, fake, 1)
        tr, tf, _, _, correct = _disc_loss_ref(real, fake, 1)
        want = np.array([t.sum().item() / n for t in (tr, tf, real.double(), fake.double())]).astype(np.float32)
        got = out6[:4].numpy()
        assert (np.abs(got - want) <= np.spacing(np.abs(want))).all(), (got, want)
        assert out6[4].item() == correct
    real, fake = randn((n,), 500 + n) * 3, randn((n,), 600 + n) * 3
    m = min(n, len(SPECIAL_LOGITS))
    real[:m] = torch.tensor(SPECIAL_LOGITS[:m])
    fake[:m] = -torch.tensor(SPECIAL_LOGITS[:m])
    out6, dr, df = _disc_loss(backend.device, real, fake, disc_type)
    tr, tf, gr, gf, correct = _disc_loss_ref(real, fake, disc_type)
    assert torch.isfinite(out6).all() and torch.isfinite(dr).all() and torch.isfinite(df).all()
    assert out6[4].item() == correct and out6[5].item() == 2 * n
    bound = (-(-n // 256) + 10) * U
    worst = 0.0
    for i, terms in enumerate((tr, tf, real.double(), fake.double())):
        scale = terms.abs().mean().item()
        err = abs(out6[i].item() - terms.mean().item())
        worst = max(worst, err / (bound * scale) if scale else err)
        assert err <= bound * scale, (i, out6[i].item(), terms.mean().item(), bound * scale)
    if disc_type == 1:
        assert torch.equal(dr, f32(gr)) and torch.equal(df, f32(gf))
        assert set(dr.tolist()) <= {f32(-0.5 / n), 0.0} and set(df.tolist()) <= {f32(0.5 / n), 0.0}
        e_d = 0.0
    else:
        e_d = n * max((dr.double() - gr).abs().max().item(), (df.double() - gf).abs().max().item())
        assert e_d <= 2e-6
    print(f"gan_disc_loss type={disc_type} n={n}: worst mean error / bound {worst:.3f}, n |d - d_ref| {e_d:.3e}")
    again, _, _ = _disc_loss(backend.device, real, fake, disc_type, grads=False)          # d_real = d_fake = NULL
    assert torch.equal(again, out6)


# ----------------------------------------------------------------------------------------------- 4. vq_colsum
def _colsum(dev, t, pixels, c, n_out, accumulate, guard=8):
    L = lib()
    need = L.size("vq_colsum_workspace", pixels, c)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    out = torch.full((n_out + guard,), 3.0, device=dev)
    adev = torch.tensor([0.25], device=dev)
    s = stream_of(t)
    rc = L.dll.vq_colsum(ptr(t), pixels, c, dtype_code(t), ptr(out), n_out, accumulate, 2.0, ptr(adev), ptr(ws), need - 1, s)
    assert rc == VQ_ERR_WORKSPACE                                   # one byte short
    L.call("vq_colsum", ptr(t), pixels, c, dtype_code(t), ptr(out), n_out, accumulate, 2.0, ptr(adev), ptr(ws), need, s)
    out = out.cpu()
    assert (out[n_out:] == 3.0).all()                               # nothing past n_out is written
    return out[:n_out]


@pytest.mark.parametrize("pixels,c,prec,n_out,accumulate", [(1, 8, "fp32", 3, 0), (1023, 24, "fp32", 17, 1), (1025, 40, "bf16", 40, 0),
                                                            (4099, 136, "fp16", 130, 1), (777, 1000, "fp32", 999, 0),
                                                            (3000, 2048, "fp32", 2048, 0), (5000, 264, "f16x3", 264, 0)])
def test_colsum(backend, pixels, c, prec, n_out, accumulate):
    """Bias gradients out[c] (+)= alpha * sum_p t[p][c], alpha = 2 * (*alpha_dev = 0.25).  A block of 1024 pixels has nps = 256 // (C/8)
    pixel lanes (3, 5, 17, 33, 125 slots per pixel leave threads of the last lane idle; 256 slots = one lane); a lane adds
    ceil(1024 / nps) values in batches of four pixels plus a tail, nps lane sums are added in LDS order, the block partials in
    fp64, and the result is rounded, scaled and (accumulate) added:  |err| <= (ceil(1024 / nps) + nps + 4) u alpha sum_p |t|.
    On the GPU the batched loads (load8_issue / vq_raw_wait) are a code path the emulator does not have.
    Measured worst error over its bound: emulator 0.002; MI355X 0.002; worst error / largest |column sum|: emulator 6.6e-7;
    MI355X 6.6e-7."""
    dev = backend.device
    nps = 256 // (c // 8)
    alpha = 0.5
    for regime in ("exact", "random"):
        x = small_ints((pixels, c), 900 + pixels) if regime == "exact" else randn((pixels, c), 1000 + pixels)
        t = store(rows_to_nchw(x), prec, dev)
        seen = load(t, c)[0, :, :, 0].t().double()                    # [pixels][c] as stored
        got = _colsum(dev, t, pixels, c, n_out, accumulate)
        ref = alpha * seen.sum(0)[:n_out] + (3.0 if accumulate else 0.0)
        if regime == "exact":
            assert torch.equal(seen, x.double())
            assert torch.equal(got, f32(ref)), (got - f32(ref)).abs().max()
        else:
            bound = (-(-1024 // nps) + nps + 4) * U * alpha * seen.abs().sum(0)[:n_out]
            err = (got.double() - ref).abs()
            print(f"colsum pixels={pixels} C={c} {prec}: worst error / bound {(err / bound).max().item():.3f}, "
                  f"/ largest |sum| {(err.max() / ref.abs().max()).item():.3e}")
            assert (err <= bound).all()


# ----------------------------------------------------------------------------------------------- 5. vq_absmax
def _absmax(dev, t, n, preset=0.0):
    out = torch.tensor([preset], device=dev)
    lib().call("vq_absmax", ptr(t), n, dtype_code(t), ptr(out), stream_of(t))
    return out.cpu().item()


@pytest.mark.parametrize("n", [8, 2056, 8 * 524288 + 24])
@pytest.mark.parametrize("prec", STORAGE)
def test_absmax(backend, prec, n):
    """out = max(out, max |t|): the EMA codebook's fixed-point scale needs a true upper bound.  The extreme is planted as a NEGATIVE
    number in the first octet, in the last octet and (largest n) in an octet only the grid-stride trip past 2048 * 256 lanes reaches;
    the result is |the value as stored|, exactly, in every storage type."""
    dev = backend.device
    n8 = n // 8
    spots = {0, n8 - 1} | ({524288 + 1} if n8 > 524288 else set())
    base = randn((1, 8, n8, 1), 1100 + n)
    for k, octet in enumerate(sorted(spots)):
        x = base.clone()
        x[0, (3 * k + 2) % 8, octet, 0] = -300.7 - k                  # not representable in bf16 / binary16: stored rounded
        t = store(x, prec, dev)
        want = load(t, 8).abs().max().item()
        assert abs(want - (300.7 + k)) <= HALF_ULP[prec] * 302 and want > 290
        assert _absmax(dev, t, n) == want, (prec, n, octet)
        assert _absmax(dev, t, n, preset=1.0) == want                 # raised from a smaller value
        assert _absmax(dev, t, n, preset=1e6) == 1e6                  # a larger one stays
    t = store(base, prec, dev)
    out = torch.zeros(1, device=dev)
    assert lib().dll.vq_absmax(ptr(t), 12, dtype_code(t), ptr(out), stream_of(t)) < 0      # not a multiple of 8


# ----------------------------------------------------------------------------------------------- 6. vq_scale, pools
@pytest.mark.parametrize("n", [1, 1025, 2048 * 1024 + 3])
def test_scale(backend, n):
    """out = x * (alpha * alpha_dev[0]): one block, two, and three elements past what 2048 blocks of 1024 cover without striding.
    One fp32 multiplication per element: bit equality with the float64 product rounded once."""
    dev = backend.device
    x = randn((n,), 1200 + n)
    xd = x.to(dev)
    alpha, a_dev = f32(0.3), f32(1.7)
    adev = torch.tensor([a_dev], device=dev)
    for dev_scalar in (None, adev):
        k = f32(alpha * a_dev) if dev_scalar is not None else alpha
        out = torch.full_like(xd, float("nan"))
        lib().call("vq_scale", ptr(xd), alpha, ptr(dev_scalar), n, ptr(out), stream_of(xd))
        assert torch.equal(out.cpu(), f32(x.double() * k))


@pytest.mark.parametrize("prec", STORAGE)
def test_sumpool(backend, prec):
    """2x2 sum pool (backward of the nearest-2x upsample) of a [2, 96, 118, 24] tensor against 4 * avg_pool2d of the stored tensor in
    float64.  (a + b) + (c + d) in fp32 is three roundings (3 u); f16x2 re-splits the sum (2^-21, twice its 2^-22); binary16 and
    bf16 round the output once (2^-11, 2^-8) — all relative to the largest output.
    Measured worst: emulator fp32 8.7e-8, f16x3 1.2e-7, fp16 4.1e-4, bf16 2.4e-3; MI355X the same."""
    dev = backend.device
    n, h, w, c = 2, 96, 118, 24
    # exact: integers in, integers out
    x = small_ints((n, c, h, w), 1301)
    t = store(x, prec, dev)
    y = store(torch.full((n, c, h // 2, w // 2), 77.0), prec, dev)         # every element must be overwritten
    lib().call("vq_sumpool2", ptr(t), ptr(y), n, h, w, c, dtype_code(t), stream_of(t))
    assert torch.equal(load(y, c), 4.0 * F.avg_pool2d(x, 2))
    # random
    t = store(randn((n, c, h, w), 1300), prec, dev)
    lib().call("vq_sumpool2", ptr(t), ptr(y), n, h, w, c, dtype_code(t), stream_of(t))
    ref = 4.0 * F.avg_pool2d(load(t, c).double(), 2)
    err = max_rel(load(y, c), ref)
    print(f"sumpool {prec}: {err:.3e}")
    assert err <= {"fp32": 3 * U, "f16x3": 2.0 ** -21, "fp16": 2.0 ** -11, "bf16": 2.0 ** -8}[prec]


@pytest.mark.parametrize("prec", STORAGE)
def test_maxpool_on_odd_extents(backend, prec):
    """nn.MaxPool2d(2, 2) and its backward on a [2, 97, 119, 24] tensor (both extents odd: the last row and column are dropped) of
    multiples of 1/8 — exact in every storage type, full of ties.  Forward bit-equal to F.max_pool2d; backward equal to autograd's
    (first maximum in scan order), alone and summed with `add`; the dropped row and column carry `add` alone, or zero."""
    dev = backend.device
    n, h, w, c = 2, 97, 119, 24
    x = small_ints((n, c, h, w), 1400, -16, 16) / 8
    gy = small_ints((n, c, h // 2, w // 2), 1401, -32, 32) / 8
    add = small_ints((n, c, h, w), 1402, -32, 32) / 8
    xr = x.clone().requires_grad_()
    yr = F.max_pool2d(xr, 2, 2)
    yr.backward(gy)
    t, dy, ad = store(x, prec, dev), store(gy, prec, dev), store(add, prec, dev)
    assert torch.equal(load(t, c), x) and torch.equal(load(dy, c), gy) and torch.equal(load(ad, c), add)
    y = store(torch.full((n, c, h // 2, w // 2), 77.0), prec, dev)
    s = stream_of(t)
    lib().call("vq_maxpool2_fwd", ptr(t), ptr(y), n, h, w, c, dtype_code(t), s)
    assert torch.equal(load(y, c), yr.detach())
    for other in (None, ad):
        dx = store(torch.full((n, c, h, w), 77.0), prec, dev)          # every element must be overwritten
        lib().call("vq_maxpool2_bwd", ptr(t), ptr(dy), ptr(other), ptr(dx), n, h, w, c, dtype_code(t), None, s)
        want = xr.grad + (add if other is not None else 0.0)
        got = load(dx, c)
        assert torch.equal(got, want), (got - want).abs().max()
        assert torch.equal(got[:, :, -1], want[:, :, -1]) and torch.equal(got[..., -1], want[..., -1])


# ----------------------------------------------------------------------------------------------- 7. vq_adamw_multi
ADAM_N = [5, 65536, 65537, 131072 + 3, 1, 1000]
ADAM_CHUNK = 65536
SENTINEL = 12345.0
HP = dict(lr=f32(3e-3), wd=f32(1e-3), b1=f32(0.9), b2=f32(0.95), eps=f32(1e-8))


class _AdamState:
    """Six tensors, each of p / g / m / v in a buffer of its own with the data `4 + shift` floats in: shift 0 = 16-byte aligned
    (the 16-bytes-per-lane path), shift 1 = every view one float off (the scalar path).  Everything around the data is a sentinel."""

    def __init__(self, dev, shift):
        self.dev, self.off = dev, 4 + shift
        self.buf = {k: [torch.full((n + 16,), SENTINEL, device=dev) for n in ADAM_N] for k in "pgmv"}
        table = (VqAdamTensor * len(ADAM_N))()
        for i, n in enumerate(ADAM_N):
            for k in "pgmv":
                setattr(table[i], k, self.buf[k][i].data_ptr() + 4 * self.off)
                assert (getattr(table[i], k) % 16 == 0) == (shift == 0)
            table[i].n = n
        self.table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        offs = [0]
        for n in ADAM_N:
            offs.append(offs[-1] + -(-n // ADAM_CHUNK))
        self.chunks = offs[-1]
        self.offs = torch.tensor(offs, dtype=torch.int64, device=dev)

    def put(self, k, values):
        for i, n in enumerate(ADAM_N):
            self.buf[k][i][self.off:self.off + n] = values[i].to(self.dev)

    def get(self, k):
        out = []
        for i, n in enumerate(ADAM_N):
            b = self.buf[k][i].cpu()
            assert (b[:self.off] == SENTINEL).all() and (b[self.off + n:] == SENTINEL).all(), (k, i)      # the guard floats
            out.append(b[self.off:self.off + n].clone())
        return out

    def step(self, t, grad_scale=1.0, flags=None, n_flags=0, stride=0):
        bc1, bc2 = f32(1.0 - HP["b1"] ** t), f32(1.0 - HP["b2"] ** t)
        lib().call("vq_adamw_multi", ptr(self.table), ptr(self.offs), len(ADAM_N), self.chunks, ADAM_CHUNK, HP["lr"], HP["wd"], HP["b1"],
                   HP["b2"], HP["eps"], bc1, bc2, grad_scale, ptr(flags), n_flags, stride, stream_of(self.table))
        return bc1, bc2


def _adam_ref(p, g, m, v, bc1, bc2):
    """torch.optim.AdamW in float64 with the hyper-parameters the kernel was handed (the fp32 values)."""
    p = p * (1.0 - HP["lr"] * HP["wd"])
    m = HP["b1"] * m + (1.0 - HP["b1"]) * g
    v = HP["b2"] * v + (1.0 - HP["b2"]) * g * g
    p = p - HP["lr"] / bc1 * m / (v.sqrt() / math.sqrt(bc2) + HP["eps"])
    return p, m, v


def _adam_tensors(seed, scale=1.0):
    return [randn((n,), seed + i) * scale for i, n in enumerate(ADAM_N)]


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "one-float-off"])
def test_adamw_multi_through_the_abi(backend, shift):
    """A six-entry table (n = 5, one chunk exactly, one chunk + 1, two chunks + 3, 1, 1000; chunk = 65536), so the binary search
    over chunk_offsets is walked, in both alignments.  One step from zero moments gives m = fl(g fl(1 - b1)) and
    v = fl(fl(fl(1 - b2) g) g) BIT FOR BIT — an element visited twice, or not at all, shows.  p within 2e-6 max(1, |p|max) of the
    float64 update (the bound of test_optim.py).  A second step: m, v within 4 u max|g|, 4 u max g^2 (two steps of at most two
    roundings each).  grad_scale = 0.5 is bit-identical to halved gradients; a raised skip flag changes nothing; flags that are all
    zero change nothing about the step.  Measured worst |p - ref|: emulator 8.6e-7; MI355X 5.9e-7 (|p| <= 5)."""
    dev = backend.device
    st = _AdamState(dev, shift)
    p0, g1, g2 = _adam_tensors(1500, 1.0), _adam_tensors(1600, 2.0), _adam_tensors(1700, 0.1)
    zeros = [torch.zeros(n) for n in ADAM_N]
    st.put("p", p0); st.put("g", g1); st.put("m", zeros); st.put("v", zeros)
    bc = st.step(1)
    p, m, v = st.get("p"), st.get("m"), st.get("v")
    c1, c2 = np.float32(1) - np.float32(HP["b1"]), np.float32(1) - np.float32(HP["b2"])
    ref, worst = [], 0.0
    for i in range(len(ADAM_N)):
        g = g1[i].numpy()
        assert np.array_equal(m[i].numpy(), g * c1), i
        assert np.array_equal(v[i].numpy(), (c2 * g) * g), i
        ref.append(_adam_ref(p0[i].double(), g1[i].double(), zeros[i].double(), zeros[i].double(), *bc))
        err = (p[i].double() - ref[i][0]).abs().max().item()
        worst = max(worst, err)
        assert err <= 2e-6 * max(1.0, ref[i][0].abs().max().item()), (i, err)
    assert [t.tolist() for t in st.get("g")] == [t.tolist() for t in g1]                  # gradients are read only
    st.put("g", g2)
    bc = st.step(2)
    p, m, v = st.get("p"), st.get("m"), st.get("v")
    for i in range(len(ADAM_N)):
        gmax = max(g1[i].abs().max().item(), g2[i].abs().max().item())
        pr, mr, vr = _adam_ref(ref[i][0], g2[i].double(), ref[i][1], ref[i][2], *bc)
        assert (m[i].double() - mr).abs().max().item() <= 4 * U * gmax, i
        assert (v[i].double() - vr).abs().max().item() <= 4 * U * gmax * gmax, i
        err = (p[i].double() - pr).abs().max().item()
        worst = max(worst, err)
        assert err <= 2e-6 * max(1.0, pr.abs().max().item()), (i, err)
    print(f"adamw_multi shift={shift}: worst |p - ref| {worst:.3e}")
    # grad_scale = 0.5 == halved gradients (a power of two), from the state after two steps
    state = {k: st.get(k) for k in "pmv"}
    g3 = _adam_tensors(1800, 1.0)
    st.put("g", g3)
    st.step(3, grad_scale=0.5)
    scaled = {k: st.get(k) for k in "pmv"}
    for k in "pmv":
        st.put(k, state[k])
    st.put("g", [0.5 * t for t in g3])
    st.step(3)
    for k in "pmv":
        assert all(torch.equal(a, b) for a, b in zip(st.get(k), scaled[k])), k
    # skip flags: three flags two ints apart, the middle one raised -> nothing changes; all three zero (the ints between them are
    # not flags) -> the same step as without flags
    for k in "pmv":
        st.put(k, state[k])
    st.put("g", g3)
    st.step(3, flags=torch.tensor([0, 9, 1, 9, 0, 9], dtype=torch.int32, device=dev), n_flags=3, stride=2)
    for k in "pmv":
        assert all(torch.equal(a, b) for a, b in zip(st.get(k), state[k])), k
    assert all(torch.equal(a, b) for a, b in zip(st.get("g"), g3))
    st.step(3, flags=torch.tensor([0, 9, 0, 9, 0, 9], dtype=torch.int32, device=dev), n_flags=3, stride=2)
    with_flags = {k: st.get(k) for k in "pmv"}
    for k in "pmv":
        st.put(k, state[k])
    st.step(3)
    for k in "pmv":
        assert all(torch.equal(a, b) for a, b in zip(st.get(k), with_flags[k])), k
        assert not all(torch.equal(a, b) for a, b in zip(st.get(k), state[k])), k


# ----------------------------------------------------------------------------------------------- 8. attention
ATTN_SHAPES = [(1, 32, 64, 64), (1, 33, 64, 8), (2, 256, 64, 16), (1, 257, 64, 32), (1, 513, 128, 64), (1, 1024, 128, 64)]


def _sdpa(qkv, go, c, hd):
    n, t = qkv.shape[:2]
    x = qkv.clone().requires_grad_()
    q, k, v = (s.reshape(n, t, c // hd, hd).transpose(1, 2) for s in x.split(c, dim=-1))
    o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(n, t, c)
    o.backward(go)
    return o.detach(), x.grad


def _attention_errors(dev, prec, n, t, c, hd, seed, q_scale=1.0):
    """-> (kernel error, fp32-CPU error) of the output and of dqkv, max-norm relative to the float64 truth on the stored tensors."""
    L = lib()
    qkv = randn((n, 3 * c, t, 1), seed)
    qkv[:, :c] *= q_scale
    qs, gs = store(qkv, prec, dev), store(randn((n, c, t, 1), seed + 1), prec, dev)        # [n, t, 1, 3c], [n, t, 1, c]
    out = torch.empty((n, t, 1, c), dtype=qs.dtype, device=dev)
    dqkv = torch.empty_like(qs)
    lse = torch.empty(n * (c // hd) * t, device=dev)
    need = L.size("vq_attention_workspace", n, t, c, hd)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s = stream_of(qs)
    L.call("vq_attention_fwd", ptr(qs), ptr(out), ptr(lse), n, t, c, hd, dtype_code(qs), s)
    L.call("vq_attention_bwd", ptr(qs), ptr(out), ptr(gs), ptr(lse), ptr(dqkv), n, t, c, hd, dtype_code(qs), ptr(ws), need, s)
    rows = lambda y, ch: load(y, ch)[..., 0].transpose(1, 2)                              # noqa: E731   -> [n, t, ch]
    q_seen, g_seen = rows(qs, 3 * c), rows(gs, c)
    o64, d64 = _sdpa(q_seen.double(), g_seen.double(), c, hd)
    o32, d32 = _sdpa(q_seen, g_seen, c, hd)
    return (max_rel(rows(out, c), o64), max_rel(o32, o64)), (max_rel(rows(dqkv, 3 * c), d64), max_rel(d32, d64))


@pytest.mark.parametrize("prec", STORAGE)
def test_attention_at_tile_and_block_boundaries(backend, prec):
    """vq_attention_fwd / _bwd in every storage type at T = one full 32-key tile, one key past it, one full 256-query block, one live
    thread in a second block, 513 and the block's real 1024 tokens; head widths 8, 16, 32, 64.  Truth = float64
    scaled_dot_product_attention on the tensors the kernel read; yardstick = the same call in fp32 on the CPU.  Max-norm relative
    error <= 4 x yardstick + 2 u (output) / + 4 u (dqkv), u = the storage type's half-ulp (2^-24, 2^-22, 2^-11, 2^-8): the kernel's
    arithmetic is fp32, its result is stored once, and the backward also reads the rounded out and dout into D = dO . O.
    Measured worst (out, dqkv): emulator fp32 1.5e-6, 1.8e-6; f16x3 1.3e-6, 1.6e-6; fp16 3.6e-4, 4.2e-4; bf16 2.6e-3, 2.3e-3.
    MI355X fp32 1.4e-6, 1.8e-6; f16x3 1.3e-6, 1.6e-6; fp16 3.6e-4, 4.2e-4; bf16 2.6e-3, 2.3e-3."""
    u = HALF_ULP[prec]
    worst = [0.0, 0.0]
    for i, (n, t, c, hd) in enumerate(ATTN_SHAPES):
        (e_o, y_o), (e_d, y_d) = _attention_errors(backend.device, prec, n, t, c, hd, 1900 + 2 * i)
        worst = [max(worst[0], e_o), max(worst[1], e_d)]
        assert e_o <= 4 * y_o + 2 * u, (prec, t, e_o, y_o)
        assert e_d <= 4 * y_d + 4 * u, (prec, t, e_d, y_d)
    print(f"attention {prec}: worst out {worst[0]:.3e}, dqkv {worst[1]:.3e}")


def test_attention_with_a_peaked_softmax(backend):
    """Logits scaled by 8 (q times 8) at T = 65, fp32 storage: exp spans its range, the online softmax rescales between tiles.  Same
    rule as above.  Measured (out, dqkv): emulator 1.2e-6, 1.1e-6; MI355X 1.2e-6, 1.1e-6."""
    (e_o, y_o), (e_d, y_d) = _attention_errors(backend.device, "fp32", 1, 65, 64, 16, 1990, q_scale=8.0)
    print(f"attention peaked: out {e_o:.3e} (fp32 CPU {y_o:.3e}), dqkv {e_d:.3e} (fp32 CPU {y_d:.3e})")
    assert e_o <= 4 * y_o + 2 * U
    assert e_d <= 4 * y_d + 4 * U


# ----------------------------------------------------------------------------------------------- 9. re-pack in one launch
PACK_WEIGHTS = [(3, 128, 3, 3), (128, 3, 3, 3), (64, 64, 1, 1), (96, 40, 3, 3), (1, 512, 4, 4), (256, 128, 3, 3), (33, 17, 2, 2)]
PACK_OPERANDS = [(VQ_BF16, 1), (VQ_BF16, 3), (VQ_BF16, 6), (VQ_F16, 1), (VQ_F16X2, 1)]


def test_repack_in_one_launch_equals_the_single_calls(backend):
    """include/vqhip.h: vq_pack_job fills a job "exactly as vq_pack_weight_* would run it".  Every (weight, direction, operand type /
    split, layout) the single calls accept is packed once by its own call and once as a job of ONE vq_pack_weights_multi launch, both
    into buffers pre-filled with 0xFF: every packed byte and every 4-float scale record must be equal (so both write the same pad
    regions), and vq_pack_job refuses nothing the single call took.  Weight magnitudes span 1e-3 .. 1e2: different binary16 scales."""
    L = lib()
    dev = backend.device
    pad8 = lambda v: (v + 7) // 8 * 8                                                      # noqa: E731
    mags = np.logspace(-3, 2, len(PACK_WEIGHTS))
    weights = [(randn(s, 2000 + i) * float(mags[i])).to(dev) for i, s in enumerate(PACK_WEIGHTS)]
    s = stream_of(weights[0])
    singles, multis, jobs, blocks = [], [], [], 0
    for w in weights:
        co, ci, r, sx = w.shape
        for dgrad in (0, 1):
            for op, split in PACK_OPERANDS:
                for layout in (0, 1):
                    rows, kch = (pad8(ci), pad8(co)) if dgrad else (pad8(co), pad8(ci))
                    elems = L.size("vq_packed_weight_elems", rows, r, sx, kch * (2 if op == VQ_F16X2 else 1), split, layout)
                    one = (torch.full((2 * elems,), 0xFF, dtype=torch.uint8, device=dev), torch.full((16,), 0xFF, dtype=torch.uint8, device=dev))
                    rc = getattr(L.dll, "vq_pack_weight_dgrad" if dgrad else "vq_pack_weight_fwd")(
                        ptr(w), co, ci, r, sx, pad8(co), pad8(ci), split, layout, op, ptr(one[1]), ptr(one[0]), s)
                    if rc != 0:
                        continue
                    many = (torch.full_like(one[0], 0xFF), torch.full_like(one[1], 0xFF))
                    job = VqPackJob()
                    L.call("vq_pack_job", C.byref(job), ptr(w), co, ci, r, sx, pad8(co), pad8(ci), split, layout, dgrad, op,
                           ptr(many[1]), ptr(many[0]))                                  # must accept what the single call accepted
                    job.block_start = blocks
                    blocks += L.size("vq_pack_job_blocks", C.byref(job))
                    singles.append(one); multis.append(many); jobs.append(job)
    tiled = sum(j.tiled for j in jobs)
    assert len(jobs) >= 100 and 0 < tiled < len(jobs), (len(jobs), tiled)                # at this commit: 112 jobs, 39 tiled
    table = torch.frombuffer(bytearray(b"".join(bytes(memoryview(j)) for j in jobs)), dtype=torch.uint8).to(dev)
    L.call("vq_pack_weights_multi", ptr(table), len(jobs), blocks, 1, s)
    for i, (one, many) in enumerate(zip(singles, multis)):
        what = (i, jobs[i].Cout_w, jobs[i].Cin_w, jobs[i].R, jobs[i].dgrad, jobs[i].op_dtype, jobs[i].split, jobs[i].layout, jobs[i].tiled)
        assert torch.equal(one[0].cpu(), many[0].cpu()), what
        assert torch.equal(one[1].cpu(), many[1].cpu()), what
        if jobs[i].op_dtype != VQ_BF16:
            amax, s_w, inv, _ = one[1].cpu().view(torch.float32).tolist()
            co, ci = jobs[i].Cout_w, jobs[i].Cin_w
            w = [x for x in weights if tuple(x.shape[:2]) == (co, ci)][0]
            assert amax == w.abs().max().item() and s_w * inv == 1.0 and 2.0 ** 14 <= amax * s_w < 2.0 ** 15, what


# ----------------------------------------------------------------------------------------------- 10. image-side kernels at size
IMG = (3, 5, 210, 190)          # 598500 elements: more than one grid of 2048 x 256 lanes


@pytest.mark.parametrize("flip_h,flip_w,neg", [(1, 0, (0, 0)), (0, 1, (0, 0)), (1, 1, (1, 3))])
def test_flip_at_size(backend, flip_h, flip_w, neg):
    """torch.flip of a non-square [3, 5, 210, 190] tensor along H, along W, and along both with channels [1, 3) negated: bitwise."""
    x = randn(IMG, 2100)
    xd = x.to(backend.device)
    y = torch.full_like(xd, float("nan"))
    lib().call("vq_flip_nchw", ptr(xd), ptr(y), *IMG, flip_h, flip_w, neg[0], neg[1], stream_of(xd))
    want = torch.flip(x, [d for d, on in ((-2, flip_h), (-1, flip_w)) if on]).clone()
    want[:, neg[0]:neg[1]] = -want[:, neg[0]:neg[1]]
    assert torch.equal(y.cpu(), want)


@pytest.mark.parametrize("k", [2, 5])
def test_area_downsample_at_size(backend, k):
    """F.interpolate(mode="area") to (105, 95) and (42, 38): a k x k window is summed in row-major order in fp32 (k^2 - 1 roundings of
    partial sums no larger than sum |x|) and divided once:  |err| <= (k^2 + 2) u mean_window |x|, per output element.
    Measured worst error over its bound: emulator 0.38 (k = 2), 0.13 (k = 5); MI355X the same."""
    n, c, h, w = IMG
    x = randn(IMG, 2200)
    xd = x.to(backend.device)
    y = torch.full((n, c, h // k, w // k), float("nan"), device=backend.device)
    lib().call("vq_area_downsample_nchw", ptr(xd), ptr(y), n, c, h, w, k, stream_of(xd))
    ref = F.interpolate(x.double(), size=(h // k, w // k), mode="area")
    bound = (k * k + 2) * U * F.avg_pool2d(x.double().abs(), k)
    err = (y.cpu().double() - ref).abs()
    print(f"area_downsample k={k}: worst error / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()
    xi = small_ints(IMG, 2201) * k * k                                 # exact: window sums divisible by k^2
    xid = xi.to(backend.device)
    lib().call("vq_area_downsample_nchw", ptr(xid), ptr(y), n, c, h, w, k, stream_of(xid))
    assert torch.equal(y.cpu(), F.avg_pool2d(xi, k))


def test_wavelet_on_a_non_square_image(backend):
    """utils.py:229-247 on a [2, 5, 130, 94] image (five channels, 65 x 47 outputs) against the oracle restatement, NCHW output:
    within 1e-6 of the largest coefficient (the bound of test_wavelet_front_end).  Measured: emulator 0 (the same fmaf chain as the oracle's convolution); MI355X 0."""
    from oracle import ops_ref
    x = randn((2, 5, 130, 94), 2300)
    got = ops.wavelet_nchw(x.to(backend.device))
    err = max_rel(got, ops_ref.wavelet_transform(x))
    print(f"wavelet: {err:.3e}")
    assert tuple(got.shape) == (2, 20, 65, 47) and err < 1e-6


@pytest.mark.parametrize("prec", STORAGE)
def test_layout_round_trip_with_channel_padding(backend, prec):
    """to_nchw(to_nhwc(x)) on [2, 13, 230, 101] (13 channels padded to 16; 46460 pixels x 2 octets x 2 images): value and gradient
    within ONE rounding of the storage type — |err| <= u |x| + the format's absolute floor (half of binary16's smallest subnormal,
    2^-25, for fp16 and for the lo piece of f16x2; divided by the loss scale for a gradient) — exact for fp32, and the padded
    channels 13..15 are exactly zero."""
    P = ops._PRECISIONS[prec]
    dev = backend.device
    x, gy = randn((2, 13, 230, 101), 2400), randn((2, 13, 230, 101), 2401)
    xd = x.to(dev).requires_grad_()
    t = ops.to_nhwc(xd, P)
    assert tuple(t.shape) == (2, 230, 101, 16)
    y = ops.to_nchw(t, 13)
    y.backward(gy.to(dev))
    assert float(load(t.detach(), 16)[:, 13:].abs().max()) == 0.0
    u = HALF_ULP[prec]
    floor = 2.0 ** -25 if P.half_range() else 0.0
    for got, want, fl in ((y.detach().cpu(), x, floor), (xd.grad.cpu(), gy, floor / P.gs())):
        if prec == "fp32":
            assert torch.equal(got, want)
        else:
            assert ((got.double() - want.double()).abs() <= u * want.double().abs() + fl).all()
