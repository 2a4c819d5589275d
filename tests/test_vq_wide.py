"""Nearest-code search at the code dimensions beyond {4, 8, 16, 32, 64}: every multiple of 8 up to 256 (vq_nearest_wide_kernel behind
vq_vq_nearest_fwd).  The contract is oracle/vq_oracle.c's — zz, ee and dot are fmaf chains over k ascending, d = (zz - 2 dot) + ee, strict
'<' over j ascending — so indices, zq and the BITS of min_dist must equal the oracle's: one dot product is one chain of dim / 2 MFMAs
onto one accumulator, and any re-association (two partial accumulators, a chunk taken out of order) changes bits.

The kernel's edges the shapes below cross: 32 tokens per wave, 128 per block; code tiles of 32, k-chunks of 32 (16 MFMAs)
with a remainder in groups of 8; code splits in multiples of 128 codes, never more of them than vq_vq_workspace (which does not know dim)
was sized for.
"""
import ctypes
import functools
import os
import sys

import pytest
import torch

import vqgan_training_amd as vq
from vqgan_training_amd._lib import lib, ptr, stream_of
from vqgan_training_amd.quantizer import VectorQuantizer, _VQLookup
from oracle import vq_oracle
from oracle import weights as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_vq_ema import assert_within_bounds, ema_ref, fixed_quantum, picked_token, run_update  # noqa: E402

VQ_ERR_UNSUPPORTED, VQ_ERR_WORKSPACE = -2, -4
CODE_TILE = 32                                   # vq_nearest_wide_kernel's codes per LDS tile


def nearest_abi(dev, z, cb, tail=0):
    """vq_vq_nearest_fwd through the C ABI with ws_bytes = vq_vq_workspace(n, K) EXACTLY, on a buffer `tail` bytes longer whose tail
    holds a pattern -> idx, zq, min_dist, the tail (all on the CPU)."""
    L = lib()
    (n, d), k = z.shape, cb.shape[0]
    need = L.size("vq_vq_workspace", n, k)
    ws = torch.full((need + tail,), 0xA5, dtype=torch.uint8, device=dev)
    zd, cd = z.contiguous().to(dev), cb.contiguous().to(dev)
    idx = torch.full((n,), -1, dtype=torch.int64, device=dev)
    zq = torch.full((n, d), float("nan"), dtype=torch.float32, device=dev)
    md = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    L.call("vq_vq_nearest_fwd", ptr(zd), ptr(cd), n, k, d, ptr(idx), ptr(zq), ptr(md), ptr(ws), need, stream_of(zd))
    return idx.cpu(), zq.cpu(), md.cpu(), ws[need:].cpu()


def random_problem(n, k, d, seed):
    """Token components with magnitudes spread over 2^-12 ... 1 (a re-associated chain rounds differently), codes in (-1, 1)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, d, generator=g).clamp(-4, 4) / 4 * torch.exp2(-12 * torch.rand(n, d, generator=g))
    cb = torch.rand(k, d, generator=g) * 2 - 1
    return z, cb


def assert_equals_oracle(z, cb, idx, zq, md):
    want, want_md = vq_oracle.nearest(z, cb)
    assert torch.equal(idx, want)
    assert torch.equal(zq, cb[want])
    assert torch.equal(md.view(torch.int32), want_md.view(torch.int32))


# ----------------------------------------------------------------------------------------------- 1: random data, bit for bit
@pytest.mark.parametrize("n,k,d", [
    (1, 1, 24), (31, 31, 72), (33, 33, 96), (127, CODE_TILE, 128), (129, 100, 200), (300, 300, 256),   # n: ragged wave, one block, two, three
    (5, 300, 256),                                # three splits of 128 codes (a small n splits the codes), four tiles each
    (300, 129, 72),                               # a split of four whole tiles and a split of one code; 72 = one k-chunk + a remainder
    (33, 1, 256), (129, CODE_TILE - 1, 24), (1, CODE_TILE + 1, 128), (31, 100, 256),                    # K around the code tile; one split, ragged last tile
    (33, 2 * CODE_TILE - 1, 256), (127, 2 * CODE_TILE, 136), (31, 2 * CODE_TILE + 1, 200),              # ... and around two tiles (both LDS buffers)
    (33, 65, 40), (127, 31, 56), (31, 33, 48), (33, 300, 248)])                                         # the other widths of each register bucket
def test_wide_dims_bit_exact_random(backend, n, k, d):
    z, cb = random_problem(n, k, d, 1000 * d + n + k)
    idx, zq, md, _ = nearest_abi(backend.device, z, cb)
    assert_equals_oracle(z, cb, idx, zq, md)


# ----------------------------------------------------------------------------------------------- 2: every component counts once
@pytest.mark.parametrize("d", [72, 128, 256])
def test_no_component_dropped_or_doubled(backend, d):
    """Token v; code 20 = v; code 3 = v with component k* raised by 1; the other codes far away: the answer is 20, at distance ~0
    against 1.  v's components lie in (-1.5, -0.75): a search whose dot product skips component k* finds code 3 NEARER, by
    2 v_k* + 1 < 0 (|e_3|^2, which does not go through the MFMA chain, still holds the raised component), and answers 3; one that
    takes a component twice moves min_dist's bits, which are compared with the oracle's.  k* covers both parities, the first and last
    component and both sides of every 32-wide k-chunk boundary below 66 and of the middle."""
    ks = sorted({k for k in (0, 1, 31, 32, 63, 64, 65, d // 2 - 1, d // 2, d - 2, d - 1) if k < d})
    g = torch.Generator().manual_seed(d)
    for ks_ in ks:
        v = -(0.75 + 0.75 * torch.rand(d, generator=g))
        cb = v + 6.0 + torch.rand(40, d, generator=g)
        cb[20] = v
        cb[3] = v
        cb[3, ks_] += 1.0
        z = v[None, :].clone()
        idx, zq, md, _ = nearest_abi(backend.device, z, cb)
        assert idx.item() == 20, (d, ks_, idx.item())
        assert_equals_oracle(z, cb, idx, zq, md)


# ----------------------------------------------------------------------------------------------- 3: ties and near-ties
def test_ties_and_near_ties_at_256(backend):
    """tests/test_vq.py::test_indices_ties_and_near_ties at D = 256: exact duplicates (the lowest index wins), codes one ulp apart,
    tokens on the bisector of code pairs — resolved exactly as the oracle's fixed fmaf order resolves them."""
    d, k = 256, 512
    cb = W.uniform_tensor((k, d), 7, -1, 1)
    cb[300] = cb[17]
    cb[301] = cb[17]
    cb[41] = torch.nextafter(cb[40], torch.full((d,), 2.0))
    z = torch.cat([cb[17:18] + 1e-3, cb[40:41], (cb[40:41] + cb[41:42]) / 2, (cb[5:6] + cb[6:7]) / 2,
                   W.uniform_tensor((60, d), 9, -1, 1)])
    a, b = cb[torch.arange(0, 200, 2)], cb[torch.arange(1, 200, 2)]
    z = torch.cat([z, (a + b) / 2])
    idx, zq, md, _ = nearest_abi(backend.device, z, cb)
    assert_equals_oracle(z, cb, idx, zq, md)
    assert idx[0].item() == 17


# ----------------------------------------------------------------------------------------------- 4: workspace contract
@functools.lru_cache(maxsize=None)
def taming_size_problem():
    """2048 tokens (two 512^2 images at f = 16) x 1024 codes x 256: the problem and the oracle's answer, computed once."""
    z, cb = random_problem(2048, 1024, 256, 5)
    return z, cb, vq_oracle.nearest(z, cb)


def _workspace_case(dev, z, cb, want):
    L = lib()
    (n, d), k = z.shape, cb.shape[0]
    idx, zq, md, tail = nearest_abi(dev, z, cb, tail=4096)
    assert torch.equal(idx, want[0]) and torch.equal(md.view(torch.int32), want[1].view(torch.int32))
    assert tail.numel() == 4096 and bool((tail == 0xA5).all())                   # nothing past vq_vq_workspace(n, K) was written
    need = L.size("vq_vq_workspace", n, k)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    zd, cd, out = z.to(dev), cb.to(dev), torch.zeros(n, dtype=torch.int64, device=dev)
    rc = L.dll.vq_vq_nearest_fwd(ptr(zd), ptr(cd), n, k, d, ptr(out), None, None, ptr(ws), need - 1, stream_of(zd))
    assert rc == VQ_ERR_WORKSPACE and L.last_error()


@pytest.mark.parametrize("n,k", [(5, 3000), (300, 129)])
def test_workspace_is_sized_without_the_dimension(backend, n, k):
    """D = 256 inside vq_vq_workspace(n, K) bytes exactly — the size callers compute without passing dim: the pattern behind it
    survives, the indices are the oracle's, and one byte less is refused."""
    z, cb = random_problem(n, k, 256, n + k)
    _workspace_case(backend.device, z, cb, vq_oracle.nearest(z, cb))


@pytest.mark.gpu
def test_workspace_is_sized_without_the_dimension_at_taming_size(hip_library):
    vq._lib._set_library_for_tests(hip_library)
    try:
        z, cb, want = taming_size_problem()
        _workspace_case(torch.device("cuda:0"), z, cb, want)
    finally:
        vq._lib._set_library_for_tests(None)


# ----------------------------------------------------------------------------------------------- 5: refusals
def test_refused_dimensions_without_a_gpu():
    """Validation precedes every HIP call, so the PRODUCT library answers on a GPU-less machine."""
    L = vq._lib.VqLibrary(vq._lib._LIB_PATH)
    n, k = 8, 8
    buf = (ctypes.c_float * (n * 512))()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ws = (ctypes.c_char * L.size("vq_vq_workspace", n, k))()
    for dim in (0, 12, 20, 257, 264, 512):
        rc = L.dll.vq_vq_nearest_fwd(p, p, n, k, dim, p, None, None, ctypes.cast(ws, ctypes.c_void_p), len(ws), None)
        assert rc == VQ_ERR_UNSUPPORTED, (dim, rc)
        msg = L.last_error()
        assert msg and str(dim) in msg and "256" in msg, (dim, msg)


# ----------------------------------------------------------------------------------------------- 6: the module
def test_quantizer_module_matches_oracle_at_128(backend):
    """tests/test_vq.py::test_quantizer_module_matches_oracle with VectorQuantizer(64, 128): same uniform(-1, 1) data, same bounds."""
    dev = backend.device
    K, D = 64, 128
    q = VectorQuantizer(n_codes=K, dim=D, beta=0.25)
    q.embedding.weight.data.copy_(W.uniform_tensor((K, D), 3, -1, 1))
    z = W.uniform_tensor((2, D, 4, 4), 4, -1, 1)
    cbr = q.embedding.weight.detach().clone().requires_grad_()
    zr = z.clone().requires_grad_()
    out_r, loss_r, idx_r = vq_oracle.quantize(zr, cbr, 0.25)
    gy = W.uniform_tensor(tuple(out_r.shape), 5)
    (out_r * gy).sum().backward(retain_graph=True)
    (3.0 * loss_r).backward()
    q = q.to(dev)
    zd = z.to(dev).requires_grad_()
    out, loss, idx = q(zd)
    ((out * gy.to(dev)).sum() + 3.0 * loss).backward()
    assert torch.equal(idx.cpu(), idx_r)
    assert len(set(idx.flatten().tolist())) > 4
    assert torch.allclose(out.detach().cpu(), out_r.detach(), atol=1e-6)
    assert abs(loss.item() - loss_r.item()) < 1e-6 * max(1.0, abs(loss_r.item()))
    assert torch.allclose(zd.grad.cpu(), zr.grad, atol=1e-6)
    assert torch.allclose(q.embedding.weight.grad.cpu(), cbr.grad, atol=1e-6)


@pytest.mark.parametrize("decay", [0.99, 0.6])   # the default; and one under which codes that win nothing fall below reseed_below in two steps
def test_ema_quantizer_at_128(backend, decay):
    """VectorQuantizer(48, 128, ema=True, init_from_data=True, reseed_below=0.5, reseed_every=2): three training forwards, each
    followed by ema_update().  Per step: indices == the oracle's on the codebook the forward saw; N, m and the codebook == the float64
    restatement of tests/test_vq_ema.py applied to the fp32 state before the step, within its derived bounds; the codes the step
    reseeds (after the second update) hold exactly the tokens the hash picks, with N = 1."""
    dev = backend.device
    K, D, eps, seed = 48, 128, 1e-5, 0
    q = VectorQuantizer(K, D, ema=True, init_from_data=True, reseed_below=0.5, reseed_every=2, decay=decay).to(dev)
    reseeded = 0
    for step in range(3):
        z = W.uniform_tensor((2, D, 4, 4), 40 + step, -1, 1)
        tok = z.permute(0, 2, 3, 1).reshape(-1, D)
        n = tok.shape[0]
        zl = z.clone().to(dev).requires_grad_()
        _, loss, idx = q(zl)
        loss.backward()
        # the state the lookup and the update start from (after the first forward's initialisation from data)
        e0, N0, m0 = (t.detach().cpu().clone() for t in (q.embedding.weight, q.ema_cluster_size, q.ema_embed_sum))
        if step == 0:
            want = torch.stack([tok[picked_token(seed, 0, c, n)] for c in range(K)])
            assert torch.equal(e0, want) and torch.equal(m0, want) and bool((N0 == 1).all())
        idx = idx.reshape(-1).cpu()
        assert torch.equal(idx, vq_oracle.nearest(tok, e0)[0])
        assert q.ema_update() is not None
        ref = ema_ref(N0, m0, tok, idx, decay, eps)
        N, m, e = q.ema_cluster_size.cpu(), q.ema_embed_sum.cpu(), q.embedding.weight.detach().cpu()
        dead = torch.zeros(K, dtype=torch.bool)
        if (step + 1) % 2 == 0:
            dead = ref["N"].float() < 0.5
            for c in dead.nonzero().flatten().tolist():
                want = tok[picked_token(seed, step, c, n)]
                assert torch.equal(e[c], want) and torch.equal(m[c], want) and N[c].item() == 1.0, (step, c)
            reseeded += int(dead.sum())
        live = ~dead
        ref_live = {key: (v[live] if torch.is_tensor(v) else v) for key, v in ref.items()}
        assert_within_bounds(N[live], m[live], e[live], ref_live, decay, fixed_quantum(tok.abs().max().item(), n))
    assert (reseeded > 0) == (decay == 0.6)


def test_ema_kernels_at_256(backend):
    """The three EMA entry points were written for any dim: one update at 64 codes x 256 within the derived bounds."""
    n, K, D, gamma, eps = 256, 64, 256, 0.99, 1e-5
    tokens, cb = random_problem(n, K, D, 11)
    g = torch.Generator().manual_seed(12)
    N = torch.rand(K, generator=g) * 5.0
    m = cb * N[:, None]
    idx = vq_oracle.nearest(tokens, cb)[0]
    Nk, mk, ek, _, amax = run_update(backend.device, tokens, idx, N, m, gamma, eps)
    assert_within_bounds(Nk, mk, ek, ema_ref(N, m, tokens, idx, gamma, eps), gamma, fixed_quantum(amax, n))


# ----------------------------------------------------------------------------------------------- 7: the train step
def test_train_step_with_a_128_wide_quantizer_matches_oracle(backend):
    """tests/test_vq.py::test_train_step_with_quantizer_matches_oracle with z_channels = 128 and K = 64 (policy fp32x3): indices
    bit-exact, the four losses to 1e-4, the codebook after the step within 1e-3."""
    from oracle import model_ref as M
    from vqgan_training_amd import ops
    dev = backend.device
    ops.set_default_precision("fp32x3")
    res, ch, mult, zc, K = (32 if backend.name == "gpu" else 16), 32, [1, 2], 128, 64
    vae = vq.ae.VAE(res, 3, ch, 3, list(mult), 1, zc, False, False, False)
    vae.load_state_dict(W.randomize_state_dict(vae.state_dict(), 1))
    lp = vq.utils.LPIPS(pretrained_path=None)
    lp.load_state_dict(W.randomize_state_dict(lp.state_dict(), 2, relu_net=True))
    quant = VectorQuantizer(K, zc, beta=0.25)
    with torch.no_grad():
        quant.embedding.weight.copy_(W.uniform_tensor((K, zc), 77, -1.5, 1.5))
    sd = dict(vae.state_dict()); sd[M.VQ_KEY] = quant.embedding.weight.detach().clone()
    st = M.RefState(sd, lp.state_dict(), None)
    vae, lp, quant = vae.to(dev), lp.to(dev).eval(), quant.to(dev)
    step = vq.vae_trainer.VAETrainStep(vae, lp, None, learning_rate_vae=1e-2, vae_ch=ch, max_steps=10, warmup_steps=1,
                                       quantizer=quant)
    x = W.image_batch(2, res, seed=8)
    o = step(x.to(dev))
    r = M.train_step_ref(st, x, learning_rate_vae=1e-2, vae_ch=ch, max_steps=10, warmup_steps=1)
    assert torch.equal(o["indices"].cpu(), r["indices"])
    for k in ("overall_vae_loss", "perceptual_loss", "vae_loss", "vq_loss"):
        a, b = float(o[k]), float(r[k])
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-7, (k, a, b)
    assert (quant.embedding.weight.detach().cpu() - st.vae[M.VQ_KEY].detach()).abs().max().item() < 1e-3
    assert len(set(o["indices"].flatten().tolist())) > 4              # the test really quantizes to several codes


# ----------------------------------------------------------------------------------------------- 8: taming's size
@pytest.mark.gpu
def test_indices_bit_exact_at_taming_size(hip_library):
    """2048 x 1024 x 256 through _VQLookup against the oracle on the host cores."""
    vq._lib._set_library_for_tests(hip_library)
    try:
        z, cb, want = taming_size_problem()
        dev = torch.device("cuda:0")
        zq, _, idx = _VQLookup.apply(z.to(dev), cb.to(dev), 0.25)
        assert torch.equal(idx.cpu(), want[0])
        assert torch.equal(zq.cpu(), cb[want[0]])
    finally:
        vq._lib._set_library_for_tests(None)
