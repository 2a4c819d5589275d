"""Pins the oracle (oracle/*.py restatement) — CPU only — against the committed golden fixtures, which were produced by the
reference's own modules (tests/golden/make_golden.py): forward / backward vectors, the state-dict surface (keys, shapes, initial
values) and a three-step training trajectory.  Nothing outside the repository is read.
The reference ships no golden vectors or known-answer tests of its own.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import model_ref as M
from oracle import ops_ref as R
from oracle import weights as W

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
from golden import make_golden as G  # noqa: E402
from golden.make_golden import VAE_CFGS, cfg_fields  # noqa: E402


def _vae_state(res, ch, mult, nrb, zc, hr=False, wav=False):
    """Key names/shapes of the reference VAE state dict, built without the reference: via our module."""
    import vqgan_training_amd as vq
    vae = vq.ae.VAE(res, 3, ch, 3, list(mult), nrb, zc, False, hr, wav)
    return W.randomize_state_dict(vae.state_dict(), seed=1)


def close(a, b, tol):
    a = torch.as_tensor(a).double(); b = torch.as_tensor(b).double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item() < tol


@pytest.mark.parametrize("name", list(VAE_CFGS))
def test_vae_restatement_matches_golden(name):
    res, ch, mult, nrb, zc, b, hr, wav = cfg_fields(name)
    g = np.load(os.path.join(GOLD, name + ".npz"))
    p = {k: v.requires_grad_() for k, v in _vae_state(res, ch, mult, nrb, zc, hr, wav).items()}
    x = W.image_batch(b, res, seed=3)
    recon, z = M.vae_forward(p, x)
    assert close(recon, g["recon"], 1e-5) and close(z, g["z"], 1e-5)
    (recon * W.uniform_tensor(tuple(recon.shape), 99)).sum().backward()
    for k in g.files:
        if k.startswith("grad:"):
            assert close(p[k[5:]].grad, g[k], 1e-4), k


def test_frontend_restatements_match_golden():
    """Wavelet front-end (utils.py:206-247) and the area resize (vae_trainer.py:531-533)."""
    g = np.load(os.path.join(GOLD, "frontend.npz"))
    assert close(R.wavelet_transform(W.image_batch(2, 16, seed=12)), g["wavelet"], 1e-6)
    assert close(R.area_resize(W.image_batch(2, 32, seed=13), (16, 16)), g["area"], 1e-6)


def _attn_state():
    import vqgan_training_amd as vq
    return W.randomize_state_dict(vq.ae.AttnBlock(128).state_dict(), seed=9)


def test_attn_block_restatement_matches_golden():
    """ae.py:56-93 (AttnBlock alone: the reference cannot instantiate it inside Encoder/Decoder)."""
    g = np.load(os.path.join(GOLD, "attn_block.npz"))
    p = {"a." + k: v.requires_grad_() for k, v in _attn_state().items()}
    x = W.uniform_tensor((2, 128, 6, 5), 61, -1.5, 1.5).requires_grad_()
    y = R.attn_block(x, p, "a.")
    (y * W.uniform_tensor(tuple(y.shape), 62)).sum().backward()
    assert close(y, g["y"], 1e-5) and close(x.grad, g["grad:x"], 1e-4)
    for k in ("norm.weight", "norm.bias", "qkv.weight", "proj_out.weight"):
        assert close(p["a." + k].grad, g["grad:" + k], 1e-4), k


def test_loss_restatements_match_golden():
    import vqgan_training_amd as vq
    g = np.load(os.path.join(GOLD, "losses.npz"))
    lp = vq.utils.LPIPS(pretrained_path=None)
    p = W.randomize_state_dict(lp.state_dict(), seed=2, relu_net=True)
    a = W.image_batch(2, 32, seed=5).requires_grad_()
    val = M.lpips_forward(p, a, W.image_batch(2, 32, seed=6))
    val.sum().backward()
    assert close(val, g["lpips_val"], 1e-5) and close(a.grad, g["lpips_grad"], 1e-4)
    dp = {k: (v.requires_grad_() if v.dtype.is_floating_point else v) for k, v in
          W.randomize_state_dict(vq.utils.PatchDiscriminator().state_dict(), seed=4, relu_net=True).items()}
    c = W.image_batch(2, 32, seed=7).requires_grad_()
    logits = M.disc_forward(dp, c)
    (logits * W.uniform_tensor(tuple(logits.shape), 11)).sum().backward()
    assert close(logits, g["disc_logits"], 1e-5) and close(c.grad, g["disc_grad_x"], 1e-4)
    assert close(dp["slice2.0.7.weight"].grad, g["disc_grad_w"], 1e-4)
    assert close(dp["binary_classifier2.0.weight"].grad, g["disc_grad_head"], 1e-4)
    real, fake = W.uniform_tensor((3, 8), 21, -2, 2), W.uniform_tensor((3, 8), 22, -2, 2)
    for kind in ("hinge", "bce"):
        l, ar, af, acc = R.gan_disc_loss(real, fake, kind)
        assert close(torch.stack([l, ar, af, acc]), g[kind], 1e-6)
    zz = W.uniform_tensor((2, 4, 8, 8), 23, -3, 3)
    want = g["vae_loss"]
    assert close(0.1 * zz.pow(2).mean(), want[0], 1e-6) and close(zz.abs().std(), want[3], 1e-6)
    gg = W.uniform_tensor((2, 3, 8, 8), 24)
    assert close(R.gradnorm_backward(gg, 0.5), g["gradnorm"], 1e-6)


def _reference_surface():
    with open(G.SURFACE_JSON) as f:
        return json.load(f)


def _shapes(rows):
    return {r[0]: tuple(r[1]) for r in rows}


def test_state_dict_surface_matches_reference():
    """Same keys, shapes and (under the same seed) the same initial values as ae.VAE / utils.* : against the surface recorded from
    the reference's own modules (tests/golden/reference_surface.json; initial values by the sha256 of every tensor)."""
    import vqgan_training_amd as vq
    ref_all = _reference_surface()
    for cfg, ref in zip(G.SURFACE_VAE_CFGS, ref_all["vae"]):
        res, ch, mult, nrb, zc = cfg
        torch.manual_seed(ref_all["vae_seed"])
        ours = vq.ae.VAE(res, 3, ch, 3, list(mult), nrb, zc, False, False, False).state_dict()
        assert [r[0] for r in ref] == list(ours)
        for k, shape, dtype, sha in ref:
            assert tuple(ours[k].shape) == tuple(shape) and str(ours[k].dtype) == "torch." + dtype, k
            assert G.tensor_sha(ours[k]) == sha, k
    our_l = vq.utils.LPIPS(pretrained_path=None).state_dict()
    assert _shapes(ref_all["lpips"]) == {k: tuple(v.shape) for k, v in our_l.items()}
    our_d = vq.utils.PatchDiscriminator().state_dict()
    assert _shapes(ref_all["disc"]) == {k: tuple(v.shape) for k, v in our_d.items()}
    ours_hr = vq.ae.VAE(32, 3, 32, 3, [1, 2], 1, 4, False, True, False).state_dict()
    assert _shapes(ref_all["vae_hr"]) == {k: tuple(v.shape) for k, v in ours_hr.items()}


def test_train_step_restatement_matches_reference_modules():
    """Three restated steps (oracle) vs the same steps assembled from the reference's own modules/functions
    (vae_trainer.py:525-708 with world_size 1, LPIPS eval, hinge GAN), recorded by tests/golden/make_golden.py train_step_fixture:
    same seeded weights (key names and shapes from the recorded surface) and batch."""
    ref_all = _reference_surface()
    res, ch = 32, 32
    assert tuple(G.SURFACE_VAE_CFGS[0]) == (res, ch, [1, 2], 1, 4)
    # (LPIPS / discriminator: this package's modules supply the constant buffers — ScalingLayer, BatchNorm statistics — that the
    # re-randomisation keeps; their surface is the reference's: test_state_dict_surface_matches_reference)
    import vqgan_training_amd as vq
    st = M.RefState(W.randomize_state_dict(G.zeros_like_surface(ref_all["vae"][0]), 1),
                    W.randomize_state_dict(vq.utils.LPIPS(pretrained_path=None).state_dict(), 2, relu_net=True),
                    W.randomize_state_dict(vq.utils.PatchDiscriminator().state_dict(), 4, relu_net=True))
    x = W.image_batch(2, res, seed=8)
    outs_ref = np.load(G.TRAIN_STEP_PREFIX + "_losses.npz")["losses"]
    ref_grads = G.load_chunked(G.TRAIN_STEP_PREFIX + "_grads")
    ref_params = G.load_chunked(G.TRAIN_STEP_PREFIX + "_params")
    assert outs_ref.shape == (3, 3) and set(ref_params) == set(st.vae) and set(ref_grads) <= set(ref_params) and len(ref_grads) > 50
    outs = []
    for it in range(3):
        o = M.train_step_ref(st, x, do_ganloss=True, disc_type="hinge", learning_rate_vae=1e-2, vae_ch=ch,
                             max_steps=10, warmup_steps=2)
        outs.append((o["overall_vae_loss"].item(), o["perceptual_loss"].item(), o["d_loss"].item()))
        if it == 0:
            # gradients before Adam (Adam turns round-off on exactly-zero gradients, e.g. a conv bias in
            # front of a GroupNorm with one channel per group, into +-lr steps — compare those loosely)
            gmax = max(g.abs().max().item() for g in ref_grads.values())
            for k, g in ref_grads.items():
                assert (o["grads"][k] - g).abs().max().item() < 1e-4 * gmax, k
    # steps 2 and 3 run on the updated parameters: the losses pin optimizer + schedule + D update
    assert close(torch.tensor(outs), torch.tensor(outs_ref), 2e-5)
    for k, v in ref_params.items():
        assert (st.vae[k] - v).abs().max().item() < 2.5e-3, k      # bounded by 3 Adam steps of <= lr


def test_checkpoints_interchange_with_reference(tmp_path):
    """N4 wire formats both ways: our bf16 safetensors export holds exactly the reference VAE's state-dict surface in bfloat16 — what
    a strict load into the reference's VAE().bfloat16() (README.hf.md:38-40) needs — and a reference-side `module.`-prefixed torch
    checkpoint (vae_trainer.py:903-907; keys and shapes from the recorded surface) loads into ours."""
    import vqgan_training_amd as vq
    from safetensors.torch import load_file
    ref_rows = _reference_surface()["vae"][0]
    args = (32, 3, 32, 3, [1, 2], 1, 4, False, False, False)
    assert tuple(G.SURFACE_VAE_CFGS[0]) == (args[0], args[2], args[4], args[5], args[6])
    ours = vq.ae.VAE(*args[:4], list(args[4]), *args[5:])
    ours.load_state_dict(W.randomize_state_dict(ours.state_dict(), 1))
    path = str(tmp_path / "x_bf16.pt")
    vq.vae_trainer.export_bf16_safetensors(ours, path)
    wire = load_file(path)
    assert set(wire) == {r[0] for r in ref_rows}                           # strict: no missing, no unexpected key
    for k, shape, dtype, _sha in ref_rows:
        want = torch.bfloat16 if getattr(torch, dtype).is_floating_point else getattr(torch, dtype)
        assert tuple(wire[k].shape) == tuple(shape) and wire[k].dtype == want, k
        assert torch.equal(wire[k], ours.state_dict()[k].to(want)), k
    ref32 = W.randomize_state_dict(G.zeros_like_surface(ref_rows), 7)
    p2 = str(tmp_path / "ref.pt")
    torch.save({"module." + k: v for k, v in ref32.items()}, p2)
    vq.vae_trainer.load_checkpoint(ours, p2)
    for k, v in ours.state_dict().items():
        assert torch.equal(v, ref32[k]), k
