"""Weight EMA: the generator's shadow weights, kept by the fused AdamW launch (include/vqhip.h, VqAdamTensor::ema; optim.FusedAdamW
ema_decay / ema_weights(); VAETrainStep ema_decay, load_ema; run_training --ema_decay).

The bound of one shadow update.  Let u = 2^-24 (fp32 unit round-off).  The kernel computes, in fp32,
    ema' = ema + (p - ema) * w,      w = fl(1 - d) = np.float32(1) - np.float32(d),      0 <= w <= 1,
where p is exactly the value it stored to p.  The float64 restatement below evaluates the same expression, with the same w, from
the p the kernel stored (read back after the launch: this isolates the EMA arithmetic from AdamW's) and the shadow before the
launch.  The fp32 evaluation carries three roundings: the difference (error <= u |p - ema| <= u (|p| + |ema|)), the product (|w| <= 1:
error <= u |p - ema|) and the sum (the result lies between ema and p: error <= u max(|p|, |ema|)), so per element
    |ema_got - ema_ref| <= 3 u (|p| + |ema_before|).
A fused multiply-add only removes the product's rounding, so the bound holds on the emulator and on the GPU alike.  Over several
steps the errors add up (each earlier error is multiplied by d <= 1): the accumulated bound is the sum of the per-step bounds."""
import ctypes
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vqgan_training_amd as vq
from oracle import weights as W
from vqgan_training_amd import ops
from vqgan_training_amd import vae_trainer as T
from vqgan_training_amd._lib import VqAdamTensor, lib, ptr, stream_of
from vqgan_training_amd.optim import FusedAdamW
from vqgan_training_amd.quantizer import VectorQuantizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
f32 = lambda x: float(np.float32(x))      # noqa: E731


def ema_ref(p_out, ema_before, d):
    """float64 restatement of one shadow update and its bound (module docstring); tensors in, float64 tensors out."""
    w = float(np.float32(1) - np.float32(d))
    p, e = p_out.double(), ema_before.double()
    return e + (p - e) * w, 3 * U * (p.abs() + e.abs())


def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


# ----------------------------------------------------------------------------------------------- 1, 2: through the ABI
# scalar tail only; the single-quad loop only (nq = 256); exactly one two-quad trip (nq = 512); a two-quad trip, a single-quad
# remainder and a scalar tail together; a full chunk; a chunk plus one; two chunks plus a ragged quad
SIZES = [1, 5, 1000, 1024, 2048, 2055, 65536, 65537, 131075]
CHUNK = 65536
SENTINEL = 12345.0
HP = dict(lr=f32(3e-3), wd=f32(1e-3), b1=f32(0.9), b2=f32(0.95), eps=f32(1e-8))
ALIGNMENTS = {"aligned": dict(p=0, g=0, m=0, v=0, e=0), "one-float-off": dict(p=1, g=1, m=1, v=1, e=1),
              "shadow-one-float-off": dict(p=0, g=0, m=0, v=0, e=1)}


class _State:
    """One table entry per size; each of p / g / m / v / e (the shadow) in a buffer of its own with the data `4 + shift[k]` floats in
    and sentinels all around.  shadow[i] False: entry i has ema = NULL (its e buffer must stay untouched)."""

    def __init__(self, dev, shift, shadow, sizes=SIZES):
        self.dev, self.sizes, self.shadow = dev, sizes, shadow
        self.off = {k: 4 + shift[k] for k in "pgmve"}
        self.buf = {k: [torch.full((n + 16,), SENTINEL, device=dev) for n in sizes] for k in "pgmve"}
        self.decay = torch.zeros(1, dtype=torch.float32, device=dev)
        table = (VqAdamTensor * len(sizes))()
        for i, n in enumerate(sizes):
            for k in "pgmv":
                setattr(table[i], k, self.buf[k][i].data_ptr() + 4 * self.off[k])
                assert (getattr(table[i], k) % 16 == 0) == (shift[k] == 0)
            table[i].n = n
            if shadow[i]:
                table[i].ema = self.buf["e"][i].data_ptr() + 4 * self.off["e"]
                table[i].ema_decay = self.decay.data_ptr()
                assert (table[i].ema % 16 == 0) == (shift["e"] == 0)
        self.table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        offs = [0]
        for n in sizes:
            offs.append(offs[-1] + -(-n // CHUNK))
        self.chunks = offs[-1]
        self.offs = torch.tensor(offs, dtype=torch.int64, device=dev)

    def put(self, k, values):
        for i, n in enumerate(self.sizes):
            self.buf[k][i][self.off[k]:self.off[k] + n] = values[i].to(self.dev)

    def get(self, k):
        out = []
        for i, n in enumerate(self.sizes):
            b, o = self.buf[k][i].cpu(), self.off[k]
            assert (b[:o] == SENTINEL).all() and (b[o + n:] == SENTINEL).all(), (k, i)      # the guard floats
            out.append(b[o:o + n].clone())
        return out

    def step(self, t, flags=None, n_flags=0, stride=0):
        bc1, bc2 = f32(1.0 - HP["b1"] ** t), f32(1.0 - HP["b2"] ** t)
        lib().call("vq_adamw_multi", ptr(self.table), ptr(self.offs), len(self.sizes), self.chunks, CHUNK, HP["lr"], HP["wd"], HP["b1"],
                   HP["b2"], HP["eps"], bc1, bc2, 1.0, ptr(flags), n_flags, stride, stream_of(self.table))


def _fill(st, sizes, seed):
    """Seeded p, g, m (any sign), v (>= 0) and a shadow that is NOT the parameters."""
    vals = {k: [randn((n,), seed + 100 * j + i) for i, n in enumerate(sizes)] for j, k in enumerate("pgme")}
    vals["v"] = [randn((n,), seed + 900 + i).abs() * 0.1 for i, n in enumerate(sizes)]
    for k in "pgmve":
        st.put(k, vals[k])
    return vals


def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_descriptor_size_and_abi_version(backend):
    """The descriptor grew by two trailing pointers (a zero-initialised ctypes entry reads them as NULL: no shadow), the version is
    12 — asserted on the numbers, not on each other."""
    assert ctypes.sizeof(VqAdamTensor) == 56
    assert [f[0] for f in VqAdamTensor._fields_] == ["p", "g", "m", "v", "n", "ema", "ema_decay"]
    lib().dll.vq_abi_version.restype = ctypes.c_int
    assert lib().dll.vq_abi_version() == 12
    assert vq._lib.ABI_VERSION == 12
    z = VqAdamTensor()
    assert z.ema is None and z.ema_decay is None


@pytest.mark.parametrize("alignment", list(ALIGNMENTS))
def test_shadow_update_through_the_abi(backend, alignment):
    """Nine table entries at the launch's edges (SIZES), chunk 65536, sentinels on both sides of every buffer, three alignments (the
    last: only the shadow one float off — the scalar path, and still right).  Three consecutive launches with the DEVICE scalar
    rewritten in between to 0.5, 0.9, 0.999 and nothing changed on the host: the decay is read on the device.  p, m, v are bitwise
    those of the same launches on a table without shadows; the shadow is within the bound of the module docstring after every
    launch; a table in which every second entry has ema = NULL updates exactly the others; d = 1 leaves the shadow's bits alone."""
    dev, shift = backend.device, ALIGNMENTS[alignment]
    n_t = len(SIZES)
    full = _State(dev, shift, [True] * n_t)
    none = _State(dev, shift, [False] * n_t)
    mixed = _State(dev, shift, [i % 2 == 0 for i in range(n_t)])
    vals = _fill(full, SIZES, 2000)
    _fill(none, SIZES, 2000)
    _fill(mixed, SIZES, 2000)
    worst = 0.0
    for t, d in enumerate((0.5, 0.9, 0.999), start=1):
        before = full.get("e")
        for st in (full, mixed):
            st.decay.fill_(d)                                   # the only thing that changes between the launches
        for st in (full, none, mixed):
            st.step(t)
        got, p_out = full.get("e"), full.get("p")
        for k in "pmv":
            assert _bits_equal(full.get(k), none.get(k)), (t, k)
            assert _bits_equal(mixed.get(k), none.get(k)), (t, k)
        assert _bits_equal(full.get("g"), vals["g"]) and _bits_equal(none.get("e"), vals["e"])     # read only / never touched
        mixed_e = mixed.get("e")
        for i in range(n_t):
            ref, bound = ema_ref(p_out[i], before[i], d)
            err = (got[i].double() - ref).abs()
            assert bool((err <= bound).all()), (t, i, SIZES[i], float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
            assert not torch.equal(got[i], before[i]), (t, i)    # every shadow moved
            want = got[i] if i % 2 == 0 else vals["e"][i]        # mixed table: shadows move, NULL entries' buffers do not
            assert torch.equal(mixed_e[i].view(torch.int32), want.view(torch.int32)), (t, i)
    print(f"shadow update [{alignment}]: worst error / bound {worst:.3f}")
    # d = 1: ema + (p - ema) * 0 — the bits stay, while p, m, v move on
    before, p_before = full.get("e"), full.get("p")
    full.decay.fill_(1.0)
    full.step(4)
    assert _bits_equal(full.get("e"), before) and not _bits_equal(full.get("p"), p_before)


def test_skipped_step_leaves_the_shadow_alone(backend):
    """One raised skip flag: p, m, v AND the shadow are bitwise unchanged (a dropped step must not pull the shadow towards parameters
    that did not move).  Flag cleared: the next launch moves all four."""
    dev = backend.device
    sizes = [5, 2055, 65537]
    st = _State(dev, ALIGNMENTS["aligned"], [True] * 3, sizes)
    _fill(st, sizes, 2100)
    st.decay.fill_(0.5)
    start = {k: st.get(k) for k in "pmve"}
    flags = torch.zeros(3 * 4, dtype=torch.int32, device=dev)
    flags[4] = 1                                               # the second of three flags, stride 4
    st.step(1, flags, 3, 4)
    for k in "pmve":
        assert _bits_equal(st.get(k), start[k]), k
    flags.zero_()
    st.step(1, flags, 3, 4)
    for k in "pmve":
        for a, b in zip(st.get(k), start[k]):
            assert not torch.equal(a, b), k
    for i in range(3):
        ref, bound = ema_ref(st.get("p")[i], start["e"][i], 0.5)
        assert bool(((st.get("e")[i].double() - ref).abs() <= bound).all()), i


# ----------------------------------------------------------------------------------------------- 3: FusedAdamW
SHAPES = [(8, 8, 3, 3), (8,), (8,), (8, 8, 3, 3), (8,)]       # a 3x3 conv weight 8 -> 8, its bias, a GroupNorm gamma | a second group


def _run_optimizer(dev, steps=4, rewind_after=None, **kw):
    """-> (optimizer, per step: [flat_p per group], [flat_ema per group] or None, the host's decay of that step)"""
    ps = [torch.nn.Parameter(W.uniform_tensor(s, 300 + i).to(dev)) for i, s in enumerate(SHAPES)]
    opt = FusedAdamW([{"params": ps[:3], "lr": 3e-3}, {"params": ps[3:], "lr": 1e-3}], weight_decay=1e-3, betas=(0.9, 0.95), **kw)
    hist = []
    for s in range(steps):
        for i, p in enumerate(ps):
            p.grad.copy_((W.uniform_tensor(tuple(p.shape), 4000 + 10 * s + i) * (10.0 ** (i % 3 - 1))).to(dev))
        opt.step()
        opt.zero_grad()
        hist.append(([f.flat_p.cpu().clone() for f in opt._flat],
                     [f.flat_ema.cpu().clone() for f in opt._flat] if opt.ema_decay is not None else None))
        if rewind_after is not None and s == rewind_after:
            opt.rewind(1)
    return opt, ps, hist


def _check_recursion(start_p, hist, decays):
    """The shadow against the float64 recursion over the parameter read-backs, within the accumulated bound."""
    n_groups = len(start_p)
    ref = [p.double() for p in start_p]                        # the shadow starts as a copy of the parameters
    acc = [torch.zeros_like(r) for r in ref]
    prev = [p.clone() for p in start_p]
    for (p_t, e_t), d in zip(hist, decays):
        for i in range(n_groups):
            w = float(np.float32(1) - np.float32(d))
            acc[i] += 3 * U * (p_t[i].double().abs() + prev[i].double().abs())
            ref[i] = ref[i] + (p_t[i].double() - ref[i]) * w
            err = (e_t[i].double() - ref[i]).abs()
            assert bool((err <= acc[i]).all()), (i, d, float((err / acc[i]).max()))
            prev[i] = e_t[i]


def _start_flat():
    return [torch.cat([W.uniform_tensor(s, 300 + i).reshape(-1) for i, s in enumerate(SHAPES)][:3]),
            torch.cat([W.uniform_tensor(s, 300 + i).reshape(-1) for i, s in enumerate(SHAPES)][3:])]


def test_fused_adamw_keeps_the_shadow(backend):
    dev = backend.device
    plain, _, h_plain = _run_optimizer(dev)
    opt, ps, h = _run_optimizer(dev, ema_decay=0.9)
    assert plain.ema_decay is None and all(f.flat_ema is None for f in plain._flat)
    assert [tuple(e.shape) for e in opt.ema_parameters()] == SHAPES
    _check_recursion(_start_flat(), h, [0.9] * 4)
    assert not torch.equal(h[-1][1][0], h[-1][0][0])            # the shadow lags behind the parameters
    # EMA on changes nothing about the parameters
    for (p_a, _), (p_b, _) in zip(h_plain, h):
        assert all(torch.equal(a, b) for a, b in zip(p_a, p_b))
    # the views follow the flat shadow, parameter by parameter
    flat = torch.cat([e.reshape(-1).cpu() for e in opt.ema_parameters()])
    assert torch.equal(flat, torch.cat(h[-1][1]))
    # snapshot(moments=True) / restore carry the shadow; a snapshot without EMA has no such key
    assert "ema" not in plain.snapshot(moments=True)
    snap = opt.snapshot(moments=True)
    for f in opt._flat:
        f.flat_ema.add_(1.0); f.flat_p.mul_(2.0)
    opt.restore(snap)
    assert all(torch.equal(f.flat_ema.cpu(), e) for f, e in zip(opt._flat, h[-1][1])) and opt._step == 4
    # ... and a parameters-only snapshot means a fresh optimizer: shadow == restored parameters
    opt.restore(opt.snapshot())
    assert all(torch.equal(f.flat_ema, f.flat_p) for f in opt._flat) and opt._step == 0
    assert all(torch.equal(f.flat_p.cpu(), p) for f, p in zip(opt._flat, h[-1][0]))


def test_fused_adamw_decay_warmup_follows_the_applied_updates(backend):
    """ema_warmup: the update that makes `_step` equal t runs with d_t = min(0.9, (1 + t) / (10 + t)); `rewind` moves t."""
    dev = backend.device
    warm = lambda t: min(0.9, (1.0 + t) / (10.0 + t))          # noqa: E731
    opt, _, h = _run_optimizer(dev, ema_decay=0.9, ema_warmup=True)
    _check_recursion(_start_flat(), h, [warm(t) for t in (1, 2, 3, 4)])
    assert float(opt._flat[0].ema_d.cpu()) == f32(warm(4)) == float(opt._flat[1].ema_d.cpu())
    # one step is taken back after the second: t runs 1, 2, 2, 3
    opt, _, h = _run_optimizer(dev, ema_decay=0.9, ema_warmup=True, rewind_after=1)
    _check_recursion(_start_flat(), h, [warm(t) for t in (1, 2, 2, 3)])
    assert opt._step == 3 and float(opt._flat[0].ema_d.cpu()) == f32(warm(3))
    # a cap the warm-up reaches: the device scalar is refilled only while the value changes
    opt, _, _ = _run_optimizer(dev, steps=1, ema_decay=0.15, ema_warmup=True)     # (1 + 1) / (10 + 1) = 0.18 > 0.15
    assert opt._ema_d == 0.15
    for f in opt._flat:
        f.ema_d.fill_(0.25)                                     # a refill would overwrite this
    opt.step()
    assert all(float(f.ema_d.cpu()) == 0.25 for f in opt._flat)


# ----------------------------------------------------------------------------------------------- 4 - 6: the tiny VAE
def _models(res, seed=1):
    ch, zc = 32, 4
    vae = vq.ae.VAE(res, 3, ch, 3, [1, 2], 1, zc, False, False, False)
    vae.load_state_dict(W.randomize_state_dict(vae.state_dict(), seed))
    lp = vq.utils.LPIPS(pretrained_path=None)
    lp.load_state_dict(W.randomize_state_dict(lp.state_dict(), 2, relu_net=True))
    return vae, lp


def _quantizer(kind):
    if kind == "plain":
        return None
    q = VectorQuantizer(64, 4, beta=0.25, ema=(kind == "vq_ema"))
    with torch.no_grad():
        q.embedding.weight.copy_(W.uniform_tensor((64, 4), 77, -1.5, 1.5))
        if kind == "vq_ema":
            q.ema_embed_sum.copy_(q.embedding.weight)
    return q


def _step(dev, res, kind, ema_decay):
    vae, lp = _models(res)
    quant = _quantizer(kind)
    vae, lp = vae.to(dev), lp.to(dev).eval()
    if quant is not None:
        quant = quant.to(dev)
    step = T.VAETrainStep(vae, lp, None, learning_rate_vae=1e-2, vae_ch=32, max_steps=10, warmup_steps=0, quantizer=quant,
                          ema_decay=ema_decay)
    return step, vae, quant


def _flat_p(step):
    return [f.flat_p.cpu().clone() for f in step.optimizer_G._flat]


def _flat_e(step):
    return [f.flat_ema.cpu().clone() for f in step.optimizer_G._flat]


LOSSES = ("overall_vae_loss", "perceptual_loss", "vae_loss")
_RUNS = {}


def _train_run(backend, kind, tmp_path_factory):
    """Three steps of the smallest step-test model (resolution 16 on the emulator, 32 on the GPU; ch 32, ch_mult [1, 2], one res
    block, seeded random LPIPS, no discriminator, batch 2, fp32x3) with ema_decay = 0 and with ema_decay = 0.5, the snapshot round
    trip, and (kind "plain") everything else tests 5 and 6 look at.  Computed once per backend and kind, shared, never changed."""
    key = (backend.name, kind)
    if key in _RUNS:
        return _RUNS[key]
    dev = backend.device
    prev = ops.default_precision()
    ops.set_default_precision("fp32x3")
    try:
        res = 32 if backend.name == "gpu" else 16
        xs = [W.image_batch(2, res, seed=8 + i).to(dev) for i in range(5)]
        R = {"res": res}
        off, _, q_off = _step(dev, res, kind, 0.0)
        R["off_losses"] = []
        for x in xs[:3]:
            o = off(x)
            R["off_losses"].append([float(o[k]) for k in LOSSES + (("vq_loss",) if q_off is not None else ())])
        R["off_p"] = _flat_p(off)
        R["off_cb"] = q_off.embedding.weight.detach().cpu().clone() if q_off is not None else None
        assert off.optimizer_G.ema_decay is None
        step, vae, quant = _step(dev, res, kind, 0.5)
        R["start_p"] = _flat_p(step)
        R["losses"], R["hist"] = [], []
        for x in xs[:3]:
            o = step(x)
            R["losses"].append([float(o[k]) for k in LOSSES + (("vq_loss",) if quant is not None else ())])
            R["hist"].append((_flat_p(step), _flat_e(step)))
        if quant is not None:
            cb = quant.embedding.weight
            R["cb_out"] = cb.detach().cpu().clone()
            names = [id(p) for g in step.optimizer_G.param_groups for p in g["params"]]
            R["cb_in_optimizer"] = id(cb) in names
            if R["cb_in_optimizer"]:
                R["cb_shadow"] = step.optimizer_G.ema_parameters()[names.index(id(cb))].detach().cpu().clone()
            with step.ema_weights():
                R["cb_in"] = cb.detach().cpu().clone()
            R["cb_after"] = cb.detach().cpu().clone()
        if kind == "plain":
            tmp = tmp_path_factory.mktemp(f"wema_{backend.name}")
            batches = [W.image_batch(2, res, seed=30).to(dev)]
            R["eval_out"] = T.evaluate(vae, batches)[1]
            T.save_checkpoint(vae, str(tmp / "ck.pt"))
            with step.ema_weights():
                R["eval_in"] = T.evaluate(vae, batches)[1]
                T.save_checkpoint(vae, str(tmp / "ck_ema.pt"))
            R["ck"], R["ck_ema"] = str(tmp / "ck.pt"), str(tmp / "ck_ema.pt")
            fresh, _ = _models(res, seed=5)
            T.load_checkpoint(fresh, R["ck_ema"])                # strict
            R["eval_fresh"] = T.evaluate(fresh.to(dev), batches)[1]
        # state_snapshot -> two more steps -> state_restore -> the same two steps again
        cb_now = (lambda: quant.embedding.weight.detach().cpu().clone()) if quant is not None else (lambda: None)
        snap = step.state_snapshot()
        R["snap_has_ema"] = "ema" in snap["G"]
        for x in xs[3:]:
            step(x)
        R["first"] = (_flat_p(step), _flat_e(step), cb_now())
        step.state_restore(snap)
        R["restored"] = (_flat_p(step), _flat_e(step))
        for x in xs[3:]:
            step(x)
        R["second"] = (_flat_p(step), _flat_e(step), cb_now())
    finally:
        ops.set_default_precision(prev)
    _RUNS[key] = R
    return R


def test_swap_puts_the_shadow_into_the_parameters_and_the_packed_operands(backend):
    """Inside ema_weights() the parameters ARE the shadow and the forward output is bitwise that of a fresh module loaded with the
    shadow's values (the packed conv operands followed); after the exit — also through an exception — parameters and output are what
    they were, and the shadow never changed.  step() inside raises; nesting raises."""
    dev = backend.device
    prev = ops.default_precision()
    ops.set_default_precision("bf16")                          # every conv reads a packed 16-bit copy of its weight
    try:
        res = 16
        vae, _ = _models(res)
        vae = vae.to(dev)
        opt = FusedAdamW(vae.parameters(), lr=1e-3, ema_decay=0.9)
        params = [p for g in opt.param_groups for p in g["params"]]
        with torch.no_grad():
            for i, e in enumerate(opt.ema_parameters()):       # a shadow well away from the parameters
                e.mul_(0.5).add_((W.uniform_tensor(tuple(e.shape), 700 + i) * 0.05).to(dev))
        x = W.image_batch(2, res, seed=8).to(dev)

        @torch.no_grad()
        def fwd(m):
            return m.decoder(m.reg(m.encoder(x))).cpu().clone()
        out_raw = fwd(vae)
        raw = [p.detach().cpu().clone() for p in params]
        shadow = [e.detach().cpu().clone() for e in opt.ema_parameters()]
        ptrs = [p.data_ptr() for p in params]
        fresh, _ = _models(res, seed=3)
        sd = fresh.state_dict()
        sd.update({k: s for (k, _), s in zip(vae.named_parameters(), shadow)})
        fresh.load_state_dict(sd, strict=True)
        out_fresh = fwd(fresh.to(dev))
        assert not torch.equal(out_fresh, out_raw)

        def check_outside():
            assert all(torch.equal(p.detach().cpu(), r) for p, r in zip(params, raw))
            assert all(torch.equal(e.detach().cpu(), s) for e, s in zip(opt.ema_parameters(), shadow))
            assert torch.equal(fwd(vae), out_raw)
        with opt.ema_weights():
            assert [p.data_ptr() for p in params] == ptrs                           # the views keep their storage
            assert all(torch.equal(p.detach().cpu(), s) for p, s in zip(params, shadow))
            assert torch.equal(fwd(vae), out_fresh)
            with pytest.raises(RuntimeError):
                opt.step()
            with pytest.raises(RuntimeError):
                with opt.ema_weights():
                    pass
            assert all(torch.equal(p.detach().cpu(), s) for p, s in zip(params, shadow))   # the refused calls changed nothing
        check_outside()
        with pytest.raises(ZeroDivisionError):
            with opt.ema_weights():
                assert torch.equal(fwd(vae), out_fresh)
                raise ZeroDivisionError
        check_outside()
        opt.step()                                             # and the optimizer steps again
    finally:
        ops.set_default_precision(prev)


@pytest.mark.parametrize("kind", ["plain", "vq", "vq_ema"])
def test_train_step_keeps_the_shadow(backend, kind, tmp_path_factory):
    """The shadow follows the float64 recursion over the per-step parameter read-backs; losses and final parameters (the codebook
    too) are bitwise those of the run with ema_decay = 0; state_snapshot -> two steps -> state_restore -> the same two steps gives
    bitwise equal parameters and shadow.  A gradient-trained codebook has a shadow (and equals it inside the context); an EMA
    codebook is no optimizer parameter, has none, and is the same inside and outside."""
    R = _train_run(backend, kind, tmp_path_factory)
    _check_recursion(R["start_p"], R["hist"], [0.5] * 3)
    assert R["losses"] == R["off_losses"]
    assert all(torch.equal(a, b) for a, b in zip(R["hist"][-1][0], R["off_p"]))
    if kind != "plain":
        assert torch.equal(R["cb_out"], R["off_cb"])
    assert not any(torch.equal(p, e) for p, e in zip(*R["hist"][-1]))
    if kind == "vq":
        assert R["cb_in_optimizer"]
        assert torch.equal(R["cb_in"], R["cb_shadow"]) and not torch.equal(R["cb_in"], R["cb_out"])
        assert torch.equal(R["cb_after"], R["cb_out"])
    if kind == "vq_ema":
        assert not R["cb_in_optimizer"]
        assert torch.equal(R["cb_in"], R["cb_out"]) and torch.equal(R["cb_after"], R["cb_out"])
    assert R["snap_has_ema"]
    assert not torch.equal(R["first"][0][0], R["restored"][0][0])
    for a, b in zip(R["restored"], R["hist"][-1]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    for a, b in zip(R["first"][:2], R["second"][:2]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    if kind != "plain":
        assert torch.equal(R["first"][2], R["second"][2])       # the codebook, trained either way, took the same two steps


def test_evaluate_and_checkpoint_with_the_shadow(backend, tmp_path_factory, caplog):
    R = _train_run(backend, "plain", tmp_path_factory)
    dev = backend.device
    assert not torch.equal(R["eval_in"], R["eval_out"])
    assert torch.equal(R["eval_in"], R["eval_fresh"])
    sd, sd_ema = torch.load(R["ck"], map_location="cpu"), torch.load(R["ck_ema"], map_location="cpu")
    assert set(sd) == set(sd_ema) and all(k.startswith("module.") for k in sd_ema)
    assert all(sd[k].shape == sd_ema[k].shape and sd[k].dtype == sd_ema[k].dtype for k in sd)
    assert T.ema_checkpoint_path("a/b/vae_step_1.pt") == "a/b/vae_step_1_ema.pt"
    # a resumed run: the regular file into the weights, the sibling into the shadow
    prev = ops.default_precision()
    ops.set_default_precision("fp32x3")
    try:
        vae, lp = _models(R["res"], seed=9)
        T.load_checkpoint(vae, R["ck"])
        step = T.VAETrainStep(vae.to(dev), lp.to(dev).eval(), None, learning_rate_vae=1e-2, vae_ch=32, max_steps=10,
                              warmup_steps=0, ema_decay=0.5)
        assert all(torch.equal(a, b) for a, b in zip(_flat_e(step), R["hist"][-1][0]))     # a fresh shadow = the weights
        assert step.load_ema(R["ck_ema"]) is True
        assert all(torch.equal(a, b) for a, b in zip(_flat_e(step), R["hist"][-1][1]))     # the shadow, bit for bit
        assert all(torch.equal(a, b) for a, b in zip(_flat_p(step), R["hist"][-1][0]))     # and the weights are still the weights
        # without the sibling file: shadow == parameters, and the log says so
        with caplog.at_level(logging.INFO):
            assert step.load_ema(R["ck_ema"] + ".missing") is False
        assert all(torch.equal(a, b) for a, b in zip(_flat_e(step), _flat_p(step)))
        assert "EMA weights start from the loaded weights" in caplog.text
    finally:
        ops.set_default_precision(prev)


def test_run_training_evaluates_checkpoints_and_resumes_with_the_shadow(backend, tmp_path, monkeypatch, caplog):
    """--ema_decay: every checkpoint is followed by `<name>_ema<ext>` with the same keys; --load_path resumes the shadow from it."""
    monkeypatch.chdir(tmp_path)
    for var in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(ops, "_default_precision", ops.default_precision())
    monkeypatch.setattr(ops, "_fp32_split", ops._fp32_split)
    res = 32 if backend.name == "gpu" else 16
    train = [W.image_batch(2, res, seed=20), W.image_batch(2, res, seed=21)]
    kw = dict(batch_size=2, vae_resolution=res, vae_ch=32, vae_ch_mult="1,2", vae_num_res_blocks=1, vae_z_channels=4,
              precision="bf16", backend="nccl" if backend.name == "gpu" else "gloo", synthetic=False, log_every=1,
              train_batches=train, test_batches=[W.image_batch(2, res, seed=30)], evaluate_every_n_steps=2, learning_rate_vae=1e-2)
    # (the schedule's warm-up gives step 0 a learning rate of zero: the checkpoint after the third step is the first whose
    # shadow can differ from the weights)
    T.run_training(run_name="wema", ema_decay=0.5, ema_warmup=True, num_epochs=2, max_steps=3, **kw)
    assert sorted(os.listdir(tmp_path / "ckpt" / "wema")) == [f"vae_epoch_0_step_{s}{e}.pt" for s in (1, 3) for e in ("", "_ema")]
    ck = tmp_path / "ckpt" / "wema" / "vae_epoch_0_step_3.pt"
    ck_ema = tmp_path / "ckpt" / "wema" / "vae_epoch_0_step_3_ema.pt"
    sd, sd_ema = torch.load(ck, map_location="cpu"), torch.load(ck_ema, map_location="cpu")
    assert set(sd) == set(sd_ema)
    assert any(not torch.equal(sd[k], sd_ema[k]) for k in sd)
    kw.update(num_epochs=1, max_steps=1)
    T.run_training(run_name="plain", **kw)                      # EMA off: no sibling file
    assert os.listdir(tmp_path / "ckpt" / "plain") == ["vae_epoch_0_step_1.pt"]
    with caplog.at_level(logging.INFO):
        T.run_training(run_name="resumed", ema_decay=0.5, load_path=str(ck), **kw)
        assert "EMA weights start from" not in caplog.text
        T.run_training(run_name="resumed2", ema_decay=0.5, load_path=str(tmp_path / "ckpt" / "plain" / "vae_epoch_0_step_1.pt"), **kw)
        assert "EMA weights start from the loaded weights" in caplog.text


# ----------------------------------------------------------------------------------------------- 7: two ranks
def test_two_ranks_keep_identical_shadows(tmp_path, emu_library):
    """Two steps on different data per rank (gloo, emulator): the shadows start from rank 0's bits (broadcast_parameters runs before
    the step object is built) and stay bitwise equal across the ranks.  (The suite asserts no BITWISE equality between two ranks'
    parameters and one process on the concatenated batch — tests/test_distributed.py compares those to a tolerance — so none is
    asserted for the shadow either.)"""
    env = dict(os.environ, VQ_WEMA_OUT=str(tmp_path), OMP_NUM_THREADS="4", VQ_EMU_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29641", os.path.join(ROOT, "tests", "weight_ema_worker.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r0, r1 = [torch.load(os.path.join(tmp_path, f"rank{k}.pt")) for k in range(2)]
    for key in ("start", "ema", "params"):
        assert all(torch.equal(a, b) for a, b in zip(r0[key], r1[key])), key
    assert any(not torch.equal(a, b) for a, b in zip(r0["ema"], r0["start"]))       # the shadow moved ...
    assert any(not torch.equal(a, b) for a, b in zip(r0["ema"], r0["params"]))      # ... and is not the parameters
