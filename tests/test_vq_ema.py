"""EMA codebook (VectorQuantizer(ema=True); vq_vq_ema_accumulate / _update / _reseed): the kernels and the module against the
float64 RESTATEMENT below of the semantics include/vqhip.h and DESIGN.md state, bit-reproducibility under token order and rank
split, reseeding, the wiring into VAETrainStep, snapshots and checkpoints, and the error contract.

The restatement (per step, tokens x_i with codes c_i over the WHOLE batch, K codes, decay g):
    n_k = #{i: c_i = k},  s_k = sum of those x_i
    N_k <- g N_k + (1-g) n_k ;  m_k <- g m_k + (1-g) s_k ;  T = sum N ;  Ns_k = (N_k + eps) / (T + K eps) * T ;  e_k = m_k / Ns_k
in float64 from the fp32 state; N, m, e are each stored rounded to fp32 once (e from the unrounded m, Ns).
Reseeding, after the update of the steps with (step + 1) % reseed_every == 0: for every k with N_k < reseed_below
    e_k = m_k = token[g_k], N_k = 1,  g_k = splitmix64(splitmix64(seed + step) + k) mod n_global
init_from_data: the same for every k on the first training forward, before its lookup.
Usage: perplexity = exp(-sum p log p), p = n_k / sum n; codes used = #{k: n_k > 0}.
Bounds (derived: one fp32 rounding, with a factor 2, plus the fixed-point quantum q = 1 / scale of the statistics):
    |m - m_ref| <= 2^-23 |m_ref| + (1-g) n_k q ;  |e - e_ref| <= 2^-23 |e_ref| + (1-g) n_k q / Ns_k ;  |N - N_ref| <= 2^-23 |N_ref|
"""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

import vqgan_training_amd as vq
from vqgan_training_amd._lib import VQ_F32, lib, ptr, stream_of
from vqgan_training_amd.quantizer import VectorQuantizer
from oracle import vq_oracle
from oracle import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
R23 = 2.0 ** -23


# ----------------------------------------------------------------------------------------------- the restatement
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def picked_token(seed, step, k, n_global):
    return splitmix64((splitmix64((seed + step) & M64) + k) & M64) % n_global


def fixed_quantum(amax, n_global):
    """q = 1 / scale, scale = 2^(60 - e - ceil(log2 n_global)) with 2^e > amax >= 2^(e-1) (vq_fixed_scale)."""
    _, e = math.frexp(amax)
    lg = 0
    while (1 << lg) < n_global:
        lg += 1
    return 2.0 ** -(60 - e - lg)


def ema_ref(N, m, tokens, idx, gamma, eps):
    """One update in float64 from fp32 state -> dict of float64 N, m, e, n, Ns, perplexity, used."""
    K = N.numel()
    idx = idx.reshape(-1)
    n = torch.bincount(idx, minlength=K).double()
    s = torch.zeros(K, tokens.shape[1], dtype=torch.float64).index_add_(0, idx, tokens.double())
    N2 = gamma * N.double() + (1.0 - gamma) * n
    m2 = gamma * m.double() + (1.0 - gamma) * s
    T = N2.sum()
    Ns = (N2 + eps) / (T + K * eps) * T
    p = n / n.sum()
    nz = p > 0
    return {"N": N2, "m": m2, "e": m2 / Ns[:, None], "n": n, "Ns": Ns,
            "perplexity": math.exp(-(p[nz] * p[nz].log()).sum().item()), "used": int(nz.sum())}


def assert_within_bounds(N, m, e, ref, gamma, q):
    nq = ((1.0 - gamma) * ref["n"] * q)[:, None]
    eN = (N.double() - ref["N"]).abs() - R23 * ref["N"].abs()
    em = (m.double() - ref["m"]).abs() - (R23 * ref["m"].abs() + nq)
    ee = (e.double() - ref["e"]).abs() - (R23 * ref["e"].abs() + nq / ref["Ns"][:, None])
    print(f"EMA update: worst excess over the bound  N {eN.max().item():.3e}  m {em.max().item():.3e}  e {ee.max().item():.3e}  "
          f"(q = {q:.3e}; max |N err| {(N.double() - ref['N']).abs().max().item():.3e}, "
          f"|m err| {(m.double() - ref['m']).abs().max().item():.3e}, |e err| {(e.double() - ref['e']).abs().max().item():.3e})")
    assert eN.max().item() <= 0.0 and em.max().item() <= 0.0 and ee.max().item() <= 0.0


def perplexity_of(idx, K):
    n = torch.bincount(idx.reshape(-1), minlength=K).double()
    p = n / n.sum()
    p = p[p > 0]
    return math.exp(-(p * p.log()).sum().item())


# ----------------------------------------------------------------------------------------------- kernel-level helpers
def run_update(dev, tokens, idx, N, m, gamma, eps):
    """absmax -> accumulate -> update through the C ABI on `dev`; -> N, m, codebook, usage (CPU), max |token|."""
    L = lib()
    K, D = m.shape
    n = tokens.shape[0]
    ws = torch.zeros(L.size("vq_vq_ema_workspace", K, D), dtype=torch.uint8, device=dev)
    amax = torch.zeros(1, dtype=torch.float32, device=dev)
    t, i = tokens.contiguous().to(dev), idx.contiguous().to(dev)
    Nd, md = N.clone().to(dev), m.clone().to(dev)
    cb = torch.zeros(K, D, dtype=torch.float32, device=dev)
    usage = torch.zeros(2, dtype=torch.float32, device=dev)
    s = stream_of(t)
    L.call("vq_absmax", ptr(t), t.numel(), VQ_F32, ptr(amax), s)
    L.call("vq_vq_ema_accumulate", ptr(t), ptr(i), n, n, K, D, ptr(amax), ptr(ws), ws.numel(), s)
    L.call("vq_vq_ema_update", ptr(ws), ws.numel(), n, ptr(amax), K, D, gamma, eps, ptr(Nd), ptr(md), ptr(cb), ptr(usage), s)
    return Nd.cpu(), md.cpu(), cb.cpu(), usage.cpu(), float(amax.cpu())


def skewed_problem(n, K, D, live, seed):
    """Random state; indices over the first `live` codes only (the others stay empty), code 0 holding about a third of the tokens;
    token magnitudes spanning 2^-20 .. 1."""
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randn(n, D, generator=g) * torch.exp2(-20 * torch.rand(n, 1, generator=g))
    idx = (torch.rand(n, generator=g) ** 3 * live).long().clamp(0, live - 1)
    N = torch.rand(K, generator=g) * 5.0 * torch.exp2(-10 * torch.rand(K, generator=g))
    m = torch.randn(K, D, generator=g) * N[:, None]
    return tokens, idx, N, m


# ----------------------------------------------------------------------------------------------- 1, 2: one update
def test_one_update_matches_the_restatement(backend):
    n, K, D, gamma, eps = 1024, 48, 8, 0.99, 1e-5
    tokens, idx, N, m = skewed_problem(n, K, D, 40, 3)
    cnt = torch.bincount(idx, minlength=K)
    assert (cnt == 0).sum() >= 8 and cnt[0] >= n // 4                     # some codes empty, one holding about a third
    Nk, mk, ek, usage, amax = run_update(backend.device, tokens, idx, N, m, gamma, eps)
    ref = ema_ref(N, m, tokens, idx, gamma, eps)
    assert amax == tokens.abs().max().item()
    assert_within_bounds(Nk, mk, ek, ref, gamma, fixed_quantum(amax, n))
    assert abs(usage[0].item() - ref["perplexity"]) <= 1e-6 * ref["perplexity"]
    assert usage[1].item() == ref["used"]


def test_update_is_independent_of_the_token_order(backend):
    n, K, D = 1024, 48, 8
    tokens, idx, N, m = skewed_problem(n, K, D, 40, 4)
    g = torch.Generator().manual_seed(5)
    outs = []
    for perm in (torch.arange(n), torch.randperm(n, generator=g), torch.arange(n).flip(0)):
        outs.append(run_update(backend.device, tokens[perm], idx[perm], N, m, 0.99, 1e-5)[:3])
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------- 3: rank split
def test_rank_split_independence(tmp_path, emu_library):
    """Two ranks with the two halves of every batch end each step with N, m and the codebook bit-identical to each other and to one
    process holding the whole batch — through initialisation from data (step 0) and reseeding (steps 1 and 3)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vq_ema_worker as Wk
    env = dict(os.environ, VQ_EMA_OUT=str(tmp_path), OMP_NUM_THREADS="4", VQ_EMU_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29623", os.path.join(ROOT, "tests", "vq_ema_worker.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    ranks = [torch.load(os.path.join(tmp_path, f"rank{k}.pt")) for k in range(2)]
    vq._lib._set_library_for_tests(emu_library)
    try:
        one = Wk.run_steps(Wk.make_quantizer(), 0, 1)
    finally:
        vq._lib._set_library_for_tests(None)
    assert ranks[0]["broadcasts"] == 1 and ranks[1]["broadcasts"] == 1    # codebook, N and m: all fp32, one coalesced buffer
    reseeded = 0
    for s in range(Wk.STEPS):
        for key in ("N", "m", "cb", "usage"):
            assert torch.equal(ranks[0]["steps"][s][key], ranks[1]["steps"][s][key]), (s, key)
            assert torch.equal(ranks[0]["steps"][s][key], one[s][key]), (s, key)
        assert torch.equal(torch.cat([ranks[0]["steps"][s]["idx"], ranks[1]["steps"][s]["idx"]]), one[s]["idx"])
        if s in (1, 3):
            reseeded += int((one[s]["N"] == 1.0).sum())
    assert reseeded > 0, "the scenario must reseed for the test to mean anything"


# ----------------------------------------------------------------------------------------------- 4: reseeding
def run_reseed(dev, N, m, cb, tokens, threshold, step, seed):
    L = lib()
    K, D = m.shape
    Nd, md, cbd, t = N.clone().to(dev), m.clone().to(dev), cb.clone().to(dev), tokens.contiguous().to(dev)
    cand = torch.full((K, D), 9.0, dtype=torch.float32, device=dev)
    args = (ptr(Nd), threshold, step, seed, ptr(t), t.shape[0], 0, t.shape[0], K, D, ptr(cand), ptr(md), ptr(cbd), stream_of(t))
    L.call("vq_vq_ema_reseed", 0, *args)
    mid = (Nd.cpu().clone(), md.cpu().clone(), cbd.cpu().clone())
    L.call("vq_vq_ema_reseed", 1, *args)
    return Nd.cpu(), md.cpu(), cbd.cpu(), mid


def test_reseeding_replaces_exactly_the_dead_codes_by_the_hashed_tokens(backend):
    K, D, n, thr, step, seed = 48, 8, 200, 0.5, 14, 3
    g = torch.Generator().manual_seed(8)
    N = torch.rand(K, generator=g) + 0.05
    N[7] = 0.5                                                           # at the threshold: not below it
    m, cb = torch.randn(K, D, generator=g), torch.randn(K, D, generator=g)
    tokens = torch.randn(n, D, generator=g)
    dead = N < thr
    assert 5 <= int(dead.sum()) <= K - 5
    N2, m2, cb2, mid = run_reseed(backend.device, N, m, cb, tokens, thr, step, seed)
    for a, b in zip(mid, (N, m, cb)):
        assert torch.equal(a, b)                                         # the first phase moves no state
    for k in range(K):
        if dead[k]:
            want = tokens[picked_token(seed, step, k, n)]
            assert torch.equal(cb2[k], want) and torch.equal(m2[k], want) and N2[k].item() == 1.0, k
        else:
            assert torch.equal(cb2[k], cb[k]) and torch.equal(m2[k], m[k]) and N2[k] == N[k], k
    # the picks depend on seed and step
    assert any(picked_token(seed, step, k, n) != picked_token(seed, step + 1, k, n) for k in range(K))
    assert any(picked_token(seed, step, k, n) != picked_token(seed + 1, step, k, n) for k in range(K))


def _train_forward(q, z):
    zl = z.clone().to(q.embedding.weight.device).requires_grad_()
    out, loss, idx = q(zl)
    loss.backward()
    return idx


def test_reseeding_cadence_and_init_from_data(backend):
    dev = backend.device
    K, D = 32, 8
    cb0 = W.uniform_tensor((K, D), 77, -1.5, 1.5)

    def make(**kw):
        q = VectorQuantizer(K, D, ema=True, decay=0.6, **kw)
        with torch.no_grad():
            q.embedding.weight.copy_(cb0)
            q.ema_embed_sum.copy_(cb0)
        return q.to(dev)
    qa, qb = make(reseed_below=0.5, reseed_every=3, seed=5), make()
    zs = [W.uniform_tensor((2, D, 4, 4), 40 + s, -1, 1) for s in range(3)]
    for s, z in enumerate(zs):
        ia, ib = _train_forward(qa, z), _train_forward(qb, z)
        assert torch.equal(ia, ib)
        qa.ema_update(); qb.ema_update()
        same = [torch.equal(a, b) for a, b in ((qa.ema_cluster_size, qb.ema_cluster_size), (qa.ema_embed_sum, qb.ema_embed_sum),
                                               (qa.embedding.weight, qb.embedding.weight))]
        if s < 2:
            assert all(same), (s, same)                                  # off the cadence: nothing is reseeded
    Nb = qb.ema_cluster_size.cpu()
    dead = Nb < 0.5                                                      # 0.6^3 = 0.216 for a code that never won a token
    assert 0 < int(dead.sum()) < K
    tok = zs[2].permute(0, 2, 3, 1).reshape(-1, D)
    Na, ma, ea = qa.ema_cluster_size.cpu(), qa.ema_embed_sum.cpu(), qa.embedding.weight.detach().cpu()
    for k in range(K):
        if dead[k]:
            want = tok[picked_token(5, 2, k, tok.shape[0])]
            assert torch.equal(ea[k], want) and torch.equal(ma[k], want) and Na[k].item() == 1.0
        else:
            assert torch.equal(ea[k], qb.embedding.weight.detach().cpu()[k]) and Na[k] == Nb[k]
    # init_from_data: on the first training forward, before its lookup, every code becomes a token of that batch
    qi = make(init_from_data=True, seed=9)
    with torch.no_grad():
        qi(zs[0].to(dev))                                                # no_grad / eval: nothing moves
    qi.eval(); qi(zs[0].to(dev)); qi.train()
    assert torch.equal(qi.embedding.weight.detach().cpu(), cb0) and qi._pending is None
    idx = _train_forward(qi, zs[0])
    tok0 = zs[0].permute(0, 2, 3, 1).reshape(-1, D)
    e = qi.embedding.weight.detach().cpu()
    for k in range(K):
        assert torch.equal(e[k], tok0[picked_token(9, 0, k, tok0.shape[0])])
    assert torch.equal(qi.ema_embed_sum.cpu(), e) and bool((qi.ema_cluster_size == 1).all())
    assert torch.equal(idx.reshape(-1).cpu(), vq_oracle.nearest(tok0, e)[0])   # the lookup saw the initialised codebook
    _train_forward(qi, zs[1])
    assert torch.equal(qi.embedding.weight.detach().cpu(), e)            # once only


# ----------------------------------------------------------------------------------------------- 5: the feature does its job
def mixture(seed):
    g = torch.Generator().manual_seed(1000 + seed)
    centres = torch.rand(16, 8, generator=g) * 2 - 1

    def batch():
        c = torch.randint(0, 16, (1024,), generator=g)
        return centres[c] + 0.05 * torch.randn(1024, 8, generator=g)
    return centres, [batch() for _ in range(30)], batch()


def simulate_ref(cb0, batches, gamma, eps, init_from_data, reseed_below, reseed_every, seed):
    """The training loop of the restatement, float64 state (nearest code by float64 squared distance, lowest index on ties)."""
    e = cb0.double().clone()
    K = e.shape[0]
    N, m = torch.ones(K, dtype=torch.float64), e.clone()
    for step, x in enumerate(batches):
        x = x.double()
        if step == 0 and init_from_data:
            e = torch.stack([x[picked_token(seed, 0, k, x.shape[0])] for k in range(K)])
            m, N = e.clone(), torch.ones(K, dtype=torch.float64)
        idx = torch.cdist(x, e).argmin(1)
        r = ema_ref(N, m, x, idx, gamma, eps)
        N, m, e = r["N"], r["m"], r["e"]
        if reseed_below > 0 and (step + 1) % reseed_every == 0:
            for k in range(K):
                if N[k] < reseed_below:
                    e[k] = m[k] = x[picked_token(seed, step, k, x.shape[0])]
                    N[k] = 1.0
    return e


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_data_init_and_reseeding_keep_the_codebook_alive(backend, seed):
    """16 Gaussian clusters in 8-D (sigma 0.05), K = 64, 1024 tokens a step, decay 0.9, 30 steps from the package's own
    uniform(-1/K, 1/K) initialisation: plain EMA collapses onto a handful of codes; initialisation from data, or reseeding alone,
    keeps the codebook in use (held-out perplexity >= 32, every cluster centre within 0.3 of a code) — in the float64 restatement
    and in the module."""
    dev = backend.device
    K, D, gamma, eps = 64, 8, 0.9, 1e-5
    centres, batches, held_out = mixture(seed)
    torch.manual_seed(seed)
    cb0 = VectorQuantizer(K, D).embedding.weight.detach().clone()          # the package's own initialisation
    assert cb0.abs().max().item() <= 1.0 / K
    variants = {"plain": {}, "data_init": {"init_from_data": True}, "reseed": {"reseed_below": 0.5, "reseed_every": 5}}
    for name, kw in variants.items():
        q = VectorQuantizer(K, D, ema=True, decay=gamma, eps=eps, seed=seed, **kw)
        with torch.no_grad():
            q.embedding.weight.copy_(cb0)
            q.ema_embed_sum.copy_(cb0)
        q = q.to(dev)
        for x in batches:
            _train_forward(q, x.t().reshape(1, D, 32, 32))               # tokens = the batch rows, in order
            q.ema_update()
        q.eval()
        idx = q(held_out.t().reshape(1, D, 32, 32).to(dev))[2].cpu()
        e = q.embedding.weight.detach().cpu()
        e_ref = simulate_ref(cb0, batches, gamma, eps, kw.get("init_from_data", False), kw.get("reseed_below", 0.0),
                             kw.get("reseed_every", 100), seed)
        got = (perplexity_of(idx, K), torch.cdist(centres, e).min(1).values.max().item())
        ref = (perplexity_of(torch.cdist(held_out.double(), e_ref).argmin(1), K),
               torch.cdist(centres.double(), e_ref).min(1).values.max().item())
        print(f"seed {seed} {name}: module perplexity {got[0]:.2f} worst centre-to-code {got[1]:.3f} | restatement {ref[0]:.2f} {ref[1]:.3f}")
        for perp, dist_ in (got, ref):
            if name == "plain":
                assert perp < 16.0, (name, perp)
            else:
                assert perp >= 32.0 and dist_ <= 0.3, (name, perp, dist_)


# ----------------------------------------------------------------------------------------------- 6, 7: the train step
def _small_step(dev, res, ema, **qkw):
    from vqgan_training_amd import ops
    ops.set_default_precision("fp32x3")
    ch, mult, zc, K = 32, [1, 2], 4, 64
    vae = vq.ae.VAE(res, 3, ch, 3, list(mult), 1, zc, False, False, False)
    vae.load_state_dict(W.randomize_state_dict(vae.state_dict(), 1))
    lp = vq.utils.LPIPS(pretrained_path=None)
    lp.load_state_dict(W.randomize_state_dict(lp.state_dict(), 2, relu_net=True))
    quant = VectorQuantizer(K, zc, beta=0.25, ema=ema, **qkw)
    with torch.no_grad():
        quant.embedding.weight.copy_(W.uniform_tensor((K, zc), 77, -1.5, 1.5))
        if ema:
            quant.ema_embed_sum.copy_(quant.embedding.weight)
    vae, lp, quant = vae.to(dev), lp.to(dev).eval(), quant.to(dev)
    step = vq.vae_trainer.VAETrainStep(vae, lp, None, learning_rate_vae=1e-2, vae_ch=ch, max_steps=10, warmup_steps=1, quantizer=quant)
    return step, vae, quant


def test_train_step_with_an_ema_quantizer(backend):
    dev = backend.device
    res = 32 if backend.name == "gpu" else 16
    x = W.image_batch(2, res, seed=8).to(dev)
    gamma, eps, beta = 0.99, 1e-5, 0.25
    step_e, vae_e, q_e = _small_step(dev, res, True, decay=gamma, eps=eps)
    cb0 = q_e.embedding.weight.detach().cpu().clone()
    # a calibration pass (and any dry step) moves neither N, m nor the codebook, and leaves no statistics behind
    step_e.calibrate_grad_scales(x)
    step_e._dry = True
    try:
        step_e(x)
    finally:
        step_e._dry = False
    assert q_e._pending is None and q_e.ema_steps == 0 and step_e.global_step == 0
    assert torch.equal(q_e.embedding.weight.detach().cpu(), cb0) and torch.equal(q_e.ema_embed_sum.cpu(), cb0)
    assert bool((q_e.ema_cluster_size == 1).all())
    # the codebook is in no optimizer and no gradient bucket
    in_opt = {p.data_ptr() for g in step_e.optimizer_G.param_groups for p in g["params"]}
    assert q_e.embedding.weight.data_ptr() not in in_opt and not q_e.embedding.weight.requires_grad
    assert sum(f.numel for f in step_e.optimizer_G._flat) == sum(p.numel() for p in vae_e.parameters())
    o_e = step_e(x)
    step_p, vae_p, q_p = _small_step(dev, res, False)
    assert q_p.embedding.weight.data_ptr() in {p.data_ptr() for g in step_p.optimizer_G.param_groups for p in g["params"]}
    o_p = step_p(x)
    tok = o_e["z"].permute(0, 2, 3, 1).reshape(-1, 4).cpu()
    assert torch.equal(o_e["indices"].cpu(), o_p["indices"].cpu())
    assert torch.equal(o_e["indices"].reshape(-1).cpu(), vq_oracle.nearest(tok, cb0)[0])
    assert len(set(o_e["indices"].flatten().tolist())) > 4
    # the codebook term never sent gradient to z: encoder and decoder take the same step
    pe, pp = dict(vae_e.named_parameters()), dict(vae_p.named_parameters())
    bit_equal = all(torch.equal(pe[k].detach(), pp[k].detach()) for k in pp)
    print(f"EMA step vs plain step: every encoder / decoder parameter bit-equal: {bit_equal}")
    if not bit_equal:                                                    # expected bit-equal; the bound, per element, otherwise
        for k in pp:
            a, b = pe[k].detach().double(), pp[k].detach().double()
            assert bool(((a - b).abs() <= 1e-6 * b.abs()).all()), k
    a, b = float(o_e["vq_loss"]), float(o_p["vq_loss"]) * beta / (1.0 + beta)
    assert abs(a - b) <= 1e-6 * abs(b), (a, b)
    # the codebook after the step = the restatement applied to out["z"] and out["indices"]
    ref = ema_ref(torch.ones(64), cb0, tok, o_e["indices"].cpu(), gamma, eps)
    assert_within_bounds(q_e.ema_cluster_size.cpu(), q_e.ema_embed_sum.cpu(), q_e.embedding.weight.detach().cpu(), ref, gamma,
                         fixed_quantum(tok.abs().max().item(), tok.shape[0]))
    assert abs(float(o_e["vq_perplexity"]) - ref["perplexity"]) <= 1e-6 * ref["perplexity"]
    assert float(o_e["vq_codes_used"]) == ref["used"]
    assert "vq_perplexity" not in o_p


def test_snapshot_restore_carries_the_ema_state(backend):
    dev = backend.device
    res = 16
    step, vae, q = _small_step(dev, res, True, decay=0.6, init_from_data=True, reseed_below=0.5, reseed_every=2, seed=3)
    xs = [W.image_batch(2, res, seed=8 + i).to(dev) for i in range(2)]
    snap = step.state_snapshot()

    def two_steps():
        for x in xs:
            step(x)
        return [t.detach().cpu().clone() for t in (q.ema_cluster_size, q.ema_embed_sum, q.embedding.weight)]
    first = two_steps()
    assert q.ema_steps == 2 and not torch.equal(first[2], snap["vq_ema"]["codebook"].cpu())
    step.state_restore(snap)
    assert q.ema_steps == 0 and torch.equal(q.embedding.weight.detach().cpu(), snap["vq_ema"]["codebook"].cpu())
    second = two_steps()
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_checkpoints_carry_the_ema_state(backend, tmp_path, monkeypatch):
    from vqgan_training_amd import ops, vae_trainer as T
    monkeypatch.chdir(tmp_path)
    for var in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(ops, "_default_precision", ops.default_precision())
    monkeypatch.setattr(ops, "_fp32_split", ops._fp32_split)
    res, zc, K = (32 if backend.name == "gpu" else 16), 4, 32
    assert set(VectorQuantizer(K, zc).state_dict()) == {"embedding.weight"}              # the plain quantizer is what it was
    quant = VectorQuantizer(K, zc, ema=True, decay=0.9, init_from_data=True)
    assert {n: b.dtype for n, b in quant.named_buffers()} == {"ema_cluster_size": torch.float32, "ema_embed_sum": torch.float32}
    train = [W.image_batch(2, res, seed=20), W.image_batch(2, res, seed=21)]
    kw = dict(batch_size=2, vae_resolution=res, vae_ch=32, vae_ch_mult="1,2", vae_num_res_blocks=1, vae_z_channels=zc,
              run_name="ema", precision="bf16", backend="nccl" if backend.name == "gpu" else "gloo", synthetic=False, log_every=1)
    hist = T.run_training(train_batches=train, test_batches=[W.image_batch(2, res, seed=30)], quantizer=quant, num_epochs=1,
                          max_steps=2, evaluate_every_n_steps=2, **kw)
    assert len(hist) == 2 and all(1.0 <= h["vq_perplexity"] <= K and 1 <= h["vq_codes_used"] <= K for h in hist)
    ck = tmp_path / "ckpt" / "ema" / "vae_epoch_0_step_1.pt"
    sd = torch.load(ck, map_location="cpu")
    assert {"quantizer.embedding.weight", "quantizer.ema_cluster_size", "quantizer.ema_embed_sum"} <= set(sd)
    assert not bool((sd["quantizer.ema_cluster_size"] == 1).all())                       # written after an update
    q2 = VectorQuantizer(K, zc, ema=True, init_from_data=True)
    vae2 = vq.ae.VAE(res, 3, 32, 3, [1, 2], 1, zc, False, False, False)
    T.load_checkpoint(vae2, str(ck), quantizer=q2)                                       # strict
    for k in ("embedding.weight", "ema_cluster_size", "ema_embed_sum"):
        assert torch.equal(q2.state_dict()[k], sd["quantizer." + k])
    assert q2._data_init_done                                                            # a loaded codebook is not re-initialised from data
    # a plain quantizer's checkpoint into an EMA quantizer: N = 1, m = the loaded codebook
    plain = VectorQuantizer(K, zc)
    T.save_checkpoint(vae2, str(tmp_path / "plain.pt"), quantizer=plain)
    q3 = VectorQuantizer(K, zc, ema=True)
    T.load_checkpoint(vae2, str(tmp_path / "plain.pt"), quantizer=q3)
    assert torch.equal(q3.embedding.weight.detach(), plain.embedding.weight.detach())
    assert torch.equal(q3.ema_embed_sum, plain.embedding.weight.detach()) and bool((q3.ema_cluster_size == 1).all())


# ----------------------------------------------------------------------------------------------- 8: error contract
def test_error_contract_of_the_ema_entry_points(emu_library):
    L = emu_library
    K, D, n = 16, 8, 32
    ws = torch.zeros(L.size("vq_vq_ema_workspace", K, D), dtype=torch.uint8)
    assert ws.numel() >= 8 * K * (D + 1)
    tok, idx, amax = torch.zeros(n, D), torch.zeros(n, dtype=torch.int64), torch.ones(1)
    N, m, cb, cand = torch.ones(K), torch.zeros(K, D), torch.zeros(K, D), torch.zeros(K, D)
    P = ptr

    def refused(name, *args):
        rc = getattr(L.dll, name)(*args)
        assert rc < 0, (name, rc)
        assert name.encode() in L.dll.vq_last_error(), (name, L.last_error())
        return rc
    acc = lambda **o: [o.get("tok", P(tok)), o.get("idx", P(idx)), n, n, o.get("K", K), D, o.get("amax", P(amax)), o.get("ws", P(ws)),
                       o.get("nws", ws.numel()), None]
    for bad in ({"tok": None}, {"idx": None}, {"amax": None}, {"ws": None}, {"K": 0}, {"K": -3}):
        assert refused("vq_vq_ema_accumulate", *acc(**bad)) == -1
    assert refused("vq_vq_ema_accumulate", *acc(nws=8 * K * (D + 1) - 8)) == -4
    upd = lambda **o: [o.get("ws", P(ws)), o.get("nws", ws.numel()), n, o.get("amax", P(amax)), o.get("K", K), D, 0.99, 1e-5,
                       o.get("N", P(N)), o.get("m", P(m)), o.get("cb", P(cb)), None, None]
    for bad in ({"ws": None}, {"amax": None}, {"N": None}, {"m": None}, {"cb": None}, {"K": 0}):
        assert refused("vq_vq_ema_update", *upd(**bad)) == -1
    assert refused("vq_vq_ema_update", *upd(nws=64)) == -4
    rs = lambda phase, **o: [phase, o.get("N", P(N)), 0.5, 0, 1, o.get("tok", P(tok)), n, 0, n, o.get("K", K), D,
                             o.get("cand", P(cand)), o.get("m", P(m)), o.get("cb", P(cb)), None]
    for phase, bad in ((0, {"N": None}), (0, {"tok": None}), (0, {"cand": None}), (0, {"K": 0}), (1, {"m": None}), (1, {"cb": None}),
                       (1, {"K": -1}), (2, {})):
        assert refused("vq_vq_ema_reseed", *rs(phase, **bad)) == -1
    assert L.size("vq_vq_ema_workspace", 0, D) == 0
    assert torch.equal(N, torch.ones(K)) and not cb.any()                 # nothing was touched


# ----------------------------------------------------------------------------------------------- 9: configs[4] size
@pytest.mark.gpu
def test_update_at_config5_size(hip_library):
    """8192 tokens x 16384 codes x 32: one update within the derived bounds; two runs and a permuted run bit-identical."""
    vq._lib._set_library_for_tests(hip_library)
    try:
        dev = torch.device("cuda:0")
        n, K, D, gamma, eps = 8192, 16384, 32, 0.99, 1e-5
        tokens, idx, N, m = skewed_problem(n, K, D, 12000, 6)
        outs = [run_update(dev, tokens, idx, N, m, gamma, eps), run_update(dev, tokens, idx, N, m, gamma, eps)]
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
        outs.append(run_update(dev, tokens[perm], idx[perm], N, m, gamma, eps))
        ref = ema_ref(N, m, tokens, idx, gamma, eps)
        Nk, mk, ek, usage, amax = outs[0]
        assert_within_bounds(Nk, mk, ek, ref, gamma, fixed_quantum(amax, n))
        assert abs(usage[0].item() - ref["perplexity"]) <= 1e-6 * ref["perplexity"] and usage[1].item() == ref["used"]
        for o in outs[1:]:
            for a, b in zip(outs[0][:4], o[:4]):
                assert torch.equal(a, b)
    finally:
        vq._lib._set_library_for_tests(None)
