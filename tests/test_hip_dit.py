"""GPU parity tests of the native DiT engine and of the BSI module surface on top of it, against the
golden vectors generated from the reference (tests/golden) and the CPU oracle.

Tolerances: the denoiser runs its contractions in bf16 MFMA with fp32 accumulation and an
fp32 residual stream, the BSI wrapper in fp32:
  * train_loss per sample rel 1e-3, batch mean rel 1e-4... measured against the fp32 reference;
  * teacher-forced one-step x_hat rel-Linf 1e-2, mu' 1e-2;
  * against an oracle that rounds the same operands to bf16 (isolates kernel bugs from bf16 rounding): 2e-3.
"""
import contextlib
import math
from unittest import mock

import pytest
import torch

from oracle import bsi_oracle as bo
from oracle import dit_oracle as do
from tests.util import TinyConv, bound, golden, max_rel, rel_linf, report, weights

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make_model(tag="dit_ff", ff=True):
    from bsi_amd.models.dit import DenoisingDiT
    from bsi_amd.nn import FourierFeatures
    m = DenoisingDiT((3, 16, 16), 2, 128, 2, 2, dropout=None,
                     fourier_features=FourierFeatures(n_min=6, n_max=8) if ff else None)
    m.load_state_dict(weights(tag))
    return m.to(DEV).eval()


def make_bsi(model, shape=(3, 16, 16), k=16):
    from bsi_amd import BSI, Discretization
    return BSI(model, data_shape=shape, lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=k, preconditioning="edm",
               discretization=Discretization.image_8bit()).to(DEV)


@contextlib.contextmanager
def replay_noise(**queues):
    """Feed recorded draws to the module's torch.rand/randn/randperm/randint calls, in order (the golden
    vectors were drawn from a CPU generator; the GPU generator has a different stream)."""
    qs = {k: list(v) for k, v in queues.items()}

    def pop(name):
        def f(*a, **kw):
            t = qs[name].pop(0)
            return t.to(kw.get("device", DEV))
        return f

    with contextlib.ExitStack() as st:
        for name in qs:
            st.enter_context(mock.patch.object(torch, name, side_effect=pop(name)))
        yield
    assert all(len(v) == 0 for v in qs.values()), "not all recorded draws were consumed"


def oracle_dit(tag, ff, md=None):
    W = weights(tag)
    return lambda mu, t: do.dit_forward(W, mu, t, patch_size=2, dim=128, depth=2, heads=2,
                                        ff=(6, 8) if ff else None, md=md)


def test_dit_forward_vs_golden_and_bf16_oracle():
    g = golden("g7_dit_fwd")
    m = make_model()
    with torch.no_grad():
        y = m(g["mu"].to(DEV), g["t"].to(DEV)).cpu()
        yb = oracle_dit("dit_ff", True, md=torch.bfloat16)(g["mu"], g["t"])
    # vs the fp32 reference: bf16 operand rounding through 2 blocks
    report("tiny_dit_forward", vs_fp32_reference=rel_linf(y, g["out"]), vs_bf16_operand_oracle=rel_linf(y, yb))
    bound("test_dit_forward_vs_golden_and_bf16_oracle:73", rel_linf(y, g["out"]), 1e-2)
    # vs the oracle with the same rounding points: only accumulation order / transcendental ulp remain
    bound("test_dit_forward_vs_golden_and_bf16_oracle:75", rel_linf(y, yb), 4e-3)


def test_models_deepcopy_after_use_and_copies_rebuild_their_caches():
    """copy.deepcopy of a model that has already run (its native caches hold ctypes tables with raw device pointers): the copy comes
    without the caches, rebuilds them on first use and gives the same output; the original keeps its caches."""
    import copy
    g = golden("g7_dit_fwd")
    m = make_model()
    mu, t = g["mu"].to(DEV), g["t"].to(DEV)
    with torch.no_grad():
        a = m(mu, t)
        pack = m._pack
        c = copy.deepcopy(m)
        assert c._pack is None and c._plan is None and m._pack is pack
        b = c(mu, t)
        assert c._pack is not None and c._pack is not pack
    assert torch.equal(a, b)
    g = golden("g7_unet_fwd")
    u = make_unet()
    mu, t = g["mu"].to(DEV), g["t"].to(DEV)
    with torch.no_grad():
        a = u(mu, t)
        c = copy.deepcopy(u)
        assert c._pack is None and c._plan is None
        assert torch.equal(a, c(mu, t))


def test_dit_tokens_blockwise():
    """Residual stream after the blocks (fp32) against the oracle with bf16 rounding points."""
    g = golden("g7_dit_fwd")
    m = make_model()
    with torch.no_grad():
        mod = m.adaln_table(g["t"].to(DEV))
        _, tok = m.forward_native(g["mu"].to(DEV), mod, return_tokens=True)
        W = weights("dit_ff")
        ref = do.dit_forward(W, g["mu"], g["t"], patch_size=2, dim=128, depth=2, heads=2, ff=(6, 8),
                             md=torch.bfloat16, return_tokens=True)
    bound("test_dit_tokens_blockwise:88", rel_linf(tok.cpu().reshape(ref.shape), ref), 1e-3)


def test_train_loss_value_vs_golden():
    for case, tag, ff in [("g4_train_dit", "dit_ff", True), ("g4_train_dit_noff", "dit_noff", False)]:
        g = golden(case)
        bsi = make_bsi(make_model(tag, ff))
        with torch.no_grad(), replay_noise(rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
            loss = bsi.train_loss(g["x"].to(DEV)).cpu()
        # bf16 denoiser vs fp32 reference (Appendix F: per-sample median 4e-5, max 2e-4 on a trained-size model)
        per, mean = max_rel(loss, g["loss"]), abs(float(loss.mean()) / float(g["loss_mean"]) - 1)
        report("tiny_dit_train_loss_vs_golden", case=case, per_sample_max=per, mean_rel=mean)
        assert per < 1e-3, per     # the stated tolerances, also on these 4-sample toy models
        assert mean < 1e-4, mean


def test_sample_history_teacher_forced_and_free_running():
    from bsi_amd import _native as N
    # --- teacher-forced, with Fourier features (free-running is chaotic)
    g = golden("g5_hist_dit_ff")
    bsi = make_bsi(make_model("dit_ff", True), k=int(g["k"]))
    k = int(g["k"])
    t = bsi.default_schedule
    lam, alpha = bsi._schedule(t)
    t_eval = torch.cat([t[:k], t.new_ones(1)])
    with torch.no_grad():
        for i in range(k + 1):
            mu_i = g["mus"][i].to(DEV)
            xh = bsi._predict_x(mu_i, t_eval[i].repeat(mu_i.shape[0]))
            bound("test_sample_history_teacher_forced_and_free_running:117", rel_linf(xh, g["x_hats"][i]), 1e-2)
            if i < k:
                mu_n = torch.empty_like(mu_i)
                y = torch.empty_like(mu_i)
                eps_i = g["eps"][i].to(DEV)
                N.check(N.lib().bsi_refine_step(N.ptr(mu_i), N.ptr(xh.contiguous()), N.ptr(eps_i),
                                                N.ptr(lam), N.ptr(alpha), None, None, i, 1, mu_i.shape[0],
                                                mu_i[0].numel(), None, N.ptr(y), N.ptr(mu_n), N.stream()))
                bound("test_sample_history_teacher_forced_and_free_running:125", rel_linf(mu_n, g["mus"][i + 1]), 1e-2)
                bound("test_sample_history_teacher_forced_and_free_running:126", rel_linf(y, g["ys"][i]), 1e-2)
    # --- free-running without Fourier features through the public API
    g = golden("g5_hist_dit_noff")
    bsi = make_bsi(make_model("dit_noff", False), k=int(g["k"]))
    draws = [g["eps0"]] + list(g["eps"])
    with torch.no_grad(), replay_noise(randn=draws):
        mus, xhs, ys = bsi.sample_history(2)
    assert mus.shape == g["mus"].shape and xhs.shape == g["x_hats"].shape and ys.shape == g["ys"].shape
    for i in range(k + 1):
        bound("test_sample_history_teacher_forced_and_free_running:135", rel_linf(xhs[i], g["x_hats"][i]), 1e-2)
        bound("test_sample_history_teacher_forced_and_free_running:136", rel_linf(mus[i], g["mus"][i]), 1e-2)
    with torch.no_grad(), replay_noise(randn=draws):
        s = bsi.sample(2)
    assert torch.equal(s, xhs[-1])  # sample == last prediction of sample_history, bit for bit


def test_generic_model_path_tinyconv():
    """BSI around an arbitrary torch denoiser (the README Conv2d): fp32 end to end, wrapper kernels native."""
    g = golden("g4_train_tinyconv")
    m = TinyConv()
    m.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("W.")})
    m = m.to(DEV)
    bsi = make_bsi(m, (3, 8, 8))
    with replay_noise(rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        loss = bsi.train_loss(g["x"].to(DEV))
    assert max_rel(loss, g["loss"]) < 1e-4   # fp32 path (MIOpen conv + native wrapper)
    loss.mean().backward()
    for name, p in m.named_parameters():
        bound("test_generic_model_path_tinyconv:164", rel_linf(p.grad, g["G." + name]), 1e-5)
    h = golden("g5_hist_tinyconv")
    m.load_state_dict({k[2:]: v for k, v in h.items() if k.startswith("W.")})
    with torch.no_grad(), replay_noise(randn=[h["eps0"]] + list(h["eps"])):
        mus, xhs, ys = bsi.sample_history(4)
    for a, b in [(mus, h["mus"]), (xhs, h["x_hats"]), (ys, h["ys"])]:
        assert rel_linf(a, b) < 1e-4  # free-running fp32 (no Fourier features): 1e-5 expected


def test_config1_at_stated_size():
    """BASELINE.json configs[0] as stated (README.md:21-35): the README Conv2d denoiser on 3x32x32, batch 32, train_loss +
    free-running sample k = 16, golden g14 generated from the reference; fp32 path: 1e-5 on the mean, 1e-4 per sample / step."""
    from tests.test_oracle_golden import config1_noise
    g = golden("g14_config1")
    off, perm, eps, eps0, eps_s = config1_noise(g)

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.layer = torch.nn.Conv2d(4, 3, 3, padding=1)

        def forward(self, mu, t):
            t = torch.movedim(t.expand((1, *mu.shape[-2:], len(t))), -1, 0)
            return self.layer(torch.cat((mu, t), dim=-3))

    m = Model()
    m.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("W.")})
    m = m.to(DEV)
    bsi = make_bsi(m, (3, 32, 32), k=int(g["k"]))
    with replay_noise(rand=[off], randperm=[perm], randn=[eps]):
        loss = bsi.train_loss(g["x"].to(DEV))
    per, mean = max_rel(loss, g["loss"]), abs(float(loss.mean()) / float(g["loss_mean"]) - 1)
    loss.mean().backward()
    gerr = max(rel_linf(p.grad, g["G." + name]) for name, p in m.named_parameters())
    with torch.no_grad(), replay_noise(randn=[eps0] + list(eps_s)):
        mus, xhs, ys = bsi.sample_history(32)
    with torch.no_grad(), replay_noise(randn=[eps0] + list(eps_s)):
        smp = bsi.sample(32)
    assert torch.equal(smp, xhs[-1])
    traj = max(rel_linf(a[i], b[i]) for a, b in [(mus[:, :4], g["mus_first4"]), (xhs[:, :4], g["x_hats_first4"]),
                                                 (ys[:, :4], g["ys_first4"])] for i in range(a.shape[0]))
    fin = max(rel_linf(smp, g["sample"]), rel_linf(mus[-1], g["mu_last"]))
    report("config1_readme_conv_32x32_b32_k16", train_loss_mean_rel=mean, per_sample_max=per, grad_rel_linf=gerr,
           trajectory_step_max=traj, final_sample=fin)
    assert mean < 1e-5 and per < 1e-4, (mean, per)
    assert gerr < 1e-3, gerr
    assert traj < 1e-4 and fin < 1e-4, (traj, fin)


def test_elbo_vs_golden():
    g = golden("g6_elbo")

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.layer = torch.nn.Conv2d(4, 3, 3, padding=1)

        def forward(self, mu, t):
            t = torch.movedim(t.expand((1, *mu.shape[-2:], len(t))), -1, 0)
            return self.layer(torch.cat((mu, t), dim=-3))

    m = Model()
    m.load_state_dict({k[2:]: v for k, v in g.items() if k.startswith("W.")})
    bsi = make_bsi(m.to(DEV), (3, 8, 8), k=16)
    x = g["x"].to(DEV)
    with torch.no_grad(), replay_noise(randn=[g["eps_r"], g["eps_m"]], rand=[g["offset"]], randperm=[g["perm"]]):
        elbo, bpd, extra = bsi.elbo(x, 3, 4, estimate_var=True)
    bound("test_elbo_vs_golden:231a", max_rel(extra["l_recon"], g["l_recon"]), 2e-4)
    bound("test_elbo_vs_golden:231b", max_rel(extra["l_measure"], g["l_measure"]), 1e-5)
    bound("test_elbo_vs_golden:232a", max_rel(elbo, g["elbo"]), 2e-4)
    bound("test_elbo_vs_golden:232b", max_rel(bpd, g["bpd"]), 1e-5)
    bound("test_elbo_vs_golden:233", max_rel(extra["bpd_var"], g["bpd_var"]), 1e-4)
    with torch.no_grad(), replay_noise(randn=[g["feps_r"], g["feps_m"]], randint=[g["fidx"]]):
        felbo, fbpd, fextra = bsi.finite_elbo(x, 3, 4, t=torch.linspace(0, 1, 17, device=DEV), estimate_var=True)
    bound("test_elbo_vs_golden:236a", max_rel(fextra["l_measure"], g["fl_measure"]), 1e-4)
    bound("test_elbo_vs_golden:236b", max_rel(felbo, g["felbo"]), 1e-5)
    with pytest.raises(AssertionError):
        with torch.no_grad():
            bsi.elbo(x, 1, 4, estimate_var=True)
    bsi.preconditioning = "bogus"
    with pytest.raises(RuntimeError, match="Unknown preconditioning"):
        bsi._predict_x(x, torch.ones(len(x), device=DEV))


def test_full_size_dit_l2_one_forward_vs_oracle():
    """DiT-L/2 (the BASELINE config) at B=2: one preconditioned evaluation against the fp32 CPU oracle."""
    from bsi_amd.models.dit import DenoisingDiT
    from bsi_amd.nn import FourierFeatures
    shape = (3, 32, 32)
    W = do.dit_random_weights(shape, 2, 1024, 24, ff=(6, 8), seed=0)
    m = DenoisingDiT(shape, 2, 1024, 24, 16, fourier_features=FourierFeatures(n_min=6, n_max=8))
    m.load_state_dict(W)
    m = m.to(DEV).eval()
    bsi = make_bsi(m, shape, k=128)
    gen = torch.Generator().manual_seed(0)
    mu = torch.randn((2, *shape), generator=gen) * 2
    t = torch.tensor([0.2, 0.9])
    f = lambda a, b: do.dit_forward(W, a, b, patch_size=2, dim=1024, depth=24, heads=16, ff=(6, 8))  # noqa: E731
    with torch.no_grad():
        got = bsi._predict_x(mu.to(DEV), t.to(DEV)).cpu()
        ref = bo.BSIOracle(f, data_shape=shape, k=128).predict_x(mu, t)
    bound("test_full_size_dit_l2_one_forward_vs_oracle:262", rel_linf(got, ref), 2e-3)
    # size-independent properties at the benchmark batch: determinism and batch-invariance of the chain
    with torch.no_grad():
        a = bsi.sample(4, torch.Generator(DEV).manual_seed(5), t=torch.linspace(0, 1, 5, device=DEV))
        b = bsi.sample(4, torch.Generator(DEV).manual_seed(5), t=torch.linspace(0, 1, 5, device=DEV))
    assert torch.equal(a, b) and torch.isfinite(a).all()


def test_dit_patch4_decoder_larger_than_lds_vs_oracle():
    """DiT-L/4 geometry (config/experiment/imagenet64.yaml: patch 4 -> 48 decoder outputs x dim 1024 = 192 KB of fp32
    decoder weights, more than the LDS holds) at depth 1 on a 32x32 image: forward and parameter gradients against
    autograd through the fp32 CPU oracle."""
    from bsi_amd.models.dit import DenoisingDiT
    from bsi_amd.nn import FourierFeatures
    shape, ps, dim, depth, heads = (3, 32, 32), 4, 1024, 1, 16
    W = do.dit_random_weights(shape, ps, dim, depth, ff=(6, 8), seed=3)
    m = DenoisingDiT(shape, ps, dim, depth, heads, fourier_features=FourierFeatures(n_min=6, n_max=8))
    m.load_state_dict(W)
    m = m.to(DEV).train()
    gen = torch.Generator().manual_seed(1)
    mu = torch.randn((4, *shape), generator=gen)
    t = torch.rand(4, generator=gen)
    r = torch.randn((4, *shape), generator=gen)
    Wr = {k: v.clone().requires_grad_(True) for k, v in W.items()}
    ref = do.dit_forward(Wr, mu, t, patch_size=ps, dim=dim, depth=depth, heads=heads, ff=(6, 8))
    (ref * r).sum().backward()
    got = m(mu.to(DEV), t.to(DEV))
    bound("test_dit_patch4_decoder_larger_than_lds_vs_oracle:289", rel_linf(got.detach().cpu(), ref.detach()), 1e-2)
    (got * r.to(DEV)).sum().backward()
    for name, p in m.named_parameters():
        gref = Wr[name].grad
        err = float((p.grad.cpu().double() - gref.double()).norm() / gref.double().norm().clamp_min(1e-30))
        bound("test_dit_patch4_decoder_larger_than_lds_vs_oracle:294", err, 1e-2)


def test_train_loss_gradients_vs_golden():
    """BSI.train_loss(...).mean().backward() through the HIP training engine vs the reference's gradients (G4)."""
    for case, tag, ff in [("g4_train_dit", "dit_ff", True), ("g4_train_dit_noff", "dit_noff", False)]:
        g = golden(case)
        model = make_model(tag, ff).train()
        bsi = make_bsi(model)
        with replay_noise(rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
            loss = bsi.train_loss(g["x"].to(DEV))
        bound("test_train_loss_gradients_vs_golden:305", max_rel(loss.detach(), g["loss"]), 1e-3)
        loss.mean().backward()
        sq, worst = 0.0, (0.0, None)
        for name, p in model.named_parameters():
            ref = g["G." + name]
            assert p.grad is not None and p.grad.shape == ref.shape, name
            sq += float((p.grad.double() ** 2).sum())
            err = float((p.grad.cpu().double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))
            worst = max(worst, (err, name))
            # bf16 operands in every product of the backward chain: relative L2 error per tensor below 3e-2
            bound("test_train_loss_gradients_vs_golden:315", err, 1e-2)
        assert abs(sq ** 0.5 / float(g["grad_norm"]) - 1) < 1e-2, (sq ** 0.5, float(g["grad_norm"]), worst)


def test_grouped_adaln_path_on_flat_parameters_matches_the_per_block_path_and_the_reference():
    """The training forward runs the per-sample adaLN MLPs of all blocks as TWO grouped launches when the blocks' matrices and biases
    lie at uniform positive strides -- which only the flat parameter buffer of DPTrainer gives (bsi_amd/csrc/dit_train.hip) -- and as
    one split-K GEMM per block and matrix otherwise (other summation order).  Same weights, same draws: the flat-parameter model's
    loss and gradient must agree with the per-block path and with the reference's golden gradients (G4, depth 2)."""
    from bsi_amd.dp import DPTrainer
    g = golden("g4_train_dit")
    plain = make_model("dit_ff", True).train()
    with replay_noise(rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        loss_p = make_bsi(plain).train_loss(g["x"].to(DEV))
    loss_p.mean().backward()
    flat_model = make_model("dit_ff", True).train()
    tr = DPTrainer(make_bsi(flat_model), lr=5e-4, max_grad_norm=1.0)      # re-homes the parameters into one flat buffer
    biases = [blk.adaLN_modulation[2].bias.data_ptr() for blk in flat_model.dit.blocks]
    assert biases[1] > biases[0]                                            # uniform positive strides: the grouped launch is taken
    with replay_noise(rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        loss_f, flat_g = tr._backward(g["x"].to(DEV), None)
    bound("test_grouped_adaln:loss_vs_per_block_path", abs(float(loss_f) / float(loss_p.mean()) - 1), 1e-5)
    bound("test_grouped_adaln:loss_vs_reference", abs(float(loss_f) / float(g["loss_mean"]) - 1), 2e-3)
    worst_p, worst_r = 0.0, 0.0
    for name, o, n in zip(tr.fp.names, tr.fp.offsets, tr.fp.sizes):
        got = flat_g[o:o + n].cpu().double()
        per_block = dict(plain.named_parameters())[name].grad.reshape(-1).cpu().double()
        ref = g["G." + name].reshape(-1).double()
        worst_p = max(worst_p, float((got - per_block).norm() / per_block.norm().clamp_min(1e-30)))
        worst_r = max(worst_r, float((got - ref).norm() / ref.norm().clamp_min(1e-30)))
    bound("test_grouped_adaln:grad_vs_per_block_path", worst_p, 1e-3)
    bound("test_grouped_adaln:grad_vs_reference", worst_r, 1e-2)


def test_fused_clip_adamw_ema_vs_golden():
    """bsi_grad_sqnorm + bsi_clip_adamw_ema against torch.optim.AdamW + clip_grad_norm_ recorded from torch (G8)."""
    import ctypes as C
    from bsi_amd import _native as N
    g = golden("g8_optimizer")
    names = sorted(k[3:] for k in g if k.startswith("p0."))
    flat_p = torch.cat([g["p0." + n].reshape(-1) for n in names]).to(DEV)
    m, v = torch.zeros_like(flat_p), torch.zeros_like(flat_p)
    ema = torch.zeros_like(flat_p)
    sq = torch.zeros(1, device=DEV)
    ws = torch.empty(N.lib().bsi_sqnorm_workspace_bytes(), dtype=torch.uint8, device=DEV)
    for step in (1, 2, 3):
        fg = torch.cat([g[f"g{step}.{n}"].reshape(-1) for n in names]).to(DEV)
        N.check(N.lib().bsi_grad_sqnorm(N.ptr(fg), fg.numel(), N.ptr(sq), N.ptr(ws), N.stream()))
        assert abs(float(sq.sqrt()) / float(g[f"norm{step}"]) - 1) < 1e-6
        N.check(N.lib().bsi_clip_adamw_ema(N.ptr(flat_p), N.ptr(fg), N.ptr(m), N.ptr(v), N.ptr(ema), fg.numel(), N.ptr(sq),
                                           1.0, 1.0, 5e-4, 0.9, 0.99, 1e-8, 1e-2, step, 1.0 if step < 3 else 0.25,
                                           N.stream()))
        ref = torch.cat([g[f"p{step}.{n}"].reshape(-1) for n in names])
        bound("test_fused_clip_adamw_ema_vs_golden:338", rel_linf(flat_p, ref), 1e-6)
        if step == 2:
            ema2 = ema.clone()
            assert torch.equal(ema, flat_p)                       # warm-up: copy
    assert rel_linf(ema, ema2 + 0.25 * (flat_p - ema2)) < 1e-6    # lerp_(p, 1 - decay)


def test_segment_forms_of_the_optimizer_kernels():
    """bsi_sqnorm_segments / bsi_sqnorm_finish / bsi_clip_adamw_ema_segments (the data-parallel step's forms, bsi_amd/dp.py):
    (a) on a table that tiles the buffer they reproduce the golden trajectory G8 like the flat kernels, with parameters, moments and
    EMA BIT-identical to bsi_clip_adamw_ema given the same squared norm; (b) a table over ONE rank's slices with the gradient in a
    compact shard buffer updates exactly those slices to the same bits and leaves the rest untouched; (c) the partial array is the
    same whether all slices are computed at once or each rank's separately and added.  Run on G8 (53 parameters) and on a random
    200 003-element problem whose slices span several chunks with ragged ends, at world 2 and 8."""
    from bsi_amd import _native as N
    from bsi_amd.dp import SQNORM_CHUNK, GradExchange
    lib = N.lib()

    def table(rows):
        arr = (N.Seg * len(rows))(*[N.Seg(*r) for r in rows])
        return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)

    def run(p0, grad_of, ref_of, norm_of, world):
        n0 = p0.numel()
        n = -(-n0 // (world * 4)) * (world * 4)
        pad = lambda t: torch.cat([t, torch.zeros(n - n0)]).to(DEV)  # noqa: E731
        a = world * 4
        cuts = [0, (n // 3) // a * a, (2 * n // 3) // a * a, n]      # three buckets, exchanged last first
        xc = GradExchange([(cuts[i], cuts[i + 1], None) for i in (2, 1, 0)], None, world)
        assert xc.covers(n)
        rows_all, ch_all = xc.segments(range(world), compact=False)
        tab_all = table(rows_all)
        P, M, V, E = pad(p0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        P2, M2, V2, E2 = P.clone(), M.clone(), V.clone(), E.clone()          # flat kernels
        P3, M3, V3, E3 = P.clone(), M.clone(), V.clone(), E.clone()          # per-rank tables + compact gradient
        sq = torch.zeros(1, device=DEV)
        part = torch.zeros(xc.total_chunks, device=DEV)
        for step in (1, 2, 3):
            fg = pad(grad_of(step))
            w = 1.0 if step < 3 else 0.25
            N.check(lib.bsi_sqnorm_segments(N.ptr(fg), N.ptr(tab_all), len(rows_all), ch_all, N.ptr(part), N.stream()))
            N.check(lib.bsi_sqnorm_finish(N.ptr(part), part.numel(), N.ptr(sq), N.stream()))
            assert abs(float(sq.sqrt()) / norm_of(step, fg) - 1) < 1e-6
            acc = torch.zeros_like(part)                                     # (c)
            shards = []
            for r in range(world):
                rows_r, ch_r = xc.segments([r], compact=True)
                shard = torch.cat([fg[po:po + ln] for po, _, ln, _, _ in rows_r])
                shards.append((rows_r, ch_r, table(rows_r), shard))
                own = torch.zeros_like(part)
                N.check(lib.bsi_sqnorm_segments(N.ptr(shard), N.ptr(shards[-1][2]), len(rows_r), ch_r, N.ptr(own), N.stream()))
                acc += own
            assert torch.equal(acc, part)
            args = (1.0, 1.0, 5e-4, 0.9, 0.99, 1e-8, 1e-2, step, w, N.stream())
            N.check(lib.bsi_clip_adamw_ema_segments(N.ptr(P), N.ptr(fg), N.ptr(M), N.ptr(V), N.ptr(E), N.ptr(tab_all), len(rows_all),
                                                    ch_all, N.ptr(sq), *args))
            N.check(lib.bsi_clip_adamw_ema(N.ptr(P2), N.ptr(fg), N.ptr(M2), N.ptr(V2), N.ptr(E2), n, N.ptr(sq), *args))
            for a_, b_ in ((P, P2), (M, M2), (V, V2), (E, E2)):
                assert torch.equal(a_, b_)                                   # (a) same arithmetic, element for element
            if ref_of is not None:
                bound("test_segment_forms_of_the_optimizer_kernels:golden", rel_linf(P[:n0], ref_of(step)), 1e-6)
            for rows_r, ch_r, tab_r, shard in shards:                        # (b) one rank at a time: only its slices move
                before = P3.clone()
                N.check(lib.bsi_clip_adamw_ema_segments(N.ptr(P3), N.ptr(shard), N.ptr(M3), N.ptr(V3), N.ptr(E3), N.ptr(tab_r),
                                                        len(rows_r), ch_r, N.ptr(sq), *args))
                own = torch.zeros(n, dtype=torch.bool, device=DEV)
                for po, _, ln, _, _ in rows_r:
                    own[po:po + ln] = True
                assert torch.equal(P3[~own], before[~own]) and torch.equal(P3[own], P[own])
            assert torch.equal(P3, P) and torch.equal(E3, E) and torch.equal(M3, M) and torch.equal(V3, V)
        return rows_all

    g = golden("g8_optimizer")
    names = sorted(k[3:] for k in g if k.startswith("p0."))
    cat = lambda pre: torch.cat([g[pre + nm].reshape(-1) for nm in names])  # noqa: E731
    run(cat("p0."), lambda s_: cat(f"g{s_}."), lambda s_: cat(f"p{s_}."), lambda s_, fg: float(g[f"norm{s_}"]), 2)
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(200003, generator=gen)
    grads = {s_: torch.randn(200003, generator=gen) * (10.0 ** -s_) for s_ in (1, 2, 3)}
    for world in (2, 8):
        rows = run(p0, lambda s_: grads[s_], None, lambda s_, fg: float(fg.double().norm()), world)
        assert any(ln % SQNORM_CHUNK for _, _, ln, _, _ in rows)
    assert any(ln > SQNORM_CHUNK for _, _, ln, _, _ in rows) or world == 8


def test_dp_trainer_single_gpu_step():
    """DPTrainer.train_step on one GPU: parameters after one step equal clip+AdamW applied to the engine's own
    gradients, EMA copies the weights during warm-up, and the bf16 shadows are refreshed for the next forward."""
    from bsi_amd.dp import DPTrainer
    g = golden("g4_train_dit")
    model = make_model("dit_ff", True).train()
    bsi = make_bsi(model)
    p0 = {n: p.detach().clone() for n, p in model.named_parameters()}
    tr = DPTrainer(bsi, lr=5e-4, betas=(0.9, 0.99), weight_decay=1e-2, max_grad_norm=1.0)
    with replay_noise(rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        loss = tr.train_step(g["x"].to(DEV))
    assert abs(float(loss) / float(g["loss_mean"]) - 1) < 2e-3
    gn = float(tr.last_grad_norm.sqrt())
    assert abs(gn / float(g["grad_norm"]) - 1) < 1e-2
    # reference update from the golden gradients (oracle restatement of clip + AdamW)
    from oracle.bsi_oracle import clip_adamw_step
    names = [n for n, _ in model.named_parameters()]
    P = [p0[n].cpu().clone() for n in names]
    G = [g["G." + n].clone() for n in names]
    M = [torch.zeros_like(p) for p in P]
    V = [torch.zeros_like(p) for p in P]
    clip_adamw_step(P, G, M, V, 1, lr=5e-4, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=1e-2, max_norm=1.0)
    for n, ref, gref in zip(names, P, G):
        got = dict(model.named_parameters())[n].detach().cpu()
        # the first Adam step moves every weight by ~lr*sign(g): compare the update where the reference gradient is
        # not numerical noise (e.g. the key bias has an analytically zero gradient: softmax is shift invariant)
        mask = gref.abs() > 1e-2 * gref.abs().max()
        du, dr = (got - p0[n].cpu())[mask], (ref - p0[n].cpu())[mask]
        bound("test_dp_trainer_single_gpu_step:373", float((du - dr).abs().mean() / dr.abs().mean()), 1e-3)
    for (n, p), (_, e) in zip(model.named_parameters(), tr.ema_model.named_parameters()):
        assert torch.equal(p.detach(), e.detach()), n
    with replay_noise(rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        loss2 = tr.train_step(g["x"].to(DEV))
    assert float(loss2) < float(loss) * 1.05 and torch.isfinite(loss2)
    assert tr.step_count == 2


@pytest.mark.parametrize("side", [16, 32, 1032])
def test_training_dropout_matches_oracle_with_same_masks(side):
    """Dropout sites of the training engine (attention weights, MLP input): the counter-based masks are exported with
    bsi_dropout_mask and applied in the CPU oracle; loss and gradients must agree as in the dropout-free case.  side = 32 gives 256
    tokens: the persistent attention kernels of the DiT-L geometry, whose dropout mask travels as 64-bit lane-mask words
    (attn_dropmask_kernel).  Case 1032 = side 32 at DiT-L's width (dim 1024, 16 heads, one block, seeded weights): there the
    words are computed by the LayerNorm pass in front of the qkv projection (tokens == 16 heads: row m -> mask block m)."""
    from bsi_amd import _native as N
    from bsi_amd.models.dit import DenoisingDiT
    from bsi_amd.nn import FourierFeatures
    p, B, d, heads, depth = 0.3, 4, 128, 2, 2
    wide = side == 1032
    if wide:
        side, B, d, heads, depth = 32, 2, 1024, 16, 1
    T = (side // 2) ** 2
    shape = (3, side, side)
    g = golden("g4_train_dit")
    model = DenoisingDiT(shape, 2, d, depth, heads, dropout=p, fourier_features=FourierFeatures(n_min=6, n_max=8))
    if wide:
        torch.manual_seed(5)
        with torch.no_grad():
            for q_ in model.parameters():
                q_.copy_(torch.randn(q_.shape) * (0.02 if q_.ndim > 1 else 0.01))
            model.dit.patch_decoder[0].weight.fill_(1.0)
        W = {k: v.clone() for k, v in model.state_dict().items()}
    else:
        W = weights("dit_ff")
        model.load_state_dict(W)
    model = model.to(DEV).train()
    bsi = make_bsi(model, shape)
    gen = torch.Generator().manual_seed(77)
    if side == 16:
        x, off, perm, eps = g["x"], g["offset"], g["perm"], g["eps"]
    else:
        x = (torch.round(255 * torch.rand((B, *shape), generator=gen)) / 255) * 2 - 1
        off, perm, eps = torch.rand((), generator=gen), torch.randperm(B, generator=gen), torch.randn((B, *shape), generator=gen)
    torch.manual_seed(123)
    with replay_noise(rand=[off], randperm=[perm], randn=[eps]):
        loss = bsi.train_loss(x.to(DEV))
    loss.mean().backward()
    seed = (torch.initial_seed() * 0x9E3779B1 + model._drop_calls * 0x85EBCA77) & 0xFFFFFFFFFFFFFFFF
    drop = {}
    for l in range(depth):
        ma = torch.empty(B * heads * T * T, dtype=torch.uint8, device=DEV)
        mm = torch.empty(B * T * d, dtype=torch.uint8, device=DEV)
        N.check(N.lib().bsi_dropout_mask(p, seed, 2 * l, B * heads * T, T, N.ptr(ma), N.stream()))
        N.check(N.lib().bsi_dropout_mask(p, seed, 2 * l + 1, B * T, d, N.ptr(mm), N.stream()))
        drop[("attn", l)] = ma.cpu().float().reshape(B, heads, T, T) / (1 - p)
        drop[("mlp", l)] = mm.cpu().float().reshape(B, T, d) / (1 - p)
        assert abs(float(ma.float().mean()) - (1 - p)) < 0.01 and abs(float(mm.float().mean()) - (1 - p)) < 0.01
    Wr = {k: v.clone().requires_grad_(True) for k, v in W.items()}
    f = lambda a, b: do.dit_forward(Wr, a, b, patch_size=2, dim=d, depth=depth, heads=heads, ff=(6, 8), drop=drop)  # noqa: E731
    o = bo.BSIOracle(f, data_shape=shape, k=16)
    ref = o.train_loss(x, off, perm, eps)
    lerr = max_rel(loss.detach(), ref.detach())
    ref.mean().backward()
    worst = (0.0, None)
    for name, q in model.named_parameters():
        r = Wr[name].grad
        worst = max(worst, (float((q.grad.cpu().double() - r.double()).norm() / r.double().norm().clamp_min(1e-30)), name))
    report("dit_dropout_vs_oracle_same_masks", tokens=T, per_sample_max=lerr, worst_tensor_rel_l2=worst[0], worst_tensor=worst[1])
    assert lerr < 1e-3, lerr          # the stated per-sample tolerance, with dropout p = 0.3 on
    assert worst[0] < 1e-2, worst     # and the gradient-tensor bound
    if side != 16:
        return
    # eval() switches dropout off: same loss as the dropout-free golden
    model.eval()
    with torch.no_grad(), replay_noise(rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        bound("test_training_dropout_matches_oracle_with_same_masks:437", max_rel(bsi.train_loss(g["x"].to(DEV)).cpu(), g["loss"]), 1e-3)


# ----------------------------------------------------------------------------------------------
# VDM-UNet on the native engine
# ----------------------------------------------------------------------------------------------
def make_unet(tag="unet_ff", ff=True):
    from bsi_amd.models.pos_emb import NyquistPositionalEmbedding
    from bsi_amd.models.vdm_unet import DenoisingVDMUNet
    from bsi_amd.nn import FourierFeatures
    m = DenoisingVDMUNet((3, 8, 8), NyquistPositionalEmbedding(32, 100), "silu", 64, 1, 4, n_attention_heads=1,
                         dropout=0.1, fourier_features=FourierFeatures(n_min=6, n_max=8) if ff else None)
    m.load_state_dict(weights(tag))
    return m.to(DEV).eval()


def test_unet_forward_vs_golden():
    from oracle import unet_oracle as uo
    g = golden("g7_unet_fwd")
    m = make_unet()
    with torch.no_grad():
        y = m(g["mu"].to(DEV), g["t"].to(DEV)).cpu()
        W = weights("unet_ff")
        yb = uo.unet_forward(W, g["mu"], g["t"], levels=1, ff=(6, 8), has_dropout_slot=True, md=torch.bfloat16)
    bound("test_unet_forward_vs_golden:461", rel_linf(y, g["out"]), 1e-2)
    bound("test_unet_forward_vs_golden:462", rel_linf(y, yb), 1e-2)


def test_unet_sampling_vs_golden():
    # teacher-forced with Fourier features
    g = golden("g5_hist_unet_ff")
    bsi = make_bsi(make_unet("unet_ff", True), (3, 8, 8), k=int(g["k"]))
    k = int(g["k"])
    t = bsi.default_schedule
    t_eval = torch.cat([t[:k], t.new_ones(1)])
    with torch.no_grad():
        for i in range(k + 1):
            mu_i = g["mus"][i].to(DEV)
            xh = bsi._predict_x(mu_i, t_eval[i].repeat(mu_i.shape[0]))
            bound("test_unet_sampling_vs_golden:476", rel_linf(xh, g["x_hats"][i]), 1e-2)
    # free-running without Fourier features through BSI.sample_history (fused native path)
    g = golden("g5_hist_unet_noff")
    bsi = make_bsi(make_unet("unet_noff", False), (3, 8, 8), k=k)
    with torch.no_grad(), replay_noise(randn=[g["eps0"]] + list(g["eps"])):
        mus, xhs, ys = bsi.sample_history(2)
    for i in range(k + 1):
        bound("test_unet_sampling_vs_golden:483", rel_linf(xhs[i], g["x_hats"][i]), 1e-2)
        bound("test_unet_sampling_vs_golden:484", rel_linf(mus[i], g["mus"][i]), 1e-2)


def test_full_size_unet_one_forward_vs_oracle():
    """VDM-UNet of the CIFAR-10 config (dim 128, levels 32, 1 head) at B=2 against the fp32 CPU oracle."""
    from oracle import unet_oracle as uo
    from bsi_amd.models.pos_emb import NyquistPositionalEmbedding
    from bsi_amd.models.vdm_unet import DenoisingVDMUNet
    from bsi_amd.nn import FourierFeatures
    shape = (3, 32, 32)
    W = uo.unet_random_weights(shape, 128, 32, seed=0, ff=(6, 8))
    m = DenoisingVDMUNet(shape, NyquistPositionalEmbedding(32, 100), "silu", 128, 32, 4, n_attention_heads=1, dropout=0.1,
                         fourier_features=FourierFeatures(n_min=6, n_max=8))
    m.load_state_dict(W)
    m = m.to(DEV).eval()
    bsi = make_bsi(m, shape, k=128)
    gen = torch.Generator().manual_seed(0)
    mu = torch.randn((2, *shape), generator=gen) * 2
    t = torch.tensor([0.2, 0.9])
    f = lambda a, b: uo.unet_forward(W, a, b, levels=32, ff=(6, 8), has_dropout_slot=True)  # noqa: E731
    with torch.no_grad():
        got = bsi._predict_x(mu.to(DEV), t.to(DEV)).cpu()
        ref = bo.BSIOracle(f, data_shape=shape, k=128).predict_x(mu, t)
    bound("test_full_size_unet_one_forward_vs_oracle:507", rel_linf(got, ref), 2e-3)


def test_unet_train_loss_gradients_vs_golden():
    """BSI.train_loss(...).mean().backward() through the HIP UNet training engine vs the reference's gradients (G4)."""
    g = golden("g4_train_unet")
    model = make_unet()
    bsi = make_bsi(model, (3, 8, 8))
    with replay_noise(rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        loss = bsi.train_loss(g["x"].to(DEV))
    bound("test_unet_train_loss_gradients_vs_golden:517", max_rel(loss.detach(), g["loss"]), 1e-3)
    loss.mean().backward()
    sq, worst = 0.0, (0.0, None)
    for name, p in model.named_parameters():
        ref = g["G." + name]
        assert p.grad is not None and p.grad.shape == ref.shape, name
        sq += float((p.grad.double() ** 2).sum())
        err = float((p.grad.cpu().double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30))
        worst = max(worst, (err, name))
        bound("test_unet_train_loss_gradients_vs_golden:526", err, 1e-2)
    assert abs(sq ** 0.5 / float(g["grad_norm"]) - 1) < 1e-2, (sq ** 0.5, float(g["grad_norm"]), worst)


def test_unet_training_dropout_and_two_levels_vs_oracle():
    """dim 128, two levels (both skip paths), 16x16, dropout 0.1 in train() mode: the masks the kernels use are exported
    with bsi_dropout_mask and applied in the CPU oracle; loss and gradients against autograd through the oracle."""
    import bsi_amd._native as N
    from oracle import unet_oracle as uo
    from bsi_amd.models.pos_emb import NyquistPositionalEmbedding
    from bsi_amd.models.vdm_unet import DenoisingVDMUNet
    from bsi_amd.nn import FourierFeatures
    shape, dim, levels, p, B = (3, 16, 16), 128, 2, 0.1, 3
    W = uo.unet_random_weights(shape, dim, levels, seed=4, ff=(6, 8))
    m = DenoisingVDMUNet(shape, NyquistPositionalEmbedding(32, 100), "silu", dim, levels, 4, n_attention_heads=1, dropout=p,
                         fourier_features=FourierFeatures(n_min=6, n_max=8))
    m.load_state_dict(W)
    m = m.to(DEV).train()
    bsi = make_bsi(m, shape)
    gen = torch.Generator().manual_seed(9)
    x = (torch.randint(0, 256, (B, *shape), generator=gen).float() / 255) * 2 - 1
    off, perm, eps = torch.rand((), generator=gen), torch.randperm(B, generator=gen), torch.randn((B, *shape), generator=gen)
    torch.manual_seed(77)
    m._drop_calls = 0
    with replay_noise(rand=[off], randperm=[perm], randn=[eps]):
        loss = bsi.train_loss(x.to(DEV))
    loss.mean().backward()
    seed = (torch.initial_seed() * 0x9E3779B1 + 1 * 0x85EBCA77) & 0xFFFFFFFFFFFFFFFF
    names = ([f"u_net.downsampling_blocks.{i}.0." for i in range(levels)] + ["u_net.center_block.0.", "u_net.center_block.2."] +
             [f"u_net.upsampling_blocks.{i}.0." for i in range(levels)])
    drop = {}
    HW = shape[1] * shape[2]
    for blk, pre in enumerate(names):
        mk = torch.empty(B * HW * dim, dtype=torch.uint8, device=DEV)
        N.check(N.lib().bsi_dropout_mask(p, seed, blk, B * HW, dim, N.ptr(mk), N.stream()))
        drop[pre] = mk.cpu().float().reshape(B, shape[1], shape[2], dim).permute(0, 3, 1, 2) / (1 - p)
        assert abs(float(mk.float().mean()) - (1 - p)) < 0.01
    Wr = {k: v.clone().requires_grad_(True) for k, v in W.items()}
    f = lambda a, b: uo.unet_forward(Wr, a, b, levels=levels, ff=(6, 8), has_dropout_slot=True, drop=drop)  # noqa: E731
    ref = bo.BSIOracle(f, data_shape=shape, k=16).train_loss(x, off, perm, eps)
    bound("test_unet_training_dropout_and_two_levels_vs_oracle:566", max_rel(loss.detach(), ref.detach()), 1e-3)
    ref.mean().backward()
    for name, q in m.named_parameters():
        r = Wr[name].grad
        err = float((q.grad.cpu().double() - r.double()).norm() / r.double().norm().clamp_min(1e-30))
        bound("test_unet_training_dropout_and_two_levels_vs_oracle:571", err, 1e-2)


def test_dp_trainer_unet_single_gpu_step():
    """DPTrainer with the UNet (one gradient bucket): loss and gradient norm of the first step match the golden, the EMA
    copies the weights during warm-up, and a second step on the same batch lowers the loss."""
    from bsi_amd.dp import DPTrainer
    g = golden("g4_train_unet")
    model = make_unet()  # eval(): dropout off, as in the golden
    bsi = make_bsi(model, (3, 8, 8))
    tr = DPTrainer(bsi, lr=5e-4, betas=(0.9, 0.99), weight_decay=1e-2, max_grad_norm=1.0)
    with replay_noise(rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        loss = tr.train_step(g["x"].to(DEV))
    assert abs(float(loss) / float(g["loss_mean"]) - 1) < 5e-3
    assert abs(float(tr.last_grad_norm.sqrt()) / float(g["grad_norm"]) - 1) < 1e-2
    for (n, p), (_, e) in zip(model.named_parameters(), tr.ema_model.named_parameters()):
        assert torch.equal(p.detach(), e.detach()), n
    with replay_noise(rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        loss2 = tr.train_step(g["x"].to(DEV))
    assert float(loss2) < float(loss) and torch.isfinite(loss2)


def test_drivers_on_the_native_path():
    """ELBO evaluation loop, schedules and sample export (bsi_amd/drivers.py) driving the HIP path: the loop reproduces
    direct `elbo` / `finite_elbo` calls made with the same generator state; non-linear schedules sample finite images."""
    from bsi_amd import Discretization, drivers as D
    model = make_model("dit_ff", True)
    bsi = make_bsi(model, k=8)
    gen = torch.Generator().manual_seed(3)
    x = (torch.randint(0, 256, (6, 3, 16, 16), generator=gen).float() / 255) * 2 - 1
    batches = [x[:4], x[4:]]
    acc = D.evaluate_elbo(bsi, batches, 2, 2, ["inf", 4], torch.Generator(DEV).manual_seed(11))
    g2 = torch.Generator(DEV).manual_seed(11)
    with torch.no_grad():
        want = [bsi.elbo(b.to(DEV), 2, 2, g2, estimate_var=True) for b in batches]
        want_f = [bsi.finite_elbo(b.to(DEV), 2, 2, g2, estimate_var=True, t=torch.linspace(0, 1, 5, device=DEV)) for b in batches]
    for a, w in ((acc["inf"], want), (acc[4], want_f)):
        bpd = torch.cat([r[1] for r in w]).cpu().double().numpy()
        var = torch.cat([r[2]["bpd_var"] for r in w]).cpu().double().numpy()
        assert abs(a.mean() - bpd.mean()) < 1e-9 and abs(a.mean_var() - (bpd.var(ddof=1) + var.mean()) / 6) < 1e-12
        assert math.isfinite(a.mc_std())
    for name in D.SCHEDULES:
        t = D.sampling_schedule(bsi, name, 8)
        assert t.device.type == "cuda" and abs(float(t[0])) < 1e-6 and abs(float(t[-1]) - 1) < 1e-6
        out = D.generate_samples(bsi, Discretization.image_8bit(), 5, 2, torch.Generator(DEV).manual_seed(1), t=t)
        assert out["samples"].shape == (5, 3, 16, 16) and out["images"].dtype == torch.uint8
        assert torch.isfinite(out["samples"]).all()


def test_dp_trainer_exchange_path_on_one_rank():
    """The multi-GPU gradient exchange (HIP events recorded by the backward, side stream, RCCL all-reduce per block bucket)
    forced on in a process group of ONE rank: the step must equal the exchange-free step bit for bit (sum over one rank,
    1/world = 1), for the DiT (bucketed) and the UNet (single bucket)."""
    import os
    import tempfile
    import torch.distributed as dist
    from bsi_amd.dp import DPTrainer
    store = tempfile.NamedTemporaryFile(delete=False)
    store.close()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method=f"file://{store.name}", rank=0, world_size=1)
    try:
        for make, gname, shape in ((lambda: make_model("dit_ff", True).train(), "g4_train_dit", (3, 16, 16)),
                                   (lambda: make_unet(), "g4_train_unet", (3, 8, 8))):
            g = golden(gname)
            outs = []
            # exchange off / all-reduce over RCCL / sharded step over RCCL (reduce_scatter_tensor into the shard buffer, the segment
            # optimizer kernels, all_gather_into_tensor in place: with one rank a slice is a whole bucket)
            for force, shard in ((False, False), (True, False), (True, True)):
                torch.manual_seed(5)
                model = make()
                model._drop_calls = 0
                tr = DPTrainer(make_bsi(model, shape), lr=5e-4, betas=(0.9, 0.99), weight_decay=1e-2, max_grad_norm=1.0,
                               force_exchange=force, shard_update=shard)
                assert tr.exchange == force
                for _ in range(2):
                    with replay_noise(rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
                        loss = tr.train_step(g["x"].to(DEV))
                tr.gather_ema()
                torch.cuda.synchronize()
                outs.append((float(loss), tr.fp.flat.clone(), tr.ema_fp.flat.clone()))
            assert abs(outs[0][0] - outs[1][0]) <= 1e-6 * abs(outs[0][0]), (gname, outs[0][0], outs[1][0])
            assert outs[2][0] == outs[1][0] and torch.equal(outs[2][1], outs[1][1]) and torch.equal(outs[2][2], outs[1][2]), gname
            # atomics in the backward make the low bits run-dependent; the two paths must agree to fp32 noise
            bound("test_dp_trainer_exchange_path_on_one_rank:651a", rel_linf(outs[1][1], outs[0][1]), 1e-5)
            bound("test_dp_trainer_exchange_path_on_one_rank:651b", rel_linf(outs[1][2], outs[0][2]), 1e-5)
    finally:
        dist.destroy_process_group()
        if os.path.exists(store.name):
            os.unlink(store.name)


@pytest.mark.gpu
def test_sample_graph_replay_matches_eager():
    """BSI.sample(graph=True): the whole chain captured as one HIP graph returns the eager path's samples bit for bit (same
    generator draws), also on a second replay with a new generator state."""
    import torch
    from bsi_amd import BSI, Discretization
    from bsi_amd.models.dit import DenoisingDiT
    from bsi_amd.nn import FourierFeatures
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    model = DenoisingDiT((3, 16, 16), 2, 128, 2, 2, dropout=0.0, fourier_features=FourierFeatures(n_min=6, n_max=7)).to(dev).eval()
    with torch.no_grad():
        for blk in model.dit.blocks:
            blk.adaLN_modulation[-1].weight.normal_(0, 0.02)
    bsi = BSI(model, data_shape=(3, 16, 16), lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=6, preconditioning="edm",
              discretization=Discretization.image_8bit()).to(dev)
    with torch.no_grad():
        for seed in (5, 6):
            a = bsi.sample(3, torch.Generator(dev).manual_seed(seed))
            b = bsi.sample(3, torch.Generator(dev).manual_seed(seed), graph=True)
            assert torch.equal(a, b)
        assert not torch.equal(a, bsi.sample(3, torch.Generator(dev).manual_seed(7), graph=True))


def test_sample_graph_survives_weight_update_and_workspace_growth():
    """the captured graph holds raw pointers to the bf16 weight shadows and the workspace.  After a DPTrainer step
    (weights change through a raw kernel: no parameter version bump) and after an eager call with a larger batch (workspace
    reallocated) a graphed sample must still equal the eager one bit for bit."""
    from bsi_amd.dp import DPTrainer
    g = golden("g4_train_dit")
    model = make_model("dit_ff", True)
    bsi = make_bsi(model, k=6)
    dev = torch.device(DEV, 0)

    def pair(seed):
        with torch.no_grad():
            a = bsi.sample(3, torch.Generator(dev).manual_seed(seed))
            b = bsi.sample(3, torch.Generator(dev).manual_seed(seed), graph=True)
        return a, b

    a0, b0 = pair(5)
    assert torch.equal(a0, b0)
    with torch.no_grad():
        bsi.sample(16, torch.Generator(dev).manual_seed(1))          # larger batch: the shared workspace is reallocated
    a1, b1 = pair(5)
    assert torch.equal(a1, b1) and torch.equal(a1, a0)
    model.train()
    tr = DPTrainer(bsi, lr=5e-2, betas=(0.9, 0.99), weight_decay=1e-2, max_grad_norm=1.0)
    with replay_noise(rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        tr.train_step(g["x"].to(DEV))
    model.eval()
    a2, b2 = pair(5)
    assert torch.equal(a2, b2)
    assert not torch.equal(a2, a0)                                   # the weights did change


def test_sample_with_device_noise():
    """BSI.sample(device_noise=True): measurement noise generated in the kernels from one seed drawn from the generator --
    reproducible for a generator state, different for another, finite, and statistically the same chain (first two moments
    of the final samples over a batch agree with the torch.randn path within sampling error)."""
    bsi = make_bsi(make_model("dit_ff", True), k=8)
    dev = torch.device(DEV, 0)
    with torch.no_grad():
        a = bsi.sample(64, torch.Generator(dev).manual_seed(3), device_noise=True)
        b = bsi.sample(64, torch.Generator(dev).manual_seed(3), device_noise=True)
        c = bsi.sample(64, torch.Generator(dev).manual_seed(4), device_noise=True)
        r = bsi.sample(64, torch.Generator(dev).manual_seed(3))
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(a).all() and a.shape == r.shape
    assert abs(float(a.mean()) - float(r.mean())) < 0.05 and abs(float(a.std()) / float(r.std()) - 1) < 0.1
    with pytest.raises(RuntimeError):
        bsi.sample(2, torch.Generator(dev).manual_seed(3), device_noise=True, graph=True)
