"""DenoisingDiT training at head dim 128 and above 256 tokens on the HIP engine: the reference's fixtures for ONE head of 128
channels (tools/gen_golden_dit_heads.py, tests/golden/g20_dit_dh128_*), and -- by the recipe of
test_training_dropout_matches_oracle_with_same_masks (tests/test_hip_dit.py) -- the CPU oracle with the masks bsi_dropout_mask
exports, at the stated tolerances: per-sample loss 1e-3, every gradient tensor relative L2 1e-2.  tests/test_dit_heads_host.py
pins the oracle at one head first."""
import pytest
import torch

from oracle import bsi_oracle as bo
from oracle import dit_oracle as do
from tests.dit_heads_cases import DEPTH, DIM, FF, HEADS, PATCH, SHAPE, train_fixture
from tests.util import bound, golden, max_rel, rel_l2, rel_linf, replay_draws, report, weights

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make_dit(shape, patch, dim, depth, heads, dropout, W=None, seed=5):
    """W given: those weights; else seeded ones as in the wide case of test_training_dropout_matches_oracle_with_same_masks."""
    from bsi_amd.models.dit import DenoisingDiT
    from bsi_amd.nn import FourierFeatures
    model = DenoisingDiT(shape, patch, dim, depth, heads, dropout=dropout, fourier_features=FourierFeatures(n_min=FF[0], n_max=FF[1]))
    if W is None:
        torch.manual_seed(seed)
        with torch.no_grad():
            for q_ in model.parameters():
                q_.copy_(torch.randn(q_.shape) * (0.02 if q_.ndim > 1 else 0.01))
            model.dit.patch_decoder[0].weight.fill_(1.0)
        W = {k: v.clone() for k, v in model.state_dict().items()}
    else:
        model.load_state_dict(W)
    return model.to(DEV), W


def calib_model(dropout=None):
    return make_dit(SHAPE, PATCH, DIM, DEPTH, HEADS, dropout, weights("dit_ff"))


def make_bsi(model, shape=SHAPE, k=16):
    from bsi_amd import BSI, Discretization
    return BSI(model, data_shape=shape, lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=k, preconditioning="edm",
               discretization=Discretization.image_8bit()).to(DEV)


def draws(B, shape, seed=77):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.round(255 * torch.rand((B, *shape), generator=gen)) / 255) * 2 - 1
    return x, torch.rand((), generator=gen), torch.randperm(B, generator=gen), torch.randn((B, *shape), generator=gen)


def against_oracle_with_same_masks(tag, shape, patch, dim, depth, heads, B, p, W=None, inputs=None):
    """Loss and every parameter gradient of one train_loss(...).mean().backward() with dropout p against the CPU oracle that applies
    the very masks of the kernels.  Returns (model, bsi)."""
    from bsi_amd import _native as N
    T = (shape[1] // patch) * (shape[2] // patch)
    model, W = make_dit(shape, patch, dim, depth, heads, p, W)
    model.train()
    bsi = make_bsi(model, shape)
    x, off, perm, eps = inputs if inputs is not None else draws(B, shape)
    torch.manual_seed(123)
    with replay_draws(DEV, rand=[off], randperm=[perm], randn=[eps]):
        loss = bsi.train_loss(x.to(DEV))
    loss.mean().backward()
    seed = (torch.initial_seed() * 0x9E3779B1 + model._drop_calls * 0x85EBCA77) & 0xFFFFFFFFFFFFFFFF
    drop = {}
    for l in range(depth):
        ma = torch.empty(B * heads * T * T, dtype=torch.uint8, device=DEV)
        mm = torch.empty(B * T * dim, dtype=torch.uint8, device=DEV)
        N.check(N.lib().bsi_dropout_mask(p, seed, 2 * l, B * heads * T, T, N.ptr(ma), N.stream()))
        N.check(N.lib().bsi_dropout_mask(p, seed, 2 * l + 1, B * T, dim, N.ptr(mm), N.stream()))
        drop[("attn", l)] = ma.cpu().float().reshape(B, heads, T, T) / (1 - p)
        drop[("mlp", l)] = mm.cpu().float().reshape(B, T, dim) / (1 - p)
        assert abs(float(ma.float().mean()) - (1 - p)) < 0.01 and abs(float(mm.float().mean()) - (1 - p)) < 0.01
    Wr = {k: v.clone().requires_grad_(True) for k, v in W.items()}
    f = lambda a, b: do.dit_forward(Wr, a, b, patch_size=patch, dim=dim, depth=depth, heads=heads, ff=FF, drop=drop)  # noqa: E731
    ref = bo.BSIOracle(f, data_shape=shape, k=16).train_loss(x, off, perm, eps)
    lerr = max_rel(loss.detach(), ref.detach())
    ref.mean().backward()
    errs = []
    for name, q in model.named_parameters():
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), name
        errs.append((rel_l2(q.grad, Wr[name].grad), name))
    worst = max(errs)
    report("dit_heads_vs_oracle_same_masks", case=tag, tokens=T, dim=dim, heads=heads, p=p, per_sample_max=lerr, worst_tensor_rel_l2=worst[0],
           worst_tensor=worst[1])
    bound(f"test_hip_dit_heads:{tag}:loss", lerr, 1e-3)
    for err, name in errs:
        bound(f"test_hip_dit_heads:{tag}:grad", err, 1e-2)
    return model, bsi


def test_one_head_train_loss_and_gradients_vs_reference():
    """Calibration weights, heads=1, 64 tokens, B 4, no dropout: loss and every gradient against the reference's fixture."""
    g = train_fixture()
    model, _ = calib_model()
    model.train()
    bsi = make_bsi(model)
    with replay_draws(DEV, rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        loss = bsi.train_loss(g["x"].to(DEV))
    lerr = max_rel(loss.detach(), g["loss"])
    loss.mean().backward()
    errs = [(rel_l2(q.grad, g["G." + name]), name) for name, q in model.named_parameters()]
    worst = max(errs)
    report("dit_dh128_train_vs_reference", per_sample_max=lerr, worst_tensor_rel_l2=worst[0], worst_tensor=worst[1])
    bound("test_one_head_train_loss_and_gradients_vs_reference:loss", lerr, 1e-3)
    for err, name in errs:
        bound("test_one_head_train_loss_and_gradients_vs_reference:grad", err, 1e-2)


def test_one_head_eval_forward_vs_reference():
    g = golden("g20_dit_dh128_fwd")
    model, _ = calib_model()
    model.eval()
    with torch.no_grad():
        y = model(g["mu"].to(DEV), g["t"].to(DEV)).cpu()
    err = rel_linf(y, g["out64"])
    report("dit_dh128_fwd_vs_reference", rel_linf=err, ref_fp32_vs_fp64=rel_linf(g["out"], g["out64"]))
    bound("test_one_head_eval_forward_vs_reference", err, 1e-2)


def test_one_head_dropout_vs_oracle_then_eval():
    g = train_fixture()
    model, bsi = against_oracle_with_same_masks("calib_h1", SHAPE, PATCH, DIM, DEPTH, HEADS, 4, 0.3, weights("dit_ff"),
                                                (g["x"], g["offset"], g["perm"], g["eps"]))
    model.eval()  # dropout off: the dropout-free loss of the fixture
    with torch.no_grad(), replay_draws(DEV, rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        bound("test_one_head_dropout_vs_oracle_then_eval:eval", max_rel(bsi.train_loss(g["x"].to(DEV)).cpu(), g["loss"]), 1e-3)


GEOMETRIES = {
    # tag: shape, patch, dim, depth, heads, B, p
    "cifar_paper": ((3, 32, 32), 2, 128, 2, 1, 2, 0.3),   # 256 tokens, one head of 128
    "tutorial": ((3, 32, 32), 4, 128, 2, 1, 2, 0.1),      # 64 tokens, P = 48
    "dim256_h2": ((3, 16, 16), 2, 256, 1, 2, 2, 0.3),     # two heads of 128
    "t384_h2": ((3, 48, 32), 2, 128, 1, 2, 2, 0.3),       # 384 tokens, head dim 64: above the resident kernels
    "t384_h1": ((3, 48, 32), 2, 128, 1, 1, 2, 0.3),       # 384 tokens, head dim 128
}


@pytest.mark.parametrize("tag", list(GEOMETRIES))
def test_geometry_with_dropout_vs_oracle(tag):
    shape, patch, dim, depth, heads, B, p = GEOMETRIES[tag]
    against_oracle_with_same_masks(tag, shape, patch, dim, depth, heads, B, p)


@pytest.mark.parametrize("tag", ["cifar_paper", "t384_h2"])
def test_backward_bit_reproducible(tag):
    shape, patch, dim, depth, heads, B, p = GEOMETRIES[tag]
    model, _ = make_dit(shape, patch, dim, depth, heads, p)
    model.train()
    bsi = make_bsi(model, shape)
    x, off, perm, eps = draws(B, shape, 3)
    grads = []
    for _ in range(2):
        model.zero_grad()
        model._drop_calls = 0
        torch.manual_seed(9)
        with replay_draws(DEV, rand=[off], randperm=[perm], randn=[eps]):
            bsi.train_loss(x.to(DEV)).mean().backward()
        grads.append(torch.cat([q.grad.reshape(-1) for q in model.parameters()]).clone())
    assert bool(torch.isfinite(grads[0]).all())
    assert torch.equal(grads[0], grads[1])


def test_dp_trainer_step_one_head():
    """DPTrainer.train_step on the heads=1 calibration model, in the manner of test_dp_trainer_single_gpu_step."""
    from bsi_amd.dp import DPTrainer
    from oracle.bsi_oracle import clip_adamw_step
    g = train_fixture()
    model, _ = calib_model()
    model.train()
    p0 = {n: q.detach().clone() for n, q in model.named_parameters()}
    tr = DPTrainer(make_bsi(model), lr=5e-4, betas=(0.9, 0.99), weight_decay=1e-2, max_grad_norm=1.0)
    with replay_draws(DEV, rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        loss = tr.train_step(g["x"].to(DEV))
    assert bool(torch.isfinite(torch.as_tensor(loss)).all())
    assert abs(float(loss) / float(g["loss_mean"]) - 1) < 2e-3
    names = [n for n, _ in model.named_parameters()]
    P = [p0[n].cpu().clone() for n in names]
    G = [g["G." + n].clone() for n in names]
    M = [torch.zeros_like(q) for q in P]
    V = [torch.zeros_like(q) for q in P]
    clip_adamw_step(P, G, M, V, 1, lr=5e-4, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=1e-2, max_norm=1.0)
    after = dict(model.named_parameters())
    for n, ref, gref in zip(names, P, G):
        got = after[n].detach().cpu()
        # as in test_dp_trainer_single_gpu_step: compare the update where the reference gradient is not numerical noise
        mask = gref.abs() > 1e-2 * gref.abs().max()
        du, dr = (got - p0[n].cpu())[mask], (ref - p0[n].cpu())[mask]
        bound("test_dp_trainer_step_one_head:update", float((du - dr).abs().mean() / dr.abs().mean()), 1e-3)
    with replay_draws(DEV, rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        loss2 = tr.train_step(g["x"].to(DEV))
    assert bool(torch.isfinite(torch.as_tensor(loss2)).all()) and tr.step_count == 2


def test_head_dim_32_builds_and_is_refused_at_first_train_loss():
    model, _ = make_dit(SHAPE, PATCH, 128, 1, 4, None)
    model.train()
    bsi = make_bsi(model)
    x, off, perm, eps = draws(2, SHAPE)
    with pytest.raises(RuntimeError, match="head dim 32"):
        with replay_draws(DEV, rand=[off], randperm=[perm], randn=[eps]):
            bsi.train_loss(x.to(DEV)).mean().backward()


REFUSED = {"head_dim_32": ((3, 16, 16), 2, 128, 4, "tokens 64, dim 128, head dim 32"),
           "tokens_2048": ((3, 64, 128), 2, 128, 1, "tokens 2048, dim 128, head dim 128"),
           "tokens_96": ((3, 16, 24), 2, 128, 1, "tokens 96, dim 128, head dim 128"),
           "heads_3": ((3, 16, 16), 2, 128, 3, "tokens 64, dim 128, head dim 42")}


@pytest.mark.parametrize("tag", list(REFUSED))
def test_both_engine_entries_refuse_the_same_geometries(tag):
    """bsi_dit_train_forward and bsi_dit_backward name tokens, dim and head dim; refused before any pointer is followed (dummy
    pointers: no device memory is touched)."""
    import ctypes as C
    from bsi_amd import _native as N
    shape, patch, dim, heads, msg = REFUSED[tag]
    lib = N.lib()
    cfg = N.DitConfig(shape[0], shape[1], shape[2], patch, dim, 1, heads, 6, 8)
    p = C.c_void_p(16)
    w, wt, g = N.DitWeights(), N.DitWeightsT(), N.DitGrads()
    w.blocks = C.cast(p, C.POINTER(N.DitBlockWeights))
    wt.blocks = C.cast(p, C.POINTER(N.DitBlockWeightsT))
    g.blocks = C.cast(p, C.POINTER(N.DitBlockGrads))
    assert lib.bsi_dit_train_forward(C.byref(cfg), C.byref(w), 2, p, p, None, None, None, p, p, 0.1, 1, None) == -1
    err = lib.bsi_last_error().decode()
    assert err.startswith("bsi_dit_train_forward: unsupported geometry") and msg in err, err
    assert lib.bsi_dit_backward(C.byref(cfg), C.byref(w), C.byref(wt), C.byref(g), 2, p, None, p, p, 0.1, 1, None) == -1
    err = lib.bsi_last_error().decode()
    assert err.startswith("bsi_dit_backward: unsupported geometry") and msg in err, err
