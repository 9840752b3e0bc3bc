"""DenoisingVDMUNet with n_attention_heads 4 and 8 (centre Attention2D at head dims 32 and 16) on the HIP engines against the
reference's fixtures (tools/gen_golden_unet_heads.py, tests/golden/g18_unet_heads_*): forward, teacher-forced sampling,
train_loss with every parameter gradient (tolerances of BASELINE.md §5: batch mean 1e-4, per sample 1e-3, x_hat 1e-2, gradient
tensors 1e-2), a DPTrainer step, reproducibility, and the refusal of a head dim the kernels do not have."""
import pytest
import torch

from tests.unet_attn_weights import FF, count_sketch
from tests.unet_heads_cases import FORWARD, HIST, TRAIN, WEIGHTS, checked_weights, heads_weights
from tests.util import bound, golden, rel_l2, rel_linf, replay_draws, report

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make_model(tag, heads, W=None):
    from bsi_amd.models.pos_emb import NyquistPositionalEmbedding
    from bsi_amd.models.vdm_unet import DenoisingVDMUNet
    from bsi_amd.nn import FourierFeatures
    shape, dim, levels, _, block_attn = WEIGHTS[tag]
    m = DenoisingVDMUNet(shape, NyquistPositionalEmbedding(32, 100), "silu", dim, levels, 4, n_attention_heads=heads, dropout=0.1,
                         downsampling_attention=block_attn, fourier_features=FourierFeatures(n_min=FF[0], n_max=FF[1]))
    m.load_state_dict(W if W is not None else heads_weights(tag))
    return m.to(DEV).eval()


def fixture_model(tag, heads):
    return make_model(tag, heads, checked_weights(tag, golden("w_unet_heads_" + tag)))


def make_bsi(model, shape, k=16):
    from bsi_amd import BSI, Discretization
    return BSI(model, data_shape=shape, lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=k, preconditioning="edm",
               discretization=Discretization.image_8bit()).to(DEV)


def images(n, shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return ((torch.randint(0, 256, (n, *shape), generator=gen).float() / 255) * 2 - 1).to(DEV)


@pytest.mark.parametrize("case", list(FORWARD))
def test_forward_vs_reference(case):
    tag, heads, _, _ = FORWARD[case]
    g = golden(case)
    assert int(g["heads"]) == heads
    m = fixture_model(tag, heads)
    with torch.no_grad():
        y = m(g["mu"].to(DEV), g["t"].to(DEV)).cpu()
    err = rel_linf(y, g["out64"])
    report("unet_heads_fwd", case=case, rel_linf=err, ref_fp32_vs_fp64=rel_linf(g["out"], g["out64"]))
    bound(f"test_forward_vs_reference:{case}", err, 1e-2)


def test_sampling_vs_reference():
    """Teacher-forced through the reference's sample_history (8 heads): x_hat of every step from the reference's mu of that step;
    then a free-running sample is finite."""
    name, tag, heads, n, k, _ = HIST
    g = golden(name)
    shape = WEIGHTS[tag][0]
    assert int(g["k"]) == k and int(g["heads"]) == heads
    bsi = make_bsi(fixture_model(tag, heads), shape, k=k)
    t = bsi.default_schedule
    t_eval = torch.cat([t[:k], t.new_ones(1)])
    worst = 0.0
    with torch.no_grad():
        for i in range(k + 1):
            mu_i = g["mus"][i].to(DEV)
            e = rel_linf(bsi._predict_x(mu_i, t_eval[i].repeat(mu_i.shape[0])), g["x_hats"][i])
            worst = max(worst, e)
            bound(f"test_sampling_vs_reference:step{i}", e, 1e-2)
        s = bsi.sample(2, torch.Generator(DEV).manual_seed(0))
    report("unet_heads_hist", worst=worst)
    assert s.shape == (2, *shape) and torch.isfinite(s).all()


def test_train_loss_gradients_vs_reference():
    """train_loss + .mean().backward() with 8 centre heads vs the reference: loss (batch mean, per sample) and every parameter
    gradient by relative L2 -- exact for tensors up to SKETCH elements, from count sketches (~2 %) above."""
    name, tag, heads, _, _ = TRAIN
    g = golden(name)
    shape = WEIGHTS[tag][0]
    model = fixture_model(tag, heads)
    bsi = make_bsi(model, shape)
    with replay_draws(DEV, rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        loss = bsi.train_loss(g["x"].to(DEV))
    lc = loss.detach().cpu()
    mean_err = float((lc.mean() - g["loss_mean"]).abs() / g["loss_mean"].abs())
    sample_err = float(((lc - g["loss"]).abs() / g["loss"].abs()).max())
    loss.mean().backward()
    worst = (0.0, None)
    errs = []
    for pname, p in model.named_parameters():
        assert p.grad is not None, pname
        ref_norm = float(g["N." + pname])
        if "G." + pname in g:
            ref = g["G." + pname]
            assert p.grad.shape == ref.shape, pname
            err = rel_l2(p.grad, ref)
        else:
            err = float((count_sketch(p.grad) - g["K." + pname]).norm()) / max(ref_norm, 1e-30)
        errs.append((err, pname))
        worst = max(worst, (err, pname))
    report("unet_heads_train", loss_mean=mean_err, loss_per_sample=sample_err, worst_grad=worst[0], worst_name=worst[1])
    bound("test_train_loss_gradients_vs_reference:loss_mean", mean_err, 1e-4)
    bound("test_train_loss_gradients_vs_reference:loss", sample_err, 1e-3)
    for err, pname in errs:
        bound("test_train_loss_gradients_vs_reference:grad", err, 1e-2)


def test_dptrainer_step_with_8_heads():
    from bsi_amd.dp import DPTrainer
    tag = "d128l1"
    shape = WEIGHTS[tag][0]
    m = make_model(tag, 8).train()
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    tr = DPTrainer(make_bsi(m, shape), lr=5e-4, max_grad_norm=1.0)
    loss = tr.train_step(images(4, shape, 4))
    assert torch.isfinite(torch.as_tensor(loss)).all()
    after = dict(m.named_parameters())
    assert all(torch.isfinite(v).all() for v in after.values())
    unchanged = [n for n, v in before.items() if torch.equal(after[n].detach(), v)]
    assert not unchanged, unchanged


@pytest.mark.parametrize("tag,heads", [("d128l2", 8), ("d64l1", 4)])
def test_training_step_bit_reproducible(tag, heads):
    shape = WEIGHTS[tag][0]
    m = make_model(tag, heads)
    bsi = make_bsi(m, shape, k=8)
    x = images(3, shape, 3)
    grads = []
    for _ in range(2):
        m.zero_grad()
        bsi.train_loss(x, torch.Generator(DEV).manual_seed(9)).mean().backward()
        grads.append(torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone())
    assert torch.isfinite(grads[0]).all()
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("heads", [16, 3])
def test_unsupported_head_count_fails_with_geometry_message(heads):
    """dim 128 with 16 heads (head dim 8) or 3 heads builds, as in the reference, and fails at first use."""
    m = make_model("d128l1", heads)
    shape = WEIGHTS["d128l1"][0]
    with pytest.raises(RuntimeError, match=rf"unsupported geometry dim=128 heads={heads}"):
        with torch.no_grad():
            m(torch.zeros((1, *shape), device=DEV), torch.zeros(1, device=DEV))
    with pytest.raises(RuntimeError, match=rf"unsupported geometry dim=128 heads={heads}"):
        make_bsi(m, shape).train_loss(images(2, shape, 1), torch.Generator(DEV).manual_seed(1)).mean().backward()
