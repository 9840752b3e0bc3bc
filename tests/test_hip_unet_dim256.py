"""DenoisingVDMUNet at dim 256 on the HIP engines against the reference's fixtures (tools/gen_golden_unet_dim256.py,
tests/golden/g19_unet_dim256_*): forward at head dims 128, 64, 32 and 16, per-block attention at head dim 64, another activation,
teacher-forced sampling, train_loss with every parameter gradient (tolerances of BASELINE.md §5: batch mean 1e-4, per sample 1e-3,
x_hat 1e-2, gradient tensors 1e-2), free-running samples, a DPTrainer step, reproducibility, the weight-shadow refresh after an
optimizer step, and the refusal of the head dims and widths the kernels do not have.

Achieved on one MI355X (profiles/r10/unet_dim256.txt): see the PARITY lines of a run."""
import pytest
import torch

from tests.unet_attn_weights import FF, count_sketch
from tests.unet_dim256_cases import DIM, FORWARD, HIST, TRAIN, WEIGHTS, checked_weights, dim256_weights
from tests.util import bound, golden, rel_l2, rel_linf, replay_draws, report

pytestmark = pytest.mark.gpu
DEV = "cuda"


def build(shape, dim, levels, heads, actfn="silu", block_attn=False):
    from bsi_amd.models.pos_emb import NyquistPositionalEmbedding
    from bsi_amd.models.vdm_unet import DenoisingVDMUNet
    from bsi_amd.nn import FourierFeatures
    return DenoisingVDMUNet(shape, NyquistPositionalEmbedding(32, 100), actfn, dim, levels, 4, n_attention_heads=heads, dropout=0.1,
                            downsampling_attention=block_attn, fourier_features=FourierFeatures(n_min=FF[0], n_max=FF[1]))


def fixture_model(tag, heads, actfn="silu"):
    shape, levels, _, block_attn = WEIGHTS[tag]
    m = build(shape, DIM, levels, heads, actfn, block_attn)
    m.load_state_dict(checked_weights(tag, golden("w_unet_dim256_" + tag)))
    return m.to(DEV).eval()


def make_bsi(model, shape, k=16, cls="BSI"):
    import bsi_amd
    from bsi_amd import Discretization
    if cls == "VDM":
        return bsi_amd.VDM(model, data_shape=shape, snr_min=6.73794699909e-3, snr_max=597195.613793, k=k,
                           discretization=Discretization.image_8bit()).to(DEV)
    return bsi_amd.BSI(model, data_shape=shape, lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=k, preconditioning="edm",
                       discretization=Discretization.image_8bit()).to(DEV)


def images(n, shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return ((torch.randint(0, 256, (n, *shape), generator=gen).float() / 255) * 2 - 1).to(DEV)


@pytest.mark.parametrize("case", list(FORWARD))
def test_forward_vs_reference(case):
    tag, heads, actfn, _, _, _ = FORWARD[case]
    g = golden(case)
    assert int(g["heads"]) == heads
    m = fixture_model(tag, heads, actfn)
    with torch.no_grad():
        y = m(g["mu"].to(DEV), g["t"].to(DEV)).cpu()
    err = rel_linf(y, g["out64"])
    report("unet_dim256_fwd", case=case, rel_linf=err, ref_fp32_vs_fp64=rel_linf(g["out"], g["out64"]))
    bound(f"test_forward_vs_reference:{case}", err, 1e-2)


def test_sampling_vs_reference():
    """Teacher-forced through the reference's sample_history (4 heads): x_hat of every step from the reference's mu of that step."""
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
    report("unet_dim256_hist", worst=worst)


@pytest.mark.parametrize("cls", ["BSI", "VDM"])
def test_free_running_samples(cls):
    tag = "d256l1"
    shape = WEIGHTS[tag][0]
    alg = make_bsi(fixture_model(tag, 4), shape, k=8, cls=cls)
    with torch.no_grad():
        s = alg.sample(2, torch.Generator(DEV).manual_seed(0))
    assert s.shape == (2, *shape) and torch.isfinite(s).all()


def test_elbo_bfn_and_deepcopy_run():
    """The remaining paths of the class at dim 256: BSI.elbo / finite_elbo and BFN.sample are finite, and a `copy.deepcopy` of a
    model that has run gives the same forward bits from rebuilt native caches."""
    import copy

    import bsi_amd
    from bsi_amd import Discretization
    tag = "d256l1"
    shape = WEIGHTS[tag][0]
    m = fixture_model(tag, 4)
    bsi = make_bsi(m, shape, k=8)
    x = images(2, shape, 7)
    with torch.no_grad():
        for fn in (bsi.elbo, bsi.finite_elbo):
            elbo, bpd, _ = fn(x, 2, 2, torch.Generator(DEV).manual_seed(3))
            assert torch.isfinite(torch.as_tensor(elbo)).all() and torch.isfinite(torch.as_tensor(bpd)).all()
        bfn = bsi_amd.BFN(m, data_shape=shape, sigma_1=1e-3, k=8, discretization=Discretization.image_8bit()).to(DEV)
        s = bfn.sample(2, torch.Generator(DEV).manual_seed(4))
        assert s.shape == (2, *shape) and torch.isfinite(s).all()
        mu, t = images(2, shape, 8), torch.tensor([0.2, 0.9], device=DEV)
        y = m(mu, t)
        assert torch.equal(copy.deepcopy(m)(mu, t), y)


@pytest.mark.parametrize("name", list(TRAIN))
def test_train_loss_gradients_vs_reference(name):
    """train_loss + .mean().backward() vs the reference: loss (batch mean, per sample) and every parameter gradient by relative
    L2 -- exact for tensors up to SKETCH elements, from count sketches above."""
    tag, heads, actfn, _, _ = TRAIN[name]
    g = golden(name)
    shape = WEIGHTS[tag][0]
    model = fixture_model(tag, heads, actfn)
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
            err = float((count_sketch(p.grad, g["K." + pname].numel()) - g["K." + pname]).norm()) / max(ref_norm, 1e-30)
        errs.append((err, pname))
        worst = max(worst, (err, pname))
    report("unet_dim256_train", case=name, loss_mean=mean_err, loss_per_sample=sample_err, worst_grad=worst[0], worst_name=worst[1])
    bound(f"test_train_loss_gradients_vs_reference:{name}:loss_mean", mean_err, 1e-4)
    bound(f"test_train_loss_gradients_vs_reference:{name}:loss", sample_err, 1e-3)
    for err, pname in errs:
        bound(f"test_train_loss_gradients_vs_reference:{name}:grad", err, 1e-2)


def test_dptrainer_step():
    from bsi_amd.dp import DPTrainer
    tag = "d256l1"
    shape = WEIGHTS[tag][0]
    m = fixture_model(tag, 4).train()
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    tr = DPTrainer(make_bsi(m, shape), lr=5e-4, max_grad_norm=1.0)
    loss = tr.train_step(images(4, shape, 4))
    assert torch.isfinite(torch.as_tensor(loss)).all()
    after = dict(m.named_parameters())
    assert all(torch.isfinite(v).all() for v in after.values())
    unchanged = [n for n, v in before.items() if torch.equal(after[n].detach(), v)]
    assert not unchanged, unchanged


@pytest.mark.parametrize("tag,heads", [("d256l1", 4), ("d256l2", 8)])
def test_training_step_bit_reproducible(tag, heads):
    shape = WEIGHTS[tag][0]
    m = fixture_model(tag, heads)
    bsi = make_bsi(m, shape, k=8)
    x = images(3, shape, 3)
    grads = []
    for _ in range(2):
        m.zero_grad()
        bsi.train_loss(x, torch.Generator(DEV).manual_seed(9)).mean().backward()
        grads.append(torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone())
    assert torch.isfinite(grads[0]).all()
    assert torch.equal(grads[0], grads[1])


def test_inference_sees_an_optimizer_step():
    """The bf16 weight shadows are refreshed after an optimizer step: the inference forward equals that of a fresh model holding
    the stepped weights, and differs from the forward before the step."""
    tag = "d256l1"
    shape = WEIGHTS[tag][0]
    m = fixture_model(tag, 4)
    mu, t = images(2, shape, 5), torch.tensor([0.3, 0.7], device=DEV)
    with torch.no_grad():
        y0 = m(mu, t).clone()
    opt = torch.optim.SGD(m.parameters(), lr=1e-2)
    make_bsi(m, shape).train_loss(images(2, shape, 6), torch.Generator(DEV).manual_seed(2)).mean().backward()
    opt.step()
    with torch.no_grad():
        y1 = m(mu, t).clone()
    fresh = build(shape, DIM, WEIGHTS[tag][1], 4)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    with torch.no_grad():
        y2 = fresh.to(DEV).eval()(mu, t)
    assert not torch.equal(y0, y1)
    assert torch.equal(y1, y2)


@pytest.mark.parametrize("dim,heads", [(256, 1), (256, 3), (96, 3)])
def test_unsupported_geometry_fails_with_message(dim, heads):
    """dim 256 with 1 head (head dim 256: no kernel) or 3 heads, and dim 96, build as in the reference and fail at first use."""
    shape = (3, 8, 8)
    m = build(shape, dim, 1, heads).to(DEV).eval()
    with pytest.raises(RuntimeError, match=rf"unsupported geometry dim={dim} heads={heads}"):
        with torch.no_grad():
            m(torch.zeros((1, *shape), device=DEV), torch.zeros(1, device=DEV))
    with pytest.raises(RuntimeError, match=rf"unsupported geometry dim={dim} heads={heads}"):
        make_bsi(m, shape).train_loss(images(2, shape, 1), torch.Generator(DEV).manual_seed(1)).mean().backward()
