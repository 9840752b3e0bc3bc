"""DenoisingDiT at decoder widths P = patch^2 * C in (64, 256] on the HIP engines, sampling and training: the reference's patch-8
fixtures (tools/gen_golden_dit_patch.py, tests/golden/g21_dit_patch8_*; tests/test_dit_patch_host.py pins the oracle on them
first) and, for the widths without a fixture, the fp64 CPU oracle (tests/dit_patch_cases.py), at the stated tolerances of
BASELINE.md section 5: x_hat 1e-2 relative L-inf, loss 1e-4 (batch mean) and 1e-3 (per sample), every gradient tensor 1e-2
relative L2.  P > 256 is refused by all three engine entries."""
import pytest
import torch

from tests import dit_patch_cases as pc
from tests.unet_attn_weights import count_sketch
from tests.util import bound, golden, max_rel, rel_l2, rel_linf, replay_draws, report

pytestmark = pytest.mark.gpu
DEV = "cuda"


def build(shape, patch, dim, depth, heads, ff, W, dropout=None):
    from bsi_amd.models.dit import DenoisingDiT
    from bsi_amd.nn import FourierFeatures
    m = DenoisingDiT(shape, patch, dim, depth, heads, dropout=dropout,
                     fourier_features=FourierFeatures(n_min=ff[0], n_max=ff[1]) if ff is not None else None)
    m.load_state_dict(W)
    return m.to(DEV)


def fixture_model(heads, dropout=None):
    return build(pc.SHAPE, pc.PATCH, pc.DIM, pc.DEPTH, heads, pc.FF, pc.checked_weights(), dropout)


def make_bsi(model, shape=pc.SHAPE, k=16):
    from bsi_amd import BSI, Discretization
    return BSI(model, data_shape=shape, lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=k, preconditioning="edm",
               discretization=Discretization.image_8bit()).to(DEV)


def grad_errors(model, g):
    """Relative L2 error of every parameter gradient against a fixture: whole tensors (G.) where stored, count sketches (K.) else."""
    errs = []
    for name, q in model.named_parameters():
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), name
        if "G." + name in g:
            assert q.grad.shape == g["G." + name].shape, name
            err = rel_l2(q.grad, g["G." + name])
        else:
            ref = g["K." + name]
            err = float((count_sketch(q.grad, ref.numel()) - ref).norm()) / max(float(g["N." + name]), 1e-30)
        errs.append((err, name))
    return errs


@pytest.mark.parametrize("name", list(pc.FWD))
def test_forward_vs_reference(name):
    """P = 192, kin = 1344, at head dim 128 and 64."""
    heads, _ = pc.FWD[name]
    g = golden(name)
    model = fixture_model(heads).eval()
    with torch.no_grad():
        y = model(g["mu"].to(DEV), g["t"].to(DEV)).cpu()
    assert bool(torch.isfinite(y).all())
    err = rel_linf(y, g["out64"])
    report("dit_patch8_fwd_vs_reference", case=name, heads=heads, rel_linf=err, ref_fp32_vs_fp64=rel_linf(g["out"], g["out64"]))
    bound(f"test_forward_vs_reference:{name}", err, pc.X_HAT)


def test_sample_history_teacher_forced_vs_reference():
    from bsi_amd import _native as N
    g = pc.hist_fixture()
    k = int(g["k"])
    bsi = make_bsi(fixture_model(pc.HIST_HEADS).eval(), k=k)
    t = bsi.default_schedule
    lam, alpha = bsi._schedule(t)
    t_eval = torch.cat([t[:k], t.new_ones(1)])
    worst = {"x_hat": 0.0, "mu": 0.0, "y": 0.0}
    with torch.no_grad():
        for i in range(k + 1):
            mu_i = g["mus"][i].to(DEV)
            xh = bsi._predict_x(mu_i, t_eval[i].repeat(mu_i.shape[0]))
            worst["x_hat"] = max(worst["x_hat"], rel_linf(xh, g["x_hats"][i]))
            if i < k:
                mu_n, y = torch.empty_like(mu_i), torch.empty_like(mu_i)
                eps_i = g["eps"][i].to(DEV)
                N.check(N.lib().bsi_refine_step(N.ptr(mu_i), N.ptr(xh.contiguous()), N.ptr(eps_i), N.ptr(lam), N.ptr(alpha), None, None,
                                                i, 1, mu_i.shape[0], mu_i[0].numel(), None, N.ptr(y), N.ptr(mu_n), N.stream()))
                worst["mu"] = max(worst["mu"], rel_linf(mu_n, g["mus"][i + 1]))
                worst["y"] = max(worst["y"], rel_linf(y, g["ys"][i]))
    report("dit_patch8_hist_teacher_forced", **worst)
    for key, v in worst.items():
        bound(f"test_sample_history_teacher_forced_vs_reference:{key}", v, pc.X_HAT)


def test_free_running_sample_graph_equals_eager():
    """BSI.sample at k 8: finite, and the captured graph returns the eager chain's bits, as test_sample_graph_replay_matches_eager
    demands at patch 2."""
    bsi = make_bsi(fixture_model(2).eval(), k=8)
    with torch.no_grad():
        a = bsi.sample(2, torch.Generator(DEV).manual_seed(5))
        b = bsi.sample(2, torch.Generator(DEV).manual_seed(5), graph=True)
    assert a.shape == (2, *pc.SHAPE) and bool(torch.isfinite(a).all())
    assert torch.equal(a, b)


def test_train_loss_and_gradients_vs_reference_bit_reproducible():
    g = pc.train_fixture()
    model = fixture_model(pc.TRAIN_HEADS).train()
    bsi = make_bsi(model)
    runs = []
    for _ in range(2):
        model.zero_grad()
        with replay_draws(DEV, rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
            loss = bsi.train_loss(g["x"].to(DEV))
        loss.mean().backward()
        runs.append((loss.detach().clone(), torch.cat([q.grad.reshape(-1) for q in model.parameters()]).clone()))
    lc = runs[0][0].cpu()
    mean_err = float((lc.mean() - g["loss_mean"]).abs() / g["loss_mean"].abs())
    sample_err = max_rel(lc, g["loss"])
    errs = grad_errors(model, g)
    worst = max(errs)
    report("dit_patch8_train_vs_reference", loss_mean=mean_err, loss_per_sample=sample_err, worst_grad=worst[0], worst_name=worst[1],
           dec_w=dict((n, e) for e, n in errs)["dit.patch_decoder.1.weight"], dec_b=dict((n, e) for e, n in errs)["dit.patch_decoder.1.bias"],
           enc_w=dict((n, e) for e, n in errs)["dit.patch_encoder.weight"])
    bound("test_train_vs_reference:loss_mean", mean_err, pc.LOSS_MEAN)
    bound("test_train_vs_reference:loss", sample_err, pc.LOSS_SAMPLE)
    for err, name in errs:
        bound("test_train_vs_reference:grad", err, pc.GRAD)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("tag", list(pc.GEOMETRIES))
def test_geometry_vs_fp64_oracle(tag):
    """Forward, loss and every gradient at the widths without a fixture against the fp64 oracle; the fp32 oracle's own distance
    from it is checked to lie ORACLE_MARGIN below each bound first (and recorded)."""
    shape, patch, ff, dim, heads, _ = pc.GEOMETRIES[tag]
    y64, l64, G64 = pc.geometry_oracle(tag, True)
    y32, l32, G32 = pc.geometry_oracle(tag, False)
    own = dict(x_hat=rel_linf(y32, y64), loss_mean=abs(float(l32.mean()) / float(l64.mean()) - 1), loss=max_rel(l32, l64),
               grad=max(rel_l2(G32[k], G64[k]) for k in G64))
    m = pc.ORACLE_MARGIN
    assert own["x_hat"] < pc.X_HAT / m and own["loss_mean"] < pc.LOSS_MEAN / m and own["loss"] < pc.LOSS_SAMPLE / m and own["grad"] < pc.GRAD / m, own
    W, mu, t, x, off, perm, eps = pc.geometry_inputs(tag)
    model = build(shape, patch, dim, pc.GEO_DEPTH, heads, ff, W)
    model.eval()
    with torch.no_grad():
        y = model(mu.to(DEV), t.to(DEV)).cpu()
    model.train()
    bsi = make_bsi(model, shape)
    with replay_draws(DEV, rand=[off], randperm=[perm], randn=[eps]):
        loss = bsi.train_loss(x.to(DEV))
    loss.mean().backward()
    lc = loss.detach().cpu()
    fwd_err = rel_linf(y, y64)
    mean_err = abs(float(lc.double().mean()) / float(l64.mean()) - 1)
    sample_err = max_rel(lc, l64)
    errs = []
    for name, q in model.named_parameters():
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), name
        errs.append((rel_l2(q.grad, G64[name]), name))
    worst = max(errs)
    report("dit_patch_geometry_vs_fp64_oracle", case=tag, P=shape[0] * patch * patch, x_hat=fwd_err, loss_mean=mean_err, loss_per_sample=sample_err,
           worst_grad=worst[0], worst_name=worst[1], fp32_oracle=own)
    bound(f"test_geometry_vs_fp64_oracle:{tag}:x_hat", fwd_err, pc.X_HAT)
    bound(f"test_geometry_vs_fp64_oracle:{tag}:loss_mean", mean_err, pc.LOSS_MEAN)
    bound(f"test_geometry_vs_fp64_oracle:{tag}:loss", sample_err, pc.LOSS_SAMPLE)
    for err, name in errs:
        bound(f"test_geometry_vs_fp64_oracle:{tag}:grad", err, pc.GRAD)


def test_dp_trainer_step_with_dropout_and_shadow_refresh():
    """One DPTrainer.train_step at patch 8 with dropout 0.1: finite loss, every parameter moved, and the inference forward after the
    step is that of a fresh model holding the stepped weights (the bf16 shadows were refreshed)."""
    from bsi_amd.dp import DPTrainer
    g = pc.train_fixture()
    model = fixture_model(pc.TRAIN_HEADS, dropout=0.1).train()
    before = {n: q.detach().clone() for n, q in model.named_parameters()}
    f = golden("g21_dit_patch8_fwd")
    mu, t = f["mu"].to(DEV), f["t"].to(DEV)
    model.eval()
    with torch.no_grad():
        y0 = model(mu, t).clone()
    model.train()
    tr = DPTrainer(make_bsi(model), lr=5e-4, max_grad_norm=1.0)
    with replay_draws(DEV, rand=[g["offset"]], randperm=[g["perm"]], randn=[g["eps"]]):
        loss = tr.train_step(g["x"].to(DEV))
    assert bool(torch.isfinite(torch.as_tensor(loss)).all())
    after = dict(model.named_parameters())
    assert all(bool(torch.isfinite(v).all()) for v in after.values())
    unchanged = [n for n, v in before.items() if torch.equal(after[n].detach(), v)]
    assert not unchanged, unchanged
    model.eval()
    with torch.no_grad():
        y1 = model(mu, t).clone()
    fresh = build(pc.SHAPE, pc.PATCH, pc.DIM, pc.DEPTH, pc.TRAIN_HEADS, pc.FF, {k: v.detach().cpu() for k, v in model.state_dict().items()}).eval()
    with torch.no_grad():
        y2 = fresh(mu, t)
    assert not torch.equal(y0, y1)
    assert torch.equal(y1, y2)


def test_all_three_engine_entries_refuse_p_320():
    """(5, 64, 64) at patch 8: P = 320 > 256.  bsi_dit_forward, bsi_dit_train_forward and bsi_dit_backward name P and the limit, before
    any pointer is followed (dummy pointers: no device memory is touched)."""
    import ctypes as C
    from bsi_amd import _native as N
    lib = N.lib()
    cfg = N.DitConfig(5, 64, 64, 8, 128, 1, 1, 6, 8)
    p = C.c_void_p(16)
    w, wt, g = N.DitWeights(), N.DitWeightsT(), N.DitGrads()
    w.blocks = C.cast(p, C.POINTER(N.DitBlockWeights))
    wt.blocks = C.cast(p, C.POINTER(N.DitBlockWeightsT))
    g.blocks = C.cast(p, C.POINTER(N.DitBlockGrads))
    calls = {
        "bsi_dit_forward": lambda: lib.bsi_dit_forward(C.byref(cfg), C.byref(w), 2, p, p, 1, None, None, None, 1, p, p, None, None),
        "bsi_dit_train_forward": lambda: lib.bsi_dit_train_forward(C.byref(cfg), C.byref(w), 2, p, p, None, None, None, p, p, 0.1, 1, None),
        "bsi_dit_backward": lambda: lib.bsi_dit_backward(C.byref(cfg), C.byref(w), C.byref(wt), C.byref(g), 2, p, None, p, p, 0.1, 1, None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        err = lib.bsi_last_error().decode()
        assert "P = patch*patch*C = 320" in err and "P <= 256" in err, (name, err)
    # the Python class builds at this width, as in the reference, and raises at first use
    from bsi_amd.models.dit import DenoisingDiT
    m = DenoisingDiT((5, 64, 64), 8, 128, 1, 1).to(DEV).eval()
    with pytest.raises(RuntimeError, match=r"P = patch\*patch\*C = 320"):
        with torch.no_grad():
            m(torch.zeros((1, 5, 64, 64), device=DEV), torch.zeros(1, device=DEV))
