"""Seeded cases for the SURFACE of the two native denoisers -- forward, deep copy, sampling (eager and graphed), train_loss +
backward through autograd and into a trainer's flat gradient buffer, two DPTrainer steps, the dropout seed -- shared by
tools/record_sampling_fixtures.py --set models, which records them with the package it is run on, and
tests/test_hip_model_surface.py, which holds the current package against that record bit for bit (digests as in
tests/sampling_cases.py).  The record is the yardstick for changes to the host-side plumbing between the nn.Modules and the C ABI
that must not change a bit: a mis-ordered gradient view, a stale weight table or another dropout seed changes these words.

Every input and every parameter is drawn from a CPU generator and moved to the device: the adaLN-Zero and zero initialisations of
fresh models turn blocks into identities, which would hide a wrong pointer table.  The models are the smallest the engines run."""
import copy
import math
import os

import torch

from tests.sampling_cases import DEV

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_surface.json")
SHAPES = {"dit": (3, 16, 16), "unet": (3, 8, 8)}
BATCH = {"dit": 3, "unet": 2}
TRAINER = dict(lr=5e-4, betas=(0.9, 0.99), weight_decay=1e-2, max_grad_norm=1.0, ema_update_after_step=0)  # tests/dp_gloo_worker.py
PAD = 1024  # elements of a trainer's gradient buffer behind the last parameter


def make_model(kind, dropout=None):
    """DiT: patch 2, dim 128, depth 2, 2 heads (64 tokens, head dim 64); UNet: dim 64, 1 level, 1 head, silu.  Every parameter is
    redrawn: norm weights around 1, biases around 0, matrices and filters at 0.7 / sqrt(fan-in)."""
    from bsi_amd.nn import FourierFeatures
    ff = FourierFeatures(n_min=6, n_max=8)
    if kind == "dit":
        from bsi_amd.models.dit import DenoisingDiT
        m = DenoisingDiT(SHAPES[kind], 2, 128, 2, 2, dropout=dropout, fourier_features=ff)
        m.cu_pair = None
    else:
        from bsi_amd.models.pos_emb import NyquistPositionalEmbedding
        from bsi_amd.models.vdm_unet import DenoisingVDMUNet
        m = DenoisingVDMUNet(SHAPES[kind], NyquistPositionalEmbedding(32, 100), "silu", 64, 1, 4, n_attention_heads=1, dropout=dropout,
                             fourier_features=ff)
    gen = torch.Generator().manual_seed(17 if kind == "dit" else 23)
    with torch.no_grad():
        for mod in m.modules():
            norm = isinstance(mod, (torch.nn.LayerNorm, torch.nn.GroupNorm))
            for name, p in mod.named_parameters(recurse=False):
                r = torch.randn(p.shape, generator=gen)
                if p.dim() > 1:
                    p.copy_(r * (0.7 / math.sqrt(p[0].numel())))
                else:
                    p.copy_(1 + 0.1 * r if norm and name == "weight" else 0.05 * r)
    return m.to(DEV)


def make_bsi(model, kind):
    from bsi_amd import BSI, Discretization
    return BSI(model, data_shape=SHAPES[kind], lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=4, preconditioning="edm",
               discretization=Discretization.image_8bit()).to(DEV)


def images(kind, seed):
    gen = torch.Generator().manual_seed(seed)
    return ((torch.randint(0, 256, (BATCH[kind], *SHAPES[kind]), generator=gen).float() / 255) * 2 - 1).to(DEV)


def flat_grads(model):
    return torch.cat([p.grad.reshape(-1) for _, p in model.named_parameters()])


def run_forward(kind):
    """model(mu, t) without gradients, and the same from a deep copy taken after the model has run (its caches are populated)."""
    model = make_model(kind).eval()
    gen = torch.Generator().manual_seed(31)
    mu = (torch.randn((BATCH[kind], *SHAPES[kind]), generator=gen) * 2).to(DEV)
    t = torch.rand(BATCH[kind], generator=gen).to(DEV)
    with torch.no_grad():
        out = model(mu, t)
        pack = model._pack
        twin = copy.deepcopy(model)
        assert twin._pack is None and twin._plan is None and twin._ws is None and model._pack is pack and pack is not None
        out_twin = twin(mu, t)
        again = model(mu, t)
    torch.cuda.synchronize()
    assert torch.equal(out_twin, out), "the deep copy computes something else"
    assert torch.equal(again, out), "taking a deep copy disturbed the original"
    return {"out": out.cpu()}


def run_sample(kind):
    bsi = make_bsi(make_model(kind).eval(), kind)
    n = BATCH[kind]
    with torch.no_grad():
        eager = bsi.sample(n, torch.Generator(DEV).manual_seed(41))
        graphed = bsi.sample(n, torch.Generator(DEV).manual_seed(41), graph=True)
    torch.cuda.synchronize()
    assert torch.equal(graphed, eager), "graph=True does not replay the eager chain"
    return {"sample": eager.cpu()}


def _loss_and_backward(bsi, x, seed):
    loss = bsi.train_loss(x, torch.Generator(DEV).manual_seed(seed))
    loss.mean().backward()
    return loss.detach()


def run_train(kind):
    """train_loss(x, g).mean().backward() through autograd (.grad per parameter), then the same into a caller's padded flat buffer
    as DPTrainer._backward asks for it: same bits in the buffer, zeros behind them, and no .grad."""
    model = make_model(kind).train()
    bsi = make_bsi(model, kind)
    x = images(kind, 51)
    loss = _loss_and_backward(bsi, x, 52)
    grad = flat_grads(model).clone()
    total = grad.numel()
    for p in model.parameters():
        p.grad = None
    buf = torch.zeros(total + PAD, dtype=torch.float32, device=DEV)
    model._last_flat_grad = None
    model._grad_buffer = buf
    model._flat_grad_only = True
    try:
        loss_flat = _loss_and_backward(bsi, x, 52)
    finally:
        model._flat_grad_only = False
        model._grad_buffer = None
    torch.cuda.synchronize()
    assert model._last_flat_grad is buf, "the backward did not use the caller's gradient buffer"
    assert all(p.grad is None for p in model.parameters()), "_flat_grad_only still handed gradients to autograd"
    assert torch.equal(loss_flat, loss)
    assert torch.equal(buf[:total], grad), "the caller's buffer does not hold the gradient of the autograd path"
    assert not bool(buf[total:].any()), "the backward wrote behind the last parameter"
    return {"loss": loss.cpu(), "grad": grad.cpu()}


def run_dp(kind):
    """Two DPTrainer.train_step calls at world size 1: the flat parameters and the EMA afterwards."""
    from bsi_amd.dp import DPTrainer
    bsi = make_bsi(make_model(kind).train(), kind)
    tr = DPTrainer(bsi, **TRAINER)
    assert tr.world == 1 and not tr.exchange
    x = images(kind, 61)
    losses = [tr.train_step(x, torch.Generator(DEV).manual_seed(62 + s)) for s in range(2)]
    torch.cuda.synchronize()
    return {"params": tr.fp.flat.cpu(), "ema": tr.ema_fp.flat.cpu(), "losses": torch.stack(losses).cpu()}


def run_dropout():
    """One training step of the DiT in train() mode with dropout 0.1: pins the dropout seed (torch.initial_seed and the model's call
    counter)."""
    model = make_model("dit", dropout=0.1).train()
    bsi = make_bsi(model, "dit")
    torch.manual_seed(1234)
    model._drop_calls = 0
    loss = _loss_and_backward(bsi, images("dit", 71), 72)
    torch.cuda.synchronize()
    assert model._drop_calls == 1
    return {"loss": loss.cpu(), "grad": flat_grads(model).cpu()}


def all_cases():
    """(id, thunk) of every recorded case."""
    cases = [(f"{kind}_{name}", (lambda fn=fn, kind=kind: fn(kind))) for kind in SHAPES
             for name, fn in (("forward", run_forward), ("sample", run_sample), ("train", run_train), ("dp", run_dp))]
    cases.append(("dit_dropout", run_dropout))
    return cases
