#!/usr/bin/env python
"""Golden vectors of the DenoisingDiT with ONE head of 128 channels (the geometry of the reference's tutorial and of the paper's
CIFAR-10 model: dim 128, heads 1), computed by the REFERENCE on CPU in the style of tools/gen_golden_unet_heads.py.  Runs only
where the reference is available (tools/ref_shim.py).  Re-run:  python tools/gen_golden_dit_heads.py

Weights: the calibration weights tests/golden/w_dit_ff.npz (dim 128, depth 2, patch 2, 3x16x16, Fourier features 6..8); to_qkv does
not depend on the head count, so the weights written for two heads serve heads=1.  Cases (g20_dit_dh128_*):
  fwd     forward, B 4, per-sample t (fp32 and fp64 outputs)
  train   train_loss + .mean().backward() with the inputs and recorded draws of g4_train_dit, dropout=None: loss, loss_mean,
          grad_norm and loss_fp64 as g4_train_dit stores them; the gradients G.<key> (fp32, whole) are spread over
          train_g0, train_g1, ... so that every file stays below 1 MiB
  hist    sample_history, n 2, k 16, with the recorded draws
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import gen_golden as gg  # noqa: E402  (loads the reference through ref_shim; writes nothing on import)
from tests.util import golden, weights  # noqa: E402

ref = gg.ref
SHAPE, PATCH, DIM, DEPTH, HEADS = (3, 16, 16), 2, 128, 2, 1
PART_BYTES = 900 * 1024  # uncompressed fp32 payload of one gradient file (random mantissas do not compress)


def model():
    m = ref.dit.DenoisingDiT(SHAPE, PATCH, DIM, DEPTH, HEADS, dropout=None, fourier_features=ref.nn.FourierFeatures(n_min=6, n_max=8))
    m.load_state_dict(weights("dit_ff"))
    return m.eval()


def forward_case(seed=200):
    m = model()
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn((4, *SHAPE), generator=g) * 2
    t = torch.rand(4, generator=g)
    with torch.no_grad():
        y = m(mu, t)
        y64 = copy.deepcopy(m).double()(mu.double(), t.double())
    gg.save("g20_dit_dh128_fwd", mu=mu, t=t, out=y, out64=y64, heads=np.int64(HEADS))


def train_case():
    src = golden("g4_train_dit")
    B, seed = 4, 30
    m = model()
    b = gg.make_bsi(m, SHAPE)
    x = gg.data(B, SHAPE, seed)
    g = torch.Generator().manual_seed(seed + 1)
    loss = b.train_loss(x, g)
    m.zero_grad()
    loss.mean().backward()
    g = torch.Generator().manual_seed(seed + 1)
    off = torch.rand((), generator=g)
    perm = torch.randperm(B, generator=g)
    eps = torch.randn((B, *SHAPE), generator=g)
    for a, k in ((x, "x"), (off, "offset"), (perm, "perm"), (eps, "eps")):
        assert torch.equal(a, src[k]), k  # the inputs and draws of g4_train_dit
    gn = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters()))
    m64 = copy.deepcopy(m).double()
    b64 = gg.make_bsi(m64, SHAPE, dtype=torch.float64)
    lam64 = b64.p_lambda.icdf(torch.remainder(perm.double() / (1 + B) + off.double(), 1))
    mu64 = torch.addcmul(((lam64 - b64.lambda_0) / lam64).view(-1, 1, 1, 1) * x.double(), torch.rsqrt(lam64).view(-1, 1, 1, 1), eps.double())
    xh64 = b64._predict_x(mu64, b64.p_lambda.cdf(lam64))
    loss64 = b64.p_lambda.reciprocal_pdf(lam64) * (x.double() - xh64).square().flatten(1).mean(1)
    parts, size = [{}], 0
    for k, p in m.named_parameters():
        n = p.grad.numel() * 4
        if size + n > PART_BYTES and parts[-1]:
            parts.append({})
            size = 0
        parts[-1]["G." + k] = p.grad
        size += n
    gg.save("g20_dit_dh128_train", x=x, offset=off, perm=perm, eps=eps, loss=loss, loss_mean=loss.mean(), grad_norm=gn, loss_fp64=loss64,
            heads=np.int64(HEADS), n_grad_files=np.int64(len(parts)))
    for i, part in enumerate(parts):
        gg.save(f"g20_dit_dh128_train_g{i}", **part)


def history_case(n=2, k=16, seed=252):
    b = gg.make_bsi(model(), SHAPE, k=k)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        mus, x_hats, ys = b.sample_history(n, g)
    g = torch.Generator().manual_seed(seed)
    eps0 = torch.randn((n, *SHAPE), generator=g)
    eps = torch.stack([torch.randn((n, *SHAPE), generator=g) for _ in range(k)])
    gg.save("g20_dit_dh128_hist", eps0=eps0, eps=eps, mus=mus, x_hats=x_hats, ys=ys, k=np.int64(k), heads=np.int64(HEADS))


if __name__ == "__main__":
    torch.set_num_threads(8)
    forward_case()
    train_case()
    history_case()
