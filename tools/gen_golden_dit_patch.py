#!/usr/bin/env python
"""Golden vectors of the DenoisingDiT at patch 8 (decoder width P = 8 * 8 * 3 = 192), computed by the REFERENCE on CPU in the
style of tools/gen_golden_dit_heads.py.  Runs only where the reference is available (tools/ref_shim.py).
Re-run:  python tools/gen_golden_dit_patch.py

Model: 3x64x64, patch 8 (64 tokens), dim 128, depth 2, Fourier features 6..8 (the patch encoder reads 1344 columns per token).
Weights: the seeded recipe of tests/dit_patch_cases.py; w_dit_patch8 stores the seed and a fingerprint (the state dict would pass
1 MiB).  Cases (g21_dit_patch8_*):
  fwd      forward, B 2, per-sample t (fp32 and fp64 outputs), heads 1 (head dim 128)
  fwd_h2   the same at heads 2 (head dim 64)
  train    train_loss + .mean().backward() with recorded draws, B 2, heads 1, dropout=None: loss, loss_mean, grad_norm, loss_fp64;
           G.<key> whole fp32 gradients of patch_decoder.*, patch_encoder.bias and of every tensor of up to SKETCH elements,
           N.<key> the norm of every gradient;  train_encw: G.dit.patch_encoder.weight (688 KB);  train_k: K.<key> count sketches
           (tests.unet_attn_weights.count_sketch) of the remaining tensors
  hist     sample_history, n 1, k 4, with the recorded draws: eps0, eps, mus;  hist_out: x_hats, ys
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
from tests import dit_patch_cases as pc  # noqa: E402
from tests.unet_attn_weights import SKETCH, count_sketch, fingerprint  # noqa: E402

ref = gg.ref


def model(heads):
    m = ref.dit.DenoisingDiT(pc.SHAPE, pc.PATCH, pc.DIM, pc.DEPTH, heads, dropout=None,
                             fourier_features=ref.nn.FourierFeatures(n_min=pc.FF[0], n_max=pc.FF[1]))
    m.load_state_dict(pc.patch8_weights())
    return m.eval()


def weights_case():
    W = pc.patch8_weights()
    gg.save("w_dit_patch8", seed=np.int64(pc.SEED), fingerprint=fingerprint(W), n_keys=np.int64(len(W)))


def forward_case(name):
    heads, seed = pc.FWD[name]
    m = model(heads)
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn((2, *pc.SHAPE), generator=g) * 2
    t = torch.rand(2, generator=g)
    with torch.no_grad():
        y = m(mu, t)
        y64 = copy.deepcopy(m).double()(mu.double(), t.double())
    gg.save(name, mu=mu, t=t, out=y, out64=y64, heads=np.int64(heads))


def train_case():
    B, seed = pc.TRAIN_B, pc.TRAIN_SEED
    m = model(pc.TRAIN_HEADS)
    b = gg.make_bsi(m, pc.SHAPE)
    x = gg.data(B, pc.SHAPE, seed)
    g = torch.Generator().manual_seed(seed + 1)
    loss = b.train_loss(x, g)
    m.zero_grad()
    loss.mean().backward()
    g = torch.Generator().manual_seed(seed + 1)  # the draws train_loss made, in its order
    off = torch.rand((), generator=g)
    perm = torch.randperm(B, generator=g)
    eps = torch.randn((B, *pc.SHAPE), generator=g)
    gn = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters()))
    m64 = copy.deepcopy(m).double()
    b64 = gg.make_bsi(m64, pc.SHAPE, dtype=torch.float64)
    lam64 = b64.p_lambda.icdf(torch.remainder(perm.double() / (1 + B) + off.double(), 1))
    mu64 = torch.addcmul(((lam64 - b64.lambda_0) / lam64).view(-1, 1, 1, 1) * x.double(), torch.rsqrt(lam64).view(-1, 1, 1, 1), eps.double())
    with torch.no_grad():
        xh64 = b64._predict_x(mu64, b64.p_lambda.cdf(lam64))
    loss64 = b64.p_lambda.reciprocal_pdf(lam64) * (x.double() - xh64).square().flatten(1).mean(1)
    main, sketches = {}, {}
    for k, p in m.named_parameters():
        main["N." + k] = p.grad.double().norm()
        if k == pc.ENC_W:
            continue
        if k.startswith(pc.WHOLE) or p.grad.numel() <= SKETCH:
            main["G." + k] = p.grad
        else:
            sketches["K." + k] = count_sketch(p.grad)
    gg.save("g21_dit_patch8_train", x=x, offset=off, perm=perm, eps=eps, loss=loss, loss_mean=loss.mean(), grad_norm=gn, loss_fp64=loss64,
            heads=np.int64(pc.TRAIN_HEADS), **main)
    gg.save("g21_dit_patch8_train_encw", **{"G." + pc.ENC_W: dict(m.named_parameters())[pc.ENC_W].grad})
    gg.save("g21_dit_patch8_train_k", **sketches)


def history_case():
    n, k, seed = pc.HIST_N, pc.HIST_K, pc.HIST_SEED
    b = gg.make_bsi(model(pc.HIST_HEADS), pc.SHAPE, k=k)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        mus, x_hats, ys = b.sample_history(n, g)
    g = torch.Generator().manual_seed(seed)
    eps0 = torch.randn((n, *pc.SHAPE), generator=g)
    eps = torch.stack([torch.randn((n, *pc.SHAPE), generator=g) for _ in range(k)])
    gg.save("g21_dit_patch8_hist", eps0=eps0, eps=eps, mus=mus, k=np.int64(k), heads=np.int64(pc.HIST_HEADS))
    gg.save("g21_dit_patch8_hist_out", x_hats=x_hats, ys=ys)


if __name__ == "__main__":
    torch.set_num_threads(8)
    weights_case()
    for name in pc.FWD:
        forward_case(name)
    train_case()
    history_case()
