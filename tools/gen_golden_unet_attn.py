#!/usr/bin/env python
"""Golden vectors of the DenoisingVDMUNet with downsampling_attention=True (dim 128: Residual(GroupNorm -> Attention2D) with
4 heads of 32 channels after every residual block), computed by the REFERENCE on CPU in the style of tools/gen_golden.py.
Runs only where the reference is available (tools/ref_shim.py).  Re-run:  python tools/gen_golden_unet_attn.py

Weights: tests/unet_attn_weights.py (deterministic recipe) loaded into the reference class; w_unet_attn_l{1,2}.npz store the
reference's state-dict keys, shapes and a fingerprint of the tensors it ran with.  Cases (g16_*):
  unet_attn_fwd1   forward, levels 1, 3x8x8, B 4 (fp32 and fp64)
  unet_attn_fwd2   forward, levels 2, 3x16x16, B 4, per-sample t (fp32 and fp64)
  unet_attn_hist   sample_history, levels 1, 3x8x8, k 16, free running, with the recorded draws
  unet_attn_train  train_loss + .mean().backward(), levels 1, 3x8x8, B 4 (recorded rand / randperm / randn as g4_train_unet);
                   per parameter: the gradient's fp64 norm (N.<key>), and the gradient itself (G.<key>, up to SKETCH elements)
                   or its count sketch (K.<key>, tests/unet_attn_weights.py) -- the relative error of a gradient is estimated from
                   the sketches to ~2 %; the whole gradients would be 18 MB
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import gen_golden as gg  # noqa: E402  (loads the reference through ref_shim; writes nothing on import)
from tests.unet_attn_weights import DIM, FF, SKETCH, count_sketch, fingerprint, unet_attn_weights  # noqa: E402

ref = gg.ref
SEEDS = {1: 160, 2: 161}


def attn_unet(shape, levels):
    m = ref.vdm_unet.DenoisingVDMUNet(
        shape, ref.pos_emb.NyquistPositionalEmbedding(32, 100), "silu", DIM, levels, 4, n_attention_heads=1, dropout=0.1,
        downsampling_attention=True, fourier_features=ref.nn.FourierFeatures(n_min=FF[0], n_max=FF[1]))
    W = unet_attn_weights(shape, levels, SEEDS[levels])
    m.load_state_dict(W)
    return m.eval()


def save_keys(levels, model):
    sd = model.state_dict()
    keys = list(sd)
    gg.save(f"w_unet_attn_l{levels}", keys=np.frombuffer("\n".join(keys).encode(), dtype=np.uint8),  # newline-joined
            shapes=np.array([list(sd[k].shape) + [0] * (4 - sd[k].dim()) for k in keys]),
            ndim=np.array([sd[k].dim() for k in keys]), seed=np.int64(SEEDS[levels]),
            fingerprint=fingerprint({k: v for k, v in sd.items()}))


def forward_case(name, levels, shape, B, seed):
    m = attn_unet(shape, levels)
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn((B, *shape), generator=g) * 2
    t = torch.rand(B, generator=g)
    t[0] = 0.0
    with torch.no_grad():
        y = m(mu, t)
        y64 = m.double()(mu.double(), t.double())
        m.float()
    gg.save(name, mu=mu, t=t, out=y, out64=y64)
    save_keys(levels, m)


def history_case():
    shape, n, k, seed = (3, 8, 8), 2, 16, 162
    m = attn_unet(shape, 1)
    b = gg.make_bsi(m, shape, k=k)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        mus, x_hats, ys = b.sample_history(n, g)
    g = torch.Generator().manual_seed(seed)
    eps0 = torch.randn((n, *shape), generator=g)
    eps = torch.stack([torch.randn((n, *shape), generator=g) for _ in range(k)])
    gg.save("g16_unet_attn_hist", eps0=eps0, eps=eps, mus=mus, x_hats=x_hats, ys=ys, k=np.int64(k))


def train_case():
    import copy
    shape, B, seed = (3, 8, 8), 4, 163
    m = attn_unet(shape, 1)
    b = gg.make_bsi(m, shape)
    x = gg.data(B, shape, seed)
    g = torch.Generator().manual_seed(seed + 1)
    loss = b.train_loss(x, g)
    m.zero_grad()
    loss.mean().backward()
    grads = {}
    for k, p in m.named_parameters():
        grads["N." + k] = p.grad.double().norm()
        if p.grad.numel() <= SKETCH:
            grads["G." + k] = p.grad
        else:
            grads["K." + k] = count_sketch(p.grad)
    gn = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters()))
    g = torch.Generator().manual_seed(seed + 1)
    off = torch.rand((), generator=g)
    perm = torch.randperm(B, generator=g)
    eps = torch.randn((B, *shape), generator=g)
    m64 = copy.deepcopy(m).double()
    b64 = gg.make_bsi(m64, shape, dtype=torch.float64)
    lam64 = b64.p_lambda.icdf(torch.remainder(perm.double() / (1 + B) + off.double(), 1))
    mu64 = torch.addcmul(((lam64 - b64.lambda_0) / lam64).view(-1, 1, 1, 1) * x.double(),
                         torch.rsqrt(lam64).view(-1, 1, 1, 1), eps.double())
    with torch.no_grad():
        xh64 = b64._predict_x(mu64, b64.p_lambda.cdf(lam64))
        loss64 = b64.p_lambda.reciprocal_pdf(lam64) * (x.double() - xh64).square().flatten(1).mean(1)
    gg.save("g16_unet_attn_train", x=x, offset=off, perm=perm, eps=eps, loss=loss, loss_mean=loss.mean(), grad_norm=gn,
            loss_fp64=loss64, **grads)


if __name__ == "__main__":
    torch.set_num_threads(8)
    forward_case("g16_unet_attn_fwd1", 1, (3, 8, 8), 4, 164)
    forward_case("g16_unet_attn_fwd2", 2, (3, 16, 16), 4, 165)
    history_case()
    train_case()
