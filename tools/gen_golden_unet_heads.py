#!/usr/bin/env python
"""Golden vectors of the DenoisingVDMUNet with n_attention_heads 4 and 8 (centre Attention2D at head dims 32 and 16), computed
by the REFERENCE on CPU in the style of tools/gen_golden_unet_attn.py.  Runs only where the reference is available
(tools/ref_shim.py).  Re-run:  python tools/gen_golden_unet_heads.py

Weights: tests/unet_heads_cases.py (deterministic recipes: oracle.unet_oracle.unet_random_weights, and
tests/unet_attn_weights.py for the per-block attention case) loaded into the reference class; w_unet_heads_<tag>.npz store
the reference's state-dict keys, shapes, the seed and a fingerprint of the tensors it ran with.  Cases (g18_*, all Fourier
features 6..8, dropout 0.1 with the model in eval mode):
  unet_heads_fwd_d128h8 / _d128h4 / _d64h4   forward, levels 1, 3x8x8, B 4, t[0] = 0 (fp32 and fp64)
  unet_heads_fwd2        forward, dim 128, 8 heads, levels 2, 3x16x16 (256 positions), B 4, per-sample t
  unet_heads_blockattn   forward, dim 128, 8 centre heads + downsampling_attention=True (4 heads per block), levels 1, 3x8x8
  unet_heads_hist        sample_history, dim 128, 8 heads, levels 1, 3x8x8, n 2, k 16, with the recorded draws
  unet_heads_train       train_loss + .mean().backward(), dim 128, 8 heads, levels 1, 3x8x8, B 4 (recorded rand / randperm /
                         randn); per parameter the gradient's fp64 norm (N.<key>) and the gradient itself (G.<key>, up to SKETCH
                         elements) or its count sketch (K.<key>)
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
from tests.unet_attn_weights import FF, SKETCH, count_sketch, fingerprint  # noqa: E402
from tests.unet_heads_cases import FORWARD, HIST, TRAIN, WEIGHTS, heads_weights  # noqa: E402

ref = gg.ref


def heads_unet(tag, heads):
    shape, dim, levels, _, block_attn = WEIGHTS[tag]
    m = ref.vdm_unet.DenoisingVDMUNet(
        shape, ref.pos_emb.NyquistPositionalEmbedding(32, 100), "silu", dim, levels, 4, n_attention_heads=heads, dropout=0.1,
        downsampling_attention=block_attn, fourier_features=ref.nn.FourierFeatures(n_min=FF[0], n_max=FF[1]))
    m.load_state_dict(heads_weights(tag))
    return m.eval()


def save_keys(tag, model):
    sd = model.state_dict()
    keys = list(sd)
    gg.save(f"w_unet_heads_{tag}", keys=np.frombuffer("\n".join(keys).encode(), dtype=np.uint8),  # newline-joined
            shapes=np.array([list(sd[k].shape) + [0] * (4 - sd[k].dim()) for k in keys]),
            ndim=np.array([sd[k].dim() for k in keys]), seed=np.int64(WEIGHTS[tag][3]),
            fingerprint=fingerprint({k: v for k, v in sd.items()}))


def forward_case(name, tag, heads, B, seed):
    shape = WEIGHTS[tag][0]
    m = heads_unet(tag, heads)
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn((B, *shape), generator=g) * 2
    t = torch.rand(B, generator=g)
    if name != "g18_unet_heads_fwd2":
        t[0] = 0.0
    with torch.no_grad():
        y = m(mu, t)
        y64 = m.double()(mu.double(), t.double())
        m.float()
    gg.save(name, mu=mu, t=t, out=y, out64=y64, heads=np.int64(heads))
    save_keys(tag, m)


def history_case():
    name, tag, heads, n, k, seed = HIST
    shape = WEIGHTS[tag][0]
    b = gg.make_bsi(heads_unet(tag, heads), shape, k=k)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        mus, x_hats, ys = b.sample_history(n, g)
    g = torch.Generator().manual_seed(seed)
    eps0 = torch.randn((n, *shape), generator=g)
    eps = torch.stack([torch.randn((n, *shape), generator=g) for _ in range(k)])
    gg.save(name, eps0=eps0, eps=eps, mus=mus, x_hats=x_hats, ys=ys, k=np.int64(k), heads=np.int64(heads))


def train_case():
    name, tag, heads, B, seed = TRAIN
    shape = WEIGHTS[tag][0]
    m = heads_unet(tag, heads)
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
    gg.save(name, x=x, offset=off, perm=perm, eps=eps, loss=loss, loss_mean=loss.mean(), grad_norm=gn, heads=np.int64(heads),
            **grads)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for name, (tag, heads, B, seed) in FORWARD.items():
        forward_case(name, tag, heads, B, seed)
    history_case()
    train_case()
