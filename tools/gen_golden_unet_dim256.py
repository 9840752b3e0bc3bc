#!/usr/bin/env python
"""Golden vectors of the DenoisingVDMUNet at dim 256 (the width of the VDM paper's ImageNet UNets), computed by the REFERENCE on
CPU in the style of tools/gen_golden_unet_heads.py.  Runs only where the reference is available (tools/ref_shim.py).
Re-run:  python tools/gen_golden_unet_dim256.py

Weights: tests/unet_dim256_cases.py (deterministic recipes) loaded into the reference class; w_unet_dim256_<tag>.npz store the
reference's state-dict keys, shapes, the seed and a fingerprint of the tensors it ran with.  Cases (g19_*, all Fourier features
6..8, dropout 0.1 with the model in eval mode):
  unet_dim256_fwd_h2 / _h4 / _h16   forward, levels 1, 3x8x8, B 4, t[0] = 0 (fp32 and fp64): head dims 128, 64, 16
  unet_dim256_fwd2        forward, 8 heads (head dim 32), levels 2, 3x16x16 (256 positions), B 4, per-sample t
  unet_dim256_attn        forward, 8 centre heads + downsampling_attention=True (4 heads of 64 channels per block), levels 1, 3x8x8
  unet_dim256_fwd_gelu    forward, 4 heads, actfn gelu, levels 1, 3x8x8
  unet_dim256_hist        sample_history, 4 heads, levels 1, 3x8x8, n 2, k 16, with the recorded draws
  unet_dim256_train / _train2 / _train_gelu   train_loss + .mean().backward(), B 4 (recorded rand / randperm / randn): levels 1 with
                          4 heads, levels 2 (3x16x16) with 8 heads, levels 1 with actfn gelu; per parameter the gradient's fp64 norm
                          (N.<key>) and the gradient itself (G.<key>, up to SKETCH elements) or its count sketch (K.<key>; SKETCH
                          buckets, 1536 for _train2: tests/unet_dim256_cases.py SKETCH_BUCKETS)
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
from tests.unet_dim256_cases import DIM, FORWARD, HIST, SKETCH_BUCKETS, TRAIN, WEIGHTS, dim256_weights  # noqa: E402

ref = gg.ref


def dim256_unet(tag, heads, actfn="silu"):
    shape, levels, _, block_attn = WEIGHTS[tag]
    m = ref.vdm_unet.DenoisingVDMUNet(
        shape, ref.pos_emb.NyquistPositionalEmbedding(32, 100), actfn, DIM, levels, 4, n_attention_heads=heads, dropout=0.1,
        downsampling_attention=block_attn, fourier_features=ref.nn.FourierFeatures(n_min=FF[0], n_max=FF[1]))
    m.load_state_dict(dim256_weights(tag))
    return m.eval()


def save_keys(tag, model):
    sd = model.state_dict()
    keys = list(sd)
    gg.save(f"w_unet_dim256_{tag}", keys=np.frombuffer("\n".join(keys).encode(), dtype=np.uint8),  # newline-joined
            shapes=np.array([list(sd[k].shape) + [0] * (4 - sd[k].dim()) for k in keys]),
            ndim=np.array([sd[k].dim() for k in keys]), seed=np.int64(WEIGHTS[tag][2]),
            fingerprint=fingerprint({k: v for k, v in sd.items()}))


def forward_case(name, tag, heads, actfn, B, seed, t0_zero):
    shape = WEIGHTS[tag][0]
    m = dim256_unet(tag, heads, actfn)
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn((B, *shape), generator=g) * 2
    t = torch.rand(B, generator=g)
    if t0_zero:
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
    b = gg.make_bsi(dim256_unet(tag, heads), shape, k=k)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        mus, x_hats, ys = b.sample_history(n, g)
    g = torch.Generator().manual_seed(seed)
    eps0 = torch.randn((n, *shape), generator=g)
    eps = torch.stack([torch.randn((n, *shape), generator=g) for _ in range(k)])
    gg.save(name, eps0=eps0, eps=eps, mus=mus, x_hats=x_hats, ys=ys, k=np.int64(k), heads=np.int64(heads))


def train_case(name, tag, heads, actfn, B, seed):
    shape = WEIGHTS[tag][0]
    m = dim256_unet(tag, heads, actfn)
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
            grads["K." + k] = count_sketch(p.grad, SKETCH_BUCKETS.get(name, SKETCH))
    gn = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters()))
    g = torch.Generator().manual_seed(seed + 1)
    off = torch.rand((), generator=g)
    perm = torch.randperm(B, generator=g)
    eps = torch.randn((B, *shape), generator=g)
    gg.save(name, x=x, offset=off, perm=perm, eps=eps, loss=loss, loss_mean=loss.mean(), grad_norm=gn, heads=np.int64(heads),
            **grads)


if __name__ == "__main__":
    torch.set_num_threads(8)
    for name, case in FORWARD.items():
        forward_case(name, *case)
    history_case()
    for name, case in TRAIN.items():
        train_case(name, *case)
