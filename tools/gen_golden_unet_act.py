#!/usr/bin/env python
"""Golden vectors of the DenoisingVDMUNet with actfn gelu, relu, softplus and tanh (bsi/models/utils.py:4-12: the ActFn after
pos_map.1 and .3 and at layers.1 / layers.4 of every residual block), computed by the REFERENCE on CPU in the style of
tools/gen_golden.py.  Runs only where the reference is available (tools/ref_shim.py).  Re-run:  python tools/gen_golden_unet_act.py

ActFn modules have no parameters, so every case loads weights that already exist: w_unet_ff (dim 64, levels 1, 3x8x8, Fourier
features 6..8, dropout slot), the seeded recipes of oracle.unet_oracle.unet_random_weights and tests/unet_attn_weights.py.
Cases (g17_*):
  unet_act_<act>       per activation, w_unet_ff: forward, B 4, t[0] = 0 (mu, t, out, out64), and train_loss + .mean().backward()
                       with the recorded rand / randperm / randn of g4_train_unet (x, offset, perm, eps, loss, loss_fp64); per
                       parameter the gradient's fp64 norm (N.<key>) and the gradient (G.<key>, up to SKETCH elements) or its count
                       sketch (K.<key>, tests/unet_attn_weights.py)
  unet_act_hist_gelu   sample_history, w_unet_ff, k 16, with the recorded draws (teacher-forced on the GPU)
  unet_act_full_gelu   CIFAR-10 geometry (dim 128, levels 32, 1 head, 3x32x32), weights unet_random_weights(.., seed=FULL_SEED,
                       ff=(6, 8)) (fingerprint stored), B 2: the forward and _predict_x
  unet_act_attn_gelu   downsampling_attention=True, dim 128, levels 1, 3x8x8, weights tests/unet_attn_weights.py (seed 160), B 4
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
from tests.unet_attn_weights import SKETCH, count_sketch, fingerprint, unet_attn_weights  # noqa: E402

ref = gg.ref
ACTS = ("gelu", "relu", "softplus", "tanh")
FULL_SEED, ATTN_SEED = 170, 160


def small_unet(actfn):
    """gen_golden.small_unet's model (its weights: tests/golden/w_unet_ff.npz) with another ActFn."""
    m = ref.vdm_unet.DenoisingVDMUNet(
        (3, 8, 8), ref.pos_emb.NyquistPositionalEmbedding(32, 100), actfn, 64, 1, 4, n_attention_heads=1, dropout=0.1,
        downsampling_attention=False, fourier_features=ref.nn.FourierFeatures(n_min=6, n_max=8))
    w = np.load(os.path.join(gg.OUT, "w_unet_ff.npz"))
    m.load_state_dict({k: torch.from_numpy(w[k]) for k in w.files if not k.startswith("_meta")})
    return m.eval()


def forward_arrays(m, shape, B, seed):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn((B, *shape), generator=g) * 2
    t = torch.rand(B, generator=g)
    t[0] = 0.0
    with torch.no_grad():
        y = m(mu, t)
        y64 = copy.deepcopy(m).double()(mu.double(), t.double())
    return dict(mu=mu, t=t, out=y, out64=y64)


def train_arrays(m, shape, B, seed):
    """tools/gen_golden_unet_attn.py train_case: gradients whole or sketched."""
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
    m.zero_grad()
    return dict(x=x, offset=off, perm=perm, eps=eps, loss=loss.detach(), loss_fp64=loss64, **grads)


def act_case(actfn, seed):
    m = small_unet(actfn)
    gg.save(f"g17_unet_act_{actfn}", **forward_arrays(m, (3, 8, 8), 4, seed), **train_arrays(m, (3, 8, 8), 4, seed + 2))


def history_case(actfn, seed):
    shape, n, k = (3, 8, 8), 2, 16
    b = gg.make_bsi(small_unet(actfn), shape, k=k)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        mus, x_hats, _ = b.sample_history(n, g)
    gg.save(f"g17_unet_act_hist_{actfn}", mus=mus, x_hats=x_hats, k=np.int64(k))


def full_case(actfn, seed):
    from oracle import unet_oracle as uo
    shape, dim, levels = (3, 32, 32), 128, 32
    W = uo.unet_random_weights(shape, dim, levels, seed=FULL_SEED, ff=(6, 8))
    m = ref.vdm_unet.DenoisingVDMUNet(
        shape, ref.pos_emb.NyquistPositionalEmbedding(32, 100), actfn, dim, levels, 4, n_attention_heads=1, dropout=0.1,
        downsampling_attention=False, fourier_features=ref.nn.FourierFeatures(n_min=6, n_max=8))
    m.load_state_dict(W)
    m.eval()
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn((2, *shape), generator=g) * 2
    t = torch.tensor([0.2, 0.9])
    b = gg.make_bsi(m, shape, k=128)
    with torch.no_grad():
        y = m(mu, t)
        xh = b._predict_x(mu, t)
    gg.save(f"g17_unet_act_full_{actfn}", mu=mu, t=t, out=y, x_hat=xh, seed=np.int64(FULL_SEED), fingerprint=fingerprint(W))


def attn_case(actfn, seed):
    shape = (3, 8, 8)
    m = ref.vdm_unet.DenoisingVDMUNet(
        shape, ref.pos_emb.NyquistPositionalEmbedding(32, 100), actfn, 128, 1, 4, n_attention_heads=1, dropout=0.1,
        downsampling_attention=True, fourier_features=ref.nn.FourierFeatures(n_min=6, n_max=8))
    m.load_state_dict(unet_attn_weights(shape, 1, ATTN_SEED))
    m.eval()
    gg.save(f"g17_unet_act_attn_{actfn}", **forward_arrays(m, shape, 4, seed), seed=np.int64(ATTN_SEED))


if __name__ == "__main__":
    torch.set_num_threads(8)
    for i, a in enumerate(ACTS):
        act_case(a, 171 + 4 * i)
    history_case("gelu", 190)
    attn_case("gelu", 191)
    full_case("gelu", 192)
