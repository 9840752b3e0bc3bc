#!/usr/bin/env python
"""Secondary benchmark: images/s of BSI.sample (k=128) with the VDM-UNet of config/experiment/cifar10-vdm.yaml
(dim 128, levels 32, 1 attention head) on one GPU; 53.47 GFLOP per evaluation per image.
--downsampling-attention: the same UNet with Residual(GroupNorm -> Attention2D) after every residual block (4 heads of 32
channels; the GFLOP figure then counts only the default UNet's work).  --train N: also time N train_loss backward steps (B images).
--actfn NAME: the model's activation (silu, the default, gelu, relu, softplus, tanh).
--heads N: n_attention_heads of the centre Attention2D (1, the default, 2, 4 or 8: head dims 128 .. 16).
--dim N: the UNet's width (128, the default, 64 or 256; the GFLOP figure is that of dim 128 and is printed for dim 128 only).  Dim 256
has no 1-head centre attention (head dim 256): give --heads 2, 4, 8 or 16.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bsi_amd import BSI, Discretization  # noqa: E402
from bsi_amd.models.pos_emb import NyquistPositionalEmbedding  # noqa: E402
from bsi_amd.models.vdm_unet import DenoisingVDMUNet  # noqa: E402
from bsi_amd.nn import FourierFeatures  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--downsampling-attention", action="store_true")
ap.add_argument("--heads", type=int, default=1, metavar="N")
ap.add_argument("--train", type=int, default=0, metavar="N")
ap.add_argument("--actfn", default="silu", choices=("silu", "gelu", "relu", "softplus", "tanh"))
ap.add_argument("--dim", type=int, default=128, metavar="N")
args = ap.parse_args()
B = int(os.environ.get("B", "256"))
K = int(os.environ.get("K", "128"))
dev = torch.device("cuda", 0)
shape = (3, 32, 32)
torch.manual_seed(0)
m = DenoisingVDMUNet(shape, NyquistPositionalEmbedding(32, 100), args.actfn, args.dim, 32, 4, n_attention_heads=args.heads, dropout=0.1,
                     downsampling_attention=args.downsampling_attention,
                     fourier_features=FourierFeatures(n_min=6, n_max=8)).to(dev).eval()
bsi = BSI(m, data_shape=shape, lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=K, preconditioning="edm",
          discretization=Discretization.image_8bit()).to(dev)
g = torch.Generator(dev).manual_seed(0)
with torch.no_grad():
    bsi.sample(B, g, t=torch.linspace(0, 1, 5, device=dev))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = bsi.sample(B, g)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
assert torch.isfinite(out).all()
tag = (" downsampling_attention" if args.downsampling_attention else "") + (f" actfn={args.actfn}" if args.actfn != "silu" else "") + (
    f" heads={args.heads}" if args.heads != 1 else "") + (f" dim={args.dim}" if args.dim != 128 else "")
flops = f", {B / dt * (K + 1) * 53.47 / 1e3:.0f} model TFLOP/s" if args.dim == 128 else ""
print(f"UNet{tag} BSI.sample k={K} B={B}: {B / dt:.2f} images/s{flops}")
if args.train:
    m.train()
    x = torch.rand((B, *shape), device=dev) * 2 - 1
    bsi.train_loss(x, g).mean().backward()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.train):
        bsi.train_loss(x, g).mean().backward()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"UNet{tag} train_loss backward B={B}: {args.train / dt:.3f} steps/s")
