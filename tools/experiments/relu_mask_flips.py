#!/usr/bin/env python
"""How far ReLU's gradient moves when only its mask decision sees a bf16-sized error (the bound of the ReLU case of
tests/test_hip_unet_actfn.py::test_train_loss_gradients_vs_reference).

Runs the fixture's train_loss backward (tests/golden/g17_unet_act_relu.npz, the reference on CPU through tools/ref_shim.py) twice:
as is, and with every ReLU's backward taking its mask from z + 2^-9 rms(z) N(0, 1) (the forward value unchanged).  Prints the five
largest relative gradient differences per trial.  Measured: 5-9 %."""
import contextlib
import os
import sys
from unittest import mock

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as gg  # noqa: E402
import gen_golden_unet_act as ga  # noqa: E402
from tests.util import golden  # noqa: E402


class NoisyMaskReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x + 2 ** -9 * x.pow(2).mean().sqrt() * torch.randn_like(x))
        return torch.relu(x)

    @staticmethod
    def backward(ctx, go):
        (xn,) = ctx.saved_tensors
        return go * (xn > 0)


class NoisyReLU(torch.nn.Module):
    def forward(self, x):
        return NoisyMaskReLU.apply(x)


def gradients(g, noisy):
    m = ga.small_unet("relu")
    if noisy:
        for mod in list(m.modules()):
            for name, c in list(mod.named_children()):
                if isinstance(c, torch.nn.ReLU):
                    setattr(mod, name, NoisyReLU())
    b = gg.make_bsi(m, (3, 8, 8))
    qs = {"rand": [g["offset"]], "randperm": [g["perm"]], "randn": [g["eps"]]}
    with contextlib.ExitStack() as st:
        for n in qs:
            st.enter_context(mock.patch.object(torch, n, side_effect=(lambda n: lambda *a, **k: qs[n].pop(0))(n)))
        loss = b.train_loss(g["x"])
    loss.mean().backward()
    return {k: p.grad.clone() for k, p in m.named_parameters()}


if __name__ == "__main__":
    g = golden("g17_unet_act_relu")
    torch.manual_seed(0)
    base = gradients(g, False)
    for trial in range(3):
        other = gradients(g, True)
        worst = sorted(((float((other[k] - base[k]).norm() / base[k].norm()), k) for k in base), reverse=True)[:5]
        print(trial, ", ".join(f"{k} {e:.3g}" for e, k in worst))
