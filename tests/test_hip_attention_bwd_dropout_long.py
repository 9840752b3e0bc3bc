"""Attention-weight dropout in the streamed attention backward (attention_bwd_stream.hip, DROP instances at head dims 64 and 128)
through bsi_attention_fwd_dropout / bsi_attention_bwd_dropout with words=None, against fp64 autograd of
softmax(q k^T / sqrt(dh)) * keep / (1 - pq) @ v with the keep flags bsi_dropout_mask exports for the same (seed, site) -- the
reference and the bounds of test_attention_dropout_forward_backward (tests/test_hip_ops.py), which the streamed kernel meets at
head dim 128 without dropout and the resident kernels meet with it.

Shapes (B, tokens, heads, dh), the smallest at which each piece can go wrong: one chunk with waves 4..7 of the block inactive;
tokens not a multiple of 128 (last block half active, the forward on 64-key chunks); two heads (row stride 768, the row hash must
use b * heads + h); head dim 64 just above the resident kernels; 16 chunks."""
import math

import pytest
import torch

from tests.util import bound, rel_linf, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN_BF16 = 0x7FC1
P, SEED, SITE = 0.3, 20240917, 6


@pytest.fixture(scope="module")
def N():
    from bsi_amd import _native
    _native.lib()
    return _native


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def nan_filled(*shape):
    return torch.full(shape, NAN_BF16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def bits(t):
    return t.view(torch.int16).cpu()


def inputs(B, tokens, heads, dh, scale=1.1):
    gen = torch.Generator().manual_seed(B * 7 + tokens + heads * 3 + dh)
    qkv = bf16r(torch.randn((B, tokens, 3, heads, dh), generator=gen) * scale)
    dout = bf16r(torch.randn((B, tokens, heads * dh), generator=gen))
    return qkv, dout


SHAPES = [(2, 64, 1, 128), (3, 192, 1, 128), (2, 256, 2, 128), (1, 320, 2, 64), (2, 1024, 1, 64)]


@pytest.mark.parametrize("B,tokens,heads,dh", SHAPES, ids=[f"b{b}_t{t}_h{h}_dh{d}" for b, t, h, d in SHAPES])
def test_streamed_backward_with_dropout(N, B, tokens, heads, dh):
    d = heads * dh
    qkv, dout = inputs(B, tokens, heads, dh)
    dq_, dd_ = qkv.to(torch.bfloat16).to(DEV).contiguous(), dout.to(torch.bfloat16).to(DEV).contiguous()
    keep = torch.empty(B * heads * tokens * tokens, dtype=torch.uint8, device=DEV)
    N.check(N.lib().bsi_dropout_mask(P, SEED, SITE, B * heads * tokens, tokens, N.ptr(keep), N.stream()))
    keep = keep.reshape(B, heads, tokens, tokens).cpu().double()
    pq = round(P * 65536) / 65536  # the kernels apply the probability rounded to 2^-16 and scale the survivors by its complement
    runs = []
    for _ in range(2):
        out = nan_filled(B, tokens, d)
        lse = torch.full((B, heads, tokens), float("nan"), device=DEV)
        dqkv = nan_filled(B, tokens, 3 * d)
        N.check(N.lib().bsi_attention_fwd_dropout(N.ptr(dq_), 3 * d, B, tokens, heads, dh, N.ptr(out), d, N.ptr(lse), P, SEED, SITE, None,
                                                  N.stream()))
        N.check(N.lib().bsi_attention_bwd_dropout(N.ptr(dq_), 3 * d, N.ptr(out), N.ptr(dd_), d, N.ptr(lse), B, tokens, heads, dh,
                                                  N.ptr(dqkv), 3 * d, P, SEED, SITE, None, N.stream()))
        torch.cuda.synchronize()
        runs.append((out, lse, dqkv))
    out, lse, dqkv = runs[0]
    x = qkv.double().requires_grad_(True)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    sc = q @ k.transpose(-1, -2) / math.sqrt(dh)
    ref_o = ((torch.softmax(sc, -1) * keep / (1 - pq)) @ v).permute(0, 2, 1, 3).reshape(B, tokens, d)
    ref_o.backward(dout.double())
    errs = {"lse": rel_linf(lse, torch.logsumexp(sc, -1).detach()), "out": rel_linf(out.cpu().float(), ref_o.detach())}
    got = dqkv.cpu().float().reshape(B, tokens, 3, heads, dh)
    finite = bool(torch.isfinite(got).all())
    for i, nm in enumerate("qkv"):
        r = x.grad[:, :, i]
        errs[nm] = rel_linf(got[:, :, i], r)
        errs[nm + "_mean"] = float((got[:, :, i].double() - r).abs().mean() / r.abs().mean())
        # per (image, head): a wrong row hash of one pair shows here, not in the maximum over the batch
        errs[nm + "_pair"] = float(((got[:, :, i].double() - r).abs().amax(dim=(1, 3)) / r.abs().amax(dim=(1, 3))).max())
    report("attention_bwd_dropout_long", B=B, tokens=tokens, heads=heads, dh=dh, **errs)
    tag = "test_streamed_backward_with_dropout:"
    assert finite, "NaN or inf in dqkv"
    bound(tag + "lse", errs["lse"], 1e-5)
    bound(tag + "out", errs["out"], 1.5e-2)
    for nm in "qkv":
        bound(tag + "linf", errs[nm], 1.5e-2)
        bound(tag + "mean", errs[nm + "_mean"], 6e-3)
        bound(tag + "pair", errs[nm + "_pair"], 3e-2)
    assert torch.equal(bits(runs[0][0]), bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1]), "two forward runs differ"
    assert torch.equal(bits(runs[0][2]), bits(runs[1][2])), "two backward runs differ"


@pytest.mark.parametrize("B,tokens,heads,dh", [(2, 192, 2, 128), (1, 320, 2, 64)])
def test_p0_is_the_plain_streamed_kernel_bit_for_bit(N, B, tokens, heads, dh):
    """At p = 0 the dropout entry runs the instance bsi_attention_bwd_long runs (the one the UNet's centre attention uses)."""
    d = heads * dh
    qkv, dout = inputs(B, tokens, heads, dh, 1.2)
    dq_, dd_ = qkv.to(torch.bfloat16).to(DEV).contiguous(), dout.to(torch.bfloat16).to(DEV).contiguous()
    out = nan_filled(B, tokens, d)
    lse = torch.full((B, heads, tokens), float("nan"), device=DEV)
    N.check(N.lib().bsi_attention_fwd_dropout(N.ptr(dq_), 3 * d, B, tokens, heads, dh, N.ptr(out), d, N.ptr(lse), 0.0, SEED, SITE, None,
                                              N.stream()))
    a, b = nan_filled(B, tokens, 3 * d), nan_filled(B, tokens, 3 * d)
    N.check(N.lib().bsi_attention_bwd_dropout(N.ptr(dq_), 3 * d, N.ptr(out), N.ptr(dd_), d, N.ptr(lse), B, tokens, heads, dh, N.ptr(a),
                                              3 * d, 0.0, SEED, SITE, None, N.stream()))
    N.check(N.lib().bsi_attention_bwd_long(N.ptr(dq_), 3 * d, N.ptr(out), N.ptr(dd_), d, N.ptr(lse), B, tokens, heads, dh, N.ptr(b),
                                           3 * d, N.stream()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a.float()).all())
    assert torch.equal(bits(a), bits(b))


REFUSALS = [(32, 64, False, "head dim 32"), (96, 64, False, "head dim 96"), (128, 100, False, "tokens=100"), (64, 100, False, "tokens=100"),
            (128, 64, True, "mask words")]


@pytest.mark.parametrize("dh,tokens,words,msg", REFUSALS, ids=[f"dh{d}_t{t}_{'words' if w else 'nowords'}" for d, t, w, _ in REFUSALS])
def test_refusals_launch_nothing(N, dh, tokens, words, msg):
    B, heads = 1, 1
    d = heads * dh
    rows = 128  # room for the rows a mistaken launch would write
    dq_ = torch.zeros((B * rows, 3 * d), dtype=torch.bfloat16, device=DEV)
    out = torch.zeros((B * rows, d), dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros((B, heads, rows), device=DEV)
    dqkv = nan_filled(B * rows, 3 * d)
    mw = torch.zeros(B * heads * 8192, dtype=torch.uint8, device=DEV) if words else None
    with pytest.raises(RuntimeError, match=msg):
        N.check(N.lib().bsi_attention_bwd_dropout(N.ptr(dq_), 3 * d, N.ptr(out), N.ptr(out), d, N.ptr(lse), B, tokens, heads, dh,
                                                  N.ptr(dqkv), 3 * d, P, SEED, SITE, N.ptr(mw) if words else None, N.stream()))
    torch.cuda.synchronize()
    assert bool((bits(dqkv) == NAN_BF16).all()), "a refused call wrote its output"
