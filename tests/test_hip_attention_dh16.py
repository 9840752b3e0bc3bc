"""Softmax attention at head dim 16 (the VDM-UNet centre Attention2D with 8 heads at dim 128, or 4 at dim 64) against fp64
softmax attention: bsi_attention_fwd / _fwd_lse / bsi_attention_bwd_long.

Bounds are the project's own for head dim 32 (tests/test_hip_unet_block_attention.py); a contraction of 16 instead of 32 products
can only do better.  Cases: the resident path (<= 256 tokens, with the 256 boundary), 128-key chunks (1024), 64-key chunks (320),
one head (rows of 16 channels) and 8 heads."""
import math

import pytest
import torch

from tests.util import rel_linf, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN_BF16 = 0x7FC1
B, DH = 2, 16


@pytest.fixture(scope="module")
def N():
    from bsi_amd import _native
    _native.lib()
    return _native


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def nan_filled(rows, cols):
    return torch.full((rows, cols), NAN_BF16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def bits(t):
    return t.view(torch.int16).cpu()


def attn_ref(qkv):
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).double() for i in range(3))
    sc = q @ k.transpose(-1, -2) / math.sqrt(DH)
    b, T, _, H, _ = qkv.shape
    return (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(b, T, H * DH), torch.logsumexp(sc, -1)


FWD = [(t, h) for t in (64, 128, 192, 256, 320, 1024) for h in (1, 8)]


@pytest.mark.parametrize("tokens,heads", FWD, ids=[f"t{t}_h{h}" for t, h in FWD])
def test_attention_dh16_forward(N, tokens, heads):
    d = heads * DH
    gen = torch.Generator().manual_seed(tokens * 7 + heads)
    qkv = bf16r(torch.randn((B, tokens, 3, heads, DH), generator=gen) * 1.5)
    ref, ref_lse = attn_ref(qkv)
    dq = qkv.to(torch.bfloat16).to(DEV).contiguous()
    outs = []
    for _ in range(2):
        out = nan_filled(B * tokens, d)
        N.check(N.lib().bsi_attention_fwd(N.ptr(dq), 3 * d, B, tokens, heads, DH, N.ptr(out), d, N.stream()))
        outs.append(out)
    out = outs[0]
    assert torch.equal(bits(outs[0]), bits(outs[1])), "two runs differ"
    o = out.cpu().double().reshape(B, tokens, d)
    err, mean = rel_linf(o, ref), float((o - ref).abs().mean() / ref.abs().mean())
    out2, lse = nan_filled(B * tokens, d), torch.full((B, heads, tokens), float("nan"), device=DEV)
    N.check(N.lib().bsi_attention_fwd_lse(N.ptr(dq), 3 * d, B, tokens, heads, DH, N.ptr(out2), d, N.ptr(lse), N.stream()))
    lse_err = float((lse.cpu().double() - ref_lse).abs().max())
    report("attention_dh16_fwd", tokens=tokens, heads=heads, rel_linf=err, rel_mean=mean, lse_abs=lse_err)
    assert err < 1e-2 and mean < 4e-3, (err, mean)
    assert torch.equal(bits(out2), bits(out)), "the log-sum-exp variant changed the output"
    assert lse_err < 2e-3, lse_err


@pytest.mark.parametrize("tokens", [192, 320, 1024])
def test_attention_dh16_padded_rows(N, tokens):
    """ld_qkv = 3*d + 64, ld_out = d + 64: NaN in the input's padding does not leak in, the output's padding keeps its bits."""
    heads = 4
    d = heads * DH
    ldq, ldo = 3 * d + 64, d + 64
    gen = torch.Generator().manual_seed(tokens + 11)
    qkv = bf16r(torch.randn((B, tokens, 3, heads, DH), generator=gen) * 1.5)
    ref, _ = attn_ref(qkv)
    buf = torch.full((B * tokens, ldq), float("nan"), dtype=torch.bfloat16)
    buf[:, :3 * d] = qkv.reshape(B * tokens, 3 * d).to(torch.bfloat16)
    dq = buf.to(DEV)
    for with_lse in (False, True):
        out = nan_filled(B * tokens, ldo)
        if with_lse:
            lse = torch.empty((B, heads, tokens), device=DEV)
            N.check(N.lib().bsi_attention_fwd_lse(N.ptr(dq), ldq, B, tokens, heads, DH, N.ptr(out), ldo, N.ptr(lse), N.stream()))
        else:
            N.check(N.lib().bsi_attention_fwd(N.ptr(dq), ldq, B, tokens, heads, DH, N.ptr(out), ldo, N.stream()))
        o = out[:, :d].cpu().double().reshape(B, tokens, d)
        err = rel_linf(o, ref)
        report("attention_dh16_padded", tokens=tokens, with_lse=int(with_lse), rel_linf=err)
        assert err < 1e-2, err
        assert bool((out[:, d:].cpu().view(torch.int16) == NAN_BF16).all()), "columns past heads*dh were written"


@pytest.mark.parametrize("tokens,heads", [(64, 4), (192, 1), (256, 8), (320, 4), (1024, 8)])
def test_attention_dh16_backward_long(N, tokens, heads):
    """bsi_attention_bwd_long at head dim 16 against fp64 autograd; two runs give the same bits."""
    d = heads * DH
    gen = torch.Generator().manual_seed(tokens * 5 + heads)
    qkv = bf16r(torch.randn((B, tokens, 3, heads, DH), generator=gen) * 1.2)
    dout = bf16r(torch.randn((B, tokens, d), generator=gen))
    dq = qkv.to(torch.bfloat16).to(DEV).contiguous()
    out = torch.empty((B, tokens, d), dtype=torch.bfloat16, device=DEV)
    lse = torch.empty((B, heads, tokens), device=DEV)
    N.check(N.lib().bsi_attention_fwd_lse(N.ptr(dq), 3 * d, B, tokens, heads, DH, N.ptr(out), d, N.ptr(lse), N.stream()))
    x = qkv.double().requires_grad_(True)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    sc = q @ k.transpose(-1, -2) / math.sqrt(DH)
    (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(B, tokens, d).backward(dout.double())
    dd = dout.to(torch.bfloat16).to(DEV)
    runs = []
    for _ in range(2):
        dqkv = torch.full((B, tokens, 3 * d), float("nan"), dtype=torch.bfloat16, device=DEV)
        N.check(N.lib().bsi_attention_bwd_long(N.ptr(dq), 3 * d, N.ptr(out), N.ptr(dd), d, N.ptr(lse), B, tokens, heads, DH,
                                               N.ptr(dqkv), 3 * d, N.stream()))
        runs.append(dqkv)
    assert torch.equal(bits(runs[0]), bits(runs[1])), "two runs differ"
    got = runs[0].cpu().float().reshape(B, tokens, 3, heads, DH)
    errs = {}
    for i, nm in enumerate("qkv"):
        errs[nm] = rel_linf(got[:, :, i], x.grad[:, :, i])
        errs[nm + "_mean"] = float((got[:, :, i].double() - x.grad[:, :, i]).abs().mean() / x.grad[:, :, i].abs().mean())
    report("attention_dh16_bwd", tokens=tokens, heads=heads, **errs)
    for nm in "qkv":
        assert errs[nm] < 1.5e-2 and errs[nm + "_mean"] < 6e-3, (nm, errs)


def test_dropout_entries_refuse_dh16(N):
    """The DiT-only dropout entries name head dim 16 in their refusal and launch nothing."""
    tokens, heads = 64, 1
    d = heads * DH
    dq = torch.zeros((B * tokens, 3 * d), dtype=torch.bfloat16, device=DEV)
    out = nan_filled(B * tokens, d)
    lse = torch.zeros((B, heads, tokens), device=DEV)
    dqkv = nan_filled(B * tokens, 3 * d)
    with pytest.raises(RuntimeError, match="head dim.*16"):
        N.check(N.lib().bsi_attention_fwd_dropout(N.ptr(dq), 3 * d, B, tokens, heads, DH, N.ptr(out), d, N.ptr(lse), 0.1, 1, 0, None,
                                                  N.stream()))
    with pytest.raises(RuntimeError, match="head dim 16"):
        N.check(N.lib().bsi_attention_bwd_dropout(N.ptr(dq), 3 * d, N.ptr(out), N.ptr(out), d, N.ptr(lse), B, tokens, heads, DH,
                                                  N.ptr(dqkv), 3 * d, 0.1, 1, 0, None, N.stream()))
    torch.cuda.synchronize()
    assert bool((bits(out) == NAN_BF16).all()) and bool((bits(dqkv) == NAN_BF16).all()), "a refused call wrote its output"
