"""The kernels under the dim-256 DenoisingVDMUNet at the shapes that model gives them, through the C ABI against fp64 torch on the
CPU: GroupNorm forward (register-resident and two-pass) and backward at 256 and 256 + 256 channels (16 channels per group), the
fused-statistics GroupNorm fed by the convolution's own partials at Cout = 256, the FiLM backward at N = 256, the convolutions
and their weight gradients at 256 / 512 / 768 channels, attention at a row pitch of 768, and the decode convolution at C = 256.
Bounds are those of the same kernel's test in tests/test_hip_ops.py, tests/test_hip_unet_actfn.py, tests/test_hip_dispatch_edges.py
and tests/test_hip_attention_dh16.py; every batch is at most 3."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from tests.util import rel_linf, report

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN_BF16 = 0x7FC1
CODES = {"none": 0, "silu": 1, "gelu": 2}
TORCH_ACT = {"none": lambda x: x, "silu": F.silu, "gelu": F.gelu}
_KEEP = []


@pytest.fixture(scope="module")
def N():
    from bsi_amd import _native
    _native.lib()
    yield _native
    torch.cuda.synchronize()
    _KEEP.clear()


def dev(t):
    d = t.to(DEV).contiguous()
    _KEEP.append(d)
    return d


def empty(*shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=DEV)


def nan_bf16(*shape):
    return torch.full(shape, NAN_BF16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def gn_ref(xc, ga, be, act):
    """GroupNorm(32) + activation of xc [B, HW, C] in the dtype of xc -> [B, HW, C]."""
    from oracle.unet_oracle import group_norm
    B, HW, Cc = xc.shape
    y = group_norm(xc.permute(0, 2, 1).reshape(B, Cc, HW, 1), 32, ga, be)
    return TORCH_ACT[act](y).reshape(B, Cc, HW).permute(0, 2, 1)


def gn_inputs(B, HW, C2, seed, offset=30.0):
    """x1 (256 channels) and x2 in the distribution of test_groupnorm_nhwc / test_groupnorm_backward; with `offset` the group of
    channels 16..31 sits that far from zero (|mean| >> std: the variance formula)."""
    gen = torch.Generator().manual_seed(seed)
    C1 = 256
    x1 = torch.randn((B, HW, C1), generator=gen) * 2 + 0.5
    x1[:, :, 16:32] += offset
    x2 = torch.randn((B, HW, C2), generator=gen) if C2 else None
    ga, be = torch.randn(C1 + C2, generator=gen), torch.randn(C1 + C2, generator=gen)
    return gen, x1, x2, ga, be


# ----------------------------------------------------------------------------------------------
# GroupNorm forward: 64 / 256 / 1024 pixels on the register-resident kernel, 2048 on the two-pass kernel
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["none", "silu"])
@pytest.mark.parametrize("C2", [0, 256])
@pytest.mark.parametrize("HW", [64, 256, 1024, 2048])
def test_groupnorm_forward(N, HW, C2, act):
    """bsi_groupnorm_nhwc / _stats_nhwc; bound of test_groupnorm_nhwc, statistics as test_conv_groupnorm_partials_and_apply."""
    B, C1 = 2, 256
    _, x1, x2, ga, be = gn_inputs(B, HW, C2, HW + C2)
    Cc = C1 + C2
    xc = torch.cat([x1, x2], 2) if C2 else x1
    ref = gn_ref(xc.double(), ga.double(), be.double(), act)
    grp = xc.double().reshape(B, HW, 32, Cc // 32).permute(0, 2, 1, 3).reshape(B, 32, -1)
    mean, rstd = grp.mean(2), 1.0 / torch.sqrt(grp.var(2, unbiased=False) + 1e-5)
    fns = [("plain", N.lib().bsi_groupnorm_nhwc, None)]
    if HW <= 1024:
        fns.append(("stats", N.lib().bsi_groupnorm_stats_nhwc, torch.full((B, 32, 2), float("nan"), device=DEV)))
    for nm, fn, stats in fns:
        out, raw = nan_bf16(B, HW, Cc), nan_bf16(B, HW, Cc)
        extra = (N.ptr(stats),) if stats is not None else ()
        N.check(fn(N.ptr(dev(x1)), C1, N.ptr(dev(x2)) if C2 else None, C2, B, HW, N.ptr(dev(ga)), N.ptr(dev(be)), 1e-5, CODES[act],
                   N.ptr(out), N.ptr(raw), *extra, N.stream()))
        err = float((out.cpu().double() - ref).abs().max())
        assert err <= float(ref.abs().max()) * 2 ** -8 + 1e-3, (nm, err)
        assert torch.equal(raw.cpu(), xc.to(torch.bfloat16))
        if stats is not None:
            st = stats.cpu().double()
            assert float((st[..., 0] - mean).abs().max()) < 1e-5 * 31, float((st[..., 0] - mean).abs().max())
            assert float(((st[..., 1] - rstd).abs() / rstd).max()) < 1e-4


# ----------------------------------------------------------------------------------------------
# convolutions: every epilogue the engines use at the shape, NaN-filled outputs; fused-statistics GroupNorm from the partials
# ----------------------------------------------------------------------------------------------
# (Cin, Cin2, Cout): conv1 / conv2 / to_out of a plain block, conv1 of an up block, conv2 of an up block (+ folded 1x1 skip of
# cat(x, skip)), to_qkv
CONV_SHAPES = [(256, 0, 256), (512, 0, 256), (256, 512, 256), (256, 0, 768)]
CONV_EPI = {(256, 0, 256): ("bias", "film", "resid"), (512, 0, 256): ("bias", "film"), (256, 512, 256): ("resid",), (256, 0, 768): ("bias",)}


def conv_case(N, B, H, Cin, Cin2, Cout, seed):
    gen = torch.Generator().manual_seed(seed)
    x = bf16r(torch.randn((B, Cin, H, H), generator=gen))
    w = bf16r(torch.randn((Cout, Cin, 3, 3), generator=gen) / math.sqrt(Cin * 9))
    bias = torch.randn(Cout, generator=gen)
    ref = F.conv2d(x.double(), w.double(), bias.double(), padding=1)
    K = 9 * Cin + Cin2
    wp = empty(Cout, K, dtype=torch.bfloat16)
    N.check(N.lib().bsi_conv_weight_pack(N.ptr(dev(w)), Cout, Cin, 9, Cin, K, 0, N.ptr(wp), N.stream()))
    zeros = torch.zeros(256, dtype=torch.uint8, device=DEV)
    _KEEP.extend([wp, zeros])
    a = N.ConvArgs(x=dev(nhwc(x).to(torch.bfloat16)).data_ptr(), w=wp.data_ptr(), bias=dev(bias).data_ptr(), zeros=zeros.data_ptr(), B=B,
                   H=H, W=H, Cin=Cin, Cin2=Cin2, Cout=Cout, taps=9, ldo=Cout)
    x2 = w2 = None
    if Cin2:
        x2 = bf16r(torch.randn((B, Cin2, H, H), generator=gen))
        w2 = bf16r(torch.randn((Cout, Cin2, 1, 1), generator=gen) / math.sqrt(Cin2))
        N.check(N.lib().bsi_conv_weight_pack(N.ptr(dev(w2)), Cout, Cin2, 1, Cin2, K, 9 * Cin, N.ptr(wp), N.stream()))
        a.x2 = dev(nhwc(x2).to(torch.bfloat16)).data_ptr()
        ref = ref + F.conv2d(x2.double(), w2.double())
    return gen, a, ref, (x, w, x2, w2)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [8, 16, 32])
@pytest.mark.parametrize("Cin,Cin2,Cout", CONV_SHAPES, ids=[f"{c[0]}+{c[1]}to{c[2]}" for c in CONV_SHAPES])
def test_conv_epilogues(N, Cin, Cin2, Cout, H, B):
    """bsi_conv_nhwc_bf16 on the ring kernel (8 x 8) and the slab / two-source slab kernels (16, 32 wide); bounds of
    test_conv_implicit_gemm (bf16 outputs 5e-3, fp32 outputs 3e-5) and of test_conv_groupnorm_partials_and_apply."""
    gen, a, ref, _ = conv_case(N, B, H, Cin, Cin2, Cout, B + H + Cin + Cin2 + Cout)
    M, HW = B * H * H, H * H
    want = nhwc(ref).reshape(M, Cout)
    errs = {}
    for epi in CONV_EPI[(Cin, Cin2, Cout)]:
        if epi == "bias":
            out = nan_bf16(M, Cout)
            a.out, a.epilogue = out.data_ptr(), N.CONV_BIAS_BF16
            N.check(N.lib().bsi_conv_nhwc_bf16(C.byref(a), N.stream()))
            errs[epi] = rel_linf(out.cpu().float(), want)
            assert errs[epi] < 5e-3, (epi, errs[epi])
        elif epi == "film":
            for act, rows in (("silu", B), ("gelu", 1)):
                film = torch.randn((rows, 2 * Cout), generator=gen) * 0.5
                out = nan_bf16(M, Cout)
                a.out, a.epilogue, a.film, a.film_rows, a.film_stride, a.act = (out.data_ptr(), N.CONV_FILM_SILU_BF16, dev(film).data_ptr(),
                                                                                 rows, 2 * Cout, CODES[act])
                N.check(N.lib().bsi_conv_nhwc_bf16(C.byref(a), N.stream()))
                fr = film.double().expand(B, 2 * Cout) if rows == 1 else film.double()
                y = TORCH_ACT[act](ref * (fr[:, :Cout, None, None] + 1) + fr[:, Cout:, None, None])
                errs[epi + act] = rel_linf(out.cpu().float(), nhwc(y).reshape(M, Cout))
                assert errs[epi + act] < 5e-3, (epi, act, errs[epi + act])
            a.film, a.film_rows, a.film_stride, a.act = None, 0, 0, 0
        else:
            res = None if Cin2 else torch.randn((M, Cout), generator=gen)
            out = torch.full((M, Cout), float("nan"), device=DEV)
            a.out, a.epilogue, a.resid = out.data_ptr(), N.CONV_BIAS_RESID_F32, (dev(res).data_ptr() if res is not None else None)
            N.check(N.lib().bsi_conv_nhwc_bf16(C.byref(a), N.stream()))
            w64 = want + (res.double() if res is not None else 0)
            errs[epi] = rel_linf(out, w64)
            assert errs[epi] < 3e-5, (epi, errs[epi])
            if HW % 128 == 0:  # with the GroupNorm partials: the same output bits, (mean, M2) of every 128-pixel x 4-channel block
                out1 = torch.full((M, Cout), float("nan"), device=DEV)
                part = torch.full((M // 128, Cout // 4, 2), float("nan"), device=DEV)
                a.out, a.gn_partial = out1.data_ptr(), part.data_ptr()
                N.check(N.lib().bsi_conv_nhwc_bf16(C.byref(a), N.stream()))
                a.gn_partial = None
                torch.cuda.synchronize()
                assert torch.equal(out, out1)
                o64 = out1.cpu().double().reshape(M // 128, 128, Cout // 4, 4)
                mean = o64.mean(dim=(1, 3))
                m2 = ((o64 - mean[:, None, :, None]) ** 2).sum(dim=(1, 3))
                pc = part.cpu().double()
                assert bool(torch.isfinite(pc).all())
                assert float((pc[..., 0] - mean).abs().max()) < 1e-5
                assert float(((pc[..., 1] - m2).abs() / m2).max()) < 2e-4
            a.resid = None
    report("dim256_conv", shape=f"{Cin}+{Cin2}->{Cout}", H=H, B=B, **errs)


@pytest.mark.parametrize("cat", [False, True], ids=["256", "256+256"])
@pytest.mark.parametrize("HW", [128, 256])
def test_groupnorm_apply_from_conv_partials(N, HW, cat):
    """bsi_groupnorm_apply_nhwc at 256 and 256 + 256 channels, fed with the partials the convolution's own epilogue wrote at
    Cout = 256, against fp64 GroupNorm of the convolution's fp32 output and against the unfused kernel on the same input; bounds of
    test_conv_groupnorm_partials_and_apply.  The first map's channels 16..31 get a residual 30 away from zero."""
    B, Cin, Cout = 3, 256, 256
    H, Wd = (8, 16) if HW == 128 else (16, 16)
    M = B * HW
    gen = torch.Generator().manual_seed(HW + cat)
    zeros = torch.zeros(256, dtype=torch.uint8, device=DEV)
    maps, parts = [], []
    for which in range(2 if cat else 1):
        x = torch.randn((M, Cin), generator=gen).to(torch.bfloat16)
        w = bf16r(torch.randn((Cout, Cin, 3, 3), generator=gen) / math.sqrt(9 * Cin))
        bias = torch.randn(Cout, generator=gen)
        res = torch.randn((M, Cout), generator=gen) * (1 + which)
        if which == 0:
            res[:, 16:32] += 30.0
        wp = empty(Cout, 9 * Cin, dtype=torch.bfloat16)
        N.check(N.lib().bsi_conv_weight_pack(N.ptr(dev(w)), Cout, Cin, 9, Cin, 9 * Cin, 0, N.ptr(wp), N.stream()))
        out = torch.full((M, Cout), float("nan"), device=DEV)
        part = torch.full((M // 128, Cout // 4, 2), float("nan"), device=DEV)
        a = N.ConvArgs(x=dev(x).data_ptr(), w=wp.data_ptr(), bias=dev(bias).data_ptr(), zeros=zeros.data_ptr(), B=B, H=H, W=Wd, Cin=Cin,
                       Cin2=0, Cout=Cout, taps=9, ldo=Cout, out=out.data_ptr(), epilogue=N.CONV_BIAS_RESID_F32, resid=dev(res).data_ptr(),
                       gn_partial=part.data_ptr())
        N.check(N.lib().bsi_conv_nhwc_bf16(C.byref(a), N.stream()))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(part).all())
        maps.append(out)
        parts.append(part)
    Cc = Cout * len(maps)
    ga, be = torch.randn(Cc, generator=gen), torch.randn(Cc, generator=gen)
    gad, bed = dev(ga), dev(be)
    xc = torch.cat([m.cpu() for m in maps], 1).reshape(B, HW, Cc)
    grp = xc.double().reshape(B, HW, 32, Cc // 32).permute(0, 2, 1, 3).reshape(B, 32, -1)
    rstd = 1.0 / torch.sqrt(grp.var(2, unbiased=False) + 1e-5)
    for act in ("silu", "none"):
        ref = gn_ref(xc.double(), ga.double(), be.double(), act)
        outn, raw = nan_bf16(B, HW, Cc), nan_bf16(B, HW, Cc)
        stats = torch.full((B, 32, 2), float("nan"), device=DEV)
        N.check(N.lib().bsi_groupnorm_apply_nhwc(N.ptr(maps[0]), Cout, N.ptr(parts[0]), N.ptr(maps[1]) if cat else None, Cout if cat else 0,
                                                 N.ptr(parts[1]) if cat else None, B, HW, N.ptr(gad), N.ptr(bed), 1e-5, CODES[act],
                                                 N.ptr(outn), N.ptr(raw), N.ptr(stats), N.stream()))
        torch.cuda.synchronize()
        scale = float(ref.abs().max())
        assert float((outn.cpu().double() - ref).abs().max()) <= scale * 2 ** -8 + 1e-3
        assert torch.equal(raw.cpu(), xc.to(torch.bfloat16))
        st = stats.cpu().double()
        assert float((st[..., 0] - grp.mean(2)).abs().max()) < 1e-5 * 31
        assert float(((st[..., 1] - rstd).abs() / rstd).max()) < 1e-4
        old = empty(B, HW, Cc, dtype=torch.bfloat16)
        N.check(N.lib().bsi_groupnorm_nhwc(N.ptr(maps[0]), Cout, N.ptr(maps[1]) if cat else None, Cout if cat else 0, B, HW, N.ptr(gad),
                                           N.ptr(bed), 1e-5, CODES[act], N.ptr(old), None, N.stream()))
        assert float((old.float() - outn.float()).abs().max()) <= scale * 2 ** -7 + 1e-3


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [8, 16, 32])
@pytest.mark.parametrize("Cin,Cin2,Cout", CONV_SHAPES, ids=[f"{c[0]}+{c[1]}to{c[2]}" for c in CONV_SHAPES])
def test_conv_weight_and_input_gradients(N, Cin, Cin2, Cout, H, B):
    """bsi_conv_wgrad_bias_nhwc_bf16 (+ unpack) and the input-gradient convolution (Cout -> Cin channels through
    bsi_conv_weight_pack_t) against fp64 autograd; bounds of test_conv_weight_and_input_gradients."""
    gen = torch.Generator().manual_seed(B + H + Cin + Cout + 9)
    x = bf16r(torch.randn((B, Cin, H, H), generator=gen)).double().requires_grad_(True)
    w = bf16r(torch.randn((Cout, Cin, 3, 3), generator=gen) / math.sqrt(Cin * 9)).double().requires_grad_(True)
    dy = bf16r(torch.randn((B, Cout, H, H), generator=gen))
    y = F.conv2d(x, w, padding=1)
    x2 = w2 = None
    if Cin2:
        x2 = bf16r(torch.randn((B, Cin2, H, H), generator=gen)).double()
        w2 = bf16r(torch.randn((Cout, Cin2, 1, 1), generator=gen) / math.sqrt(Cin2)).double().requires_grad_(True)
        y = y + F.conv2d(x2, w2)
    y.backward(dy.double())
    zeros = torch.zeros(256, dtype=torch.uint8, device=DEV)
    M, K = B * H * H, 9 * Cin + Cin2
    dyd = dev(nhwc(dy).reshape(M, Cout).to(torch.bfloat16))
    xd = dev(nhwc(x.detach().float()).reshape(M, Cin).to(torch.bfloat16))
    x2d = dev(nhwc(x2.float()).reshape(M, Cin2).to(torch.bfloat16)) if Cin2 else None
    lib = N.lib()
    ws = empty(lib.bsi_conv_wgrad_workspace_bytes(M, Cin, Cin2, Cout, 9), dtype=torch.uint8)
    packed, dbias = torch.full((Cout, K), float("nan"), device=DEV), torch.full((Cout,), float("nan"), device=DEV)
    N.check(lib.bsi_conv_wgrad_bias_nhwc_bf16(N.ptr(dyd), Cout, N.ptr(xd), N.ptr(x2d) if Cin2 else None, N.ptr(zeros), B, H, H, Cin, Cin2,
                                              Cout, 9, N.ptr(packed), N.ptr(dbias), 0, N.ptr(ws), N.stream()))
    gw = torch.full((Cout, Cin, 3, 3), float("nan"), device=DEV)
    N.check(lib.bsi_conv_wgrad_unpack(N.ptr(packed), Cout, Cin, 9, Cin, K, 0, 0, N.ptr(gw), N.stream()))
    e_w = rel_linf(gw, w.grad)
    assert e_w < 2e-5, e_w
    if Cin2:
        gw2 = torch.full((Cout, Cin2, 1, 1), float("nan"), device=DEV)
        N.check(lib.bsi_conv_wgrad_unpack(N.ptr(packed), Cout, Cin2, 1, Cin2, K, 9 * Cin, 0, N.ptr(gw2), N.stream()))
        assert rel_linf(gw2, w2.grad) < 2e-5
    assert rel_linf(dbias, dyd.cpu().double().sum(0)) < 2e-5
    wt = empty(Cin, 9 * Cout, dtype=torch.bfloat16)
    N.check(lib.bsi_conv_weight_pack_t(N.ptr(dev(w.detach().float())), Cout, Cin, 9, 9 * Cout, N.ptr(wt), N.stream()))
    dx = torch.full((M, Cin), float("nan"), device=DEV)
    a = N.ConvArgs(x=dyd.data_ptr(), w=wt.data_ptr(), zeros=zeros.data_ptr(), out=dx.data_ptr(), B=B, H=H, W=H, Cin=Cout, Cin2=0, Cout=Cin,
                   taps=9, ldo=Cin, epilogue=N.CONV_BIAS_RESID_F32)
    N.check(lib.bsi_conv_nhwc_bf16(C.byref(a), N.stream()))
    e_x = rel_linf(dx, nhwc(x.grad).reshape(M, Cin))
    assert e_x < 2e-5, e_x
    report("dim256_conv_grad", shape=f"{Cin}+{Cin2}->{Cout}", H=H, B=B, dw=e_w, dx=e_x)


# ----------------------------------------------------------------------------------------------
# GroupNorm backward: the streaming kernel (64, 256, 2048 pixels) and the register-resident instances (1024 pixels)
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["none", "silu", "gelu"])
@pytest.mark.parametrize("C2", [0, 256])
@pytest.mark.parametrize("HW", [64, 256, 1024, 2048])
def test_groupnorm_backward(N, HW, C2, act):
    """bsi_groupnorm_bwd_nhwc (statistics recomputed, atomics into dgamma / dbeta) and bsi_groupnorm_bwd_cast_nhwc (the forward's
    saved statistics where the forward saves them) against fp64 autograd; bounds of test_groupnorm_backward.  The cast form run
    twice gives the same bits in both input gradients.

    Inputs are drawn as in the test the 2e-5 bound is taken from (mean 0.5, std 2; no far-off group): where the statistics are
    recomputed the streaming kernel forms the variance as E[x^2] - mean^2 in fp32, whose relative error grows with (mean / std)^2
    (about 2^-23 * 225 = 2.7e-5 at the forward test's offset of 30), so that bound belongs to this distribution.  The far-off group
    is the forward tests' subject, where the engines' statistics come from."""
    B, C1 = 2, 256
    gen, x1, x2, ga, be = gn_inputs(B, HW, C2, HW + C2 + 7, offset=0.0)
    Cc = C1 + C2
    da = bf16r(torch.randn((B, HW, Cc), generator=gen))
    add = torch.randn((B, HW, Cc), generator=gen)
    add_b = torch.randn((B, HW, C1), generator=gen)
    xcat = torch.cat([x1, x2], 2) if C2 else x1
    xc = xcat.double().requires_grad_(True)
    gad, bed = ga.double().requires_grad_(True), be.double().requires_grad_(True)
    gn_ref(xc, gad, bed, act).backward(da.double())
    want = xc.grad + add.double()
    want[:, :, :C1] += add_b.double()
    xg = xcat.reshape(B, HW, 32, Cc // 32).permute(0, 2, 1, 3).reshape(B, 32, -1)
    mean = xg.mean(dim=2)
    rstd = 1.0 / torch.sqrt(((xg - mean[:, :, None]) ** 2).mean(dim=2) + 1e-5)
    stats = dev(torch.stack((mean, rstd), dim=2).contiguous()) if HW <= 1024 else None
    dda, dx1, dx2 = dev(da.to(torch.bfloat16)), dev(x1), (dev(x2) if C2 else None)
    dga, dbe, dadd, daddb = dev(ga), dev(be), dev(add), dev(add_b)

    def run(fn, extra):
        out1 = torch.full((B, HW, C1), float("nan"), device=DEV)
        out2 = torch.full((B, HW, C2), float("nan"), device=DEV) if C2 else None
        dg, db = torch.ones(Cc, device=DEV), torch.ones(Cc, device=DEV)  # accumulated on top of existing values
        N.check(fn(N.ptr(dda), N.ptr(dx1), C1, N.ptr(dx2) if C2 else None, C2, B, HW, N.ptr(dga), N.ptr(dbe), 1e-5, CODES[act], N.ptr(dadd),
                   N.ptr(daddb), N.ptr(out1), N.ptr(out2) if C2 else None, N.ptr(dg), N.ptr(db), *extra, N.stream()))
        return out1, out2, dg, db

    errs = {}
    for nm in ("plain", "cast", "cast_again"):
        if nm == "plain":
            o1, o2, dg, db = run(N.lib().bsi_groupnorm_bwd_nhwc, ())
        else:
            obf = nan_bf16(B, HW, C1)
            o1, o2, dg, db = run(N.lib().bsi_groupnorm_bwd_cast_nhwc, (N.ptr(obf), N.ptr(stats) if stats is not None else None))
            assert torch.equal(obf.view(torch.int16), o1.to(torch.bfloat16).view(torch.int16))
            if nm == "cast":
                first = (o1.clone(), o2.clone() if C2 else None)
            else:
                assert torch.equal(o1, first[0]) and (not C2 or torch.equal(o2, first[1]))
        errs[nm] = rel_linf(o1, want[:, :, :C1])
        assert errs[nm] < 2e-5, (nm, errs[nm])
        if C2:
            assert rel_linf(o2, want[:, :, C1:]) < 2e-5, nm
        assert rel_linf(dg - 1, gad.grad) < 2e-5 and rel_linf(db - 1, bed.grad) < 2e-5, nm
    report("dim256_gn_bwd", HW=HW, C2=C2, act=act, **errs)


# ----------------------------------------------------------------------------------------------
# FiLM backward at N = 256
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ["one", "B"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("HW", [64, 256])
@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_film_act_backward_n256(N, act, HW, p, rows):
    """bsi_film_act / bsi_film_act_bwd at 256 channels, one FiLM row for all images or one per image (then dfilm per row; with one
    row the images' sums land in that row); bounds of test_film_act_dropout_forward_backward."""
    B, Nc = 3, 256
    R = 1 if rows == "one" else B
    gen = torch.Generator().manual_seed(HW + R + int(p * 10))
    M = B * HW
    h1 = bf16r(torch.randn((M, Nc), generator=gen) * 2)
    film = torch.randn((R, 2 * Nc), generator=gen) * 0.5
    dy = bf16r(torch.randn((M, Nc), generator=gen))
    seed, site, lib = 4321, 3, N.lib()
    keep = torch.ones(M * Nc, dtype=torch.uint8, device=DEV)
    if p > 0:
        N.check(lib.bsi_dropout_mask(p, seed, site, M, Nc, N.ptr(keep), N.stream()))
    mask = keep.cpu().double().reshape(M, Nc) / (1 - p)
    hd, fd = h1.double().requires_grad_(True), film.double().requires_grad_(True)
    fr = fd.expand(B, 2 * Nc) if R == 1 else fd
    y = TORCH_ACT[act](hd * (fr[:, :Nc].repeat_interleave(HW, 0) + 1) + fr[:, Nc:].repeat_interleave(HW, 0)) * mask
    y.backward(dy.double())
    h1d, fdv = dev(h1.to(torch.bfloat16)), dev(film)
    yb = nan_bf16(M, Nc)
    N.check(lib.bsi_film_act(N.ptr(h1d), M, Nc, HW, N.ptr(fdv), R, 2 * Nc, CODES[act], p, seed, site, N.ptr(yb), N.stream()))
    ef = rel_linf(yb.float(), y.detach())
    # dfilm has one row per IMAGE (the engine's layout); the gradient of a shared FiLM row is their sum
    dh1, dfilm = nan_bf16(M, Nc), torch.zeros((B, 2 * Nc), device=DEV)
    N.check(lib.bsi_film_act_bwd(N.ptr(dev(dy.to(torch.bfloat16))), N.ptr(h1d), M, Nc, HW, N.ptr(fdv), R, 2 * Nc, CODES[act], p, seed, site,
                                 N.ptr(dh1), N.ptr(dfilm), 2 * Nc, N.stream()))
    got = dfilm.cpu().double().sum(0, keepdim=True) if R == 1 else dfilm
    eh, efi = rel_linf(dh1.float(), hd.grad), rel_linf(got, fd.grad)
    assert ef < 5e-3 and eh < 5e-3 and efi < 1e-4, (ef, eh, efi)
    report("dim256_film", act=act, HW=HW, p=p, rows=R, fwd=ef, dh1=eh, dfilm=efi)


# ----------------------------------------------------------------------------------------------
# attention at the row pitch of the dim-256 model (ld_qkv = 768), decode at C = 256
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens", [64, 256])
@pytest.mark.parametrize("heads,dh", [(2, 128), (4, 64), (8, 32), (16, 16)])
def test_attention_ld768(N, heads, dh, tokens):
    """bsi_attention_fwd_lse and bsi_attention_bwd_long (the training engine's entry); bounds of test_attention_dh32_forward /
    _backward_long (test_attention_forward_sequence_lengths, test_attention_backward_sequence_lengths)."""
    B, d = 2, 256
    gen = torch.Generator().manual_seed(tokens * 3 + heads)
    qkv = bf16r(torch.randn((B, tokens, 3, heads, dh), generator=gen) * 1.2)
    dout = bf16r(torch.randn((B, tokens, d), generator=gen))
    x = qkv.double().requires_grad_(True)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    sc = q @ k.transpose(-1, -2) / math.sqrt(dh)
    ref = (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(B, tokens, d)
    ref.backward(dout.double())
    dq = qkv.to(torch.bfloat16).to(DEV).contiguous()
    out, lse = nan_bf16(B * tokens, d), torch.full((B, heads, tokens), float("nan"), device=DEV)
    N.check(N.lib().bsi_attention_fwd_lse(N.ptr(dq), 3 * d, B, tokens, heads, dh, N.ptr(out), d, N.ptr(lse), N.stream()))
    o = out.cpu().double().reshape(B, tokens, d)
    err, mean = rel_linf(o, ref.detach()), float((o - ref.detach()).abs().mean() / ref.detach().abs().mean())
    assert err < 1e-2 and mean < 4e-3, (err, mean)
    lse_err = float((lse.cpu().double() - torch.logsumexp(sc.detach(), -1)).abs().max())
    assert lse_err < 2e-3, lse_err
    dqkv = nan_bf16(B * tokens, 3 * d)
    dd = dout.to(torch.bfloat16).to(DEV)
    N.check(N.lib().bsi_attention_bwd_long(N.ptr(dq), 3 * d, N.ptr(out), N.ptr(dd), d, N.ptr(lse), B, tokens, heads, dh, N.ptr(dqkv), 3 * d,
                                           N.stream()))
    got = dqkv.cpu().float().reshape(B, tokens, 3, heads, dh)
    errs = {}
    for i, nm in enumerate("qkv"):
        errs[nm] = rel_linf(got[:, :, i], x.grad[:, :, i])
        errs[nm + "_mean"] = float((got[:, :, i].double() - x.grad[:, :, i]).abs().mean() / x.grad[:, :, i].abs().mean())
        assert errs[nm] < 1.5e-2 and errs[nm + "_mean"] < 6e-3, (nm, errs)
    report("dim256_attention", tokens=tokens, heads=heads, dh=dh, fwd=err, fwd_mean=mean, lse_abs=lse_err, **errs)


def test_decode_forward_backward_c256(N):
    """bsi_unet_decode (with the preconditioning coefficients) and bsi_unet_decode_bwd at C = 256, Cout = 3; bounds of
    test_unet_decode_backward (1e-5), which the fp32 forward meets as well."""
    gen = torch.Generator().manual_seed(12)
    B, HW, Cc, Co = 3, 320, 256, 3
    h = torch.randn((B * HW, Cc), generator=gen)
    w = torch.randn((Co, Cc), generator=gen) / math.sqrt(Cc)
    bias = torch.randn(Co, generator=gen)
    mu = torch.randn((B, Co, HW), generator=gen)
    g = torch.randn((B, Co, HW), generator=gen)
    c_skip, c_out = torch.rand(B, generator=gen), torch.rand(B, generator=gen) + 0.5
    hd, wd, bd = h.double().requires_grad_(True), w.double().requires_grad_(True), bias.double().requires_grad_(True)
    f = (hd @ wd.t() + bd).reshape(B, HW, Co).permute(0, 2, 1)
    xh = c_skip.double()[:, None, None] * mu.double() + c_out.double()[:, None, None] * f
    xh.backward(g.double())
    out = torch.full((B, Co, HW), float("nan"), device=DEV)
    N.check(N.lib().bsi_unet_decode(N.ptr(dev(h)), B, HW, Cc, N.ptr(dev(w)), N.ptr(dev(bias)), Co, N.ptr(dev(mu)), N.ptr(dev(c_skip)),
                                    N.ptr(dev(c_out)), 1, N.ptr(out), N.stream()))
    assert rel_linf(out, xh.detach()) < 1e-5
    dh = torch.full((B * HW, Cc), float("nan"), device=DEV)
    dw, db = torch.zeros((Co, Cc), device=DEV), torch.zeros(Co, device=DEV)
    N.check(N.lib().bsi_unet_decode_bwd(N.ptr(dev(g)), N.ptr(dev(c_out)), 1, N.ptr(dev(h)), B, HW, Cc, N.ptr(dev(w)), Co, N.ptr(dh),
                                        N.ptr(dw), N.ptr(db), N.stream()))
    assert rel_linf(dh, hd.grad) < 1e-5 and rel_linf(dw, wd.grad) < 1e-5 and rel_linf(db, bd.grad) < 1e-5
