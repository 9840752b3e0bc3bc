"""The kernels at the edges of their dispatch predicates, and the DiT engine at a few images per call.

The kernels choose their code path from thresholds on M, K, N and the sequence length, not from the model, while the rest of the
suite mostly runs the benchmark's regime (256 tokens, dense operands, 64+ images).  Here every GEMM branch of `launch_epi`,
`splitk_plan`, `splitk_plan_f32` and `bsi_gemm_emits_colsum` (gemm_bf16.hip) is run from both sides of each predicate, with padded
leading dimensions whose padding must stay untouched; attention at sequence lengths other than 64 * 2^n; the LayerNorm pass at widths
that are not multiples of 64.  Every result is compared with fp64 on the CPU from the same bf16-rounded operands, with the bounds of
tests/test_hip_ops.py.  Then the small-batch DiT-L/2 regime, where fc2 (K = 4096) takes split-K: what a batch split changes there and
what it does not, and the CU-pair entry, which must return the one-stream bits for every B >= 2."""
import ctypes as C
import math

import pytest
import torch

from oracle import dit_oracle as do
from tests.util import bound, rel_linf, report

DEV = "cuda"
NAN_BF16 = 0x7FC1  # a quiet NaN whose bits no kernel writes by accident


@pytest.fixture(scope="module")
def N():
    from bsi_amd import _native
    _native.lib()
    return _native


_KEEP = []  # device copies stay alive until the test ends (kernels are enqueued asynchronously)


@pytest.fixture(autouse=True)
def _release_device_copies():
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _KEEP.clear()


def dev(t):
    d = t.to(DEV).contiguous()
    _KEEP.append(d)
    return d


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def nan_filled(rows, cols, dtype):
    """A device buffer whose every element is NaN (bf16: the pattern NAN_BF16, so that a stored NaN is told apart)."""
    if dtype == torch.bfloat16:
        return torch.full((rows, cols), NAN_BF16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    return torch.full((rows, cols), float("nan"), dtype=dtype, device=DEV)


def assert_padding_untouched(buf, cols, what):
    pad = buf[:, cols:].cpu()
    if buf.dtype == torch.bfloat16:
        assert bool((pad.view(torch.int16) == NAN_BF16).all()), f"{what}: columns past N were written"
    else:
        assert bool(torch.isnan(pad).all()), f"{what}: columns past N were written"
        assert bool((pad.view(torch.int32) == torch.tensor(float("nan")).view(torch.int32)).all()), f"{what}: padding bits changed"


# ----------------------------------------------------------------------------------------------
# GEMM: the dispatch predicates restated, and shapes on both sides of each
# ----------------------------------------------------------------------------------------------
# The arguments must have K % 64 == 0 (bsi_gemm_bf16 rejects anything else), so the "K >= 96" test of launch_epi separates K = 64 from
# K >= 128, and K = 96 itself is a rejection (test_gemm_rejects_k_96).
def splitk_plan(M, Nn, K, cus):  # gemm_bf16.hip splitk_plan: bf16 epilogues through bsi_gemm_bf16_ws
    if M <= 128 or M > 2048 or K < 2048 or K % 128 != 0 or Nn % 4 != 0:
        return 1
    tiles = ((M + 255) // 256) * ((Nn + 255) // 256)
    best = 1
    for sp in (2, 4, 8):
        if K % (sp * 128) == 0 and K // sp >= 256 and tiles * sp <= cus:
            best = sp
    return best


def splitk_plan_f32(M, Nn, K):  # gemm_bf16.hip splitk_plan_f32: BIAS_F32 through bsi_gemm_bf16_ws
    if M > 2048 or K < 1024 or Nn % 4 != 0:
        return 1
    sp = 8 if K >= 4096 else 4
    return sp if K % (sp * 128) == 0 else 1


def launch_branch(M, K, bf16_out):  # gemm_bf16.hip launch_epi, production variant 12
    if bf16_out and M > 128 and K >= 128 and K % 64 == 0:
        return "k64_ring"
    if M > 128 and K >= 96:
        return "k32_ring"
    return "tile_256x256" if M > 128 else "tile_small_m"


# Each chain is a conjunction evaluated in order; a term is DECISIVE for a shape when every term before it holds, and the sweep must
# reach both values of every term where it is decisive (the last terms of the split-K chains choose the slice count).
def _tiles(M, Nn):
    return ((M + 255) // 256) * ((Nn + 255) // 256)


PREDICATES = {
    "launch_epi (bf16 out)": [("M > 128", lambda M, Nn, K, cus: M > 128),
                              ("K >= 128 && K % 64 == 0", lambda M, Nn, K, cus: K >= 128 and K % 64 == 0)],
    "launch_epi (fp32 out)": [("M > 128", lambda M, Nn, K, cus: M > 128),
                              ("K >= 96", lambda M, Nn, K, cus: K >= 96)],
    "splitk_plan": [("M > 128", lambda M, Nn, K, cus: M > 128),
                    ("M <= 2048", lambda M, Nn, K, cus: M <= 2048),
                    ("K >= 2048", lambda M, Nn, K, cus: K >= 2048),
                    ("K % 128 == 0", lambda M, Nn, K, cus: K % 128 == 0),
                    ("tiles * 2 <= cus", lambda M, Nn, K, cus: _tiles(M, Nn) * 2 <= cus),
                    ("tiles * 8 <= cus (8 slices)", lambda M, Nn, K, cus: _tiles(M, Nn) * 8 <= cus)],
    "splitk_plan_f32": [("M <= 2048", lambda M, Nn, K, cus: M <= 2048),
                        ("K >= 1024", lambda M, Nn, K, cus: K >= 1024),
                        ("K % (sp * 128) == 0", lambda M, Nn, K, cus: K % ((8 if K >= 4096 else 4) * 128) == 0),
                        ("K >= 4096 (8 slices)", lambda M, Nn, K, cus: K >= 4096)],
    "bsi_gemm_emits_colsum": [("M > 128", lambda M, Nn, K, cus: M > 128),
                              ("K >= 128 && K % 64 == 0", lambda M, Nn, K, cus: K >= 128 and K % 64 == 0)],
}

LARGE_N = 3072
# (M, N, K); the comment names what the shape decides
GEMM_SHAPES = [
    (1, 16, 64),            # small-M tile, K = 64; no f32 split (K < 1024)
    (1, 272, 1024),         # small-M tile; f32 split, 4 slices at M = 1
    (1, 48, 4096),          # f32 split, 8 slices
    (127, 48, 128),         # small-M tile, ragged N
    (127, 272, 2112),       # K % 64 == 0 but not % 128: no f32 split
    (128, 16, 192),         # last M of the small tile
    (128, 256, 2048),       # no bf16 split at M = 128; f32 split
    (128, 48, 1024),
    (129, 48, 64),          # first M of the large kernels, K = 64: 256x256 tile
    (129, 16, 192),         # K = 64 ring / K = 32 ring, K below every split
    (129, 256, 2048),       # first M of the bf16 split
    (129, 16, 4096),
    (129, LARGE_N, 4096),   # 12 tiles, 8 slices
    (256, 272, 1024),       # bf16: K < 2048 does not split; f32 does
    (300, LARGE_N, 1024),
    (512, 272, 2112),       # K % 128 != 0: no bf16 split
    (1024, 1024, 2048),     # 16 tiles: 8 slices
    (2048, 16, 2048),       # last M of both splits
    (2048, 48, 2112),
    (2048, 256, 4096),
    (2048, 2048, 2048),     # 64 tiles: 4 slices
    (2048, 8192, 2048),     # 256 tiles: not even 2 slices fit the chip
    (2049, 256, 4096),      # first M past both splits
    (2049, 16, 1024),
    (2049, 272, 64),        # 256x256 tile with a ragged M and N
    (2049, 48, 128),
]

REF_ROWS = 512  # above ~1e9 multiply-adds the fp64 reference is taken on this many sampled rows (every tile edge included)


def _ref_rows(M, Nn, K):
    if M * Nn * K <= 1.2e9:
        return None
    gen = torch.Generator().manual_seed(M + Nn)
    edges = {0, 1, 127, 128, 129, 255, 256, M // 2, M - 2, M - 1}
    rows = set(torch.randint(0, M, (REF_ROWS,), generator=gen).tolist()) | {r for r in edges if 0 <= r < M}
    return torch.tensor(sorted(rows))


def _coverage(shapes, cus):
    seen = {}
    for chain, terms in PREDICATES.items():
        for M, Nn, K in shapes:
            for name, f in terms:
                v = bool(f(M, Nn, K, cus))
                seen.setdefault((chain, name), set()).add(v)
                if not v:
                    break
    return seen


def test_gemm_sweep_covers_every_branch_from_both_sides():
    """No GPU: the sweep's shapes reach both values of every predicate term where it decides (at the MI355X's 256 CUs), and every
    branch of launch_epi for bf16 and fp32 outputs."""
    seen = _coverage(GEMM_SHAPES, 256)
    missing = [(k, v) for k, sides in seen.items() for v in (True, False) if v not in sides]
    assert not missing, f"the GEMM sweep lost coverage: {missing}"
    assert len(seen) == sum(len(t) for t in PREDICATES.values())
    for bf16_out in (True, False):
        got = {launch_branch(M, K, bf16_out) for M, Nn, K in GEMM_SHAPES}
        want = {"k64_ring", "tile_256x256", "tile_small_m"} if bf16_out else {"k32_ring", "tile_256x256", "tile_small_m"}
        assert got == want, (bf16_out, got)
    assert {splitk_plan(M, Nn, K, 256) for M, Nn, K in GEMM_SHAPES} >= {1, 8}
    assert {splitk_plan_f32(M, Nn, K) for M, Nn, K in GEMM_SHAPES} == {1, 4, 8}
    assert {m for m, _, _ in GEMM_SHAPES} >= {1, 127, 128, 129, 2048, 2049}
    assert {k for _, _, k in GEMM_SHAPES} >= {64, 128, 192, 1024, 2048, 2112, 4096}
    assert {n for _, n, _ in GEMM_SHAPES} >= {16, 48, 256, 272, LARGE_N}


def _gemm_operands(M, Nn, K, lda, ldw, seed):
    """bf16-rounded A [M, K] and W [N, K] inside buffers of row pitch lda / ldw whose padding is NaN (a kernel that reads it poisons
    its output)."""
    gen = torch.Generator().manual_seed(seed)
    A = bf16r(torch.randn((M, K), generator=gen))
    W = bf16r(torch.randn((Nn, K), generator=gen) / math.sqrt(K))
    bias = torch.randn(Nn, generator=gen)
    Ab = torch.full((M, lda), float("nan"), dtype=torch.bfloat16)
    Ab[:, :K] = A.to(torch.bfloat16)
    Wb = torch.full((Nn, ldw), float("nan"), dtype=torch.bfloat16)
    Wb[:, :K] = W.to(torch.bfloat16)
    return A, W, bias, dev(Ab), dev(Wb), dev(bias), gen


def _device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.gpu
@pytest.mark.parametrize("M,Nn,K", GEMM_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in GEMM_SHAPES])
def test_gemm_dispatch_edges(N, M, Nn, K):
    """Every epilogue through bsi_gemm_bf16 and the plain ones through bsi_gemm_bf16_ws with the full workspace, against fp64; the
    workspace queries say "split" exactly where splitk_plan / splitk_plan_f32 do."""
    lib = N.lib()
    cus = _device_cus()
    assert lib.bsi_compute_cus() == cus, "a CU reserve is set: the split plans below assume the whole chip"
    sp, sp32 = splitk_plan(M, Nn, K, cus), splitk_plan_f32(M, Nn, K)
    assert lib.bsi_gemm_splitk_workspace_bytes(M, Nn, K) == (sp * M * Nn * 4 if sp > 1 else 0)
    assert lib.bsi_gemm_splitk_f32_workspace_bytes(M, Nn, K) == (sp32 * M * Nn * 4 if sp32 > 1 else 0)
    A, W, bias, dA, dW, db, gen = _gemm_operands(M, Nn, K, K, K, M * 31 + Nn * 7 + K)
    rows = _ref_rows(M, Nn, K)
    sel = slice(None) if rows is None else rows
    ref = A[sel].double() @ W.double().t() + bias.double()

    def pick(o):
        o = o.cpu() if rows is None else o[rows.to(DEV)].cpu()
        return o.double()

    def run(epi, out, ws=None, **kw):
        a = N.GemmArgs(A=dA.data_ptr(), W=dW.data_ptr(), bias=db.data_ptr(), out=out.data_ptr(), M=M, N=Nn, K=K, lda=K, ldw=K,
                       ldo=Nn, epilogue=epi, **kw)
        if ws is None:
            N.check(lib.bsi_gemm_bf16(C.byref(a), N.stream()))
        else:
            N.check(lib.bsi_gemm_bf16_ws(C.byref(a), N.ptr(ws), ws.numel(), N.stream()))
        return out

    need = max(lib.bsi_gemm_splitk_workspace_bytes(M, Nn, K), lib.bsi_gemm_splitk_f32_workspace_bytes(M, Nn, K), 256)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    errs = {}
    for entry, w in (("plain", None), ("ws", ws)):
        # fp32 accumulation of exact bf16 products: 2e-5 of the output scale; bf16 outputs one rounding on top: 5e-3
        errs[f"{entry}_f32"] = rel_linf(pick(run(N.EPI_BIAS_F32, nan_filled(M, Nn, torch.float32), w)), ref)
        assert errs[f"{entry}_f32"] < 2e-5, (entry, errs)
        for name, epi, fn in (("bf16", N.EPI_BIAS_BF16, lambda r: r), ("gelu", N.EPI_BIAS_GELU_BF16, do.gelu_tanh),
                              ("silu", N.EPI_BIAS_SILU_BF16, do.silu)):
            errs[f"{entry}_{name}"] = rel_linf(pick(run(epi, nan_filled(M, Nn, torch.bfloat16), w)), fn(ref))
            assert errs[f"{entry}_{name}"] < 5e-3, (entry, name, errs)
    # the epilogues whose branch differs from the plain ones: fp32 read-modify-write, positional rows, the training pair
    gate_rows, tokens = 3, 5
    gate = torch.randn((gate_rows, 3 * Nn), generator=gen)
    x0 = torch.randn((M, Nn), generator=gen)
    xg, dgate = dev(x0), dev(gate)
    run(N.EPI_GATE_RESID, xg, gate=dgate.data_ptr() + 4 * Nn, gate_rows=gate_rows, gate_stride=3 * Nn, tokens=1)
    ridx = torch.arange(M)[sel]
    want = x0[sel].double() + gate[ridx % gate_rows, Nn:2 * Nn].double() * ref
    errs["gate_resid"] = rel_linf(pick(xg), want)
    assert errs["gate_resid"] < 2e-5, errs
    pos = torch.randn((tokens, Nn), generator=gen)
    o = run(N.EPI_BIAS_POS_F32, nan_filled(M, Nn, torch.float32), pos=dev(pos).data_ptr(), tokens=tokens)
    errs["bias_pos"] = rel_linf(pick(o), ref + pos[ridx % tokens].double())
    assert errs["bias_pos"] < 2e-5, errs
    out, out2 = nan_filled(M, Nn, torch.bfloat16), nan_filled(M, Nn, torch.bfloat16)
    run(N.EPI_BIAS_GELU_DUAL, out, out2=out2.data_ptr())
    errs["dual_pre"] = rel_linf(pick(out2), ref)
    errs["dual_act"] = rel_linf(pick(out), do.gelu_tanh(ref))
    assert errs["dual_pre"] < 5e-3 and errs["dual_act"] < 5e-3, errs
    aux = bf16r(torch.randn((M, Nn), generator=gen) * 1.5)
    x = aux[sel].double().requires_grad_(True)
    do.gelu_tanh(x).sum().backward()
    want = ref * x.grad
    dx = dev(aux.to(torch.bfloat16))
    o = run(N.EPI_MUL_GELUGRAD_BF16, nan_filled(M, Nn, torch.bfloat16), aux=dx.data_ptr())
    errs["gelugrad"] = rel_linf(pick(o), want)
    assert errs["gelugrad"] < 5e-3, errs
    # column sums of the MUL_GELUGRAD output: an output of the K = 64 ring only, refused everywhere else
    slabs = (M + 127) // 128
    colsum = nan_filled(slabs, Nn, torch.float32)
    a = N.GemmArgs(A=dA.data_ptr(), W=dW.data_ptr(), bias=db.data_ptr(), out=o.data_ptr(), aux=dx.data_ptr(), M=M, N=Nn, K=K, lda=K,
                   ldw=K, ldo=Nn, epilogue=N.EPI_MUL_GELUGRAD_BF16, colsum_rows=colsum.data_ptr())
    if M > 128 and K >= 128 and K % 64 == 0:
        N.check(lib.bsi_gemm_bf16(C.byref(a), N.stream()))
        of = o.cpu().double()
        want_rows = torch.stack([of[128 * i:128 * (i + 1)].sum(0) for i in range(slabs)])
        assert float((colsum.cpu().double() - want_rows).abs().max()) < 2e-6 * float(of.abs().sum(0).max())
    else:
        assert lib.bsi_gemm_bf16(C.byref(a), N.stream()) == -1
        assert b"colsum_rows" in lib.bsi_last_error()
    report("gemm_dispatch_edges", M=M, N=Nn, K=K, branch_bf16=launch_branch(M, K, True), branch_f32=launch_branch(M, K, False),
           splits_bf16=sp, splits_f32=sp32, sampled_rows=0 if rows is None else len(rows), **errs)


PADDED_SHAPES = [(1, 272, 1024), (127, 48, 128), (129, 48, 64), (129, 256, 2048), (2048, 16, 2048), (2049, 16, 1024)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,Nn,K", PADDED_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in PADDED_SHAPES])
def test_gemm_padded_operands_leave_padding_alone(N, M, Nn, K):
    """lda = ldw = K + 64 (NaN in the padding of both operands) and ldo = N + 16 (NaN in the output's padding): the result equals fp64
    and the output padding keeps its bits -- bf16 and fp32 outputs, the ordinary kernels and the split-K finishing kernels."""
    lib = N.lib()
    lda = ldw = K + 64
    ldo = Nn + 16
    A, W, bias, dA, dW, db, _ = _gemm_operands(M, Nn, K, lda, ldw, M + 3 * Nn + 5 * K)
    ref = A.double() @ W.double().t() + bias.double()
    need = max(lib.bsi_gemm_splitk_workspace_bytes(M, Nn, K), lib.bsi_gemm_splitk_f32_workspace_bytes(M, Nn, K), 256)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    errs = {}
    for entry in ("plain", "ws"):
        for name, epi, dt, fn, tol in (("f32", N.EPI_BIAS_F32, torch.float32, lambda r: r, 2e-5),
                                       ("bf16", N.EPI_BIAS_BF16, torch.bfloat16, lambda r: r, 5e-3),
                                       ("gelu", N.EPI_BIAS_GELU_BF16, torch.bfloat16, do.gelu_tanh, 5e-3)):
            out = nan_filled(M, ldo, dt)
            a = N.GemmArgs(A=dA.data_ptr(), W=dW.data_ptr(), bias=db.data_ptr(), out=out.data_ptr(), M=M, N=Nn, K=K, lda=lda, ldw=ldw,
                           ldo=ldo, epilogue=epi)
            if entry == "plain":
                N.check(lib.bsi_gemm_bf16(C.byref(a), N.stream()))
            else:
                N.check(lib.bsi_gemm_bf16_ws(C.byref(a), N.ptr(ws), need, N.stream()))
            errs[f"{entry}_{name}"] = rel_linf(out[:, :Nn].cpu(), fn(ref))
            assert errs[f"{entry}_{name}"] < tol, (entry, name, errs)
            assert_padding_untouched(out, Nn, f"{entry}/{name}")
    report("gemm_padded_operands", M=M, N=Nn, K=K, splits_bf16=splitk_plan(M, Nn, K, _device_cus()), splits_f32=splitk_plan_f32(M, Nn, K),
           **errs)


@pytest.mark.gpu
def test_gemm_rejects_k_96(N):
    """K = 96 passes the K >= 96 test of launch_epi on paper but is not a whole number of 64-column K tiles: refused before any launch
    (no device memory is touched)."""
    lib = N.lib()
    for fn in (lambda a: lib.bsi_gemm_bf16(C.byref(a), None), lambda a: lib.bsi_gemm_bf16_ws(C.byref(a), C.c_void_p(16), 1 << 30, None)):
        a = N.GemmArgs(A=16, W=16, out=16, M=256, N=256, K=96, lda=96, ldw=96, ldo=256, epilogue=N.EPI_BIAS_BF16)
        assert fn(a) == -1
        assert b"K=96" in lib.bsi_last_error()


# ----------------------------------------------------------------------------------------------
# attention at sequence lengths other than 64 * 2^n
# ----------------------------------------------------------------------------------------------
def _attn_ref(qkv, dh):
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).double() for i in range(3))
    sc = q @ k.transpose(-1, -2) / math.sqrt(dh)
    B, T, _, H, _ = qkv.shape
    return (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(B, T, H * dh), torch.logsumexp(sc, -1)


ATTN_FWD = [(t, dh) for t in (128, 192, 320, 384, 576) for dh in (64, 128)]


@pytest.mark.gpu
@pytest.mark.parametrize("tokens,dh", ATTN_FWD, ids=[f"t{t}_dh{d}" for t, d in ATTN_FWD])
def test_attention_forward_sequence_lengths(N, tokens, dh):
    """The resident path (<= 256 tokens), the chunked one above it, and for head dim 128 both key-chunk widths (tokens % 128)."""
    B, heads = 2, 2
    d = heads * dh
    gen = torch.Generator().manual_seed(tokens * 3 + dh)
    qkv = bf16r(torch.randn((B, tokens, 3, heads, dh), generator=gen) * 1.5)
    ref, ref_lse = _attn_ref(qkv, dh)
    dq = dev(qkv.to(torch.bfloat16))
    out = nan_filled(B * tokens, d, torch.bfloat16)
    N.check(N.lib().bsi_attention_fwd(N.ptr(dq), 3 * d, B, tokens, heads, dh, N.ptr(out), d, N.stream()))
    o = out.cpu().double().reshape(B, tokens, d)
    # P is rounded to bf16 before the PV product and O is stored as bf16: 1e-2 of the max, 4e-3 on average
    err, mean = rel_linf(o, ref), float((o - ref).abs().mean() / ref.abs().mean())
    assert err < 1e-2 and mean < 4e-3, (err, mean)
    out2, lse = nan_filled(B * tokens, d, torch.bfloat16), torch.full((B, heads, tokens), float("nan"), device=DEV)
    N.check(N.lib().bsi_attention_fwd_lse(N.ptr(dq), 3 * d, B, tokens, heads, dh, N.ptr(out2), d, N.ptr(lse), N.stream()))
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16)), "the log-sum-exp variant changed the output"
    lse_err = float((lse.cpu().double() - ref_lse).abs().max())
    assert lse_err < 2e-3, lse_err
    report("attention_fwd_seq", tokens=tokens, dh=dh, rel_linf=err, rel_mean=mean, lse_abs=lse_err)


@pytest.mark.gpu
@pytest.mark.parametrize("tokens,dh", [(320, 64), (192, 128), (256, 64)])
def test_attention_forward_padded_rows(N, tokens, dh):
    """ld_qkv = 3*d + 64 and ld_out = d + 64: NaN in the input's padding must not leak in, the output's padding keeps its bits."""
    B, heads = 2, 2
    d = heads * dh
    ldq, ldo = 3 * d + 64, d + 64
    gen = torch.Generator().manual_seed(tokens + 7 * dh)
    qkv = bf16r(torch.randn((B, tokens, 3, heads, dh), generator=gen) * 1.5)
    ref, ref_lse = _attn_ref(qkv, dh)
    buf = torch.full((B * tokens, ldq), float("nan"), dtype=torch.bfloat16)
    buf[:, :3 * d] = qkv.reshape(B * tokens, 3 * d).to(torch.bfloat16)
    dq = dev(buf)
    errs = {}
    for with_lse in (False, True):
        out = nan_filled(B * tokens, ldo, torch.bfloat16)
        if with_lse:
            lse = torch.full((B, heads, tokens), float("nan"), device=DEV)
            N.check(N.lib().bsi_attention_fwd_lse(N.ptr(dq), ldq, B, tokens, heads, dh, N.ptr(out), ldo, N.ptr(lse), N.stream()))
            errs["lse_abs"] = float((lse.cpu().double() - ref_lse).abs().max())
            assert errs["lse_abs"] < 2e-3, errs
        else:
            N.check(N.lib().bsi_attention_fwd(N.ptr(dq), ldq, B, tokens, heads, dh, N.ptr(out), ldo, N.stream()))
        o = out[:, :d].cpu().double().reshape(B, tokens, d)
        key = "lse_out" if with_lse else "out"
        errs[key] = rel_linf(o, ref)
        assert errs[key] < 1e-2 and float((o - ref).abs().mean() / ref.abs().mean()) < 4e-3, errs
        assert_padding_untouched(out, d, f"attention ld_out={ldo}")
    report("attention_fwd_padded", tokens=tokens, dh=dh, ld_qkv=ldq, ld_out=ldo, **errs)


ATTN_BWD = [(192, 64, 0), (256, 64, 0), (320, 64, 1), (576, 64, 1), (320, 128, 1), (576, 128, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("tokens,dh,long", ATTN_BWD, ids=[f"t{t}_dh{d}_{'long' if lg else 'short'}" for t, d, lg in ATTN_BWD])
def test_attention_backward_sequence_lengths(N, tokens, dh, long):
    """bsi_attention_bwd (64..256 tokens) and bsi_attention_bwd_long against fp64 autograd of softmax attention."""
    B, heads = 2, 2
    d = heads * dh
    gen = torch.Generator().manual_seed(tokens * 5 + dh + long)
    qkv = bf16r(torch.randn((B, tokens, 3, heads, dh), generator=gen) * 1.2)
    dout = bf16r(torch.randn((B, tokens, d), generator=gen))
    dq = dev(qkv.to(torch.bfloat16))
    out = torch.empty((B, tokens, d), dtype=torch.bfloat16, device=DEV)
    lse = torch.empty((B, heads, tokens), device=DEV)
    N.check(N.lib().bsi_attention_fwd_lse(N.ptr(dq), 3 * d, B, tokens, heads, dh, N.ptr(out), d, N.ptr(lse), N.stream()))
    x = qkv.double().requires_grad_(True)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    sc = q @ k.transpose(-1, -2) / math.sqrt(dh)
    ref_o = (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(B, tokens, d)
    assert rel_linf(lse, torch.logsumexp(sc, -1).detach()) < 1e-5
    ref_o.backward(dout.double())
    dqkv = torch.full((B, tokens, 3 * d), float("nan"), dtype=torch.bfloat16, device=DEV)
    fn = N.lib().bsi_attention_bwd_long if long else N.lib().bsi_attention_bwd
    N.check(fn(N.ptr(dq), 3 * d, N.ptr(out), N.ptr(dev(dout.to(torch.bfloat16))), d, N.ptr(lse), B, tokens, heads, dh, N.ptr(dqkv),
               3 * d, N.stream()))
    got = dqkv.cpu().float().reshape(B, tokens, 3, heads, dh)
    errs = {}
    # P and dS are rounded to bf16 before the second products, O and the outputs are bf16 (bounds of test_attention_backward)
    for i, nm in enumerate("qkv"):
        errs[nm] = rel_linf(got[:, :, i], x.grad[:, :, i])
        errs[nm + "_mean"] = float((got[:, :, i].double() - x.grad[:, :, i]).abs().mean() / x.grad[:, :, i].abs().mean())
        assert errs[nm] < 1.5e-2 and errs[nm + "_mean"] < 6e-3, (nm, errs)
    report("attention_bwd_seq", tokens=tokens, dh=dh, entry="long" if long else "short", **errs)


@pytest.mark.gpu
def test_attention_rejects_unsupported_shapes(N):
    """Refused before any launch (dummy pointers: no device memory is touched), each with a message."""
    lib = N.lib()
    p = C.c_void_p(16)
    assert lib.bsi_attention_fwd(p, 192, 1, 100, 1, 64, p, 64, None) == -1
    assert b"tokens=100" in lib.bsi_last_error()
    assert lib.bsi_attention_fwd_lse(p, 288, 1, 128, 1, 96, p, 96, p, None) == -1
    assert b"head dim 96" in lib.bsi_last_error()
    assert lib.bsi_attention_bwd(p, 192, p, p, 64, p, 1, 320, 1, 64, p, 192, None) == -1
    assert b"tokens=320" in lib.bsi_last_error()
    assert lib.bsi_attention_bwd_long(p, 192, p, p, 64, p, 1, 100, 1, 64, p, 192, None) == -1
    assert b"tokens=100" in lib.bsi_last_error()


# ----------------------------------------------------------------------------------------------
# LayerNorm + modulate at widths that are not multiples of 64
# ----------------------------------------------------------------------------------------------
LN_CASES = [(d, M, mod_rows, tokens) for d in (4, 12, 100, 1028, 2044, 2048)
            for M, mod_rows, tokens in ((1, 1, 1), (3, 3, 1), (300, 1, 300), (300, 3, 100))]


@pytest.mark.gpu
@pytest.mark.parametrize("d,M,mod_rows,tokens", LN_CASES, ids=[f"d{d}_M{m}_r{r}" for d, m, r, _ in LN_CASES])
def test_ln_modulate_widths(N, d, M, mod_rows, tokens):
    """bsi_ln_modulate and bsi_resid_ln_modulate (gated update + LayerNorm + modulate) against the fp64 formula of test_ln_modulate:
    fp32 statistics and one bf16 rounding -> within 2^-8 of the largest output; the fp32 residual row is exact."""
    gen = torch.Generator().manual_seed(d * 7 + M + mod_rows)
    x = torch.randn((M, d), generator=gen) * 2 + 0.3
    delta = bf16r(torch.randn((M, d), generator=gen))
    mod = torch.randn((mod_rows, 6 * d), generator=gen) * 0.3
    rows = (torch.arange(M) // tokens) % mod_rows
    md = mod.double()
    dmod = dev(mod)
    out = nan_filled(M, d, torch.bfloat16)
    N.check(N.lib().bsi_ln_modulate(N.ptr(dev(x)), M, d, 1e-5, dmod.data_ptr() + 4 * 3 * d, dmod.data_ptr() + 4 * 4 * d, mod_rows,
                                    6 * d, tokens, None, None, N.ptr(out), N.stream()))
    ref = torch.addcmul(md[rows, 3 * d:4 * d], md[rows, 4 * d:5 * d] + 1, do.layer_norm(x.double()))
    e1 = float((out.cpu().double() - ref).abs().max() / ref.abs().max())
    assert e1 <= 2 ** -8, e1
    x_ref = torch.addcmul(x, mod[rows, 2 * d:3 * d], delta)  # fp32 fma in both
    y_ref = torch.addcmul(md[rows, 3 * d:4 * d], md[rows, 4 * d:5 * d] + 1, do.layer_norm(x_ref.double()))
    dx, buf = dev(x.clone()), dev(delta.to(torch.bfloat16))  # delta aliases the output buffer, as in the engine
    N.check(N.lib().bsi_resid_ln_modulate(N.ptr(dx), M, d, 1e-5, N.ptr(buf), dmod.data_ptr() + 4 * 2 * d, dmod.data_ptr() + 4 * 3 * d,
                                          dmod.data_ptr() + 4 * 4 * d, mod_rows, 6 * d, tokens, None, None, N.ptr(buf), N.stream()))
    assert torch.equal(dx.cpu(), x_ref)
    e2 = float((buf.cpu().double() - y_ref).abs().max() / y_ref.abs().max())
    assert e2 <= 2 ** -8, e2
    report("ln_modulate_widths", d=d, M=M, mod_rows=mod_rows, ln_mod=e1, resid_ln_mod=e2)


@pytest.mark.gpu
def test_ln_modulate_rejects_d_2052(N):
    lib = N.lib()
    p = C.c_void_p(16)
    assert lib.bsi_ln_modulate(p, 4, 2052, 1e-5, p, p, 1, 6 * 2052, 1, None, None, p, None) == -1
    assert b"d=2052" in lib.bsi_last_error()
    assert lib.bsi_resid_ln_modulate(p, 4, 2052, 1e-5, p, p, p, p, 1, 6 * 2052, 1, None, None, p, None) == -1
    assert b"d=2052" in lib.bsi_last_error()
    assert lib.bsi_ln_modulate(p, 4, 102, 1e-5, p, p, 1, 6 * 104, 1, None, None, p, None) == -1  # d % 4 != 0


# ----------------------------------------------------------------------------------------------
# DiT-L/2 at a few images per call
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dit_l2():
    from tests.test_hip_fullsize_properties import _bsi, _dit
    model = _dit()
    model.cu_pair = None
    return model, _bsi(model, (3, 32, 32))


def engine_plans(N, model, B):
    """The split count bsi_gemm_bf16_ws gives each GEMM of the block loop (qkv, out, fc1, fc2) for B images on the whole chip, from
    the workspace query (bytes = splits * M * N * 4; 0 = not split), and the side of M = 128."""
    lib = N.lib()
    cfg = model.native_pack()[0]
    dim, M = cfg.dim, B * lib.bsi_dit_tokens(C.byref(cfg))
    out = []
    for Nn, K in ((3 * dim, dim), (dim, dim), (4 * dim, dim), (dim, 4 * dim)):
        out.append(lib.bsi_gemm_splitk_workspace_bytes(M, Nn, K) // (M * Nn * 4))
    return tuple(out), M > 128


def _conditioning(bsi, model, B, seed):
    gen = torch.Generator(DEV).manual_seed(seed)
    mu = torch.randn((B, 3, 32, 32), device=DEV, generator=gen) * 2
    t = torch.rand(B, device=DEV, generator=gen)
    c_skip, c_out, c_in = bsi._edm_preconditioning(t)
    return mu, model.adaln_table(t), c_in.contiguous(), c_skip.contiguous(), c_out.contiguous()


@pytest.mark.gpu
def test_dit_l2_small_batches_against_one_large_call(N, dit_l2):
    """x_hat of B in {1, 2, 4, 8, 9, 16} images against the same images inside one 64-image call, and images [0, 8) + [8, 16) against
    the 16-image call.  The engine guarantees the BITS only where every GEMM of both calls runs the same kernel with the same split-K
    plan; elsewhere (a few images per call: fc2, K = 4096, splits for 128 < M <= 2048, the slice count from the CUs) the K slices
    sum in another order, and the result agrees to bf16 operand accuracy (the x_hat bound of the parity tests, 1e-2 relative)."""
    model, bsi = dit_l2
    mu, mod, c_in, c_skip, c_out = _conditioning(bsi, model, 64, 17)

    def f(lo, hi):
        s = slice(lo, hi)
        return model.forward_native(mu[s].contiguous(), mod[s].contiguous(), c_in=c_in[s].contiguous(), c_skip=c_skip[s].contiguous(),
                                    c_out=c_out[s].contiguous(), coef_stride=1)

    with torch.no_grad():
        full = f(0, 64)
        assert bool(torch.isfinite(full).all())
        cases = [(b, (0, b), full[:b], engine_plans(N, model, 64)) for b in (1, 2, 4, 8, 9, 16)]
        b16 = f(0, 16)
        cases += [(8, (lo, lo + 8), b16[lo:lo + 8], engine_plans(N, model, 16)) for lo in (0, 8)]
        kinds = set()
        for b, (lo, hi), want, want_plan in cases:
            got = f(lo, hi)
            plan = engine_plans(N, model, b)
            same = plan == want_plan
            err = rel_linf(got, want)
            if same:
                assert torch.equal(got, want), f"B={b} images [{lo},{hi}): same GEMM plans {plan}, bits differ (rel {err:.2e})"
            else:
                bound("dit_l2_small_batch_x_hat", err, 1e-2)
            kinds.add(same)
            report("dit_l2_small_batch_split", B=b, images=[lo, hi], plans=list(plan[0]), reference_plans=list(want_plan[0]),
                   bit_exact=bool(torch.equal(got, want)), rel_linf=err)
    # on any chip with 64+ CUs a few images split fc2 and 9 or more do not: both kinds of comparison ran
    assert kinds == {True, False}, kinds


def _pair_vs_one_stream(N, model, bsi, Bs, h_cus, seed):
    from bsi_amd.models.dit import cu_pair_handle
    lib = N.lib()
    results = []
    for B in Bs:
        mu, mod, c_in, c_skip, c_out = _conditioning(bsi, model, B, seed + B)
        with torch.no_grad():
            ref = model.forward_native(mu, mod, c_in=c_in, c_skip=c_skip, c_out=c_out, coef_stride=1)
            cfg, w, _, _ = model.native_pack()
            ws = model._workspace(lib.bsi_dit_workspace_bytes(C.byref(cfg), B), mu.device)
            got = torch.full_like(mu, float("nan"))
            N.check(lib.bsi_dit_forward_pair(C.byref(cfg), C.byref(w), B, N.ptr(mu), N.ptr(mod), mod.shape[0], N.ptr(c_in), N.ptr(c_skip),
                                             N.ptr(c_out), 1, N.ptr(got), N.ptr(ws), cu_pair_handle(mu.device, h_cus), 0, N.stream()))
            torch.cuda.synchronize()
        results.append((B, torch.equal(got, ref), rel_linf(got, ref)))
    assert lib.bsi_compute_cus() == _device_cus(), "the pair left a CU reserve behind"
    return results


@pytest.mark.gpu
def test_cu_pair_small_batches_dit_l2(N, dit_l2):
    """bsi_dit_forward_pair called directly (below the Python PAIR_MIN_BATCH guard): the one-stream bits for every B >= 2, also where
    the halves alone would take another split-K plan than the whole batch (B = 16, 17 on a 256-CU chip with h_cus = 32)."""
    model, bsi = dit_l2
    res = _pair_vs_one_stream(N, model, bsi, (2, 3, 8, 16, 17, 32), 32, 100)
    report("cu_pair_small_batches", model="dit_l2", h_cus=32, results=[[b, int(eq), e] for b, eq, e in res])
    assert all(eq for _, eq, _ in res), f"pair differs from one stream: {[(b, e) for b, eq, e in res if not eq]}"


@pytest.mark.gpu
def test_cu_pair_small_batches_small_model(N):
    from tests.test_hip_cu_pair import _bsi, _dit
    shape = (3, 32, 32)
    model = _dit(shape, 2, 128, 3, 2)
    res = _pair_vs_one_stream(N, model, _bsi(model, shape, 4), (2, 5), 32, 200)
    report("cu_pair_small_batches", model="small", h_cus=32, results=[[b, int(eq), e] for b, eq, e in res])
    assert all(eq for _, eq, _ in res), f"pair differs from one stream: {[(b, e) for b, eq, e in res if not eq]}"
