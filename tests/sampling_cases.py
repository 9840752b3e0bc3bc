"""Seeded cases for the DiT sampling kernels outside the GEMMs (persistent attention, the LayerNorm + modulate passes, the final
kernel, a small engine), shared by tools/record_sampling_fixtures.py -- which records their outputs with the build it is run on --
and tests/test_hip_sampling_fixtures.py, which holds the current build against that record bit for bit.

Every case draws its inputs from a CPU generator, runs on the GPU and returns {name: CPU tensor}.  The record keeps, per tensor,
the SHA-256 of its bytes and a strided sample of its words: the outputs themselves (9 MB for the 272-pair attention case alone)
do not belong in the repository, and equal digests are equal bits."""
import ctypes as C
import hashlib
import json
import os

import torch

DEV = "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_kernels.json")
SAMPLE = 64  # words of every tensor kept verbatim beside its digest


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _words(t):
    """The tensor's elements as integers of its own width (a view of the bits)."""
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).reshape(-1)


def digest(t):
    w = _words(t.cpu())
    step = max(1, w.numel() // SAMPLE)
    return {"shape": list(t.shape), "dtype": str(t.dtype).replace("torch.", ""),
            "sha256": hashlib.sha256(w.numpy().tobytes()).hexdigest(), "sample_step": step,
            "sample": [int(v) for v in w[::step][:SAMPLE]]}


def load_fixture(path=FIXTURE):
    with open(path) as f:
        return json.load(f)


def assert_matches(case, got, fixture):
    """`got` ({name: tensor}) against the recorded entry of `case`: the sample with torch.equal (a readable first difference), then
    the digest of all bytes."""
    want = fixture[case]
    assert sorted(got) == sorted(want), (case, sorted(got), sorted(want))
    for name, t in got.items():
        rec, w = want[name], _words(t.cpu())
        assert list(t.shape) == rec["shape"] and str(t.dtype).replace("torch.", "") == rec["dtype"], (case, name, t.shape, t.dtype)
        sample = torch.tensor(rec["sample"], dtype=w.dtype)
        assert torch.equal(w[::rec["sample_step"]][:SAMPLE], sample), f"{case}/{name}: sampled words differ from the recorded build"
        assert hashlib.sha256(w.numpy().tobytes()).hexdigest() == rec["sha256"], f"{case}/{name}: bits differ from the recorded build"


# ----------------------------------------------------------------------------------------------
# attention, 256 tokens, head dim 64 (the persistent kernel)
# ----------------------------------------------------------------------------------------------
ATTN_CASES = {  # id -> (B, heads, CU reserve)
    "attn_1pair": (1, 1, 0),
    "attn_3pairs": (1, 3, 0),
    "attn_272pairs": (17, 16, 0),       # more pairs than CUs: some workgroups take a second pair
    "attn_272pairs_reserve64": (17, 16, 64),
}
ATTN_DROP = ("attn_drop_lse_3pairs", 1, 3, 0.1, 0x5EEDC0FFEE, 3)  # id, B, heads, p, seed, site


def attn_input(case):
    B, heads = (ATTN_DROP[1], ATTN_DROP[2]) if case == ATTN_DROP[0] else ATTN_CASES[case][:2]
    gen = torch.Generator().manual_seed(1000 + 16 * B + heads)
    return bf16r(torch.randn((B, 256, 3, heads, 64), generator=gen) * 1.5)


def run_attention(N, case):
    lib = N.lib()
    qkv = attn_input(case)
    B, _, _, heads, dh = qkv.shape
    d = heads * dh
    dq = qkv.to(torch.bfloat16).to(DEV).contiguous()
    out = torch.full((B * 256, d), float("nan"), dtype=torch.bfloat16, device=DEV)
    if case == ATTN_DROP[0]:
        _, _, _, p, seed, site = ATTN_DROP
        lse = torch.full((B, heads, 256), float("nan"), device=DEV)
        words = torch.zeros((B * heads, 16, 64), dtype=torch.int64, device=DEV)
        N.check(lib.bsi_attention_fwd_dropout(N.ptr(dq), 3 * d, B, 256, heads, dh, N.ptr(out), d, N.ptr(lse), p, seed, site, N.ptr(words),
                                              N.stream()))
        alone = torch.zeros_like(words)
        N.check(lib.bsi_attention_dropout_words(p, seed, site, B * heads, N.ptr(alone), N.stream()))
        torch.cuda.synchronize()
        assert torch.equal(words, alone), "the forward's mask words are not those of bsi_attention_dropout_words"
        return {"out": out.cpu(), "lse": lse.cpu(), "words": words.cpu()}
    reserve = ATTN_CASES[case][2]
    try:
        N.check(lib.bsi_set_cu_reserve(reserve))
        N.check(lib.bsi_attention_fwd(N.ptr(dq), 3 * d, B, 256, heads, dh, N.ptr(out), d, N.stream()))
        torch.cuda.synchronize()
    finally:
        N.check(lib.bsi_set_cu_reserve(0))
    return {"out": out.cpu()}


# ----------------------------------------------------------------------------------------------
# LayerNorm + modulate passes at d = 1024 (four waves per workgroup: M = 17 is 4 * 4 + 1)
# ----------------------------------------------------------------------------------------------
LN_D, LN_TOKENS = 1024, 3  # three rows per image: with M = 5 and 17 the last image is partial, and images straddle workgroups
LN_CASES = [(M, shared, upd, write_x) for M in (1, 5, 17) for shared in (1, 0)
            for upd, write_x in (("none", 1), ("one", 1), ("one", 0), ("two", 1), ("two", 0))]


def ln_id(M, shared, upd, write_x):
    return f"ln_M{M}_{'row1' if shared else 'rowB'}_{upd}_w{write_x}"


def ln_inputs(M, shared, upd, write_x):
    d = LN_D
    images = (M + LN_TOKENS - 1) // LN_TOKENS
    gen = torch.Generator().manual_seed(7 * M + 3 * shared + len(upd) + write_x)
    x = torch.randn((M, d), generator=gen) * 2 + 0.3
    d0 = bf16r(torch.randn((M, d), generator=gen))
    d1 = bf16r(torch.randn((M, d), generator=gen))
    mod = torch.randn((1 if shared else images, 6 * d), generator=gen) * 0.3  # chunks: gate0, gate, shift, scale (0, 2, 3, 4)
    return x, d0, d1, mod


def run_ln(N, M, shared, upd, write_x):
    lib = N.lib()
    d = LN_D
    x, d0, d1, mod = ln_inputs(M, shared, upd, write_x)
    dx, dmod = x.to(DEV), mod.to(DEV)
    b0, b1 = d0.to(torch.bfloat16).to(DEV), d1.to(torch.bfloat16).to(DEV)
    out = torch.full((M, d), float("nan"), dtype=torch.bfloat16, device=DEV)
    col = lambda k: C.c_void_p(dmod.data_ptr() + 4 * k * d)  # noqa: E731
    rows = mod.shape[0]
    if upd == "none":
        N.check(lib.bsi_ln_modulate(N.ptr(dx), M, d, 1e-5, col(3), col(4), rows, 6 * d, LN_TOKENS, None, None, N.ptr(out), N.stream()))
    else:
        two = upd == "two"
        N.check(lib.bsi_resid2_ln_modulate(N.ptr(dx), M, d, 1e-5, N.ptr(b0) if two else None, col(0) if two else None, N.ptr(b1), col(2),
                                           write_x, col(3), col(4), rows, 6 * d, LN_TOKENS, N.ptr(out), N.stream()))
    torch.cuda.synchronize()
    return {"x": dx.cpu(), "out": out.cpu()}


# ----------------------------------------------------------------------------------------------
# engines: the final kernel through bsi_dit_forward, one training forward (the MASKGEN pass), a small DiT
# ----------------------------------------------------------------------------------------------
ENGINE_CASES = {  # id -> (data shape, patch, dim, depth, heads, images)
    "final_p12_64tok": ((3, 16, 16), 2, 1024, 1, 16, 1),      # dit_final_kernel<4, true>, P = 12, Mtok = 64
    "final_p12_768tok": ((3, 32, 32), 2, 1024, 1, 16, 3),     # Mtok = 3 x 256
    "final_p48_l2weights": ((3, 32, 32), 4, 1024, 1, 16, 1),  # P = 48: 192 KB of decoder weights, the WLDS = false instance
    "engine_dim128": ((3, 32, 32), 2, 128, 2, 2, 3),          # whole engine: two blocks, tokens_out and out
}
TRAIN_CASE = ("train_maskgen_256rows", (3, 32, 32), 2, 1024, 1, 16, 1, 0.1, 0xD1CE5EED)  # M = 256 = B * heads * 16: the smallest


def make_dit(shape, patch, dim, depth, heads, dropout=None):
    """A DenoisingDiT whose every parameter is seeded on the CPU (the decoder of a fresh model is zero: it would hide the final kernel)."""
    from bsi_amd.models.dit import DenoisingDiT
    from bsi_amd.nn import FourierFeatures
    torch.manual_seed(0)
    m = DenoisingDiT(shape, patch, dim, depth, heads, dropout=dropout, fourier_features=FourierFeatures(n_min=6, n_max=8))
    gen = torch.Generator().manual_seed(dim + 10 * patch + depth)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.randn(p.shape, generator=gen) * 0.02)
    m.cu_pair = None
    return m.to(DEV)


def _engine_inputs(shape, B, seed):
    gen = torch.Generator().manual_seed(seed)
    mu = torch.randn((B, *shape), generator=gen) * 2
    t = torch.rand(B, generator=gen)
    c = torch.rand((3, B), generator=gen) + 0.5
    return mu.to(DEV), t.to(DEV), [c[i].contiguous().to(DEV) for i in range(3)]


def run_engine(N, case):
    shape, patch, dim, depth, heads, B = ENGINE_CASES[case]
    model = make_dit(shape, patch, dim, depth, heads).eval()
    mu, t, (c_in, c_skip, c_out) = _engine_inputs(shape, B, 50 + dim + patch + B)
    with torch.no_grad():
        mod = model.adaln_table(t)
        out, tokens = model.forward_native(mu, mod, c_in=c_in, c_skip=c_skip, c_out=c_out, coef_stride=1, return_tokens=True)
        shared, _ = model.forward_native(mu, mod[:1].contiguous(), c_in=c_in, c_skip=c_skip, c_out=c_out, coef_stride=1, return_tokens=True)
    torch.cuda.synchronize()
    # `out_shared_row`: one modulation row for all images, as in sampling (the LayerNorm passes take their inference instance)
    return {"out": out.cpu(), "tokens_out": tokens.cpu(), "out_shared_row": shared.cpu()}


def run_train(N):
    _, shape, patch, dim, depth, heads, B, p, seed = TRAIN_CASE
    lib = N.lib()
    model = make_dit(shape, patch, dim, depth, heads, dropout=p).train()
    mu, t, (c_in, c_skip, c_out) = _engine_inputs(shape, B, 77)
    with torch.no_grad():
        cfg, w, _, _ = model.native_pack()
        out = torch.full_like(mu, float("nan"))
        tape = torch.empty(lib.bsi_dit_tape_bytes(C.byref(cfg), B), dtype=torch.uint8, device=DEV)
        N.check(lib.bsi_dit_train_forward(C.byref(cfg), C.byref(w), B, N.ptr(mu), N.ptr(t), N.ptr(c_in), N.ptr(c_skip), N.ptr(c_out),
                                          N.ptr(out), N.ptr(tape), p, seed, N.stream()))
    torch.cuda.synchronize()
    return {"out": out.cpu()}


def all_cases(N):
    """(id, thunk) of every recorded case."""
    cases = [(c, (lambda c=c: run_attention(N, c))) for c in list(ATTN_CASES) + [ATTN_DROP[0]]]
    cases += [(ln_id(*a), (lambda a=a: run_ln(N, *a))) for a in LN_CASES]
    cases += [(c, (lambda c=c: run_engine(N, c))) for c in ENGINE_CASES]
    cases.append((TRAIN_CASE[0], lambda: run_train(N)))
    return cases
