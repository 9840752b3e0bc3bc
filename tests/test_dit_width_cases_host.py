"""Vet tests/dit_width_cases.py before the GPU tests rely on it: the fp32 restatement of every reference stays ORACLE_MARGIN inside
the bound the GPU result will be held to (so a bound means something), and the geometries and kernel widths reach both sides of
every dispatch decision the restatement knows.  CPU only."""
import pytest
import torch

from tests import dit_width_cases as wc
from tests.util import max_rel, rel_l2, rel_linf

M = wc.ORACLE_MARGIN


@pytest.mark.parametrize("tag", list(wc.GEOMETRIES))
def test_fp32_oracle_error_is_a_factor_below_the_bounds(tag):
    y64, l64, G64 = wc.geometry_oracle(tag, True)
    y32, l32, G32 = wc.geometry_oracle(tag, False)
    assert bool(torch.isfinite(y64).all()) and float(l64.min()) > 0
    assert rel_linf(y32, y64) < wc.X_HAT / M, rel_linf(y32, y64)
    assert abs(float(l32.mean()) / float(l64.mean()) - 1) < wc.LOSS_MEAN / M
    assert max_rel(l32, l64) < wc.LOSS_SAMPLE / M, max_rel(l32, l64)
    for k in G64:
        assert float(G64[k].norm()) > 0, k
        assert rel_l2(G32[k], G64[k]) < wc.GRAD / M, (k, rel_l2(G32[k], G64[k]))
        if G64[k].ndim == 2 or k.endswith("bias"):
            worst = max(wc.block_errors(G32[k], G64[k]))
            assert worst < wc.GRAD / M, (k, worst)


def test_block_statistic_sees_what_the_whole_tensor_figure_misses():
    """One wrong column among 320, a wrong block of 64 in a bias, a missing 64-row slab of 3: the block statistic reads 0.1 or more."""
    gen = torch.Generator().manual_seed(3)
    ref = torch.randn(320, generator=gen, dtype=torch.float64)
    got = ref.clone()
    got[300] += ref.pow(2).mean().sqrt()          # one element off by the tensor's RMS
    assert rel_l2(got, ref) < 0.06 and max(wc.block_errors(got, ref)) >= 0.1
    got = ref.clone()
    got[256:] *= 1 - 1 / 3                         # columns 256..319 lack one slab of three
    assert max(wc.block_errors(got, ref)) >= 0.3 and max(wc.block_errors(got, ref)[:4]) == 0.0
    w = torch.randn((320, 40), generator=gen, dtype=torch.float64)
    assert len(wc.block_errors(w, w)) == 5 and max(wc.block_errors(w, w)) == 0.0


@pytest.mark.parametrize("d", wc.GATE_D)
def test_gate_and_ln_mod_fp32_restatement_margin(d):
    for Bs, tokens in wc.GATE_ROWS:
        g64, g32 = wc.gate_reference(d, Bs, tokens, torch.float64), wc.gate_reference(d, Bs, tokens, torch.float32)
        assert rel_linf(g32["ddelta"], g64["ddelta"]) < wc.DDELTA / M
        assert rel_linf(wc.chunk(g32["dmod"], d, wc.G_A), wc.chunk(g64["dmod"], d, wc.G_A)) < wc.SUMS / M
        c = wc.bwd_inputs(d, Bs, tokens)
        rewound = g32["x2"] - wc.chunk(c["mod"], d, wc.G_A)[c["rows"]] * c["delta"]  # x2 - gate * delta in fp32
        assert rel_linf(rewound, g64["x1"]) < wc.REWIND / M
        l64, l32 = wc.ln_mod_reference(d, Bs, tokens, torch.float64), wc.ln_mod_reference(d, Bs, tokens, torch.float32)
        assert rel_linf(l32["dX"], l64["dX"]) < wc.DX / M, (d, Bs, tokens, rel_linf(l32["dX"], l64["dX"]))
        for c in (wc.SH_M, wc.SC_M):
            e = rel_linf(wc.chunk(l32["dmod"], d, c), wc.chunk(l64["dmod"], d, c))
            assert e < wc.SUMS / M, (d, Bs, tokens, c, e)
        # the other block's half and the chunks this kernel does not own stay what they were
        keep = torch.ones(wc.DEPTH_ROWS * 6 * d, dtype=torch.bool)
        for c in (wc.SH_M, wc.SC_M):
            keep[wc.chunk_offset(d, c):wc.chunk_offset(d, c) + d] = False
        assert torch.equal(l64["dmod"][:, keep], wc.bwd_inputs(d, Bs, tokens)["dmod0"].double()[:, keep])
        assert float(wc.bwd_inputs(d, Bs, tokens)["dmod0"].abs().min()) > 0  # accumulation is visible everywhere


@pytest.mark.parametrize("d", wc.FUSED_D)
def test_fused_fp32_restatement_margin(d):
    for Bs, tokens in wc.FUSED_ROWS:
        for mode in wc.FUSED_MODES:
            ln, gt = mode != "gate", mode != "ln"
            r64 = wc.fused_reference(d, Bs, tokens, torch.float64, ln, gt)
            r32 = wc.fused_reference(d, Bs, tokens, torch.float32, ln, gt)
            assert rel_linf(r32["dX"], r64["dX"]) < wc.DX / M, (d, Bs, tokens, mode, rel_linf(r32["dX"], r64["dX"]))
            if gt:
                assert rel_linf(r32["ddelta"], r64["ddelta"]) < wc.DDELTA / M
            for c in ((wc.SH_M, wc.SC_M) if ln else ()) + ((wc.G_A,) if gt else ()):
                e = rel_linf(wc.chunk(r32["dmod"], d, c), wc.chunk(r64["dmod"], d, c))
                assert e < wc.SUMS / M, (d, Bs, tokens, mode, c, e)
        # the fp32 statistics the kernel is handed are those of the fp64 rows to fp32 accuracy
        x = wc.fused_reference(d, Bs, tokens, torch.float64)["x"]
        st = wc.forward_stats(x)
        assert max_rel(st[:, 1], torch.rsqrt(x.var(dim=1, unbiased=False) + 1e-5)) < 1e-6


@pytest.mark.parametrize("shape", wc.TN_SHAPES + tuple((m, n1, k) for m, n1, n2, k in wc.TN_PAIR_SHAPES))
def test_gemm_tn_fp32_restatement_margin(shape):
    w64, c64 = wc.tn_reference(*shape, torch.float64)
    w32, c32 = wc.tn_reference(*shape, torch.float32)
    assert rel_linf(w32, w64) < wc.TN / M, rel_linf(w32, w64)
    assert rel_linf(c32, c64) < wc.COLSUM / M, rel_linf(c32, c64)


def test_geometries_reach_every_dispatch_decision_from_both_sides():
    """At the MI355X's 256 CUs: both values of rel_dd, rel_fc1, rel_qkv and pair; a partly filled and a full vector for VPL 1 and for
    VPL 4 in the kernel sweeps, partly filled ones at both VPLs in the engines; each tag decides what its table row says."""
    D = {t: wc.dispatch(t) for t in wc.GEOMETRIES}
    for key in ("rel_dd", "rel_fc1", "rel_qkv", "pair"):
        assert {d[key] for d in D.values()} == {True, False}, key
    assert (D["w192"]["rel_dd"], D["w192"]["rel_fc1"], D["w192"]["vpl"], D["w192"]["slots"]) == (False, True, 1, (48, 64))
    assert (D["w320"]["rel_dd"], D["w320"]["pair"], D["w320"]["vpl"], D["w320"]["slots"], D["w320"]["depth"]) == (True, False, 4, (80, 256), 2)
    assert (D["w384_dh128"]["dh"], D["w384_dh128"]["rel_qkv"]) == (128, False)
    assert D["w960"]["slots"] == (240, 256) and D["w960"]["rel_dd"]
    assert (D["s384_t256"]["rel_dd"], D["s384_t256"]["rel_qkv"], D["s384_t256"]["pair"]) == (True, True, False)
    assert D["w512_t256"]["pair"] and D["w512_t256"]["tn"]["pair"][:3] == (512, 1536 + 512, 512)
    assert D["b768_t256"]["pair"] and D["b768_t256"]["tn"]["pair"][:3] == (512, 2304 + 768, 768) and D["b768_t256"]["depth"] == 2
    assert (D["w320_m128"]["rel_dd"], D["w320_m128"]["rel_fc1"]) == (True, False)
    # rel_dd && rel_qkv without pair, and with it
    assert {(d["rel_dd"] and d["rel_qkv"], d["pair"]) for d in D.values()} >= {(True, False), (True, True), (False, False)}
    # the dropout runs: hash masks at 64 tokens (two-pass attention backward); at 256 tokens x head dim 64 the mask words, which the
    # attention forward computes itself where tokens != 16 * heads
    a, b = wc.dispatch("w320", wc.DROPOUT["w320"]), wc.dispatch("b768_t256", wc.DROPOUT["b768_t256"])
    assert a["hash_masks"] and not a["rel_qkv"]
    assert not b["hash_masks"] and b["rel_qkv"] and b["pair"] and not b["mask_ride"]
    # every head count of the issue; every tag is a geometry the engines document as supported
    assert {g[2] for g in wc.GEOMETRIES.values()} >= {3, 5, 6, 8, 12, 15}
    for t, (shape, dim, heads, depth, B, _) in wc.GEOMETRIES.items():
        assert dim % 64 == 0 and 128 < dim < 1024 and dim // heads in (64, 128) and dim % heads == 0 and wc.tokens_of(t) in (64, 256), t
    # kernel sweeps
    for fused, widths in ((False, wc.GATE_D), (True, wc.FUSED_D)):
        fill = {}
        for d in widths:
            v, used, slots = wc.lane_fill(d, fused)
            fill.setdefault(v, set()).add(used < slots)
        assert fill[1] == {True, False} and fill[4] == {True, False}, (fused, fill)
        if not fused:
            assert fill[8] == {True, False}
        # both neighbours of each instance threshold
        assert {252, 256, 260} <= set(widths) and {1020, 1024} <= set(widths)
    assert wc.vpl(2052, False) is None and wc.vpl(102, False) is None and wc.vpl(1028, True) is None and wc.vpl(1028, False) == 8
    assert all(t % 32 == 0 for _, t in wc.GATE_ROWS) and all(t % 64 == 0 for _, t in wc.FUSED_ROWS)


def test_tn_shapes_are_the_engines_and_split_as_stated():
    issued = {s[:3] for t in wc.GEOMETRIES for s in wc.dispatch(t)["tn"].values()}
    for shape in ((192, 320, 1280), (192, 1280, 320), (192, 16, 320), (3, 1920, 320), (512, 1152, 384), (512, 384, 128)):
        assert shape in issued and shape in wc.TN_SHAPES, shape
    # 1056 rows: two ragged token ranges; the engine's own 512 rows are one range
    for shape in ((1056, 768, 3072), (1056, 2304, 768)):
        assert wc.tn_splits(*shape) == (2, 544) and shape in wc.TN_SHAPES
    assert wc.tn_splits(512, 2304, 768)[0] == 1 and wc.tn_splits(192, 1280, 320)[0] == 1
    assert wc.tn_splits(1056, 2304 + 768, 768) == (2, 544)
    # the benchmark's regime, as gemm_tn.hip's comment on the qkv gradient states it: 48 tiles, 5 token ranges
    assert wc.tn_splits(16384, 3072, 1024)[0] == 5
    for m, n1, n2, k in wc.TN_PAIR_SHAPES:
        assert n1 % 256 == 0 and n1 == 3 * n2 and k == n2


@pytest.mark.parametrize("tag", list(wc.GEOMETRIES))
def test_backward_workspace_holds_every_weight_gradient_slab(tag):
    """The slabs of every weight-gradient launch the restatement lists fit the workspace the engine asks for (the patch-8 work found
    them undersized for one geometry)."""
    import ctypes as C
    from bsi_amd import _native as N
    lib = N.lib()
    shape, dim, heads, depth, B, _ = wc.GEOMETRIES[tag]
    cfg = N.DitConfig(shape[0], shape[1], shape[2], wc.PATCH, dim, depth, heads, wc.FF[0], wc.FF[1])
    total = lib.bsi_dit_backward_workspace_bytes(C.byref(cfg), B)
    d = wc.dispatch(tag)
    assert lib.bsi_dit_kpad(C.byref(cfg)) == d["tn"]["enc"][2]
    widest = max(lib.bsi_gemm_tn_workspace_bytes(d["M"], 4 * dim, dim), lib.bsi_gemm_tn_workspace_bytes(*d["tn"]["enc"][:3]))
    assert total >= widest
    for name, (m, n, k, splits, _) in d["tn"].items():
        slabs = splits * n * k * 4 if splits > 1 else 0   # a single token range writes the gradient in place
        assert slabs + (splits * n * 4 if splits > 1 else 0) <= widest, (name, slabs, widest)


@pytest.mark.parametrize("dim,heads,shape", [(512, 8, (3, 16, 16)), (1024, 16, (3, 16, 16)), (768, 12, (3, 32, 32))])
def test_backward_workspace_holds_the_adaln_bias_slabs_at_1024_images(dim, heads, shape):
    """From 1024 images on, tn_splits cuts the B sample rows of the adaLN output layer's weight gradient [6 dim, dim] in two, and
    bsi_gemm_tn_bias_bf16 keeps its bias-gradient slabs behind 16 x N x K floats of the region it is handed.  That region lies between
    regions whose sizes are known; the workspace has to hold all of them.  (The region used to be sized for fc1 / fc2 [4 dim, dim] alone:
    the slabs then lay 10 MB past the end of the workspace at dim 512.)"""
    import ctypes as C
    from bsi_amd import _native as N
    lib = N.lib()
    B, tokens = 1024, (shape[1] // wc.PATCH) * (shape[2] // wc.PATCH)
    M = B * tokens
    cfg = N.DitConfig(shape[0], shape[1], shape[2], wc.PATCH, dim, 1, heads, wc.FF[0], wc.FF[1])
    splits, _ = wc.tn_splits(B, 6 * dim, dim)
    assert splits == 2
    before = M * dim * 4 + M * dim * 2 + M * 4 * dim * 2 + M * dim * 2 + 2 * (tokens // 64) * B * 6 * dim * 4 + B * 6 * dim * 2  # dX .. dmod_bf
    slabs_end = 16 * 6 * dim * dim * 4 + splits * 6 * dim * 4
    after = 2 * (M // 64) * dim * 4 + (M // 128) * 4 * dim * 4 + B * 3 * dim * 4  # rows_fc2, rows_out, rows_fc1, rows_qkv
    assert lib.bsi_dit_backward_workspace_bytes(C.byref(cfg), B) >= before + slabs_end + after
    # below 1024 images the gradient is written in place and no slab is touched
    assert wc.tn_splits(1023, 6 * dim, dim)[0] == 1
