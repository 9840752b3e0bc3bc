#!/usr/bin/env python
"""First measurements of the DenoisingDiT at patch 8 (decoder width P = 192) on one GPU.

  (a) the two decoder kernels alone at d = 1024 and equal token count M: P = 48 (3x64x64 at patch 4, the kernels as they were) against
      P = 192 (3x128x128 at patch 8), HIP events around repeated launches after warm-up, the two widths alternating window by window.
      The kernels' launchers are internal C++ functions of libbsi_hip.so (dit_ops.h), not part of the C ABI; this tool calls them
      through their mangled names.
  (b) DiT-L/8 (dim 1024, depth 24, 16 heads, Fourier features 6..8) at 3x64x64 and 3x128x128: images/s of BSI.sample k = 128, the
      share of the final kernel in it (bsi_prof classes of the inference engine), and ms per DPTrainer step.

    python tools/dit_patch_bench.py [--quick] > profiles/rN/dit_patch8.txt
"""
import argparse
import ctypes as C
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bsi_amd import BSI, Discretization  # noqa: E402
from bsi_amd import _native as N  # noqa: E402
from bsi_amd.models.dit import DenoisingDiT  # noqa: E402
from bsi_amd.nn import FourierFeatures  # noqa: E402

DEV = torch.device("cuda", 0)
FINAL = "_Z20bsi_dit_final_launchPKfiiiS0_S0_S0_S0_iiiiS0_S0_S0_iPKvS0_iiPfP12ihipStream_t"
FINAL_BWD = "_Z24bsi_dit_final_bwd_launchPKfiiiS0_S0_S0_iiiiS0_S0_iPfPvS2_S1_S1_S1_S1_P12ihipStream_t"
PARTS = "_Z30bsi_dit_final_bwd_parts_floatsiii"


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def event_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def decoder_case(shape, patch, d, B):
    """Buffers and the two launch closures of one decoder geometry."""
    raw = C.CDLL(N.LIB_PATH)
    p, i, vp = C.c_void_p, C.c_int, C.c_void_p
    fin, bwd, parts_fn = getattr(raw, FINAL), getattr(raw, FINAL_BWD), getattr(raw, PARTS)
    fin.restype = bwd.restype = i
    fin.argtypes = [p, i, i, i, p, p, p, p, i, i, i, i, p, p, p, i, p, p, i, i, p, vp]
    bwd.argtypes = [p, i, i, i, p, p, p, i, i, i, i, p, p, i, p, p, p, p, p, p, p, vp]
    parts_fn.restype, parts_fn.argtypes = C.c_size_t, [i, i, i]
    Cc, H, W = shape
    P, tokens = Cc * patch * patch, (H // patch) * (W // patch)
    M, Pp = B * tokens, (P + 7) // 8 * 8
    g = torch.Generator(DEV).manual_seed(P)
    r = lambda *s: torch.randn(s, device=DEV, generator=g)  # noqa: E731
    x, lnw, lnb, dw, db = r(M, d), 1 + 0.05 * r(d), 0.05 * r(d), r(P, d) / d ** 0.5, 0.01 * r(P)
    mu, cs, co, out, gx = r(B, *shape), torch.rand(B, device=DEV), torch.rand(B, device=DEV), torch.empty(B, *shape, device=DEV), r(B, *shape)
    dX, yb, dYb = torch.empty(M, d, device=DEV), torch.empty(M, d, dtype=torch.bfloat16, device=DEV), torch.empty(M, Pp, dtype=torch.bfloat16, device=DEV)
    ddb, dlw, dlb = torch.empty(P, device=DEV), torch.empty(d, device=DEV), torch.empty(d, device=DEV)
    parts = torch.empty(parts_fn(M, d, P), device=DEV)
    keep = (x, lnw, lnb, dw, db, mu, cs, co, out, gx, dX, yb, dYb, ddb, dlw, dlb, parts)
    q = lambda t: t.data_ptr()  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream

    def fwd():
        assert fin(q(x), M, d, P, q(lnw), q(lnb), q(dw), q(db), Cc, H, W, patch, q(mu), q(cs), q(co), 1, None, None, 1, 0, q(out), st) == 0

    def back():
        assert bwd(q(x), M, d, P, q(lnw), q(lnb), q(dw), Cc, H, W, patch, q(gx), q(co), 1, q(dX), q(yb), q(dYb), q(ddb), q(dlw), q(dlb), q(parts), st) == 0

    return dict(P=P, M=M, d=d, fwd=fwd, bwd=back, keep=keep, out=out, dX=dX)


def decoder_kernels(B, n, windows):
    print(f"(a) decoder kernels alone, d = 1024, B = {B} images of 256 tokens (M = {B * 256}); microseconds per call, {windows} windows of {n} calls,")
    print("    the two widths alternating; bsi_dit_final_bwd_launch = the kernel + its three slab reductions (+ the copy at odd P)")
    cases = [decoder_case((3, 64, 64), 4, 1024, B), decoder_case((3, 128, 128), 8, 1024, B)]
    for c in cases:
        for _ in range(5):
            c["fwd"](); c["bwd"]()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(c["out"]).all()) and bool(torch.isfinite(c["dX"]).all())
    res = {(c["P"], k): [] for c in cases for k in ("fwd", "bwd")}
    for _ in range(windows):
        for k in ("fwd", "bwd"):
            for c in cases:
                res[(c["P"], k)].append(1e3 * event_ms(c[k], n))
    for k, name in (("fwd", "dit_final"), ("bwd", "dit_final_bwd")):
        for c in cases:
            v = res[(c["P"], k)]
            flop = 2.0 * c["M"] * c["P"] * c["d"]
            print(f"  {name:14s} P = {c['P']:3d}:  " + "  ".join(f"{t:7.1f}" for t in v) + f"   median {median(v):7.1f} us   "
                  f"{flop / median(v) / 1e6:6.2f} TFLOP/s fp32, x row stream {c['M'] * c['d'] * 4 / median(v) / 1e6:5.2f} TB/s")
        a, b = median(res[(cases[0]["P"], k)]), median(res[(cases[1]["P"], k)])
        print(f"  {name}: P = 192 takes {b / a:.2f} x the time of P = 48 for 4 x the decoder arithmetic")
    return {k: median(v) for k, v in res.items()}


def dit_l8(shape, B_sample, B_train, k, steps):
    from bsi_amd.dp import DPTrainer
    torch.manual_seed(0)
    model = DenoisingDiT(shape, 8, 1024, 24, 16, dropout=0.05, fourier_features=FourierFeatures(n_min=6, n_max=8))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for blk in model.dit.blocks:
            lin = blk.adaLN_modulation[2]
            lin.weight.copy_(0.02 * torch.randn(lin.weight.shape, generator=g))
            lin.bias.copy_(0.02 * torch.randn(lin.bias.shape, generator=g))
    model = model.to(DEV).eval()
    bsi = BSI(model, data_shape=shape, lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=k, preconditioning="edm",
              discretization=Discretization.image_8bit()).to(DEV)
    tokens = (shape[1] // 8) * (shape[2] // 8)
    print(f"  DiT-L/8 at {shape[0]}x{shape[1]}x{shape[2]}: {tokens} tokens, P = 192, encoder K = 1344")
    gen = torch.Generator(DEV).manual_seed(2)
    with torch.no_grad():
        s = bsi.sample(B_sample, gen)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(s).all())
        rates = []
        for _ in range(2):
            t0 = time.perf_counter()
            bsi.sample(B_sample, gen)
            torch.cuda.synchronize()
            rates.append(B_sample / (time.perf_counter() - t0))
        print(f"    BSI.sample k = {k}, {B_sample} images per call:  " + "  ".join(f"{r:.1f}" for r in rates) + " images/s")
        N.check(N.lib().bsi_prof_enable(0x3FF))
        bsi.sample(B_sample, gen)
        torch.cuda.synchronize()
        tot, per = 0.0, {}
        for name, cls in (("gemm_qkv", 0), ("gemm_out", 1), ("gemm_fc1", 2), ("gemm_fc2", 3), ("attention", 4), ("ln_modulate", 5),
                          ("prologue", 6), ("final", 7), ("gemm_enc", 8), ("adaln", 9)):
            cnt, ms = C.c_int(), C.c_double()
            N.check(N.lib().bsi_prof_read(cls, C.byref(cnt), C.byref(ms)))
            per[name] = (cnt.value, ms.value)
            tot += ms.value
        N.check(N.lib().bsi_prof_enable(0))
        evals = max(per["final"][0], 1)
        block = sum(per[n][1] for n in ("gemm_qkv", "gemm_out", "gemm_fc1", "gemm_fc2", "attention", "ln_modulate")) / evals / 24
        fin = per["final"][1] / evals
        print(f"    kernel classes of one such call (HIP events, {evals} evaluations): " + ", ".join(f"{n} {v[1]:.1f} ms" for n, v in per.items()))
        print(f"    dit_final {1e3 * fin:.1f} us per evaluation = {100 * per['final'][1] / tot:.2f} % of the kernel time; one DiT block of the same "
              f"pass {1e3 * block:.1f} us; encoder GEMM (K = 1344) {1e3 * per['gemm_enc'][1] / evals:.1f} us")
    model.train()
    tr = DPTrainer(bsi, lr=5e-4, betas=(0.9, 0.99), weight_decay=1e-2, max_grad_norm=1.0)
    x = (torch.round(255 * torch.rand((B_train, *shape), device=DEV, generator=gen)) / 255) * 2 - 1
    for _ in range(2):
        loss = tr.train_step(x, gen)
    torch.cuda.synchronize()
    ms = []
    for _ in range(2):
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = tr.train_step(x, gen)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / steps)
    assert bool(torch.isfinite(torch.as_tensor(loss)).all())
    print(f"    DPTrainer step, batch {B_train}, dropout 0.05:  " + "  ".join(f"{m:.1f}" for m in ms) + f" ms per step = {B_train / min(ms) * 1e3:.0f} images/s"
          f"; one block's forward + backward ~ step / 24 = {min(ms) / 24:.2f} ms")
    return dict(tokens=tokens, B_train=B_train, step_ms=min(ms), block_fwd_us=1e3 * block, final_us=1e3 * fin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="small batches and k = 16: a functional pass, not a measurement")
    a = ap.parse_args()
    print("DenoisingDiT at patch 8: decoder kernels and DiT-L/8, measured ONCE on ONE box (" + torch.cuda.get_device_name(0) + ")")
    print("=" * 110)
    kern = decoder_kernels(8 if a.quick else 64, 5 if a.quick else 20, 2 if a.quick else 4)
    print()
    print("(b) DiT-L/8 = DenoisingDiT(shape, patch 8, dim 1024, depth 24, heads 16, Fourier features 6..8)")
    k = 16 if a.quick else 128
    r64 = dit_l8((3, 64, 64), 8 if a.quick else 256, 8 if a.quick else 256, k, 2 if a.quick else 5)
    r128 = dit_l8((3, 128, 128), 4 if a.quick else 64, 4 if a.quick else 64, k, 2 if a.quick else 5)
    print()
    # the 3x128x128 training batch has the token count of (a): B_train * 256 tokens
    if not a.quick and r128["B_train"] * r128["tokens"] == 64 * 256:
        share = kern[(192, "bwd")] / 1e3 / r128["step_ms"]
        print(f"(c) dit_final_bwd (P = 192, M = 16384) = {kern[(192, 'bwd')]:.0f} us = {100 * share:.2f} % of the 3x128x128 train step; "
              f"one block's forward + backward of that step ~ {r128['step_ms'] / 24 * 1e3:.0f} us")
        print(f"    dit_final (P = 192, M = 16384) = {kern[(192, 'fwd')]:.0f} us; one block of the sampling pass at 64 images of 256 tokens: see (b)")


if __name__ == "__main__":
    main()
