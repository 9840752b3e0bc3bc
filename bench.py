#!/usr/bin/env python
"""Headline benchmark: images/s of BSI.sample (k=128, DiT-L/2, 3x32x32) on N MI355X GPUs of one node.

    python bench.py --gpus N --steps K --warmup W          (starts the N rank processes itself)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One process per GPU.  Launched WITHOUT torchrun and with --gpus N > 1, the parent process starts N children of itself
(RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set) before it has made any GPU call, relays rank 0's JSON line and exits with
the worst child status; it refuses (non-zero) when fewer than N devices are visible instead of measuring one GPU.

One "step" = one full `BSI.sample` call (k measure/refine steps = k+1 denoiser evaluations) of `--batch`
images per GPU, synthetic inputs (Gaussian noise from the device generator), random-init weights of the
BASELINE architecture (config/experiment/imagenet32.yaml:33-39 of the reference) with the adaLN output
layers ~N(0, 0.02^2) so that blocks are not the identity.  Sampling is embarrassingly parallel: ranks draw
rank-distinct chains, no data-path collective; value = images of all ranks / max-over-ranks wall time
(weak scaling).  Prints ONE JSON line on rank 0 with `roofline` (dominant kernel: the fc1 bf16 MFMA GEMM,
timed with HIP events around every launch inside the timed region) and `cpu_baseline` (the CPU oracle
timed on the host cores on a bounded sample).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0   # dense bf16 MFMA peak of the MI355X
FWD_GFLOP_PER_IMG = 161.46  # DiT-L/2 forward, 2*MAC


def pmc_traffic(batch):
    """Fabric-side bytes per fc1 launch from the committed rocprofv3 PMC passes (tools/pmc_traffic.py writes the file;
    counters cannot be collected from inside the benchmark).  None when no measurement at this batch is committed."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "fc1_traffic.json")
    try:
        with open(path) as f:
            rec = json.load(f)
        if rec.get("images_per_gpu") != batch:
            return None, None
        m = rec.get("measured", {})
        return rec["traffic_bytes_per_launch"], f"profiles/fc1_traffic.json ({m.get('date', '?')}, commit {m.get('commit', '?')}; rocprofv3 PMC passes, not this run)"
    except (OSError, KeyError, ValueError):
        return None, None


# Test hook (tests/test_hip_multigpu.py, one-GPU boxes): BSI_BENCH_ONE_DEVICE=1 puts every rank on cuda:0 and uses the gloo backend
# over device tensors, so that the WHOLE multi-rank code path of this file (self-launch, barriers, max-over-ranks timing, the
# DPTrainer exchange, the comm breakdown) runs where only one GPU is visible.  Never set by the driver; the line says so in `config`.
ONE_DEVICE = os.environ.get("BSI_BENCH_ONE_DEVICE") == "1"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=512,
                    help="images per GPU per sample() call (512 = eval_batch_size of the reference's configs, SURVEY section 8(d); "
                         "256 and 64 are reported under `secondary`)")
    ap.add_argument("--k", type=int, default=128, help="sampling steps")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--breakdown", action="store_true", help="print a per-kernel-class time breakdown to stderr")
    ap.add_argument("--train-steps", type=int, default=10, help="timed optimizer steps of the train benchmark (0 = skip)")
    ap.add_argument("--train-batch", type=int, default=512, help="GLOBAL batch of the train benchmark (split over ranks)")
    ap.add_argument("--train-timeout", type=int, default=300, help="seconds before the train benchmark is abandoned")
    ap.add_argument("--cu-reserve", type=int, default=16,
                    help="compute units the persistent kernels leave to the RCCL kernels during a data-parallel train step "
                         "(DPTrainer cu_reserve; N > 1 only, and the per-rank rehearsal at N = 1); the rank processes get "
                         "NCCL_MAX_NCHANNELS = this unless the environment already sets it")
    ap.add_argument("--no-secondary", action="store_true", help="skip the secondary measurements (UNet, DiT-L/4, ELBO)")
    ap.add_argument("--secondary-budget", type=float, default=150.0,
                    help="seconds the secondary block may use; entries that would not fit are reported as skipped")
    ap.add_argument("--secondary-only", action="store_true",
                    help="(internal) run only the secondary block and print its JSON: the main process starts this as a fresh child "
                         "so that a hang or a GPU fault in a secondary kernel cannot take the measured headline with it")
    ap.add_argument("--launch-timeout", type=int, default=3600, help="seconds before a self-launched multi-rank run is abandoned")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed sample() call returned on rank 0 as DIR/<name>.npy "
                         "(float32, at most 64 MB; a fixed seeded subset of the images beyond that) so that two builds can be "
                         "compared output for output: with the same arguments the inputs are identical from run to run")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if a.cu_reserve < 0 or a.cu_reserve % 8 or a.cu_reserve > 64:
        ap.error("--cu-reserve must be 0 or a multiple of 8 up to 64 (bsi_set_cu_reserve)")
    return a


def build_model(dev):
    from bsi_amd import BSI, Discretization
    from bsi_amd.models.dit import DenoisingDiT
    from bsi_amd.nn import FourierFeatures

    shape = (3, 32, 32)
    torch.manual_seed(0)  # identical weights on every rank
    model = DenoisingDiT(shape, 2, 1024, 24, 16, dropout=0.05, fourier_features=FourierFeatures(n_min=6, n_max=8))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for blk in model.dit.blocks:
            lin = blk.adaLN_modulation[2]
            lin.weight.copy_(0.02 * torch.randn(lin.weight.shape, generator=g))
            lin.bias.copy_(0.02 * torch.randn(lin.bias.shape, generator=g))
    model = model.to(dev).eval()
    return model, shape


def host_threads():
    """Threads actually usable on this box: CPU affinity mask, cgroup CPU quota, capped at 32 (beyond that the
    fp32 oracle's GEMMs at B=4 do not scale and oversubscription makes it slower)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 32))


def cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.lower().startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(k, reps=3):
    """CPU oracle (a port of the reference's algorithm, oracle/) on the host cores: 2 complete sampling steps
    (denoiser evaluation + measure/refine update) + the final prediction at B=8, extrapolated to k+1 evaluations per
    image.  Protocol of BASELINE.md §4: 1 warm-up run + `reps` timed repetitions, the MEDIAN is reported, with the CPU
    model and the thread count.  Bounded: (1 + reps) x 3 DiT-L/2 evaluations of 8 images (about 3.9 TFLOP of fp32 each)."""
    from oracle import bsi_oracle as bo
    from oracle import dit_oracle as do

    threads = host_threads()
    torch.set_num_threads(threads)
    shape, B = (3, 32, 32), 8
    W = do.dit_random_weights(shape, 2, 1024, 24, ff=(6, 8), seed=0)
    f = lambda m, t: do.dit_forward(W, m, t, patch_size=2, dim=1024, depth=24, heads=16, ff=(6, 8))  # noqa: E731
    o = bo.BSIOracle(f, data_shape=shape, k=k)
    g = torch.Generator().manual_seed(0)
    tt = torch.linspace(0, 1, k + 1)[[0, k // 2, k]]  # 2 steps taken from the k-step schedule
    eps0 = torch.randn((B, *shape), generator=g)
    eps = torch.randn((2, B, *shape), generator=g)
    times = []
    with torch.no_grad():
        for i in range(1 + reps):
            t0 = time.perf_counter()
            o.sample_history(eps0, eps, t=tt)          # 2 steps + final prediction = 3 evaluations
            dt = time.perf_counter() - t0
            if i > 0:                                  # run 0 is the warm-up
                times.append(dt)
    times.sort()
    med = times[len(times) // 2]
    per_eval = med / 3.0
    return {"value": B / (per_eval * (k + 1)), "unit": "images/s", "cores": threads, "kind": "port", "cpu": cpu_model(),
            "repetitions": reps, "run_seconds": [round(t, 3) for t in times],
            "sample": f"oracle (torch-CPU fp32, {threads} threads, {cpu_model()}) DiT-L/2, B={B}: 3 denoiser evaluations + 2 "
                      f"refine steps, 1 warm-up + {reps} timed runs, median {med:.2f} s, extrapolated to k+1={k + 1} "
                      "evaluations per image"}


def _timed_train(tr, x, g, n, barrier, dev, world):
    """n optimizer steps between barriers; max over ranks; (seconds, (fwd+bwd+exchange ms, optimizer ms), last loss)."""
    tr.stage_ms()
    tr.time_stages = True
    barrier()
    t0 = time.perf_counter()
    for _ in range(n):
        loss = tr.train_step(x, g)
    barrier()
    dt = time.perf_counter() - t0
    stages = tr.stage_ms()
    tr.time_stages = False
    if world > 1:
        tm = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(tm, op=torch.distributed.ReduceOp.MAX)
        dt = float(tm.item())
    return dt, stages, loss


def _without_exchange(tr, x, g, n, barrier, dev):
    """The same steps WITHOUT the gradient exchange (compute alone).  Those steps would apply each rank's own gradient / world and
    let the replicas drift apart, so the trainer's state (parameters, moments, EMA, step count) is snapshotted and restored."""
    tr.sync_params()  # an overlapped all-gather of the last timed step may still be writing the parameters
    bufs = [tr.fp.flat, tr.m, tr.v] + ([tr.ema_fp.flat] if tr.ema_fp else [])
    snap = [t.clone() for t in bufs]
    step0, ex = tr.step_count, tr.exchange
    tr.exchange = False
    try:
        tr.train_step(x, g)
        barrier()
        t1 = time.perf_counter()
        for _ in range(n):
            tr.train_step(x, g)
        barrier()
        d2 = torch.tensor([time.perf_counter() - t1], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(d2, op=torch.distributed.ReduceOp.MAX)
    finally:
        tr.exchange = ex
        tr.sync_params()
        for dst, src in zip(bufs, snap):
            dst.copy_(src)
        tr.step_count = step0
        tr.stage_ms()
    return 1e3 * float(d2.item()) / n


def _bucket_busbw(dev, world, barrier, elems=20 * 1024 * 1024, reps=5):
    """Ring bus bandwidth of ONE gradient bucket (80 MB fp32, the size of a DiT-L/2 block's bucket) all-reduced in isolation."""
    t = torch.ones(elems, dtype=torch.float32, device=dev)
    torch.distributed.all_reduce(t)
    barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        torch.distributed.all_reduce(t)
    barrier()
    sec = (time.perf_counter() - t0) / reps
    return {"bytes": 4 * elems, "ms": 1e3 * sec, "busbw_GBps": 2 * (world - 1) / world * 4 * elems / 1e9 / sec}


def train_bench(a, bsi, model, dev, world, rank, barrier):
    """Second half of the BASELINE metric: optimizer steps/s of the ImageNet32 DiT-L/2 recipe
    (config/experiment/imagenet32.yaml: global batch 512, AdamW lr 5e-4 betas (0.9, 0.99) wd 1e-2, dropout 0.05,
    clip 1.0, EMA, warm-up + cosine LR) — BSI.train_loss forward + hand-written backward + gradient exchange over
    RCCL + fused clip/AdamW/EMA.  The global batch is split per rank as bsi/data/h5image.py:312 (strong scaling).

    N > 1: the step is measured in three variants so that the first hardware run can be read -- all-reduce with the CU reserve off,
    all-reduce with `--cu-reserve` CUs left to RCCL during the backward, and the sharded step (reduce-scatter / slice update /
    all-gather) -- each with the same steps without the exchange (exposed communication = the difference); `value` is the
    all-reduce step with the reserve off (the DDP-equivalent one), the others stand beside it in `variants` and `fastest_variant`
    names the quickest.  Plus the bus bandwidth of one 80 MB bucket all-reduced in isolation and the RCCL channel cap in force."""
    from bsi_amd.dp import DPTrainer, split_batch, warmup_cosine_lr

    nb = split_batch(a.train_batch, world, rank)
    model.train()
    sched = lambda s: warmup_cosine_lr(s, base_lr=5e-4, warmup_steps=1000, max_steps=1000000, start_lr=1e-8, end_lr=5e-5)  # noqa: E731
    recipe = dict(lr=5e-4, betas=(0.9, 0.99), weight_decay=1e-2, max_grad_norm=1.0, lr_schedule=sched)
    g = torch.Generator(dev).manual_seed(99 + rank)

    def images(n):
        u = torch.rand((n, 3, 32, 32), device=dev, generator=g)
        return (torch.round(255 * u) / 255) * 2 - 1    # synthetic 8-bit images in [-1, 1]

    x = images(nb)
    variants = [("allreduce", dict(cu_reserve=0))]
    if world > 1:
        if a.cu_reserve:
            # (the reserve variant also switches the tile queue on -- off by default in DPTrainer until a run like this one has
            # exercised it beside real RCCL kernels; DPTrainer self-checks it against the static schedule first)
            variants.append((f"allreduce_cu_reserve_{a.cu_reserve}", dict(cu_reserve=a.cu_reserve, tile_queue=True)))
        variants.append(("sharded_update", dict(cu_reserve=0, shard_update=True)))
        # the sharded step with its parameter all-gather overlapped with the next forward (block-by-block gates)
        variants.append(("sharded_update_overlap", dict(cu_reserve=0, shard_update=True, overlap_gather=True)))
    runs, comm_runs = {}, {}
    for i, (name, kw) in enumerate(variants):
        try:
            tr = DPTrainer(bsi, **recipe, **kw)
            loss = tr.train_step(x, g)                      # warm-up (also builds the transposed weight shadows)
            dt, stages, loss = _timed_train(tr, x, g, a.train_steps, barrier, dev, world)
            assert torch.isfinite(loss)
            runs[name] = {"ms_per_step": 1e3 * dt / a.train_steps, "fwd_bwd_exchange_ms": stages[0] if stages else None,
                          "optimizer_ms": stages[1] if stages else None, "loss": float(loss)}
            if world > 1:
                ms_no = _without_exchange(tr, x, g, max(1, min(3, a.train_steps)), barrier, dev)
                comm_runs[name] = {"ms_per_step": runs[name]["ms_per_step"], "ms_per_step_without_exchange": ms_no,
                                   "exposed_comm_ms": runs[name]["ms_per_step"] - ms_no, "optimizer_ms": runs[name]["optimizer_ms"]}
            nbytes = 4 * tr.fp.flat.numel()
            nbuckets = len(tr.xchg.plan)
            del tr
        except Exception as e:  # noqa: BLE001  (every rank runs the same code on the same inputs: a variant fails on all ranks or none)
            if i == 0:
                raise
            runs[name] = comm_runs[name] = {"error": f"{type(e).__name__}: {e}"}
        torch.cuda.empty_cache()
    # Headline = the DDP-equivalent step (bucketed all-reduce, every rank applies the whole update, the EMA complete on every rank
    # after every step: bsi/tasks/bsi.py:163-198).  The other variants are reported beside it under `variants`, never as `value`:
    # the sharded step leaves each rank's EMA copy complete only on the slices it owns until gather_ema() runs, and beyond two
    # ranks a reduce-scatter sums in another ring order than an all-reduce (equal to rounding, not to the bit).
    head = "allreduce"
    fastest = min((n for n in runs if "error" not in runs[n]), key=lambda n: runs[n]["ms_per_step"])
    ms = runs[head]["ms_per_step"]
    comm = None
    if world > 1:
        c = comm_runs[head]
        comm = {"allreduce_bytes": nbytes, "buckets": nbuckets, "cu_reserve": a.cu_reserve if "cu_reserve" in head else 0,
                "nccl_max_nchannels": os.environ.get("NCCL_MAX_NCHANNELS"),
                "ms_per_step_without_exchange": c["ms_per_step_without_exchange"], "exposed_comm_ms": c["exposed_comm_ms"],
                "variants": comm_runs, "bucket_allreduce_alone": _bucket_busbw(dev, world, barrier)}
    per_rank = None
    if world == 1 and a.train_batch >= 8:
        # The per-rank workloads of the multi-GPU configurations (BASELINE configs[3]: the global batch split over 2 / 4 / 8
        # ranks, bsi/data/h5image.py:309-312), measured on this one GPU: the compute half of the 2- / 4- / 8-GPU step, with and
        # without the CU reserve, and the optimizer as that rank of a sharded step runs it (1 / world of every bucket; the
        # replicated optimizer is `optimizer_ms` of the headline).  Isolated: a failure here leaves the headline untouched.
        try:
            per_rank = []
            for w_ in (2, 4, 8):
                b_ = a.train_batch // w_
                xs = images(b_)
                rec = {"world": w_, "per_gpu_batch": b_, "cu_reserve": a.cu_reserve}
                for key, r_ in (("", 0), ("_cu_reserve", a.cu_reserve)):
                    if key and not r_:
                        continue
                    tr = DPTrainer(bsi, **recipe, cu_reserve=r_, tile_queue=bool(r_), rehearse=(w_, 0), shard_update=True)
                    tr.train_step(xs, g)
                    n_ = max(3, min(a.train_steps, 5))
                    dt_, st_, _ = _timed_train(tr, xs, g, n_, barrier, dev, 1)
                    rec["ms_per_step" + key] = 1e3 * dt_ / n_
                    rec["fwd_bwd_ms" + key] = st_[0]
                    rec["optimizer_ms_sharded" + key] = st_[1]
                    del tr
                    torch.cuda.empty_cache()
                # the same rank's step with the gated forward of the overlapped gather (per-block casts and adaLN launches instead
                # of one grouped launch each; no communication in a rehearsal): what the gates themselves cost
                tr = DPTrainer(bsi, **recipe, cu_reserve=0, rehearse=(w_, 0), shard_update=True, overlap_gather=True)
                tr.train_step(xs, g)
                tr.train_step(xs, g)
                dt_, st_, _ = _timed_train(tr, xs, g, n_, barrier, dev, 1)
                rec["ms_per_step_gated_forward"] = 1e3 * dt_ / n_
                tr.sync_params()
                del tr
                torch.cuda.empty_cache()
                rec["optimizer_ms_replicated"] = runs[head]["optimizer_ms"]
                rec["model_tflops"] = b_ * 3 * FWD_GFLOP_PER_IMG / rec["ms_per_step"]
                per_rank.append(rec)
        except Exception as e:  # noqa: BLE001
            per_rank = {"error": f"{type(e).__name__}: {e}"}
    model.eval()
    steps_per_s = 1e3 / ms
    return {"comm": comm, "metric": "train steps/s (DiT-L/2, global batch %d, fwd+bwd+gradient exchange+clip+AdamW+EMA, dropout 0.05)" % a.train_batch,
            "value": steps_per_s, "unit": "steps/s", "ms_per_step": ms, "global_batch": a.train_batch, "headline_variant": head,
            "fastest_variant": fastest,
            "per_gpu_batch": nb, "images_per_s": steps_per_s * a.train_batch, "scaling": "strong",
            "model_tflops_per_gpu": steps_per_s * a.train_batch * 3 * FWD_GFLOP_PER_IMG / 1e3 / world,
            "fwd_bwd_exchange_ms": runs[head]["fwd_bwd_exchange_ms"], "optimizer_ms": runs[head]["optimizer_ms"],
            "variants": runs if world > 1 else None,
            "per_rank_workloads_on_one_gpu": per_rank, "loss": runs[head]["loss"]}


def secondary_bench(a, bsi, dev, budget_s):
    """Secondary workloads of SURVEY §8(d) on rank 0 at N = 1, so that they are in the driver-visible record: VDM-UNet
    (config 2) sampling and training, DiT-L/4 64x64 k = 256 sampling (config 5) and ELBO evaluation.  `frac` = model
    TFLOP/s / 2500 (dense bf16 peak).  Bounded by `budget_s`: an entry is skipped (and says so) once the budget is spent."""
    from bsi_amd import BSI, Discretization
    from bsi_amd.dp import DPTrainer
    from bsi_amd.models.dit import DenoisingDiT
    from bsi_amd.models.pos_emb import NyquistPositionalEmbedding
    from bsi_amd.models.vdm_unet import DenoisingVDMUNet
    from bsi_amd.nn import FourierFeatures

    t_start = time.perf_counter()
    out = {}

    def left():
        return budget_s - (time.perf_counter() - t_start)

    def mk(model, shape, k):
        return BSI(model, data_shape=shape, lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=k, preconditioning="edm",
                   discretization=Discretization.image_8bit()).to(dev)

    def timed(fn, warm, reps=1):
        warm()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps, r

    def entry(name, need_s, fn):
        if left() < need_s:
            out[name] = {"skipped": f"secondary budget ({budget_s:.0f} s) spent"}
            return
        try:
            out[name] = fn()
        except Exception as e:  # a secondary failure must not take the headline line with it
            out[name] = {"error": f"{type(e).__name__}: {e}"}

    g = torch.Generator(dev).manual_seed(7)
    t4 = lambda b_: torch.linspace(0, 1, 5, device=dev)  # noqa: E731  (4-step schedule for warm-up calls)

    def elbo():
        b = 512
        x = (torch.randint(0, 256, (b, 3, 32, 32), device=dev).float() / 255) * 2 - 1
        with torch.no_grad():
            dt, (_, bpd, _) = timed(lambda: bsi.elbo(x, 1, 1, g), lambda: bsi.elbo(x, 1, 1, g), reps=3)  # warm-up at the timed size: its buffers are allocated there
        assert torch.isfinite(bpd).all()
        tf = b / dt * 2 * FWD_GFLOP_PER_IMG / 1e3
        return {"workload": "DiT-L/2 32x32 BSI.elbo(n_recon=1, n_measure=1), 2 denoiser evaluations per image",
                "images_per_call": b, "value": b / dt, "unit": "images/s", "model_tflops": tf, "frac": tf / PEAK_BF16_TFLOPS}

    def unet():
        shape = (3, 32, 32)
        torch.manual_seed(0)
        m = DenoisingVDMUNet(shape, NyquistPositionalEmbedding(32, 100), "silu", 128, 32, 4, n_attention_heads=1,
                             dropout=0.1, fourier_features=FourierFeatures(n_min=6, n_max=8)).to(dev).eval()
        ub = mk(m, shape, 128)
        b = 512  # = eval_batch_size of the reference's configs; 3 % above 256 images per call (4 instead of 2 tiles per CU)
        with torch.no_grad():
            dt, s = timed(lambda: ub.sample(b, g), lambda: ub.sample(b, g, t=t4(b)))
        assert torch.isfinite(s).all()
        tf = b / dt * 129 * 53.47 / 1e3
        res = {"sample": {"workload": "CIFAR10 VDM-UNet (dim 128, 32 levels, 1 head) BSI.sample k=128", "images_per_call": b,
                          "value": b / dt, "unit": "images/s", "model_tflops": tf, "frac": tf / PEAK_BF16_TFLOPS}}
        m.train()
        tr = DPTrainer(ub, lr=2e-4, betas=(0.9, 0.99), weight_decay=1e-2, max_grad_norm=1.0)
        gb = 128
        x = (torch.randint(0, 256, (gb, *shape), device=dev).float() / 255) * 2 - 1
        dt, loss = timed(lambda: tr.train_step(x, g), lambda: tr.train_step(x, g), reps=10)
        assert torch.isfinite(loss)
        tf = gb / dt * 3 * 53.47 / 1e3
        res["train"] = {"workload": "CIFAR10 VDM-UNet train step (fwd+bwd+clip+AdamW+EMA, dropout 0.1), global batch 128",
                        "value": 1 / dt, "unit": "steps/s", "ms_per_step": 1e3 * dt, "model_tflops": tf,
                        "frac": tf / PEAK_BF16_TFLOPS, "loss": float(loss)}
        return res

    def dit64():
        shape = (3, 64, 64)
        torch.manual_seed(0)
        m = DenoisingDiT(shape, 4, 1024, 24, 16, dropout=0.05, fourier_features=FourierFeatures(n_min=6, n_max=8))
        with torch.no_grad():
            for blk in m.dit.blocks:
                blk.adaLN_modulation[-1].weight.normal_(0, 0.02)
        db = mk(m.to(dev).eval(), shape, 256)
        b = 128
        with torch.no_grad():
            dt, s = timed(lambda: db.sample(b, g), lambda: db.sample(b, g, t=t4(b)))
        assert torch.isfinite(s).all()
        tf = b / dt * 257 * 161.61 / 1e3
        return {"workload": "ImageNet64 DiT-L/4 (3x64x64) BSI.sample k=256", "images_per_call": b, "value": b / dt,
                "unit": "images/s", "model_tflops": tf, "frac": tf / PEAK_BF16_TFLOPS}

    def dit_batch(b, **kw):
        def run():
            with torch.no_grad():
                dt, s = timed(lambda: bsi.sample(b, g, **kw), lambda: bsi.sample(b, g, t=t4(b), **kw))
            assert torch.isfinite(s).all()
            tf = b / dt * (a.k + 1) * FWD_GFLOP_PER_IMG / 1e3
            return {"workload": f"DiT-L/2 32x32 BSI.sample k={a.k}" + (", Gaussian noise generated in the refine kernel (Philox4x32-10)"
                                                                       if kw.get("device_noise") else ""),
                    "images_per_call": b, "value": b / dt, "unit": "images/s", "model_tflops": tf, "frac": tf / PEAK_BF16_TFLOPS}
        return run

    entry("dit_l2_elbo", 10, elbo)
    entry("dit_l2_sample_256", 12, dit_batch(256))
    entry("dit_l2_sample_128", 8, dit_batch(128))
    entry("dit_l2_sample_64", 6, dit_batch(64))
    entry("dit_l2_sample_256_device_noise", 12, dit_batch(256, device_noise=True))
    entry("vdm_unet", 25, unet)
    entry("dit_l4_64x64_k256", 40, dit64)

    def torch_yardstick():
        """What plain PyTorch (eager, bf16 autocast, nn.Linear / F.scaled_dot_product_attention / F.layer_norm -- the way the
        reference runs its DiT) needs for one denoiser evaluation of the headline workload on THIS GPU, measured live: a yardstick
        for `value`, not a parity check (random weights, no wrapper ops).  tools/experiments/torch_yardstick.py has the train step
        and the torch.compile arm."""
        import torch.nn as nn
        import torch.nn.functional as F
        dim, depth, heads, T, kin, P = 1024, 24, 16, 256, 84, 12

        class Blk(nn.Module):
            def __init__(self):
                super().__init__()
                self.qkv, self.out = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)
                self.fc1, self.fc2 = nn.Linear(dim, 4 * dim), nn.Linear(4 * dim, dim)
                self.ada = nn.Sequential(nn.Linear(dim, dim), nn.SiLU(), nn.Linear(dim, 6 * dim))

            def forward(self, x, c):
                sa, ca, ga, sm, cm, gm = self.ada(c).unsqueeze(1).chunk(6, dim=-1)
                h = F.layer_norm(x, (dim,)) * (1 + ca) + sa
                q, k, v = self.qkv(h).reshape(x.shape[0], T, 3, heads, dim // heads).permute(2, 0, 3, 1, 4)
                a_ = F.scaled_dot_product_attention(q, k, v)
                x = torch.addcmul(x, ga, self.out(a_.transpose(1, 2).reshape(x.shape[0], T, dim)))
                h = F.layer_norm(x, (dim,)) * (1 + cm) + sm
                return torch.addcmul(x, gm, self.fc2(F.gelu(self.fc1(h), approximate="tanh")))

        class Net(nn.Module):
            def __init__(self):
                super().__init__()
                self.enc, self.dec = nn.Linear(kin, dim), nn.Linear(dim, P)
                self.blocks = nn.ModuleList(Blk() for _ in range(depth))
                self.tw = nn.Parameter(torch.randn(dim))

            def forward(self, tok, t_):
                c = torch.sin(t_[:, None] * self.tw)
                x = self.enc(tok)
                for blk in self.blocks:
                    x = blk(x, c)
                return self.dec(F.layer_norm(x, (dim,)))

        b = 512
        net = Net().to(dev).eval()
        tok, t_ = torch.randn((b, T, kin), device=dev), torch.rand(b, device=dev)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            dt, _ = timed(lambda: net(tok, t_), lambda: net(tok, t_), reps=5)
        return {"workload": "DiT-L/2 forward in plain PyTorch (eager, bf16 autocast, SDPA), 512 images, one evaluation", "ms_per_evaluation": 1e3 * dt,
                "images_per_s_at_129_evaluations": b / (129 * dt), "note": "yardstick on this GPU for the headline value; not the reference's code"}

    entry("torch_eager_yardstick", 20, torch_yardstick)
    out["seconds"] = time.perf_counter() - t_start
    return out


def secondary_in_child(a):
    """Run the secondary block in a FRESH child process (started with subprocess, never an exec of this GPU-initialised
    process) and return its JSON; a crash, GPU fault or hang of a secondary kernel leaves {"error": ...} in the line while the
    headline and train results, measured before, are still printed."""
    import subprocess

    cmd = [sys.executable, os.path.abspath(__file__), "--secondary-only", "--k", str(a.k), "--secondary-budget", str(a.secondary_budget)]
    limit = a.secondary_budget + 180.0  # model builds + first-call compilation of the child on top of its own budget
    try:
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        try:
            out, err = p.communicate(timeout=limit)
        except subprocess.TimeoutExpired:
            p.kill()
            p.communicate()
            return {"error": f"secondary block did not finish within {limit:.0f} s (child killed)"}
        if p.returncode != 0:
            return {"error": f"secondary child exited with status {p.returncode}", "stderr_tail": err.decode(errors="replace")[-400:]}
        return json.loads(out.decode().strip().splitlines()[-1])
    except Exception as e:  # noqa: BLE001
        return {"error": f"{type(e).__name__}: {e}"}


DUMP_LIMIT_BYTES = 64 * 2 ** 20


def dump_outputs(dirname, arrays, limit=DUMP_LIMIT_BYTES):
    """Write each tensor of `arrays` as dirname/<name>.npy (float64 stays float64, every other dtype becomes float32).  Beyond
    `limit` bytes in all, every array keeps the same share of its leading-dimension rows, a fixed seeded choice kept in order, so
    that two runs with the same arguments write the same rows.  Returns {name: {shape, dtype, rows, of_rows}} for the JSON line."""
    import numpy as np

    os.makedirs(dirname, exist_ok=True)
    host = {k: v.detach().cpu() for k, v in arrays.items()}
    host = {k: v if v.dtype == torch.float64 else v.float() for k, v in host.items()}
    total = sum(v.numel() * v.element_size() for v in host.values())
    share = min(1.0, limit / max(total, 1))
    info = {}
    for name, v in host.items():
        rows = v.shape[0] if v.dim() else 1
        if share < 1.0 and v.dim():
            keep = max(1, int(rows * share))
            idx = torch.randperm(rows, generator=torch.Generator().manual_seed(0))[:keep].sort().values
            v = v[idx]
        arr = v.contiguous().numpy()
        np.save(os.path.join(dirname, name + ".npy"), arr)
        info[name] = {"shape": list(arr.shape), "dtype": str(arr.dtype), "rows": int(arr.shape[0]) if arr.ndim else 1, "of_rows": rows}
    return info


def summary(line):
    """The numbers a reader of the line's TAIL must not miss (the driver keeps the last 2000 characters): sampling value, the train
    half of the metric, the per-rank rehearsal, the secondary values -- compact, last key of the line."""
    def get(d, *ks):
        for k in ks:
            d = d.get(k) if isinstance(d, dict) else None
        return d

    def r2(v):
        return round(v, 2) if isinstance(v, (int, float)) else v

    tr, sec = line.get("train") or {}, line.get("secondary") or {}
    pr = tr.get("per_rank_workloads_on_one_gpu")
    out = {"sample_images_per_s": r2(line.get("value")), "sample_frac_of_peak": r2(line.get("model_frac_of_peak")),
           "fc1_roofline_frac": round(get(line, "roofline", "frac") or 0, 3), "n_gpus": line.get("n_gpus"),
           # box yardstick (register-only random-operand bf16 MFMA stream, GPU otherwise idle) and the model's rate as a share of it
           "mfma_probe_tflops": r2(get(line, "box_probe", "tflops")), "mfma_probe_mhz": r2(get(line, "box_probe", "mhz")),
           "sample_tflops_per_probe_tflops": round((line.get("model_tflops_per_gpu") or 0) / get(line, "box_probe", "tflops"), 4)
           if get(line, "box_probe", "tflops") else None,
           "train_steps_per_s": r2(tr.get("value")), "train_ms_per_step": r2(tr.get("ms_per_step")),
           "train_frac_of_peak": r2((tr.get("model_tflops_per_gpu") or 0) / PEAK_BF16_TFLOPS) if tr.get("value") else None,
           "train_optimizer_ms": r2(tr.get("optimizer_ms")), "train_error": tr.get("error"),
           "train_variants_ms": {k: r2(v.get("ms_per_step")) for k, v in (tr.get("variants") or {}).items()} or None,
           "exposed_comm_ms": r2(get(tr, "comm", "exposed_comm_ms")),
           "bucket_busbw_GBps": r2(get(tr, "comm", "bucket_allreduce_alone", "busbw_GBps")),
           # per rank of a 2 / 4 / 8-GPU step on this one GPU: [world, fwd+bwd ms, fwd+bwd ms under the CU reserve, sharded optimizer ms]
           "per_rank_ms": [[r["world"], r2(r.get("fwd_bwd_ms")), r2(r.get("fwd_bwd_ms_cu_reserve")), r2(r.get("optimizer_ms_sharded"))]
                           for r in pr] if isinstance(pr, list) else pr,
           # whole step of that rank: plain sharded step / with the gated forward of the overlapped all-gather
           "per_rank_step_ms_plain_vs_gated": [[r["world"], r2(r.get("ms_per_step")), r2(r.get("ms_per_step_gated_forward"))]
                                               for r in pr] if isinstance(pr, list) else None,
           "sample_256_128_64": [r2(get(sec, k, "value")) for k in ("dit_l2_sample_256", "dit_l2_sample_128", "dit_l2_sample_64")],
           "elbo_images_per_s": r2(get(sec, "dit_l2_elbo", "value")),
           "unet_images_per_s": r2(get(sec, "vdm_unet", "sample", "value")), "unet_train_steps_per_s": r2(get(sec, "vdm_unet", "train", "value")),
           "dit64_images_per_s": r2(get(sec, "dit_l4_64x64_k256", "value")),
           "torch_eager_images_per_s": r2(get(sec, "torch_eager_yardstick", "images_per_s_at_129_evaluations")),
           "cpu_images_per_s": round(get(line, "cpu_baseline", "value") or 0, 4)}
    return out


def launch_ranks(a, command=None):
    """`python bench.py --gpus N` without torchrun: start the N rank processes (one per GPU) as children of this
    process, which itself makes NO GPU call (device_count() does not initialise the runtime on this image).  Rank 0's
    stdout (the JSON line) is relayed; the exit status is the worst child status."""
    import socket
    import subprocess

    n_dev = torch.cuda.device_count()
    if n_dev < a.gpus and not ONE_DEVICE:
        print(f"bench.py: --gpus {a.gpus} requested but only {n_dev} GPU(s) are visible; refusing to measure fewer ranks "
              "than asked for", file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(a.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.gpus), LOCAL_WORLD_SIZE=str(a.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # a user's setting wins
        if getattr(a, "cu_reserve", 0) > 0:
            env.setdefault("NCCL_MAX_NCHANNELS", str(a.cu_reserve))  # RCCL: at most as many workgroups as CUs are reserved for it
        procs.append(subprocess.Popen(command or ([sys.executable, os.path.abspath(__file__)] + sys.argv[1:]), env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    # rank 0's stdout is drained by a thread while all children are POLLED: when one exits non-zero (bad device, out of memory)
    # the others would sit in init_process_group / a collective until the RCCL timeout -- terminate them and return its status
    import threading
    chunks = []
    rd = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    rd.start()
    deadline = time.monotonic() + a.launch_timeout
    rc = None
    while rc is None:
        codes = [p.poll() for p in procs]
        bad = [c for c in codes if c not in (None, 0)]
        if bad:
            rc = max(abs(c) for c in bad)
        elif all(c == 0 for c in codes):
            rc = 0
        elif time.monotonic() > deadline:
            print(f"bench.py: ranks did not finish within {a.launch_timeout} s; terminating them", file=sys.stderr)
            rc = 5
        else:
            time.sleep(0.2)
    for p in procs:  # exact PIDs of the children this process started
        if p.poll() is None:
            p.terminate()
    for p in procs:
        try:
            p.wait(timeout=30)
        except subprocess.TimeoutExpired:
            p.kill()
    rd.join(timeout=10)
    sys.stdout.write(b"".join(chunks).decode())
    sys.stdout.flush()
    return rc


def main():
    a = parse()
    if a.secondary_only:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        from bsi_amd import BSI, Discretization
        model, shape = build_model(dev)
        bsi = BSI(model, data_shape=shape, lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=a.k, preconditioning="edm",
                  discretization=Discretization.image_8bit()).to(dev)
        print(json.dumps(secondary_bench(a, bsi, dev, a.secondary_budget)), flush=True)
        return
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(a))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(a.gpus, 1):
        print(f"bench.py: launched with WORLD_SIZE={world} but --gpus {a.gpus}", file=sys.stderr)
        sys.exit(2)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if a.cu_reserve > 0:
            os.environ.setdefault("NCCL_MAX_NCHANNELS", str(a.cu_reserve))  # before init_process_group (torchrun launches land here)
        if ONE_DEVICE:
            local = 0
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    from bsi_amd import _native as N
    from bsi_amd import BSI, Discretization

    model, shape = build_model(dev)
    bsi = BSI(model, data_shape=shape, lambda_0=1e-2, alpha_M=1e6, alpha_R=2e6, k=a.k, preconditioning="edm",
              discretization=Discretization.image_8bit()).to(dev)
    gen = torch.Generator(dev).manual_seed(1234 + rank)  # rank-distinct chains

    def barrier():
        if world > 1:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    def step():
        with torch.no_grad():
            return bsi.sample(a.batch, gen)

    # Box yardstick (GPU otherwise idle, before anything is timed): a register-only random-operand bf16 MFMA stream on every CU, twice
    # 50 ms -- the second run is the reported one (the first takes the clock from idle to its power-limited state).  Boxes of the pool
    # differ by a few per cent in what they sustain; `value` / probe is comparable across boxes and rounds, `value` alone is not.
    probe = None
    try:
        N.mfma_probe(50000, dev)
        probe = N.mfma_probe(50000, dev)
    except Exception as e:  # noqa: BLE001  (a yardstick must never cost the measurement)
        probe = {"error": f"{type(e).__name__}: {e}"}

    for _ in range(a.warmup):
        step()
    N.prof_enable(["gemm_fc1"])
    N.prof_read("gemm_fc1")
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = step()
    barrier()
    elapsed = time.perf_counter() - t0
    cnt, tot_ms = N.prof_read("gemm_fc1")
    N.prof_enable([])
    assert torch.isfinite(out).all()
    if world > 1:
        tmax = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(tmax.item())

    line = None
    if rank == 0:
        n_gpus = world
        imgs = a.batch * a.steps * n_gpus
        value = imgs / elapsed
        # dominant kernel: fc1 GEMM  [B*256, 1024] x [4096, 1024]^T  (+bias, GELU-tanh, bf16 store)
        flops_per_launch = 2.0 * (a.batch * 256) * 1024 * 4096
        avg_ms = tot_ms / max(cnt, 1)
        achieved = flops_per_launch / (avg_ms * 1e-3) / 1e12
        line = {
            "metric": f"images/sec BSI.sample k={a.k} (DiT, 3x32x32)",
            "value": value, "unit": "images/s", "n_gpus": n_gpus, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": 1e3 * elapsed / a.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": "ImageNet32 DiT-L/2 (dim 1024, depth 24, heads 16, patch 2, Fourier features 6..8), "
                                   f"BSI.sample k={a.k}, EDM preconditioning, {a.batch} images per GPU per call, "
                                   "random-init weights",
                       "images_per_gpu": a.batch, "k": a.k, "parallelism": f"independent chains x{n_gpus}",
                       **({"test_hook": "BSI_BENCH_ONE_DEVICE: all ranks on one GPU over gloo -- not a multi-GPU measurement"} if ONE_DEVICE else {})},
            "box_probe": probe,
            "model_tflops_per_gpu": value / n_gpus * (a.k + 1) * FWD_GFLOP_PER_IMG / 1e3,
            "model_frac_of_peak": value / n_gpus * (a.k + 1) * FWD_GFLOP_PER_IMG / 1e3 / PEAK_BF16_TFLOPS,
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / PEAK_BF16_TFLOPS, "traffic": pmc_traffic(a.batch)[0], "traffic_source": pmc_traffic(a.batch)[1],
                         "kernel": N.fc1_kernel_name(),
                         "launches": cnt, "avg_launch_ms": avg_ms, "flops_per_launch": flops_per_launch},
        }

    if a.dump_outputs and rank == 0:
        # what a caller of the timed path received from its last call (rank 0's chains; other ranks draw other noise)
        line["dump_outputs"] = {"dir": a.dump_outputs, "arrays": dump_outputs(a.dump_outputs, {"samples": out})}

    if a.breakdown and rank == 0:
        names = list(N.PROF_CLASSES)
        N.prof_enable(names)
        step()
        torch.cuda.synchronize()
        rows = [(n, *N.prof_read(n)) for n in names]
        N.prof_enable([])
        tot = sum(r[2] for r in rows)
        for n, c, ms in rows:
            print(f"  {n:12s} {c:6d} launches {ms:10.2f} ms  {100 * ms / max(tot, 1e-9):5.1f} %", file=sys.stderr)

    train = None
    if a.train_steps > 0:
        # The train measurement is the second half of the metric.  If it hangs (e.g. a collective deadlock) the watchdog
        # still emits the sampling line, marked with the error, and the process exits NON-ZERO (never a silent success).
        import threading

        def give_up():
            if line is not None:
                line["train"] = {"error": "train benchmark did not finish within %d s" % a.train_timeout}
                print(json.dumps(line), flush=True)
            os._exit(3)

        dog = threading.Timer(a.train_timeout, give_up)
        dog.daemon = True
        dog.start()
        try:
            train = train_bench(a, bsi, model, dev, world, rank, barrier)
        except Exception as e:
            train = {"error": f"{type(e).__name__}: {e}"}
            model.eval()
        dog.cancel()
        torch.cuda.empty_cache()

    rc = 0
    if rank == 0:
        if train is not None:
            line["train"] = train
            rc = 4 if "error" in train else 0
        if world == 1 and not a.no_secondary:
            line["secondary"] = secondary_in_child(a)
        if not a.no_cpu_baseline and world == 1:
            t_cpu = time.perf_counter()
            line["cpu_baseline"] = cpu_baseline(a.k)
            line["cpu_baseline"]["wall_seconds_gpu_idle"] = time.perf_counter() - t_cpu
        # what an outside clock sees around this process: the GPU idles while the model is built, while the CPU baseline runs
        # (wall_seconds_gpu_idle above) and while the secondary child starts; `value` is timed between barriers around the calls only
        line["wall_note"] = ("value / ms_per_step are timed around the sampling calls; model construction, the CPU baseline "
                             "(cpu_baseline.wall_seconds_gpu_idle) and process start-up of the secondary child run with the GPU idle")
        line["summary"] = summary(line)  # LAST key: a reader that keeps only the tail of the line still sees both halves of the metric
        print(json.dumps(line), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    sys.exit(rc)


if __name__ == "__main__":
    main()
