"""Training path of the native DenoisingDiT behind the shared `torch.autograd.Function` (models/native.py): its forward records a
tape in device memory (`bsi_dit_train_forward`), its backward is the hand-written HIP backward (`bsi_dit_backward`) below.
torch's autograd only carries the parameter gradients out; no torch op computes anything.

Geometries: heads of 64 or 128 channels, a multiple of 64 tokens up to 1024, dim <= 1024.  Heads of 64 channels at up to 256 tokens
use the resident / persistent attention backward, everything else the streamed one (with the same counter-based dropout mask);
both engine entry points refuse anything else with a message naming tokens, dim and head dim.

Replaces autograd over bsi/models/dit.py:87-103,174-181 of the reference inside
`BSI.train_loss(...).mean().backward()` (bsi/tasks/bsi.py:187-194)."""
import ctypes as C

import torch
from torch import Tensor

from .. import _native as N
from .native import flat_grad_views

_BLOCK_PARAMS = (("attn.to_qkv.weight", "qkv_w"), ("attn.to_qkv.bias", "qkv_b"), ("attn.to_out.weight", "out_w"),
                 ("attn.to_out.bias", "out_b"), ("mlp.0.weight", "fc1_w"), ("mlp.0.bias", "fc1_b"),
                 ("mlp.2.weight", "fc2_w"), ("mlp.2.bias", "fc2_b"), ("adaLN_modulation.0.weight", "ada0_w"),
                 ("adaLN_modulation.0.bias", "ada0_b"), ("adaLN_modulation.2.weight", "ada2_w"),
                 ("adaLN_modulation.2.bias", "ada2_b"))


def transposed_pack(model):
    """bf16 W^T shadows ([in][out]) of the block weights for the input-gradient GEMMs: persistent buffers that join the model's
    cast plan (`DenoisingDiT.native_pack`) on first use, after which ONE launch per parameter version refreshes both layouts."""
    key = model._weights_key()
    if model._pack_t is not None and model._pack_t_key == key:
        return model._pack_t
    cfg, _, _, _ = model.native_pack()  # builds / refreshes the plan; if it already carries the transposes, they are current now
    if model._pack_t is not None and model._pack_t_key == key:
        return model._pack_t
    plan = model._plan
    dev = model.dit.patch_encoder.weight.device
    keep = []
    by_src = {d[0].data_ptr(): d for d in plan["descs"]}

    def shadow_t(w: Tensor):
        d = by_src[w.detach().data_ptr()]
        rows, cols = w.shape
        out = torch.empty((cols, rows), dtype=torch.bfloat16, device=dev)
        keep.append(out)
        d[2], d[6] = out, rows
        return out.data_ptr()

    blocks = (N.DitBlockWeightsT * cfg.depth)()
    for i, blk in enumerate(model.dit.blocks):
        b = blocks[i]
        b.qkv_wT = shadow_t(blk.attn.to_qkv.weight)
        b.out_wT = shadow_t(blk.attn.to_out.weight)
        b.fc1_wT = shadow_t(blk.mlp[0].weight)
        b.fc2_wT = shadow_t(blk.mlp[2].weight)
        b.ada2_wT = shadow_t(blk.adaLN_modulation[2].weight)
    wt = N.DitWeightsT()
    wt.blocks = C.cast(blocks, C.POINTER(N.DitBlockWeightsT))
    plan["pack_t"] = (wt, blocks, keep)
    model._finish_table(plan)
    table, n, tiles = plan["table"]
    with torch.no_grad():
        N.check(N.lib().bsi_cast_batch_bf16(N.ptr(table), n, tiles, N.stream()))  # first time: fills the transposes (and re-casts the rest)
    model._pack_t, model._pack_t_key = plan["pack_t"], key
    return model._pack_t


def engine_backward(model, ctx, g_out: Tensor, flat):
    """`bsi_dit_backward` into `flat` (a trainer's gradient buffer, or None for a fresh one): (flat, views, order) of
    `flat_grad_views`, built per call."""
    lib = N.lib()
    B = ctx.B
    cfg, w, _, _ = model.native_pack()
    wt, _, _ = transposed_pack(model)
    dev = g_out.device
    kpad = lib.bsi_dit_kpad(C.byref(cfg))
    flat, views, order = flat_grad_views(model, flat)
    enc_pad = torch.empty((cfg.dim, kpad), dtype=torch.float32, device=dev)
    blocks = (N.DitBlockGrads * cfg.depth)()
    for i in range(cfg.depth):
        for pname, field in _BLOCK_PARAMS:
            setattr(blocks[i], field, views[f"dit.blocks.{i}.{pname}"].data_ptr())
    g = N.DitGrads()
    g.enc_w_padded = enc_pad.data_ptr()
    g.enc_b = views["dit.patch_encoder.bias"].data_ptr()
    g.dec_ln_w = views["dit.patch_decoder.0.weight"].data_ptr()
    g.dec_ln_b = views["dit.patch_decoder.0.bias"].data_ptr()
    g.dec_w = views["dit.patch_decoder.1.weight"].data_ptr()
    g.dec_b = views["dit.patch_decoder.1.bias"].data_ptr()
    g.blocks = C.cast(blocks, C.POINTER(N.DitBlockGrads))
    ws = torch.empty(lib.bsi_dit_backward_workspace_bytes(C.byref(cfg), B), dtype=torch.uint8, device=dev)
    # launch schedule of THIS backward (DPTrainer: CU reserve / tile queue while gradient buckets are in flight).  The switches are
    # per launching thread, and this function runs on autograd's device thread, not on the caller's: they are applied here, around
    # the one call whose launches they are meant for, and nothing else in the process sees them.
    reserve, queue = model._bwd_sched or (0, False)
    try:
        if reserve:
            N.check(lib.bsi_set_cu_reserve(int(reserve)))
        if queue:
            N.check(lib.bsi_set_tile_queue(1))
        N.check(lib.bsi_dit_backward(C.byref(cfg), C.byref(w), C.byref(wt), C.byref(g), B, N.ptr(g_out), N.ptr(ctx.c_out),
                                     N.ptr(ctx.tape), N.ptr(ws), ctx.drop[0], ctx.drop[1], N.stream()))
    finally:
        if reserve:
            N.check(lib.bsi_set_cu_reserve(0))
        if queue:
            N.check(lib.bsi_set_tile_queue(0))
    ctx.tape = None
    enc_w = views["dit.patch_encoder.weight"]
    enc_w.copy_(enc_pad[:, :enc_w.shape[1]])
    return flat, views, order
