"""What the native denoisers (DenoisingDiT, DenoisingVDMUNet) share between the nn.Module that holds the fp32 parameters and the C
ABI: the caches of bf16 shadows, plans and workspace with their keys, deep copies, the forward dispatch, the slots through which a
trainer (bsi_amd.dp.DPTrainer) talks to the training engine, and the one `torch.autograd.Function` of the training path."""
import copy

import torch
from torch import Tensor, nn

_FN_ARGS = 8  # arguments of _NativeTrainFn.apply in front of the parameters


class NativeDenoiser(nn.Module):
    """Base of the denoisers that run on a HIP engine.  It registers no parameter, buffer or submodule.  A subclass supplies
    `_config`, `_build_plan(skey)`, `native_pack`, `adaln_table`, `forward_native`, `forward_train` and, for training,
    `_tape_bytes`, `_engine_train_forward` and `_engine_backward`.

    Native caches (class-level defaults, all None; rebuilt on demand): `_pack` / `_pack_t` (weight tables over the bf16 shadows and
    the transposed ones of the backward) with the `_weights_key` they were cast for in `_pack_key` / `_pack_t_key`; `_plan` /
    `_plan_t` (persistent shadow buffers + descriptor tables, valid for one `_storage_key`); `_plan_g` (the UNet's gradient
    tables over a trainer's buffer); `_ws` (engine workspace).
    Trainer-facing slots: `_grad_buffer` (flat fp32 buffer, padded or not, that the backward writes instead of a fresh one),
    `_flat_grad_only` (False; True: the backward hands autograd no per-parameter gradients), `_last_flat_grad` (the buffer the last
    backward wrote), `_params_pending_sync` (callable that makes the current stream wait for an all-gather of the parameters still in
    flight; `native_pack` calls it before casting), `_bwd_sched` ((CU reserve, tile queue) of the next backward's launches: honoured
    by the DiT engine only).  `_drop_calls` counts the training forwards that drew a dropout seed.

    Not unified here: the UNet asserts contiguous parameters, the DiT makes strided ones dense in place."""

    _pack = _pack_key = _pack_t = _pack_t_key = _plan = _plan_t = _plan_g = _ws = None
    _last_flat_grad = _grad_buffer = _params_pending_sync = _bwd_sched = None
    _flat_grad_only = False
    _drop_calls = 0
    _NATIVE_CACHES = ("_pack", "_pack_key", "_pack_t", "_pack_t_key", "_plan", "_plan_t", "_plan_g", "_ws", "_last_flat_grad",
                      "_grad_buffer", "_params_pending_sync", "_bwd_sched")

    def __deepcopy__(self, memo):
        """`copy.deepcopy(model)` (EMA copies, checkpoint tooling) after the model has run: the native caches hold ctypes tables with raw
        device pointers into THIS model's buffers, and the trainer slots a trainer's buffers and bound methods -- they are neither
        picklable nor valid for a copy.  The copy starts with every one of them None; the original keeps its own."""
        saved = {k: self.__dict__.pop(k) for k in self._NATIVE_CACHES if k in self.__dict__}
        try:
            new = self.__class__.__new__(self.__class__)
            memo[id(self)] = new
            new.__dict__ = copy.deepcopy(self.__dict__, memo)
        finally:
            self.__dict__.update(saved)
        return new

    def _name(self):
        return f"bsi_amd.{type(self).__name__}"

    def _weights_key(self):
        ps = list(self.parameters())
        return (ps[0].device, ps[0].data_ptr(), sum(p._version for p in ps))

    def _storage_key(self):
        """Identity of the parameters' STORAGE: a plan bakes every parameter's raw pointer into device-side descriptor tables and
        into the ctypes weight tables, so the key names every one of them (a re-pack costs far more) -- replacing the storage of any
        parameter (`p.data = ...`, `load_state_dict(assign=True)`, a per-module `.to()`) must rebuild the plan."""
        ps = list(self.parameters())
        return (ps[0].device, len(ps), hash(tuple(p.data_ptr() for p in ps)))

    def _current_plan(self, slot="_plan"):
        """The plan cached in `slot`, rebuilt by `_build<slot>(skey)` when the parameters' storage moved."""
        skey = self._storage_key()
        plan = getattr(self, slot)
        if plan is None or plan["skey"] != skey:
            plan = getattr(self, "_build" + slot)(skey)
            setattr(self, slot, plan)
        return plan

    def invalidate_native(self, plans=False):
        """Forget the cast shadows after a parameter update that moved no version counter (a raw kernel wrote the parameters): the
        next use casts them again.  plans=True also drops the persistent buffers and tables, the gradient buffer and the workspace."""
        self._pack = self._pack_t = None
        if plans:
            self._plan = self._plan_t = self._plan_g = self._grad_buffer = self._ws = None

    def _workspace(self, nbytes: int, dev):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != dev:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return self._ws

    def _prepare_input(self, mu: Tensor, out):
        """(contiguous mu, B, out) of one engine call."""
        if mu.dtype != torch.float32:
            raise RuntimeError(f"{self._name()}: input must be fp32 (bf16 is used inside the kernels)")
        mu = mu.contiguous()
        assert tuple(mu.shape[1:]) == self.data_shape, f"expected [B,{self.data_shape}], got {tuple(mu.shape)}"
        return mu, mu.shape[0], torch.empty_like(mu) if out is None else out

    def forward(self, mu: Tensor, t: Tensor) -> Tensor:
        """f(mu, t): mu [B, *data_shape] fp32, t [B] in [0, 1]  (dit.py:225-233, vdm_unet.py:92-100)."""
        if not mu.is_cuda:
            raise RuntimeError(f"{self._name()}: input is not on a HIP device; there is no CPU path")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return self.forward_train(mu, t)  # backward kernels live in the training engine
        return self.forward_native(mu, self.adaln_table(t))


def native_denoiser(model):
    """`model` if it runs on a native engine (BSI, VDM and BFN then call the engine with their coefficients), else None."""
    return model if hasattr(model, "forward_native") and hasattr(model, "adaln_table") else None


def dropout_seed(model) -> int:
    """Seed of the counter-based dropout masks of the next training forward: from `torch.initial_seed()` and the model's call
    counter (the reference draws its masks from the device's global generator, which cannot be reproduced bit for bit anyway)."""
    model._drop_calls += 1
    return (torch.initial_seed() * 0x9E3779B1 + model._drop_calls * 0x85EBCA77) & 0xFFFFFFFFFFFFFFFF


def flat_grad_views(model, flat=None):
    """(flat, views, order): one flat fp32 buffer for all gradients -- `flat` (a trainer's, possibly padded) or a fresh one -- and
    views of it shaped like the parameters, in `named_parameters` order."""
    named = dict(model.named_parameters())
    total = sum(p.numel() for p in named.values())
    if flat is None:
        flat = torch.empty(total, dtype=torch.float32, device=next(iter(named.values())).device)
    assert flat.numel() >= total and flat.dtype == torch.float32 and flat.is_contiguous()
    views, off = {}, 0
    for n, p in named.items():
        views[n] = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    return flat, views, list(named)


class _NativeTrainFn(torch.autograd.Function):
    """Tape-recording HIP forward + hand-written HIP backward; torch's autograd only carries the parameter gradients out."""

    @staticmethod
    def forward(ctx, model, drop_p, seed, mu, t, c_in, c_skip, c_out, *params):
        cfg, w, _, _ = model.native_pack()
        mu = mu.contiguous()
        t = t.detach().to(torch.float32).contiguous()
        B = mu.shape[0]
        out = torch.empty_like(mu)
        tape = torch.empty(model._tape_bytes(cfg, B), dtype=torch.uint8, device=mu.device)
        model._engine_train_forward(cfg, w, B, mu, t, c_in, c_skip, c_out, out, tape, drop_p, seed)
        ctx.model, ctx.tape, ctx.c_out, ctx.B = model, tape, c_out, B
        ctx.drop = (drop_p, seed)
        return out

    @staticmethod
    def backward(ctx, g_out):
        model = ctx.model
        # the model builds (or, for a trainer's persistent buffer, may cache) the views of `flat_grad_views` and its gradient tables,
        # and releases ctx.tape as soon as its backward is enqueued, before its own workspace goes (releasing the tape after the
        # workspace measured 0.8 ms, 0.3 %, slower per DiT-L/2 train step on an MI355X)
        flat, views, order = model._engine_backward(ctx, g_out.contiguous(), model._grad_buffer)
        model._last_flat_grad = flat  # the data-parallel trainer all-reduces and consumes this buffer directly
        if model._flat_grad_only:
            # the data-parallel trainer consumes `_last_flat_grad` itself: handing the views to autograd would make it copy every
            # one of them into a .grad tensor nobody reads (one copy kernel per parameter tensor)
            return (None,) * (_FN_ARGS + len(order))
        return (None,) * _FN_ARGS + tuple(views[n] for n in order)


def native_forward_train(model, drop_p: float, mu: Tensor, t: Tensor, c_in=None, c_skip=None, c_out=None) -> Tensor:
    """x_hat = c_skip*mu + c_out*f(c_in*mu, t) (or f(mu, t)) with gradients w.r.t. the model parameters; dropout with probability
    `drop_p` (0 outside `train()` mode) under a counter-based mask (`dropout_seed`)."""
    seed = dropout_seed(model) if drop_p > 0.0 else 0
    return _NativeTrainFn.apply(model, drop_p, seed, mu, t, c_in, c_skip, c_out, *[q for _, q in model.named_parameters()])
