"""The plumbing both native denoisers inherit from bsi_amd/models/native.py, on CPU-built models (no library, no device): the
declared cache and trainer slots, deep copies that leave them behind, the flat gradient views, the dropout seed, invalidation.
(State-dict keys and strict loading of the golden weights: tests/test_native_abi.py.)"""
import copy
import threading

import pytest
import torch


def models():
    from bsi_amd.models.dit import DenoisingDiT
    from bsi_amd.models.pos_emb import NyquistPositionalEmbedding
    from bsi_amd.models.vdm_unet import DenoisingVDMUNet
    from bsi_amd.nn import FourierFeatures
    ff = FourierFeatures(n_min=6, n_max=8)
    return [DenoisingDiT((3, 16, 16), 2, 128, 2, 2, dropout=0.1, fourier_features=ff),
            DenoisingVDMUNet((3, 8, 8), NyquistPositionalEmbedding(32, 100), "silu", 64, 1, 4, n_attention_heads=1, fourier_features=ff)]


class _Trainer:
    """Stands in for a trainer whose bound method sits in `_params_pending_sync`: it cannot be deep-copied."""

    def __init__(self):
        self.lock = threading.Lock()

    def sync_params(self):
        pass


def test_one_set_of_declared_slots():
    from bsi_amd.models.native import NativeDenoiser
    dit, unet = models()
    assert type(dit)._NATIVE_CACHES is type(unet)._NATIVE_CACHES is NativeDenoiser._NATIVE_CACHES
    assert set(NativeDenoiser._NATIVE_CACHES) == {"_pack", "_pack_key", "_pack_t", "_pack_t_key", "_plan", "_plan_t", "_plan_g", "_ws",
                                                  "_last_flat_grad", "_grad_buffer", "_params_pending_sync", "_bwd_sched"}
    for m in (dit, unet):
        assert isinstance(m, NativeDenoiser)
        assert all(getattr(m, k) is None for k in m._NATIVE_CACHES)
        assert m._flat_grad_only is False and m._drop_calls == 0
        assert not any(k.startswith("_") for k in m.state_dict())
    # the base class registers nothing: the module tree and the state dict are the subclass's own
    base = NativeDenoiser()
    assert not list(base.children()) and not list(base.parameters()) and not list(base.buffers()) and not base.state_dict()


@pytest.mark.parametrize("i", [0, 1], ids=["dit", "unet"])
def test_deepcopy_leaves_every_slot_behind(i):
    m = models()[i]
    trainer = _Trainer()
    with pytest.raises(TypeError):
        copy.deepcopy(trainer.sync_params)
    planted = {k: threading.Lock() for k in m._NATIVE_CACHES}
    planted["_params_pending_sync"] = trainer.sync_params
    for k, v in planted.items():
        setattr(m, k, v)
    m._drop_calls = 3
    twin = copy.deepcopy(m)
    assert type(twin) is type(m) and twin is not m
    assert all(getattr(twin, k) is None for k in m._NATIVE_CACHES)
    assert all(m.__dict__[k] is v for k, v in planted.items())
    assert m._params_pending_sync.__self__ is trainer
    assert twin._drop_calls == 3 and twin.data_shape == m.data_shape
    sd, sd2 = m.state_dict(), twin.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) and sd[k].data_ptr() != sd2[k].data_ptr() for k in sd)


@pytest.mark.parametrize("i", [0, 1], ids=["dit", "unet"])
def test_flat_grad_views(i):
    from bsi_amd.models.native import flat_grad_views
    m = models()[i]
    named = list(m.named_parameters())
    total = sum(p.numel() for _, p in named)
    flat, views, order = flat_grad_views(m)
    assert flat.shape == (total,) and flat.dtype == torch.float32 and order == [n for n, _ in named] == list(views)
    buf = torch.zeros(total + 1000)  # a trainer's padded buffer
    flat, views, order = flat_grad_views(m, buf)
    assert flat is buf
    off = 0
    for n, p in named:
        v = views[n]
        assert v.shape == p.shape and v.is_contiguous() and v.data_ptr() == buf.data_ptr() + 4 * off, n
        off += p.numel()
    assert off == total
    for k, n in enumerate(order):
        views[n].fill_(k + 1)
    want = torch.cat([torch.full((p.numel(),), float(k + 1)) for k, (_, p) in enumerate(named)])
    assert torch.equal(buf[:total], want) and not buf[total:].any()
    for bad in (torch.zeros(total - 1), torch.zeros(total, dtype=torch.float64), torch.zeros(2 * total)[::2]):
        with pytest.raises(AssertionError):
            flat_grad_views(m, bad)


def test_native_denoiser_tells_the_models_from_plain_modules():
    from bsi_amd.models.native import native_denoiser
    for m in models():
        assert native_denoiser(m) is m
    assert native_denoiser(torch.nn.Linear(2, 2)) is None


def test_dropout_seed_formula_and_counter():
    from bsi_amd.models.native import dropout_seed
    torch.manual_seed(1234)
    for model in models():
        for call in (1, 2, 3):
            got = dropout_seed(model)
            assert model._drop_calls == call
            seed = (torch.initial_seed() * 0x9E3779B1 + model._drop_calls * 0x85EBCA77) & 0xFFFFFFFFFFFFFFFF
            assert got == seed and 0 <= got < 2 ** 64
    assert torch.initial_seed() == 1234


def test_invalidate_native():
    for m in models():
        marks = {k: object() for k in m._NATIVE_CACHES}
        for k, v in marks.items():
            setattr(m, k, v)
        m._drop_calls = 5
        m.invalidate_native()
        assert m._pack is None and m._pack_t is None
        assert all(getattr(m, k) is marks[k] for k in m._NATIVE_CACHES if k not in ("_pack", "_pack_t"))
        m.invalidate_native(plans=True)
        cleared = ("_pack", "_pack_t", "_plan", "_plan_t", "_plan_g", "_grad_buffer", "_ws")
        assert all(getattr(m, k) is None for k in cleared)
        assert all(getattr(m, k) is marks[k] for k in m._NATIVE_CACHES if k not in cleared)
        assert m._drop_calls == 5
