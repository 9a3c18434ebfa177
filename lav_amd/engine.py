"""Engine: the cache of packed layers between an nn.Module and the C ABI - which packed weights a forward runs on, and when they
are re-packed or rebuilt after the parameters changed.  One definition for every inference module."""
from __future__ import annotations

from torch import nn


def _refreshable(obj):
    """Every layer object with a refresh() inside an engine (nested dicts / lists / tuples)."""
    if isinstance(obj, dict):
        for v in obj.values():
            yield from _refreshable(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _refreshable(v)
    elif hasattr(obj, "refresh"):
        yield obj


def _bn_tuple(bn):
    return (bn.running_mean, bn.running_var, bn.weight, bn.bias)


class Engine(nn.Module):
    """Mixin: cache of packed layers, `_eng` = {"device", "tensor_ids", one entry per key (_engine_for)}.  When the parameters may
    have changed IN PLACE (a train()/eval() toggle around optimiser steps, load_state_dict) the cached engine is marked stale and
    re-packed on the device from the live parameters at its next use (ConvLayer.refresh: one gather launch per layer - the trainer's
    per-step log inference used to rebuild ~45 layers on the host per step); when the tensors themselves may have been replaced
    (_apply: .to() / .float()) it is dropped.  A module whose engine is plain copies without a refresh() overrides _mark_stale
    to drop."""

    def _drop(self):
        object.__setattr__(self, "_eng", None)
        object.__setattr__(self, "_stale", False)

    def _mark_stale(self):
        if self.__dict__.get("_eng") is not None:
            object.__setattr__(self, "_stale", True)

    def _tensor_ids(self):
        return tuple(id(t) for t in self.parameters()) + tuple(id(t) for t in self.buffers())

    def _fresh(self, device):
        """The cached engine for `device`, brought up to date; None when there is none (or when a parameter OBJECT was replaced -
        load_state_dict(assign=True), module.weight = nn.Parameter(...) - since the engine was packed: the layers re-pack from
        the tensors they were built from, so such an engine is dropped and rebuilt from the module)."""
        eng = self.__dict__.get("_eng")
        if eng is None or eng.get("device") != device:
            return None
        if self.__dict__.get("_stale"):
            if eng["tensor_ids"] != self._tensor_ids():
                self._drop()
                return None
            for layer in _refreshable(eng):
                layer.refresh()
            object.__setattr__(self, "_stale", False)
        return eng

    def _engine_for(self, device, key, build):
        """The engine's entry `key` on `device`, up to date: the cached one, else build() - stored, with the identities of the
        tensors it was packed from recorded here, where it is built (not at its first use)."""
        eng = self._fresh(device) or dict(device=device)
        if key not in eng:
            eng[key] = build()
            eng["tensor_ids"] = self._tensor_ids()
            object.__setattr__(self, "_eng", eng)
        return eng[key]

    def _apply(self, fn, *a, **k):
        self._drop()
        return super()._apply(fn, *a, **k)

    def train(self, mode: bool = True):
        if mode != self.training:     # packed engines only go stale when the mode really changes (or weights do: _apply / load)
            self._mark_stale()
        return super().train(mode)

    def _load_from_state_dict(self, *a, **k):
        self._mark_stale()
        return super()._load_from_state_dict(*a, **k)

    def _need_eval(self):
        if self.training:
            raise NotImplementedError(f"{type(self).__name__}: the fused HIP path is eval-only; train mode runs forward_train")
