"""What every weight-holding sub-module is built from: ``_register`` (HF-named parameters), ``_WeightHolder`` (marks its owner's weights
dirty) and ``_Ref`` (the back reference to that owner).  Imports neither the encoder nor the decoder."""
from __future__ import annotations

import torch
from torch import nn


def _register(root: nn.Module, dotted: str, shape, init: float = 0.0):
    """Create nested containers so that root.state_dict() yields the HF key `dotted`."""
    parts = dotted.split(".")
    mod = root
    for name in parts[:-1]:
        if not hasattr(mod, name):
            mod.add_module(name, nn.Module())
        mod = getattr(mod, name)
    p = nn.Parameter(torch.full(tuple(shape), float(init)), requires_grad=False)
    mod.register_parameter(parts[-1], p)


class _WeightHolder(nn.Module):
    """A sub-module (prenet / wrapped_encoder) that only owns HF-named parameters."""

    def __init__(self, owner_ref):
        super().__init__()
        self._owner_ref = owner_ref

    def _mark_dirty(self):
        owner = self._owner_ref()
        if owner is not None:
            owner._weights_dirty = True

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        sd = self._translate(dict(state_dict))
        res = super().load_state_dict(sd, strict=strict, assign=assign)
        self._mark_dirty()
        return res

    def _translate(self, sd):
        return sd

    def _apply(self, fn, recurse=True):
        self._mark_dirty()
        return super()._apply(fn, recurse)


class _Ref:
    """weak-ish back reference that nn.Module does not register as a child."""

    def __init__(self):
        self.obj = None

    def __call__(self):
        return self.obj
