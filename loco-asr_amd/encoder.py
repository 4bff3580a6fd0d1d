"""Host-side mirror of the HuggingFace module contract the reference scripts use.

    model.speecht5.encoder.wrapped_encoder.load_state_dict(encoder_state_dict)     (…base…py:99)
    model.speecht5.encoder.prenet.load_state_dict(speech_prenet_state_dict)        (…base…py:100)
    model.eval(); with torch.no_grad(): out = model.speecht5.encoder(**audios)     (…base…py:102-108)
    embeddings = out.last_hidden_state.cpu().detach().numpy()                      (…base…py:109)

(`…base…py` = /root/reference/speech_text/extract_speecht5_base_embeddings_slurp.py; the fine-tuned
script makes the same call at :104-106.)  `SpeechT5EncoderWithSpeechPrenetMI355X` keeps exactly that
surface -- the same sub-module names, the same state-dict keys (HF 5.x spelling and the 4.30.2
``weight_g/weight_v`` spelling the reference's pickles use), keyword ``forward(input_values,
attention_mask=None, output_attentions=None, output_hidden_states=None, return_dict=None)`` returning an
object with ``.last_hidden_state`` (HF modeling_speecht5.py:1339-1358) -- but every FLOP runs in the
hand-written gfx950 kernels behind the C ABI of ``include/loco_asr.h``.  PyTorch is used for what it
is good at here: owning device memory, streams and (in ``dp.py``) the RCCL process group.

There is no fallback: on a machine without the built HIP library or without a ROCm device the
constructor/forward raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
import time
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
from torch import nn

from . import _lib
from .synth import (CONV_DIM, CONV_KERNEL, FFN, HEAD_DIM, HEADS, HIDDEN, LAYERS, POS_CONV_GROUPS, POS_CONV_K, REL_MAX)

PAD_TOKEN_ID = 1
MAX_SPEECH_POSITIONS = 4000


@dataclass
class Pack:
    """Several reference batches laid out as one [B, L] problem (``pack_batches``; include/loco_asr.h, loco_forward_packed)."""
    wav: torch.Tensor                       # f32 [B, L] device
    mask: Optional[torch.Tensor]            # i32 [B, L] device, or None when valid_len is given / every sample is present
    valid_len: Optional[list]               # per clip: present samples (the row sums of the batches' masks), or None
    pad_len: list                           # per clip: padded length of its own batch
    spans: list                             # per batch: (first clip, clips, output frames)


@dataclass
class BaseModelOutput:
    """Field-compatible stand-in for transformers.modeling_outputs.BaseModelOutput."""
    last_hidden_state: torch.Tensor = None
    hidden_states: Optional[Tuple[torch.Tensor, ...]] = None
    attentions: Optional[Tuple[torch.Tensor, ...]] = None

    def to_tuple(self):
        return tuple(v for v in (self.last_hidden_state, self.hidden_states, self.attentions) if v is not None)

    def __getitem__(self, i):
        return self.to_tuple()[i] if isinstance(i, int) else getattr(self, i)

    def __iter__(self):
        return iter(self.to_tuple())


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


def sinusoid_table(rows: int, dim: int = HIDDEN) -> torch.Tensor:
    """HF SpeechT5SinusoidalPositionalEmbedding.get_embedding (modeling_speecht5.py:305-321), same torch
    expression so that the table is bit-identical to the one HF builds at module init (weights, not hot path)."""
    half = dim // 2
    w = torch.exp(torch.arange(half, dtype=torch.int64).float() * -(math.log(10000) / (half - 1)))
    ang = torch.arange(rows, dtype=torch.int64).float().unsqueeze(1) * w.unsqueeze(0)
    tab = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1).view(rows, -1)
    tab[PAD_TOKEN_ID, :] = 0
    return tab


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


class SpeechT5SpeechEncoderPrenetMI355X(_WeightHolder):
    """Parameter names of HF SpeechT5SpeechEncoderPrenet (modeling_speecht5.py:513-532)."""

    def __init__(self, owner_ref):
        super().__init__(owner_ref)
        _register(self, "masked_spec_embed", (HIDDEN,))
        for i, k in enumerate(CONV_KERNEL):
            _register(self, f"feature_encoder.conv_layers.{i}.conv.weight", (CONV_DIM, 1 if i == 0 else CONV_DIM, k))
        _register(self, "feature_encoder.conv_layers.0.layer_norm.weight", (CONV_DIM,), 1.0)
        _register(self, "feature_encoder.conv_layers.0.layer_norm.bias", (CONV_DIM,))
        _register(self, "feature_projection.layer_norm.weight", (CONV_DIM,), 1.0)
        _register(self, "feature_projection.layer_norm.bias", (CONV_DIM,))
        _register(self, "feature_projection.projection.weight", (HIDDEN, CONV_DIM))
        _register(self, "feature_projection.projection.bias", (HIDDEN,))
        _register(self, "pos_conv_embed.conv.bias", (HIDDEN,))
        _register(self, "pos_conv_embed.conv.parametrizations.weight.original0", (1, 1, POS_CONV_K), 1.0)
        _register(self, "pos_conv_embed.conv.parametrizations.weight.original1", (HIDDEN, HIDDEN // POS_CONV_GROUPS, POS_CONV_K))

    def _translate(self, sd):
        # transformers 4.30.2 (the reference's pin) spells the weight-norm pair weight_g / weight_v, and the
        # reference's pickled prenet dict also carries the sinusoid buffer (map_speecht5_hf.py:164-166).
        for old, new in (("pos_conv_embed.conv.weight_g", "pos_conv_embed.conv.parametrizations.weight.original0"),
                         ("pos_conv_embed.conv.weight_v", "pos_conv_embed.conv.parametrizations.weight.original1")):
            if old in sd:
                sd[new] = sd.pop(old)
        sd.pop("pos_sinusoidal_embed.weights", None)
        return sd


class SpeechT5EncoderMI355X(_WeightHolder):
    """Parameter names of HF SpeechT5Encoder (modeling_speecht5.py:1212-1232)."""

    def __init__(self, owner_ref, layers: int):
        super().__init__(owner_ref)
        _register(self, "layer_norm.weight", (HIDDEN,), 1.0)
        _register(self, "layer_norm.bias", (HIDDEN,))
        _register(self, "embed_positions.pe_k.weight", (2 * REL_MAX, HEAD_DIM))
        for l in range(layers):
            b = f"layers.{l}."
            for proj in ("q_proj", "k_proj", "v_proj", "out_proj"):
                _register(self, f"{b}attention.{proj}.weight", (HIDDEN, HIDDEN))
                _register(self, f"{b}attention.{proj}.bias", (HIDDEN,))
            for ln in ("layer_norm", "final_layer_norm"):
                _register(self, f"{b}{ln}.weight", (HIDDEN,), 1.0)
                _register(self, f"{b}{ln}.bias", (HIDDEN,))
            _register(self, f"{b}feed_forward.intermediate_dense.weight", (FFN, HIDDEN))
            _register(self, f"{b}feed_forward.intermediate_dense.bias", (FFN,))
            _register(self, f"{b}feed_forward.output_dense.weight", (HIDDEN, FFN))
            _register(self, f"{b}feed_forward.output_dense.bias", (HIDDEN,))


class _Slot:
    """Everything ONE forward in flight owns: a stream, a workspace, a pinned status block (include/loco_asr.h,
    loco_forward_async) and the ticket of the forward currently using them."""

    def __init__(self, device, status_bytes):
        self.stream = torch.cuda.Stream(device)
        self.workspace = None
        self.status = torch.zeros(status_bytes, dtype=torch.uint8).pin_memory()
        self.ticket = None


class ForwardTicket:
    """A forward that has been enqueued and not yet checked.  ``result()`` waits for it (an event, not a device-wide
    synchronisation), reads its numeric-range status and -- under range_policy "fp32" -- runs the batch once more on the
    exact-fp32 kernels when the fp16 planes' range was left; then returns what ``forward`` would have returned (for a packed
    forward: the list of per-batch outputs ``forward_packed`` returns).

    A failure (range_policy "raise" on a batch outside the fp16 planes' range, a HIP error in the re-run) belongs to THIS ticket:
    it is stored, the ticket is marked resolved and its slot released either way, and only ``result()`` of this ticket raises it
    -- the slot's next forward, ``drain()`` and ``set_inflight()`` settle the ticket without re-raising somebody else's error."""

    def __init__(self, enc, slot, x, m, out, frames, precision, pack=None):
        self._enc, self._slot = enc, slot
        self._x, self._m = x, m  # kept alive until the forward has consumed them
        self._out, self._frames = out, frames
        self._precision = precision
        self._pack = pack  # packed forward: per-clip lengths and per-batch spans
        self._spans = pack.spans if pack is not None else None
        self._hidden = None  # packed forward with output_hidden_states: layers + 1 tensors [B, T, 768]
        self._done = torch.cuda.Event()
        self._resolved = False
        self._error = None
        self._lock = threading.Lock()  # result() may be called from the thread that enqueues (slot reuse) and from a consumer thread
        self.used_fp32 = False

    def done(self) -> bool:
        return self._done.query()

    def result(self):
        with self._lock:
            self._settle_locked()
            if self._error is not None:
                raise self._error
            return self._value()

    def settle(self):
        """Wait for the forward and release its slot; a failure stays with the ticket (``result()`` raises it)."""
        with self._lock:
            self._settle_locked()

    def packed_output(self):
        """After ``result()`` of a packed forward: (out [B, T, 768] of the whole pack, spans [(first clip, clips, frames) per batch])
        -- for consumers that move the pack as ONE tensor (the sink's single D2H copy) instead of batch by batch."""
        return self._out, self._spans

    def _value(self):
        if self._spans is None:
            return BaseModelOutput(last_hidden_state=self._out, hidden_states=None, attentions=None)
        hs = self._hidden
        return [BaseModelOutput(last_hidden_state=self._out[b0:b0 + nb, :t],
                                hidden_states=tuple(h[b0:b0 + nb, :t] for h in hs) if hs is not None else None, attentions=None)
                for (b0, nb, t) in self._spans]

    def _settle_locked(self):
        if self._resolved:
            return
        enc, slot = self._enc, self._slot
        try:
            self._done.synchronize()
            if enc.range_policy != "off" and self._precision != "f32":
                rc = enc._lib.loco_status_check(C.c_void_p(slot.status.data_ptr()), None, 0)
                if rc == -5 and enc.range_policy == "fp32":
                    with torch.cuda.device(self._out.device), torch.cuda.stream(slot.stream):
                        extra = () if self._pack is None else (self._pack, self._hidden)
                        enc._enqueue(slot, self._x, self._m, self._out, self._frames, "f32", *extra)
                        slot.stream.synchronize()
                    self.used_fp32 = True
                elif rc < 0:
                    _lib.check(rc, "loco_forward_async")
            enc.last_range_fallback = self.used_fp32
            enc.last_frames = self._frames
        except BaseException as e:  # noqa: BLE001 -- stored; raised to the callers of this ticket's result() only
            self._error = e
        finally:
            self._resolved = True
            self._x = self._m = None
            if slot.ticket is self:
                slot.ticket = None


class _Ref:
    """weak-ish back reference that nn.Module does not register as a child."""

    def __init__(self):
        self.obj = None

    def __call__(self):
        return self.obj


class SpeechT5EncoderWithSpeechPrenetMI355X(nn.Module):
    """Drop-in for ``SpeechT5ForSpeechToText(...).speecht5.encoder`` (HF modeling_speecht5.py:1325-1358)."""

    # "f16x3" (default): GEMMs and attention products as three fp16 MFMAs per fp32-class product (hi/lo operand split,
    # fp32 accumulate) -- ~1e-6 relative L2 of an fp64 evaluation end to end, 2.4x the speed of "f32";
    # "f32": every contraction on the exact fp32 MFMA (~1e-6).  Both are far inside the 1e-3 bar.
    # "f16x2" (opt-in, never the default): the weights of every projection / conv GEMM rounded to fp16 (after their
    # per-tensor power-of-two scale), activations still hi + lo, attention products still three-term -- ~9e-4 on the goldens: AT the
    # 1e-3 bar, not inside it with margin (no guarantee on other weights), and no longer fp32 class; a third fewer matrix
    # instructions in the GEMMs.
    PRECISIONS = {"f32": 0, "f16x3": 1, "f16x2": 2}

    def __init__(self, layers: int = LAYERS, precision: str = "f16x3"):
        super().__init__()
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(self.PRECISIONS)}")
        self.precision = precision
        self._lib = _lib.load()  # raises when the HIP library is missing: no fallback
        ref = _Ref()
        self.prenet = SpeechT5SpeechEncoderPrenetMI355X(ref)
        self.wrapped_encoder = SpeechT5EncoderMI355X(ref, layers)
        ref.obj = self
        self.num_layers = layers
        self._handle = None
        self._handle_device = None
        self._weights_dirty = True
        self._workspace = None
        self._sin_rows = 0
        self._taps = None
        # further (key prefix, module) pairs whose tensors go to the same handle: the model's decoder halves (decoder.py); empty for an
        # encoder-only model, which then loads exactly what it always has
        self._extra_weights = []
        self._decoder_layers = 0
        self._decoder_vocab = 0
        # large batches run as two half-batches on two HIP streams (bit-identical, ~2 % faster: include/loco_asr.h,
        # loco_set_streams); set to 1 to keep everything on the caller's stream
        self.streams = 2
        # Numeric range of precision "f16x3" (include/loco_asr.h): "fp32" = a batch whose activations leave the range the fp16
        # planes represent is run again on the library's exact-fp32 MFMA kernels (the default: a caller never sees NaNs or a
        # silently degraded embedding); "raise" = LocoError instead; "off" = no check and no host synchronisation (the
        # forward stays fully asynchronous; loco_forward_status can still be queried through range_report()).
        self.range_policy = "fp32"
        self.last_range_fallback = False
        # forwards in flight (forward_async): slots of (stream, workspace, status block), used round-robin
        self._slots = []
        self._next_slot = 0
        self._workspace_floor = 0
        self.submit_profile = {} if os.environ.get("LOCO_EXTRACT_PROFILE") == "1" else None
        self.eval()

    # -- lifetime ----------------------------------------------------------------------------------------
    def __del__(self):
        try:
            if getattr(self, "_handle", None):
                self._lib.loco_destroy(self._handle)
                self._handle = None
        except Exception:
            pass

    def _device(self) -> torch.device:
        return next(self.prenet.parameters()).device

    def _ensure_handle(self, device: torch.device):
        if device.type != "cuda":
            raise RuntimeError(
                f"{type(self).__name__} runs only on an AMD GPU through its HIP kernels "
                f"(got device {device}); move the module and its inputs with .to('cuda'). There is no CPU path.")
        if self._handle is not None and self._handle_device != device:
            self._lib.loco_destroy(self._handle)
            self._handle = None
        if self._handle is None:
            cfg = _lib.LocoConfig()
            self._lib.loco_default_config(C.byref(cfg))
            cfg.layers = self.num_layers
            with torch.cuda.device(device):
                h = self._lib.loco_create(C.byref(cfg))
            if not h:
                raise _lib.LocoError("loco_create: " + self._lib.loco_last_error().decode())
            self._handle = C.c_void_p(h)
            self._handle_device = device
            self._weights_dirty = True
            self._sin_rows = 0

    def _sync_weights(self, device: torch.device, min_sin_rows: int):
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        if self._weights_dirty:
            self.drain()  # forwards still in flight on the slots' streams read the planes that are about to be rebuilt
            for prefix, mod in [("prenet.", self.prenet), ("wrapped_encoder.", self.wrapped_encoder)] + list(self._extra_weights):
                for name, p in mod.state_dict().items():
                    t = p.detach()
                    if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                        t = t.to(device=device, dtype=torch.float32).contiguous()
                    shape = (C.c_int64 * t.dim())(*t.shape)
                    _lib.check(self._lib.loco_set_weight(self._handle, (prefix + name).encode(), C.c_void_p(t.data_ptr()),
                                                         shape, t.dim()), "load_state_dict")
            self._sin_rows = 0
        if self._sin_rows < min_sin_rows:
            rows = max(MAX_SPEECH_POSITIONS + PAD_TOKEN_ID + 1 + 2, min_sin_rows + 2)
            tab = sinusoid_table(rows).contiguous()
            shape = (C.c_int64 * 2)(rows, HIDDEN)
            _lib.check(self._lib.loco_set_weight(self._handle, b"prenet.pos_sinusoidal_embed.weights",
                                                 C.c_void_p(tab.data_ptr()), shape, 2), "sinusoid table")
            self._sin_rows = rows
        if self._weights_dirty and self._extra_weights:
            from .decoder import MAX_TEXT_POSITIONS
            tab = sinusoid_table(MAX_TEXT_POSITIONS + PAD_TOKEN_ID + 1).contiguous()  # HF's decoder table, bit for bit (452 rows)
            _lib.check(self._lib.loco_set_weight(self._handle, b"decoder.prenet.embed_positions.weights", C.c_void_p(tab.data_ptr()),
                                                 (C.c_int64 * 2)(tab.shape[0], HIDDEN), 2), "decoder position table")
        if self._weights_dirty:
            _lib.check(self._lib.loco_finalize_weights(self._handle, stream), "finalize_weights")
            self._weights_dirty = False

    # -- tools for tests / bench -------------------------------------------------------------------------
    def set_profiling(self, on: bool):
        self._ensure_handle(self._device())
        _lib.check(self._lib.loco_set_profiling(self._handle, int(on)))

    def set_profiling_filter(self, bucket: Optional[str]):
        """Bracket only the launches of one kernel bucket (a name profile_read returns); None = all."""
        self._ensure_handle(self._device())
        _lib.check(self._lib.loco_set_profiling_filter(self._handle, (bucket or "").encode()))

    def profile_reset(self):
        _lib.check(self._lib.loco_profile_reset(self._handle))

    def profile_read(self):
        arr = (_lib.KernelStat * 16)()
        n = _lib.check(self._lib.loco_profile_read(self._handle, arr, 16))
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches, ms=arr[i].ms, flops=arr[i].flops,
                     bytes=arr[i].bytes) for i in range(n)]

    def range_report(self):
        """max|x| of every tensor the last f16x3 forward stored as fp16 planes: [(name, layer or -1, amax)] -- call after the
        forward has completed (the numbers follow it to host memory on its stream)."""
        out, i = [], 0
        amax, layer, name = C.c_float(), C.c_int32(), C.create_string_buffer(160)
        while i < self._lib.loco_forward_range(self._handle, i, C.byref(amax), C.byref(layer), name, 160):
            out.append((name.value.decode(), int(layer.value), float(amax.value)))
            i += 1
        return out

    def _forward_call(self, args, stream):
        """loco_forward under the module's range policy (include/loco_asr.h, 'numeric range of precision mode f16x3')."""
        self.last_range_fallback = False
        if self.range_policy == "off":
            _lib.check(self._lib.loco_forward(self._handle, *args, stream), "loco_forward")
            return
        if self.range_policy not in ("fp32", "raise"):
            raise ValueError("range_policy must be 'fp32', 'raise' or 'off'")
        _lib.check(self._lib.loco_set_range_policy(self._handle, 1 if self.range_policy == "fp32" else 0), "set_range_policy")
        used = C.c_int32(0)
        _lib.check(self._lib.loco_forward_checked(self._handle, *args, stream, C.byref(used)), "loco_forward")
        self.last_range_fallback = bool(used.value)

    # -- several forwards in flight ----------------------------------------------------------------------------
    def set_inflight(self, k: int):
        """Allow up to ``k`` forwards of this module in flight at once (forward_async).  The reference encodes one batch of two
        utterances at a time (…base…py:67-68); such a batch is ~125 launches of 5-16 us and cannot fill the GPU, but nothing
        orders batch k+1 behind batch k: each slot has its own stream, workspace and status block, the batches stay what they
        are and so do their results (bit for bit)."""
        if k < 1:
            raise ValueError("inflight must be >= 1")
        device = self._device()
        self._ensure_handle(device)
        self.drain()
        n = int(self._lib.loco_status_bytes())
        with torch.cuda.device(device):
            self._slots = [_Slot(device, n) for _ in range(k)]
        self._next_slot = 0
        self._workspace_floor = 0  # a reservation belongs to the slots it was made for

    def drain(self):
        """Resolve every forward still in flight (their tickets stay valid)."""
        for slot in self._slots:
            if slot.ticket is not None:
                slot.ticket.settle()

    def reserve_workspace(self, batch: int, samples: int):
        """Size the in-flight slots' workspaces for a [batch, samples] problem at their next (re)allocation: a caller that knows
        its largest batch (extract.py --pack: the longest pack of a sorted window) avoids growing a multi-GB workspace step by
        step -- every step is a hipMalloc of the new size, and hipFree of the old one synchronises the device."""
        self._ensure_handle(self._device())
        self._workspace_floor = max(self._workspace_floor, int(self._lib.loco_workspace_bytes(self._handle, batch, samples)))

    def _enqueue(self, slot, x, m, out, frames, precision, pack=None, hidden=None):
        B, L = x.shape
        need = int(self._lib.loco_workspace_bytes(self._handle, B, L))
        if slot.workspace is None or slot.workspace.numel() < need:
            t0 = time.perf_counter()
            slot.workspace = None
            # grown with headroom: packs of a length-sorted window ask for a little more each time
            slot.workspace = torch.empty(max(need + need // 4, self._workspace_floor), dtype=torch.uint8, device=x.device)
            if self.submit_profile is not None:
                self.submit_profile["workspace (re)allocations"] = self.submit_profile.get("workspace (re)allocations", 0.0) + 1.0
                self.submit_profile["workspace allocation, s"] = self.submit_profile.get("workspace allocation, s", 0.0) + time.perf_counter() - t0
        mp = C.c_void_p(m.data_ptr()) if m is not None else None
        if pack is None:
            _lib.check(self._lib.loco_forward_async(
                self._handle, self.PRECISIONS[precision], C.c_void_p(x.data_ptr()), mp, B, L, C.c_void_p(out.data_ptr()),
                C.c_void_p(frames.data_ptr()), None, C.c_void_p(slot.workspace.data_ptr()), slot.workspace.numel(),
                C.c_void_p(slot.stream.cuda_stream), C.c_void_p(slot.status.data_ptr())), "loco_forward_async")
        else:
            vl = (C.c_int64 * B)(*pack.valid_len) if pack.valid_len is not None else None
            hs_ptrs = (C.c_void_p * len(hidden))(*[t.data_ptr() for t in hidden]) if hidden is not None else None
            _lib.check(self._lib.loco_forward_packed(
                self._handle, self.PRECISIONS[precision], C.c_void_p(x.data_ptr()), mp, vl, B, L, (C.c_int64 * B)(*pack.pad_len),
                C.c_void_p(out.data_ptr()), C.c_void_p(frames.data_ptr()), hs_ptrs, C.c_void_p(slot.workspace.data_ptr()),
                slot.workspace.numel(), C.c_void_p(slot.stream.cuda_stream), C.c_void_p(slot.status.data_ptr())), "loco_forward_packed")

    @torch.no_grad()
    def forward_async(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, **kwargs) -> ForwardTicket:
        """Enqueue one forward on the next slot and return its ticket without waiting; ``ticket.result()`` is the
        BaseModelOutput.  Inputs are read after everything already queued on the CURRENT stream (the H2D copies that made
        them); the slot's previous forward, if still unresolved, is resolved first."""
        if self.training:
            raise RuntimeError("the MI355X encoder path is inference-only; call .eval()")
        if input_values.dim() != 2:
            raise ValueError(f"input_values must be [batch, samples], got {tuple(input_values.shape)}")
        device = input_values.device
        self._ensure_handle(device)
        if self._device() != device:
            raise RuntimeError(f"module parameters are on {self._device()} but input_values on {device}")
        if self._weights_dirty:
            self.drain()  # re-finalising overwrites the weight planes in place: nothing may be reading them
        if not self._slots:
            self.set_inflight(2)
        x = input_values
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(torch.float32).contiguous()
        B, L = x.shape
        T = int(self._lib.loco_output_frames(L))
        if T < 1:
            raise ValueError(f"input of {L} samples is shorter than one encoder frame (400 samples)")
        m = None
        if attention_mask is not None:
            if attention_mask.shape != x.shape:
                raise ValueError(f"attention_mask {tuple(attention_mask.shape)} does not match input_values {tuple(x.shape)}")
            m = attention_mask.to(device=device, dtype=torch.int32).contiguous()
        return self._submit(x, m, T)

    def _submit(self, x, m, T, pack=None, hidden_states=False):
        """Enqueue one (plain or packed) forward on the next slot.  ``out`` / ``frames`` are allocated on the CALLER's current
        stream (the slot's stream is ordered behind it before the forward, and the caller's stream behind the forward's completion
        event is what ``result()`` provides on the host): a consumer that uses them on its own stream after ``result()`` needs no
        ``record_stream`` for the allocator's sake -- the block returns to the stream it came from."""
        device = x.device
        B = x.shape[0]
        prof = self.submit_profile  # None, or seconds per phase (LOCO_EXTRACT_PROFILE=1: where a slow enqueue spends its time)
        t0 = time.perf_counter() if prof is not None else 0.0
        slot = self._slots[self._next_slot]
        self._next_slot = (self._next_slot + 1) % len(self._slots)
        if slot.ticket is not None:
            slot.ticket.settle()
        t1 = time.perf_counter() if prof is not None else 0.0
        with torch.cuda.device(device):
            self._sync_weights(device, T + 2)  # also grows the sinusoid table BEFORE anything is in flight on a longer clip
            _lib.check(self._lib.loco_set_streams(self._handle, int(self.streams)), "set_streams")
            cur = torch.cuda.current_stream(device)
            n_out = B * T * HIDDEN
            if pack is not None:
                # packs differ in size from one to the next: a request rounded up to 16 MB finds a cached block of the allocator far
                # more often than an exact one (a miss is a hipMalloc of tens of MB on the enqueuing thread)
                out = torch.empty(((n_out + (1 << 22) - 1) >> 22) << 22, dtype=torch.float32, device=device)[:n_out].view(B, T, HIDDEN)
            else:
                out = torch.empty((B, T, HIDDEN), dtype=torch.float32, device=device)
            frames = torch.empty((B,), dtype=torch.int32, device=device)
            hidden = [torch.empty_like(out) for _ in range(self.num_layers + 1)] if (hidden_states and pack is not None) else None
            slot.stream.wait_stream(cur)
            with torch.cuda.stream(slot.stream):
                for t in [x, m, out, frames] + (hidden or []):
                    if t is not None:
                        t.record_stream(slot.stream)
                ticket = ForwardTicket(self, slot, x, m, out, frames, self.precision, pack)
                ticket._hidden = hidden
                t2 = time.perf_counter() if prof is not None else 0.0
                self._enqueue(slot, x, m, out, frames, self.precision, pack, hidden)
                t3 = time.perf_counter() if prof is not None else 0.0
                ticket._done.record(slot.stream)
        slot.ticket = ticket
        if prof is not None:
            for k_, v_ in (("wait for the slot's previous forward", t1 - t0), ("allocate outputs, order streams", t2 - t1),
                           ("workspace + enqueue (C ABI)", t3 - t2), ("forwards", 1.0)):
                prof[k_] = prof.get(k_, 0.0) + v_
        return ticket

    # -- packed forward: several reference batches in one launch sequence (include/loco_asr.h, loco_forward_packed) ------------
    def pack_batches(self, batches, device=None) -> Pack:
        """Lay the clips of several reference batches out as ONE [B, L] problem: ``batches`` is a list of mappings with
        ``input_values`` f32 [B_i, L_i] and optionally ``attention_mask`` [B_i, L_i] (what SpeechT5FeatureExtractor returns per
        batch, …base…py:60), on the host or on the device.  Clip b keeps the padded length of its own batch (pad_len[b] = L_i);
        spans[i] = (first clip, B_i, output frames of batch i).  Host batches are packed in pinned memory and cross PCIe as one
        copy; their masks are reduced on the host to what HF reduces them to anyway -- the number of present samples per clip
        (modeling_speecht5.py:569-582) -- so no mask is shipped or counted on the device.  Device batches are packed by device-side
        copies and keep their masks."""
        if not batches:
            raise ValueError("pack_batches: no batches")
        device = device or self._device()
        xs = [b["input_values"] for b in batches]
        ms = [b.get("attention_mask") if hasattr(b, "get") else None for b in batches]
        for x, mk in zip(xs, ms):
            if x.dim() != 2:
                raise ValueError(f"input_values must be [batch, samples], got {tuple(x.shape)}")
            if mk is not None and mk.shape != x.shape:
                raise ValueError(f"attention_mask {tuple(mk.shape)} does not match input_values {tuple(x.shape)}")
        B = sum(int(x.shape[0]) for x in xs)
        L = max(int(x.shape[1]) for x in xs)
        L = (L + 7) // 8 * 8  # rows start 16-byte aligned
        on_host = all(not x.is_cuda for x in xs) and all(mk is None or not mk.is_cuda for mk in ms)
        kw = dict(pin_memory=True) if on_host else dict(device=device)
        wav = torch.zeros((B, L), dtype=torch.float32, **kw)
        any_mask = any(mk is not None for mk in ms)
        mask = torch.zeros((B, L), dtype=torch.int32, device=device) if (any_mask and not on_host) else None
        valid_len = [] if (any_mask and on_host) else None
        pad_len, spans, b0 = [], [], 0
        for x, mk in zip(xs, ms):
            nb, li = int(x.shape[0]), int(x.shape[1])
            t = int(self._lib.loco_output_frames(li))
            if t < 1:
                raise ValueError(f"input of {li} samples is shorter than one encoder frame (400 samples)")
            wav[b0:b0 + nb, :li] = x
            if mask is not None:
                if mk is not None:
                    mask[b0:b0 + nb, :li] = mk
                else:
                    mask[b0:b0 + nb, :li] = 1
            elif valid_len is not None:
                valid_len += [int(v) for v in mk.sum(dim=1).tolist()] if mk is not None else [li] * nb
            pad_len += [li] * nb
            spans.append((b0, nb, t))
            b0 += nb
        if on_host:
            wav = wav.to(device, non_blocking=True)
        return Pack(wav=wav, mask=mask, valid_len=valid_len, pad_len=pad_len, spans=spans)

    @torch.no_grad()
    def forward_packed_async(self, batches=None, *, packed: Optional[Pack] = None, output_hidden_states: bool = False) -> ForwardTicket:
        """Enqueue the reference batches in ``batches`` (see pack_batches) -- or an already packed ``Pack`` -- as one launch
        sequence; ``ticket.result()`` is a list with one BaseModelOutput per batch whose ``last_hidden_state`` [B_i, T_i, 768] (a
        view into the pack's output) is what ``forward`` returns for that batch alone up to the fp32 summation order of the GEMMs
        (<= 5e-6 relative L2).  The batches are NOT merged: GroupNorm statistics, the positional conv's zero padding, sinusoid
        positions and the key mask all follow each clip's own batch (include/loco_asr.h)."""
        if self.training:
            raise RuntimeError("the MI355X encoder path is inference-only; call .eval()")
        device = self._device()
        self._ensure_handle(device)
        if self._weights_dirty:
            self.drain()
        if not self._slots:
            self.set_inflight(2)
        pk = packed if packed is not None else self.pack_batches(batches, device)
        if pk.wav.device != device:
            raise RuntimeError(f"module parameters are on {device} but the pack on {pk.wav.device}")
        B = pk.wav.shape[0]
        if len(pk.pad_len) != B or (pk.valid_len is not None and len(pk.valid_len) != B):
            raise ValueError("pad_len / valid_len must hold one entry per clip of the pack")
        if B > int(self._lib.loco_max_pack_clips()):
            raise ValueError(f"a pack holds at most {int(self._lib.loco_max_pack_clips())} clips")
        T = int(self._lib.loco_output_frames(pk.wav.shape[1]))
        return self._submit(pk.wav, pk.mask, T, pk, hidden_states=bool(output_hidden_states))

    def forward_packed(self, batches=None, *, packed=None, output_hidden_states: bool = False):
        """``forward_packed_async(...).result()``: list of per-batch outputs (``output_hidden_states=True``: each with the 13 hidden
        states of its batch, HF modeling_speecht5.py:1287-1313; keeps the pack on one stream)."""
        return self.forward_packed_async(batches, packed=packed, output_hidden_states=output_hidden_states).result()

    def workspace_bytes(self, batch: int, samples: int) -> int:
        self._ensure_handle(self._device())
        return int(self._lib.loco_workspace_bytes(self._handle, batch, samples))

    # -- forward -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                output_attentions: Optional[bool] = None, output_hidden_states: Optional[bool] = None,
                return_dict: Optional[bool] = None, stage_taps: Optional[dict] = None, **kwargs):
        """HF's SpeechT5Encoder call.  ``output_attentions=True`` also returns ``attentions``: one fp32 [B, 12, T, T] tensor per
        layer (softmax over the valid keys, masked keys exactly 0; HF modeling_speecht5.py:930-955), formed by a separate kernel
        after each layer's attention launch -- ``layers * B * 12 * T^2 * 4`` bytes on the input's device (12 layers of 30 s x 8:
        10.3 GB).  ``return_dict=False`` returns (last_hidden_state, hidden_states, attentions) without the Nones."""
        if self.training:
            raise RuntimeError("the MI355X encoder path is inference-only (the reference calls it under "
                               "model.eval() + torch.no_grad()); call .eval()")
        if input_values.dim() != 2:
            raise ValueError(f"input_values must be [batch, samples], got {tuple(input_values.shape)}")
        device = input_values.device
        self._ensure_handle(device)
        if self._device() != device:
            raise RuntimeError(f"module parameters are on {self._device()} but input_values on {device}")
        x = input_values
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(torch.float32).contiguous()
        B, L = x.shape
        T = int(self._lib.loco_output_frames(L))
        if T < 1:
            raise ValueError(f"input of {L} samples is shorter than one encoder frame (400 samples)")
        m = None
        if attention_mask is not None:
            if attention_mask.shape != x.shape:
                raise ValueError(f"attention_mask {tuple(attention_mask.shape)} does not match input_values {tuple(x.shape)}")
            m = attention_mask.to(device=device, dtype=torch.int32).contiguous()
        with torch.cuda.device(device):
            self._sync_weights(device, T + 2)
            _lib.check(self._lib.loco_set_precision(self._handle, self.PRECISIONS[self.precision]), "set_precision")
            _lib.check(self._lib.loco_set_streams(self._handle, int(self.streams)), "set_streams")
            need = int(self._lib.loco_workspace_bytes(self._handle, B, L))
            if self._workspace is None or self._workspace.numel() < need or self._workspace.device != device:
                self._workspace = None
                self._workspace = torch.empty(need, dtype=torch.uint8, device=device)
            out = torch.empty((B, T, HIDDEN), dtype=torch.float32, device=device)
            frames = torch.empty((B,), dtype=torch.int32, device=device)
            hs, hs_ptrs = None, None
            if output_hidden_states:
                hs = [torch.empty_like(out) for _ in range(self.num_layers + 1)]
                hs_ptrs = (C.c_void_p * (self.num_layers + 1))(*[t.data_ptr() for t in hs])
            taps, attn = None, None
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            try:
                if stage_taps is not None:
                    taps = dict(conv_stack=torch.empty((B, T, CONV_DIM), dtype=torch.float32, device=device),
                                feature_projection=torch.empty_like(out), prenet=torch.empty_like(out))
                    _lib.check(self._lib.loco_set_taps(self._handle, taps["conv_stack"].data_ptr(),
                                                       taps["feature_projection"].data_ptr(), taps["prenet"].data_ptr()))
                if output_attentions:
                    attn = bind_attention_outputs(self._lib, self._handle, self.num_layers, B, T, device)
                self._forward_call((C.c_void_p(x.data_ptr()), C.c_void_p(m.data_ptr()) if m is not None else None, B, L,
                                    C.c_void_p(out.data_ptr()), C.c_void_p(frames.data_ptr()), hs_ptrs,
                                    C.c_void_p(self._workspace.data_ptr()), self._workspace.numel()), stream)
            finally:
                if taps is not None:
                    _lib.check(self._lib.loco_set_taps(self._handle, None, None, None))
                if attn is not None:
                    _lib.check(self._lib.loco_set_attention_outputs(self._handle, None, 0))
        if stage_taps is not None:
            stage_taps.update(taps)
            stage_taps["frames"] = frames
        self.last_frames = frames
        hidden = tuple(hs) if hs is not None else None
        if return_dict is False:
            return tuple(v for v in (out, hidden, attn) if v is not None)
        return BaseModelOutput(last_hidden_state=out, hidden_states=hidden, attentions=attn)


def bind_attention_outputs(lib, handle, layers: int, B: int, T: int, device) -> tuple:
    """Allocate the per-layer [B, 12, T, T] fp32 probability tensors of output_attentions=True and bind them to the handle
    (loco_set_attention_outputs); the caller unbinds after the forward.  A zero-layer encoder binds nothing and returns ()."""
    probs = tuple(torch.empty((B, HEADS, T, T), dtype=torch.float32, device=device) for _ in range(layers))
    if layers:
        ptrs = (C.c_void_p * layers)(*[t.data_ptr() for t in probs])
        _lib.check(lib.loco_set_attention_outputs(handle, ptrs, layers), "loco_set_attention_outputs")
    return probs


def _decoder_layer_names(layer: int):
    from .decoder import decoder_layer_keys
    return decoder_layer_keys(layer)


class _SpeechT5Core(nn.Module):
    def __init__(self, encoder, decoder=None):
        super().__init__()
        self.encoder = encoder
        if decoder is not None:
            self.decoder = decoder


class SpeechT5ForSpeechToTextMI355X(nn.Module):
    """HF's SpeechT5ForSpeechToText as the reference uses it: ``.speecht5.encoder`` (the embedding path), and -- when decoder
    weights are loaded (``decoder_layers > 0``) -- ``.speecht5.decoder`` / ``.text_decoder_postnet`` with ``forward(...,
    decoder_input_ids=...)`` and greedy ``generate`` (decoder.py).  An encoder-only model is exactly what it was."""

    def __init__(self, layers: int = LAYERS, precision: str = "f16x3", decoder_layers: int = 0, vocab_size: Optional[int] = None):
        super().__init__()
        encoder = SpeechT5EncoderWithSpeechPrenetMI355X(layers, precision)
        decoder = None
        if decoder_layers:
            from . import decoder as dec
            ref = _Ref()
            ref.obj = encoder
            decoder, postnet = dec.make_decoder_modules(ref, decoder_layers, vocab_size or dec.TEXT_VOCAB)
            encoder._extra_weights = [("decoder.", decoder), ("text_decoder_postnet.", postnet)]
            encoder._decoder_layers = decoder_layers
            encoder._decoder_vocab = vocab_size or dec.TEXT_VOCAB
            self._decoder_runtime = dec.DecoderRuntime(encoder)
        self.speecht5 = _SpeechT5Core(encoder, decoder)
        if decoder is not None:
            self.text_decoder_postnet = postnet
        self.eval()

    @property
    def has_decoder(self) -> bool:
        return hasattr(self, "text_decoder_postnet")

    def _require_decoder(self, what: str):
        if not self.has_decoder:
            why = getattr(self, "_no_decoder_reason", None)
            raise RuntimeError(f"{what} needs the decoder, and this model was loaded without one: speecht5.decoder.* and "
                               "text_decoder_postnet.lm_head.weight are missing (from_pretrained on a full speech-to-text checkpoint, or "
                               "from_state_dicts(..., decoder_state_dict=, postnet_state_dict=))" + (f" -- {why}" if why else ""))

    def _encode(self, input_values, attention_mask):
        out = self.speecht5.encoder(input_values=input_values, attention_mask=attention_mask)
        return out.last_hidden_state, self.speecht5.encoder.last_frames

    def _encode_with_attentions(self, input_values, attention_mask):
        out = self.speecht5.encoder(input_values=input_values, attention_mask=attention_mask, output_attentions=True)
        return out.last_hidden_state, self.speecht5.encoder.last_frames, out.attentions

    @torch.no_grad()
    def forward(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                decoder_input_ids: Optional[torch.Tensor] = None, output_hidden_states: Optional[bool] = None,
                labels: Optional[torch.Tensor] = None, output_attentions: Optional[bool] = None, **kwargs):
        """``model(**audios, decoder_input_ids=ids)``: teacher-forced logits [B, S, vocab] and ``encoder_last_hidden_state``
        (``output_hidden_states=True``: also the 7 ``decoder_hidden_states``).  Causal self-attention over the ids as given (no
        decoder attention mask, as in the reference's calls); cross-attention over each clip's valid encoder frames.

        ``labels`` [B, S] (token ids, -100 = not counted): also ``loss``, HF's mean cross-entropy over the counted labels, and
        ``token_logprobs`` [B, S].  Without ``decoder_input_ids`` the decoder reads the labels shifted right (decoder.shift_tokens_right),
        as HF does; with both, the given ids are read and the loss is taken against ``labels``.

        ``output_attentions=True``: also ``decoder_attentions`` (6 x [B, 12, S, S], key j visible to query i iff j <= i),
        ``cross_attentions`` (6 x [B, 12, S, T_enc], key j visible iff it is a valid frame of its clip) and ``encoder_attentions`` (the
        encoder's own flag), fp32, masked entries exactly 0; formed by launches of their own (csrc/decoder_probs.hip), so logits
        and hidden states are the same bits with and without the flag."""
        for k in kwargs:
            if k in ("decoder_attention_mask", "past_key_values", "encoder_outputs", "use_cache"):
                raise NotImplementedError(f"forward({k}=...) is not implemented")
            raise TypeError(f"forward() got an unexpected keyword argument '{k}'")
        self._require_decoder("forward(labels=...)" if labels is not None and decoder_input_ids is None else "forward(decoder_input_ids=...)")
        if decoder_input_ids is None and labels is None:
            raise ValueError("You have to specify `decoder_input_ids` (for embeddings alone call model.speecht5.encoder)")
        from . import decoder as dec
        targets = None
        if labels is not None:  # on the host, before any launch
            host = dec.check_labels(labels, int(input_values.shape[0]), self.speecht5.encoder._decoder_vocab,
                                    decoder_input_ids.shape if decoder_input_ids is not None else None)
            if decoder_input_ids is None:
                decoder_input_ids = dec.shift_tokens_right(host)
            targets = host.to(torch.int32)
        enc_attn = self_attn = cross_attn = None
        if output_attentions:
            enc_out, frames, enc_attn = self._encode_with_attentions(input_values, attention_mask)
        else:
            enc_out, frames = self._encode(input_values, attention_mask)
        if decoder_input_ids.dim() != 2 or decoder_input_ids.shape[0] != enc_out.shape[0]:
            raise ValueError(f"decoder_input_ids must be [batch, tokens] with batch {enc_out.shape[0]}, got {tuple(decoder_input_ids.shape)}")
        ids = decoder_input_ids.to(device=enc_out.device, dtype=torch.int32).contiguous()
        with torch.cuda.device(enc_out.device):
            if output_attentions:
                logits, hidden, self_attn, cross_attn = self._decoder_runtime.forward_attn(enc_out, frames, ids, bool(output_hidden_states))
            else:
                logits, hidden = self._decoder_runtime.forward(enc_out, frames, ids, bool(output_hidden_states))
            loss = logprobs = None
            if targets is not None:
                logprobs, _, _, loss, _ = dec.score_logits(self.speecht5.encoder._lib, logits, targets.to(enc_out.device).contiguous(), *ids.shape)
        return dec.Seq2SeqLMOutput(logits=logits, encoder_last_hidden_state=enc_out, decoder_hidden_states=hidden, loss=loss, token_logprobs=logprobs,
                                   decoder_attentions=self_attn, cross_attentions=cross_attn, encoder_attentions=enc_attn)

    @torch.no_grad()
    def align(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None,
              alignment_heads=None, return_attention: bool = False):
        """Where in the audio each token of the transcripts ``labels`` [B, S] was spoken: a decoder.TokenAlignment with ``start_frames`` /
        ``end_frames`` i32 [B, S] (encoder frames, end exclusive, -1 where the label is -100) and ``start_times`` / ``end_times`` in seconds
        (frames x 320 / 16000, the conv stack's stride; its receptive-field offset is ignored).  -100 may only pad the end of a row.

        One teacher-forced pass on the labels shifted right; the mean of the cross-attention probabilities over ``alignment_heads``
        ((layer, head) pairs; None = all 72) is the soft alignment A [B, S, T_enc] (``return_attention=True`` hands it out), and a
        monotone DTW over -A from (0, 0) to (n_b - 1, frames_b - 1) -- on the device, in double -- gives every token its frames."""
        self._require_decoder("align()")
        if labels is None:
            raise ValueError("align() needs labels")
        from . import decoder as dec
        enc = self.speecht5.encoder
        host = dec.check_labels(labels, int(input_values.shape[0]), enc._decoder_vocab)
        counts = dec.alignment_counts(host)
        heads, pairs = dec.check_alignment_heads(alignment_heads, enc._decoder_layers)
        enc_out, frames = self._encode(input_values, attention_mask)
        return self._align_encoded(enc_out, frames, host, counts, heads, pairs, return_attention)

    def _align_encoded(self, enc_out, frames, labels_host, counts, heads, pairs, return_attention):
        from . import decoder as dec
        device = enc_out.device
        ids = dec.shift_tokens_right(labels_host).to(device=device, dtype=torch.int32).contiguous()
        with torch.cuda.device(device):
            start, end, A = self._decoder_runtime.align(enc_out, frames, ids, counts.to(device).contiguous(), heads, pairs, return_attention)
            seconds = lambda f: torch.where(f < 0, -1.0, f.to(torch.float32) * dec.FRAME_SECONDS).to(torch.float32)  # noqa: E731
            return dec.TokenAlignment(start_frames=start, end_frames=end, start_times=seconds(start), end_times=seconds(end), attention=A)

    @torch.no_grad()
    def align_many(self, batches, labels, pack: int = 8, alignment_heads=None, return_attention: bool = False):
        """Token timestamps of a corpus, built the way ``score_many`` is: ``batches`` is what ``generate_many`` takes, ``labels`` one
        1-D LongTensor per utterance in input order (no -100 needed: each row is padded to its pack's longest).  The batches are
        encoded ``pack`` at a time through ``forward_packed``; each pack's clips go through ONE ``align`` pass on the packed output and
        its frame counts.  Returns a list, in input order, of decoder.TokenAlignment whose fields are the utterance's own 1-D slices
        (``attention`` [len, T of its pack]).  An utterance's A is that of ``align`` on its own batch up to the fp32 summation order
        of the packed encoder and of the decoder's products; its path is the DTW of that A."""
        from . import decoder as dec
        self._require_decoder("align_many()")
        batches = [b for b in batches if b["input_values"].shape[0]]
        labels = list(labels)
        total = sum(int(b["input_values"].shape[0]) for b in batches)
        if len(labels) != total:
            raise ValueError(f"align_many: {len(labels)} label rows for {total} utterances")
        if int(pack) < 1:
            raise ValueError("pack must be >= 1")
        enc = self.speecht5.encoder
        heads, pairs = dec.check_alignment_heads(alignment_heads, enc._decoder_layers)
        hosts = []
        for u, lab in enumerate(labels):
            if not torch.is_tensor(lab) or lab.dim() != 1:
                raise ValueError(f"align_many: labels[{u}] must be a 1-D tensor of token ids")
            hosts.append(dec.check_labels(lab[None], 1, enc._decoder_vocab)[0])
            dec.alignment_counts(hosts[-1][None])
        results, u0 = [], 0
        for g0 in range(0, len(batches), int(pack)):
            group = batches[g0:g0 + int(pack)]
            ticket = enc.forward_packed_async(group)
            ticket.result()
            out, _ = ticket.packed_output()
            n = int(out.shape[0])
            rows = hosts[u0:u0 + n]
            S = max(int(r.shape[0]) for r in rows)
            lab = torch.full((n, S), dec.IGNORE_INDEX, dtype=torch.long)
            for i, r in enumerate(rows):
                lab[i, :r.shape[0]] = r
            al = self._align_encoded(out, enc.last_frames, lab, dec.alignment_counts(lab), heads, pairs, return_attention)
            for i, r in enumerate(rows):
                k = int(r.shape[0])
                results.append(dec.TokenAlignment(start_frames=al.start_frames[i, :k], end_frames=al.end_frames[i, :k], start_times=al.start_times[i, :k],
                                                  end_times=al.end_times[i, :k], attention=al.attention[i, :k] if al.attention is not None else None))
            u0 += n
        return results

    @torch.no_grad()
    def score(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None):
        """How likely the model finds the transcripts ``labels`` [B, S] (-100 = not counted) for these clips: decoder.TranscriptScores
        with ``token_logprobs`` [B, S], ``sequence_logprob`` [B], ``tokens`` [B] and ``loss`` -- ``forward(labels=...)``'s pass, without
        handing the logits out."""
        self._require_decoder("score()")
        if labels is None:
            raise ValueError("score() needs labels")
        from . import decoder as dec
        host = dec.check_labels(labels, int(input_values.shape[0]), self.speecht5.encoder._decoder_vocab)
        enc_out, frames = self._encode(input_values, attention_mask)
        return self._score_encoded(enc_out, frames, host)

    def _score_encoded(self, enc_out, frames, labels_host):
        from . import decoder as dec
        device = enc_out.device
        ids = dec.shift_tokens_right(labels_host).to(device=device, dtype=torch.int32).contiguous()
        with torch.cuda.device(device):
            logits, _ = self._decoder_runtime.forward(enc_out, frames, ids)
            lp, seq, cnt, loss, _ = dec.score_logits(self.speecht5.encoder._lib, logits, labels_host.to(device=device, dtype=torch.int32).contiguous(),
                                                     *ids.shape)
        return dec.TranscriptScores(token_logprobs=lp, sequence_logprob=seq, tokens=cnt, loss=loss)

    @torch.no_grad()
    def score_many(self, batches, labels, pack: int = 8):
        """Scores of a corpus: ``batches`` is what ``generate_many`` takes, ``labels`` one 1-D LongTensor per utterance in input order.
        The batches are encoded ``pack`` at a time through ``forward_packed``; each pack's clips go through ONE teacher-forced
        decoder pass on the packed output and its frame counts, their labels padded with -100 to the pack's longest, and are scored
        in one launch.  Returns a list, in input order, of (``token_logprobs`` 1-D of the utterance's own length, its sum 0-d), both
        on the device.  An utterance's scores are those of ``score`` on its own batch up to the fp32 summation order of the packed
        encoder and of the decoder's products, whatever ``pack`` is; the scoring kernel itself adds nothing to that (a row's
        log-probability is a function of the row's logits alone)."""
        from . import decoder as dec
        self._require_decoder("score_many()")
        batches = [b for b in batches if b["input_values"].shape[0]]
        labels = list(labels)
        total = sum(int(b["input_values"].shape[0]) for b in batches)
        if len(labels) != total:
            raise ValueError(f"score_many: {len(labels)} label rows for {total} utterances")
        if int(pack) < 1:
            raise ValueError("pack must be >= 1")
        enc = self.speecht5.encoder
        hosts = []
        for u, lab in enumerate(labels):
            if not torch.is_tensor(lab) or lab.dim() != 1:
                raise ValueError(f"score_many: labels[{u}] must be a 1-D tensor of token ids")
            hosts.append(dec.check_labels(lab[None], 1, enc._decoder_vocab)[0])
        results, u0 = [], 0
        for g0 in range(0, len(batches), int(pack)):
            group = batches[g0:g0 + int(pack)]
            ticket = enc.forward_packed_async(group)
            ticket.result()
            out, _ = ticket.packed_output()
            n = int(out.shape[0])
            rows = hosts[u0:u0 + n]
            S = max(int(r.shape[0]) for r in rows)
            lab = torch.full((n, S), dec.IGNORE_INDEX, dtype=torch.long)
            for i, r in enumerate(rows):
                lab[i, :r.shape[0]] = r
            sc = self._score_encoded(out, enc.last_frames, lab)
            for i, r in enumerate(rows):
                results.append((sc.token_logprobs[i, :r.shape[0]], sc.sequence_logprob[i]))
            u0 += n
        return results

    @torch.no_grad()
    def generate(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, max_length: Optional[int] = None,
                 max_new_tokens: Optional[int] = None, return_logits: bool = False, return_dict_in_generate: bool = False,
                 output_scores: bool = False, **kwargs):
        """Greedy search as HF's ``generate`` runs it for this model: LongTensor [B, S] starting with decoder_start_token_id 2, a
        row that has emitted </s> (2) is filled with <pad> (1), S = the longest row or ``max_length`` (total, start token included;
        ``max_new_tokens`` counts the tokens after it).  ``return_logits=True``: also the logits [S - 1, B, vocab] each step chose from.

        ``return_dict_in_generate=True``: a decoder.GreedySearchOutput whose ``sequences`` are those ids; with ``output_scores=True``
        it also carries ``scores`` (the S - 1 step logits [B, vocab]), ``token_logprobs`` [B, S - 1] and ``sequence_logprobs`` [B].
        ``output_scores`` alone changes nothing, as in HF."""
        from . import decoder as dec
        dec.check_generate_kwargs(kwargs)
        self._require_decoder("generate()")
        n = dec.resolve_max_length(max_length, max_new_tokens)
        enc_out, frames = self._encode(input_values, attention_mask)
        with_scores = bool(return_dict_in_generate) and bool(output_scores)
        with torch.cuda.device(enc_out.device):
            rt = self._decoder_runtime
            res = rt.generate(enc_out, frames, n, return_logits or with_scores)
            if not return_dict_in_generate:
                return res
            ids, steps = res if (return_logits or with_scores) else (res, None)
            out = dec.GreedySearchOutput(sequences=ids)
            if with_scores:
                B, S = ids.shape
                # targets: the returned ids, -100 from each row's length on (the host holds ids' lengths already)
                cols = torch.arange(1, S)[None, :]
                targets = torch.where(cols < rt.last_lengths[:, None].long(), ids[:, 1:].cpu(), torch.tensor(dec.IGNORE_INDEX)).to(torch.int32)
                by_row = steps.permute(1, 0, 2).contiguous()  # [B, S - 1, V]: a row's steps form one sequence
                lp, seq, _, _, _ = dec.score_logits(self.speecht5.encoder._lib, by_row, targets.to(enc_out.device).contiguous(), B, S - 1)
                out.scores, out.token_logprobs, out.sequence_logprobs = tuple(steps[t] for t in range(S - 1)), lp, seq
            return (out, steps) if return_logits else out

    @torch.no_grad()
    def generate_many(self, batches, max_length=None, max_new_tokens: Optional[int] = None, slots: int = 64, return_logits: bool = False,
                      pack: int = 8, return_scores: bool = False, **kwargs):
        """Greedy transcripts of a corpus: ``batches`` is what ``pack_batches`` takes (reference batches of ``input_values`` /
        ``attention_mask``), ``max_length`` an int or one int per utterance (total length, start token included).  The batches are
        encoded ``pack`` at a time through ``forward_packed`` -- every clip keeps its own batch's padded length -- and decoded in a
        pool of ``slots`` decoder rows in which a row that ends hands its slot to the next utterance (decoder.DecoderPool).

        Returns a list, in input order, of 1-D LongTensors (host): <s> ... up to and including </s>, or the utterance's cap of tokens
        for a row that never ended -- row u of ``generate(**batch_k, max_length=cap_u)`` without its trailing <pad>, up to the fp32
        summation order of the packed encoder and of the attention's key splits.  An utterance's result does not depend on the
        utterances decoded beside it.  ``return_logits=True``: (ids, logits) with one [len - 1, vocab] device tensor per utterance.
        ``return_scores=True``: (ids, scores) with one [len - 1] device tensor per utterance, the log-probability of every generated
        token (both: (ids, logits, scores))."""
        from . import decoder as dec
        dec.check_generate_kwargs(kwargs)
        self._require_decoder("generate_many()")
        batches = list(batches)
        sizes = [int(b["input_values"].shape[0]) for b in batches]
        total = sum(sizes)
        caps = dec.resolve_caps(total, max_length, max_new_tokens)
        if int(pack) < 1:
            raise ValueError("pack must be >= 1")
        most = int(self.speecht5.encoder._lib.loco_decoder_max_batch())
        if not 1 <= int(slots) <= most:
            raise ValueError(f"generate_many: slots = {slots} is outside 1 .. {most}, the decode step's limit of rows")
        extras = int(bool(return_logits)) + int(bool(return_scores))
        if total == 0:
            return ([],) * (1 + extras) if extras else []
        enc = self.speecht5.encoder
        lib = enc._lib
        device = enc._device()
        T_cap = max(int(lib.loco_output_frames(int(b["input_values"].shape[1]))) for b in batches if b["input_values"].shape[0])
        if T_cap < 1:
            raise ValueError("input shorter than one encoder frame (400 samples)")
        pool = None
        results, key, nxt = {}, 0, 0
        batches = [b for b in batches if b["input_values"].shape[0]]
        with torch.cuda.device(device):
            while nxt < len(batches) or (pool is not None and pool.busy):
                if nxt < len(batches) and (pool is None or len(pool.waiting) < int(slots)):
                    ticket = enc.forward_packed_async(batches[nxt:nxt + int(pack)])
                    nxt += int(pack)
                    ticket.result()
                    out, spans = ticket.packed_output()
                    frames = enc.last_frames
                    if pool is None:  # after the first forward: the handle exists and carries the decoder's weights
                        pool = dec.DecoderPool(enc, min(int(slots), total), T_cap, max(caps), device,
                                               return_logits=return_logits, return_scores=return_scores)
                    items = []
                    for b0, nb, t in spans:
                        for c in range(b0, b0 + nb):
                            items.append(dec.PoolItem(key=key, enc_out=out, frames=frames, clip=c, rows=t, cap=caps[key]))
                            key += 1
                    pool.submit(items)
                    continue
                for k, *rest in pool.round():
                    results[k] = rest
        out = [[results[k][0] for k in range(total)]]
        if return_logits:
            out.append([results[k][1] for k in range(total)])
        if return_scores:
            out.append([results[k][2] for k in range(total)])
        return tuple(out) if extras else out[0]

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, precision: str = "f16x3", **_unused):
        """``SpeechT5ForSpeechToText.from_pretrained(...)`` of the fine-tuned script (…finetuned…py:95) for a checkpoint ON
        DISK: a directory holding ``model.safetensors`` / ``pytorch_model.bin`` (or their sharded index), one such file, or a hub
        name that is already in the local HuggingFace cache -- nothing is ever downloaded.  Keeps ``speecht5.encoder.prenet.*``
        and ``speecht5.encoder.wrapped_encoder.*`` (either spelling of the weight-normed positional conv) and, when the file has
        them, ``speecht5.decoder.*`` and ``text_decoder_postnet.*`` (the tied embedding / lm_head pair may be present once); takes
        the layer counts from the keys, and fails BY NAME on anything the encoder needs and the file lacks
        (load_state_dict(strict=True)).  The decoder is kept only when the file holds a COMPLETE one (checkpoint_map.decoder_problem):
        a file with the encoder and stray or partial decoder tensors gives the encoder-only model it always gave, and ``generate`` /
        ``decoder_input_ids`` then raise with the name of the first decoder tensor that is missing or misshapen."""
        import re
        from . import checkpoint_map
        checkpoint_map.check_hf_config(str(pretrained_model_name_or_path))
        pre, enc = checkpoint_map.load_hf_checkpoint(str(pretrained_model_name_or_path))
        ids = [int(m_.group(1)) for m_ in (re.match(r"layers\.(\d+)\.", k) for k in enc) if m_]
        if not ids:
            raise KeyError(f"{pretrained_model_name_or_path}: no speecht5.encoder.wrapped_encoder.layers.N.* tensors")
        dec_sd, post_sd = checkpoint_map.load_hf_decoder(str(pretrained_model_name_or_path))
        problem = checkpoint_map.decoder_problem(dec_sd, post_sd)
        if problem is not None:  # no (complete) decoder in the file: the encoder-only model this call has always returned
            model = cls.from_state_dicts(pre, enc, layers=max(ids) + 1, precision=precision)
            model._no_decoder_reason = f"{pretrained_model_name_or_path}: {problem}"
            return model
        known = {"prenet.embed_tokens.weight"} | {"wrapped_decoder." + n for l in range(64) for n, _, _ in _decoder_layer_names(l)}
        dec_sd = {k: v for k, v in dec_sd.items() if k in known}  # e.g. a stray wrapped_decoder.layer_norm of another architecture
        return cls.from_state_dicts(pre, enc, layers=max(ids) + 1, precision=precision, decoder_state_dict=dec_sd,
                                    postnet_state_dict={k: v for k, v in post_sd.items() if k == "lm_head.weight"})

    @classmethod
    def from_state_dicts(cls, prenet_state_dict, encoder_state_dict, layers: int = LAYERS, precision: str = "f16x3",
                         decoder_state_dict=None, postnet_state_dict=None):
        """What the base script does after from_pretrained (…base…py:98-100), minus the hub download.  With ``decoder_state_dict``
        (keys ``prenet.embed_tokens.weight``, ``wrapped_decoder.layers.N.*``) and / or ``postnet_state_dict`` (``lm_head.weight``)
        the model also decodes; of the tied pair embed_tokens / lm_head one may be absent (it is taken from the other)."""
        import re
        dec_layers, vocab = 0, None
        if decoder_state_dict is not None or postnet_state_dict is not None:
            decoder_state_dict = dict(decoder_state_dict or {})
            postnet_state_dict = dict(postnet_state_dict or {})
            emb, head = decoder_state_dict.get("prenet.embed_tokens.weight"), postnet_state_dict.get("lm_head.weight")
            if emb is None and head is None:
                raise KeyError("decoder weights without prenet.embed_tokens.weight or lm_head.weight (the tied pair: one of them is needed)")
            decoder_state_dict.setdefault("prenet.embed_tokens.weight", head)
            postnet_state_dict.setdefault("lm_head.weight", emb)
            ids = [int(m_.group(1)) for m_ in (re.match(r"wrapped_decoder\.layers\.(\d+)\.", k) for k in decoder_state_dict) if m_]
            if not ids:
                raise KeyError("decoder_state_dict: no wrapped_decoder.layers.N.* tensors")
            dec_layers, vocab = max(ids) + 1, int(decoder_state_dict["prenet.embed_tokens.weight"].shape[0])
        model = cls(layers, precision, decoder_layers=dec_layers, vocab_size=vocab)
        model.speecht5.encoder.wrapped_encoder.load_state_dict(encoder_state_dict)
        model.speecht5.encoder.prenet.load_state_dict(prenet_state_dict)
        if dec_layers:
            as_t = lambda d: {k: (v if torch.is_tensor(v) else torch.as_tensor(v)) for k, v in d.items()}  # noqa: E731
            model.speecht5.decoder.load_state_dict(as_t(decoder_state_dict))
            model.text_decoder_postnet.load_state_dict(as_t(postnet_state_dict))
        return model
