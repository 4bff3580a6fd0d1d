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
from .holders import _Ref, _register, _WeightHolder
from .synth import (CONV_DIM, CONV_KERNEL, FFN, HEAD_DIM, HEADS, HIDDEN, LAYERS, MAX_TEXT_POSITIONS, POS_CONV_GROUPS, POS_CONV_K, REL_MAX)

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


def sinusoid_table(rows: int, dim: int = HIDDEN) -> torch.Tensor:
    """HF SpeechT5SinusoidalPositionalEmbedding.get_embedding (modeling_speecht5.py:305-321), same torch
    expression so that the table is bit-identical to the one HF builds at module init (weights, not hot path)."""
    half = dim // 2
    w = torch.exp(torch.arange(half, dtype=torch.int64).float() * -(math.log(10000) / (half - 1)))
    ang = torch.arange(rows, dtype=torch.int64).float().unsqueeze(1) * w.unsqueeze(0)
    tab = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1).view(rows, -1)
    tab[PAD_TOKEN_ID, :] = 0
    return tab


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


class _EncoderBase(nn.Module):
    """Everything a forward through the library needs whatever feeds the 12 layers: the handle and the weights' way to it, the slots
    of forwards in flight, ``forward`` and ``forward_async``.  A front end -- speech below, text in text_encoder.py -- passes its
    prenet module to ``__init__`` and implements the hooks at the end of this class; it overrides none of the above."""

    # "f16x3" (default): GEMMs and attention products as three fp16 MFMAs per fp32-class product (hi/lo operand split,
    # fp32 accumulate) -- ~1e-6 relative L2 of an fp64 evaluation end to end, 2.4x the speed of "f32";
    # "f32": every contraction on the exact fp32 MFMA (~1e-6).  Both are far inside the 1e-3 bar.
    # "f16x2" (opt-in, never the default): the weights of every projection / conv GEMM rounded to fp16 (after their
    # per-tensor power-of-two scale), activations still hi + lo, attention products still three-term -- ~9e-4 on the goldens: AT the
    # 1e-3 bar, not inside it with margin (no guarantee on other weights), and no longer fp32 class; a third fewer matrix
    # instructions in the GEMMs.
    PRECISIONS = {"f32": 0, "f16x3": 1, "f16x2": 2}

    def __init__(self, prenet: _WeightHolder, layers: int, precision: str, streams: int):
        super().__init__()
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(self.PRECISIONS)}")
        self.precision = precision
        self._lib = _lib.load()  # raises when the HIP library is missing: no fallback
        self.prenet = prenet
        self.wrapped_encoder = SpeechT5EncoderMI355X(prenet._owner_ref, layers)
        prenet._owner_ref.obj = self
        self.num_layers = layers
        self._handle = None
        self._handle_device = None
        self._weights_dirty = True
        self._workspace = None
        # further (key prefix, module) pairs whose tensors go to the same handle: the model's decoder halves (decoder.py); empty for an
        # encoder-only model, which then loads exactly what it always has
        self._extra_weights = []
        self._decoder_layers = 0
        self._decoder_vocab = 0
        # speech: large batches run as two half-batches on two HIP streams (bit-identical, ~2 % faster: include/loco_asr.h,
        # loco_set_streams); 1 keeps everything on the caller's stream (the library runs text that way whatever is set)
        self.streams = streams
        # Numeric range of precision "f16x3" (include/loco_asr.h): "fp32" = a batch whose activations leave the range the fp16
        # planes represent is run again on the library's exact-fp32 MFMA kernels (the default: a caller never sees NaNs or a
        # silently degraded embedding); "raise" = LocoError instead; "off" = no check and no host synchronisation (the
        # forward stays fully asynchronous; loco_forward_status can still be queried through range_report()).
        self.range_policy = "fp32"
        self.last_range_fallback = False
        self.last_frames = None
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

    def _sync_weights(self, device: torch.device, min_rows: int):
        dirty = self._weights_dirty
        if dirty:
            self.drain()  # forwards still in flight on the slots' streams read the planes that are about to be rebuilt

        def put(key, t, what="load_state_dict"):
            t = t.detach()
            if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                t = t.to(device=device, dtype=torch.float32).contiguous()
            if t.dim() == 0:
                t = t.reshape(1)
            shape = (C.c_int64 * t.dim())(*t.shape)
            _lib.check(self._lib.loco_set_weight(self._handle, key.encode(), C.c_void_p(t.data_ptr()), shape, t.dim()), what)

        if dirty:
            for prefix, mod in self._weight_sources():
                for name, p in mod.state_dict().items():
                    put(prefix + name, p)
        self._load_tables(put, dirty, min_rows)
        if dirty:
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
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

    def workspace_bytes(self, batch: int, length: int) -> int:
        self._ensure_handle(self._device())
        return self._workspace_need(batch, length)

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

    def reserve_workspace(self, batch: int, length: int):
        """Size the in-flight slots' workspaces for a [batch, length] problem at their next (re)allocation: a caller that knows
        its largest batch (extract.py --pack: the longest pack of a sorted window) avoids growing a multi-GB workspace step by
        step -- every step is a hipMalloc of the new size, and hipFree of the old one synchronises the device."""
        self._workspace_floor = max(self._workspace_floor, self.workspace_bytes(batch, length))

    def _enqueue(self, slot, x, m, out, frames, precision, pack=None, hidden=None):
        """One forward on ``slot`` (``_submit``, and the fp32 re-run of its ticket): grow the slot's workspace, then the front end's call."""
        need = self._workspace_need(*x.shape)
        if slot.workspace is None or slot.workspace.numel() < need:
            t0 = time.perf_counter()
            slot.workspace = None
            # grown with headroom: packs of a length-sorted window ask for a little more each time
            slot.workspace = torch.empty(max(need + need // 4, self._workspace_floor), dtype=torch.uint8, device=x.device)
            if self.submit_profile is not None:
                self.submit_profile["workspace (re)allocations"] = self.submit_profile.get("workspace (re)allocations", 0.0) + 1.0
                self.submit_profile["workspace allocation, s"] = self.submit_profile.get("workspace allocation, s", 0.0) + time.perf_counter() - t0
        self._launch(slot, x, m, out, frames, precision, pack, hidden)

    def _begin(self, device: torch.device, why: str = ""):
        """What every forward starts with: inference only, a handle on the inputs' device, the parameters there too."""
        if self.training:
            raise RuntimeError(f"the MI355X encoder path is inference-only{why}; call .eval()")
        self._ensure_handle(device)
        if self._device() != device:
            raise RuntimeError(f"module parameters are on {self._device()} but input_values on {device}")

    def _begin_async(self, device: torch.device):
        self._begin(device)
        if self._weights_dirty:
            self.drain()  # re-finalising overwrites the weight planes in place: nothing may be reading them
        if not self._slots:
            self.set_inflight(2)

    @torch.no_grad()
    def forward_async(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, **kwargs) -> ForwardTicket:
        """Enqueue one forward on the next slot and return its ticket without waiting; ``ticket.result()`` is the
        BaseModelOutput.  Inputs are read after everything already queued on the CURRENT stream (the H2D copies that made
        them); the slot's previous forward, if still unresolved, is resolved first."""
        self._begin_async(input_values.device)
        return self._submit(*self._prepare(input_values, attention_mask))

    def forward_packed(self, batches=None, **kwargs):
        """``forward_packed_async(...).result()``: list of per-batch outputs (speech, ``output_hidden_states=True``: each with the 13
        hidden states of its batch, HF modeling_speecht5.py:1287-1313; keeps the pack on one stream)."""
        return self.forward_packed_async(batches, **kwargs).result()

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

    # -- forward -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                output_attentions: Optional[bool] = None, output_hidden_states: Optional[bool] = None,
                return_dict: Optional[bool] = None, **kwargs):
        """HF's SpeechT5Encoder call.  ``output_attentions=True`` also returns ``attentions``: one fp32 [B, 12, T, T] tensor per
        layer (softmax over the valid keys, masked keys exactly 0; HF modeling_speecht5.py:930-955), formed by a separate kernel
        after each layer's attention launch -- ``layers * B * 12 * T^2 * 4`` bytes on the input's device (12 layers of 30 s x 8:
        10.3 GB); a range fallback re-run overwrites them with its own.  ``return_dict=False`` returns (last_hidden_state,
        hidden_states, attentions) without the Nones."""
        device = input_values.device
        self._begin(device, " (the reference calls it under model.eval() + torch.no_grad())")
        if self.range_policy not in ("fp32", "raise", "off"):
            raise ValueError("range_policy must be 'fp32', 'raise' or 'off'")
        x, m, T = self._prepare(input_values, attention_mask)
        B, L = x.shape
        with torch.cuda.device(device):
            self._sync_weights(device, T + 2)
            _lib.check(self._lib.loco_set_precision(self._handle, self.PRECISIONS[self.precision]), "set_precision")
            _lib.check(self._lib.loco_set_streams(self._handle, int(self.streams)), "set_streams")
            need = self._workspace_need(B, L)
            if self._workspace is None or self._workspace.numel() < need or self._workspace.device != device:
                self._workspace = None
                self._workspace = torch.empty(need, dtype=torch.uint8, device=device)
            out = torch.empty((B, T, HIDDEN), dtype=torch.float32, device=device)
            frames = torch.empty((B,), dtype=torch.int32, device=device)
            hs, hs_ptrs = None, None
            if output_hidden_states:
                hs = [torch.empty_like(out) for _ in range(self.num_layers + 1)]
                hs_ptrs = (C.c_void_p * (self.num_layers + 1))(*[t.data_ptr() for t in hs])
            attn = None
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            try:
                if output_attentions:
                    attn = bind_attention_outputs(self._lib, self._handle, self.num_layers, B, T, device)
                self.last_range_fallback = False
                self._forward_call((C.c_void_p(x.data_ptr()), C.c_void_p(m.data_ptr()) if m is not None else None, B, L,
                                    C.c_void_p(out.data_ptr()), C.c_void_p(frames.data_ptr()), hs_ptrs,
                                    C.c_void_p(self._workspace.data_ptr()), self._workspace.numel()), stream)
            finally:
                if attn is not None:
                    _lib.check(self._lib.loco_set_attention_outputs(self._handle, None, 0))
        self.last_frames = frames
        hidden = tuple(hs) if hs is not None else None
        if return_dict is False:
            return tuple(v for v in (out, hidden, attn) if v is not None)
        return BaseModelOutput(last_hidden_state=out, hidden_states=hidden, attentions=attn)

    # -- what a front end supplies -----------------------------------------------------------------------------
    def _weight_sources(self):
        """[(key prefix, module)]: every tensor of each module's state_dict goes to the handle under prefix + its name."""
        raise NotImplementedError

    def _load_tables(self, put, dirty: bool, min_rows: int):
        """``put(key, tensor)`` the tables that are no parameters: all of them when ``dirty`` (the other weights have just been
        loaded and are about to be finalised), otherwise only one that has to grow to ``min_rows`` rows."""
        raise NotImplementedError

    def _prepare(self, input_values, attention_mask):
        """Check the inputs of one forward; returns (x [B, L] as the library reads it, i32 mask [B, L] or None, output frames T)."""
        raise NotImplementedError

    def _workspace_need(self, B: int, L: int) -> int:
        raise NotImplementedError

    def _launch(self, slot, x, m, out, frames, precision, pack, hidden):
        """The asynchronous C call alone, on the slot's stream, workspace and status block."""
        raise NotImplementedError

    def _forward_call(self, args, stream):
        """The synchronous C call on ``args`` (input, mask, B, L, out, frames, hidden states, workspace, its size) under
        ``range_policy``, which ``forward`` has validated; sets ``last_range_fallback`` when it ran the batch again in fp32."""
        raise NotImplementedError


class SpeechT5EncoderWithSpeechPrenetMI355X(_EncoderBase):
    """Drop-in for ``SpeechT5ForSpeechToText(...).speecht5.encoder`` (HF modeling_speecht5.py:1325-1358)."""

    def __init__(self, layers: int = LAYERS, precision: str = "f16x3"):
        super().__init__(SpeechT5SpeechEncoderPrenetMI355X(_Ref()), layers, precision, streams=2)
        self._sin_rows = 0
        self._stage_taps = None  # the dict ``forward(stage_taps=)`` is filling, for the length of that call

    def _weight_sources(self):
        return [("prenet.", self.prenet), ("wrapped_encoder.", self.wrapped_encoder)] + list(self._extra_weights)

    def _load_tables(self, put, dirty, min_rows):
        if dirty:
            self._sin_rows = 0
        if self._sin_rows < min_rows:
            rows = max(MAX_SPEECH_POSITIONS + PAD_TOKEN_ID + 1 + 2, min_rows + 2)
            put("prenet.pos_sinusoidal_embed.weights", sinusoid_table(rows), "sinusoid table")
            self._sin_rows = rows
        if dirty and self._extra_weights:  # HF's decoder table, bit for bit (452 rows)
            put("decoder.prenet.embed_positions.weights", sinusoid_table(MAX_TEXT_POSITIONS + PAD_TOKEN_ID + 1), "decoder position table")

    def _prepare(self, input_values, attention_mask):
        if input_values.dim() != 2:
            raise ValueError(f"input_values must be [batch, samples], got {tuple(input_values.shape)}")
        x = input_values
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(torch.float32).contiguous()
        T = int(self._lib.loco_output_frames(x.shape[1]))
        if T < 1:
            raise ValueError(f"input of {x.shape[1]} samples is shorter than one encoder frame (400 samples)")
        m = None
        if attention_mask is not None:
            if attention_mask.shape != x.shape:
                raise ValueError(f"attention_mask {tuple(attention_mask.shape)} does not match input_values {tuple(x.shape)}")
            m = attention_mask.to(device=x.device, dtype=torch.int32).contiguous()
        return x, m, T

    def _workspace_need(self, B, L):
        return int(self._lib.loco_workspace_bytes(self._handle, B, L))

    def _launch(self, slot, x, m, out, frames, precision, pack, hidden):
        B, L = x.shape
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

    def _forward_call(self, args, stream):
        """loco_forward under the module's range policy (include/loco_asr.h, 'numeric range of precision mode f16x3'), with the
        stage taps of ``forward(stage_taps=)`` bound for its length."""
        taps = None
        if self._stage_taps is not None:
            B, T, dev = args[2], int(self._lib.loco_output_frames(args[3])), self._handle_device
            taps = dict(conv_stack=torch.empty((B, T, CONV_DIM), dtype=torch.float32, device=dev),
                        feature_projection=torch.empty((B, T, HIDDEN), dtype=torch.float32, device=dev),
                        prenet=torch.empty((B, T, HIDDEN), dtype=torch.float32, device=dev))
            _lib.check(self._lib.loco_set_taps(self._handle, taps["conv_stack"].data_ptr(),
                                               taps["feature_projection"].data_ptr(), taps["prenet"].data_ptr()))
        try:
            if self.range_policy == "off":
                _lib.check(self._lib.loco_forward(self._handle, *args, stream), "loco_forward")
            else:
                _lib.check(self._lib.loco_set_range_policy(self._handle, 1 if self.range_policy == "fp32" else 0), "set_range_policy")
                used = C.c_int32(0)
                _lib.check(self._lib.loco_forward_checked(self._handle, *args, stream, C.byref(used)), "loco_forward")
                self.last_range_fallback = bool(used.value)
        finally:
            if taps is not None:
                _lib.check(self._lib.loco_set_taps(self._handle, None, None, None))
        if taps is not None:
            self._stage_taps.update(taps)

    def forward(self, input_values: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                output_attentions: Optional[bool] = None, output_hidden_states: Optional[bool] = None,
                return_dict: Optional[bool] = None, stage_taps: Optional[dict] = None, **kwargs):
        """The shared forward; ``stage_taps``, a dict, is filled with the conv stack's output [B, T, 512], the feature projection and
        the prenet output [B, T, 768] and ``frames``."""
        self._stage_taps = stage_taps
        try:
            res = super().forward(input_values, attention_mask, output_attentions, output_hidden_states, return_dict)
        finally:
            self._stage_taps = None
        if stage_taps is not None:
            stage_taps["frames"] = self.last_frames
        return res

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
        device = self._device()
        self._begin_async(device)
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


def bind_attention_outputs(lib, handle, layers: int, B: int, T: int, device) -> tuple:
    """Allocate the per-layer [B, 12, T, T] fp32 probability tensors of output_attentions=True and bind them to the handle
    (loco_set_attention_outputs); the caller unbinds after the forward.  A zero-layer encoder binds nothing and returns ()."""
    probs = tuple(torch.empty((B, HEADS, T, T), dtype=torch.float32, device=device) for _ in range(layers))
    if layers:
        ptrs = (C.c_void_p * layers)(*[t.data_ptr() for t in probs])
        _lib.check(lib.loco_set_attention_outputs(handle, ptrs, layers), "loco_set_attention_outputs")
    return probs
