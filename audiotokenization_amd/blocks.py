"""Composite blocks of the BigCodec stacks (vq/module.py:74-167) and the fused data flow.

Every conv in the reference is preceded by an Activation1d (Snake).  The HIP path computes each
Snake once, in the epilogue of the kernel that PRODUCES its input; a producer whose raw output is
still needed (as a ResidualUnit skip input) writes both raw and activated tensors.  The flow is
expressed with producer functions that take

    want_raw : does any consumer still need the raw output?
    next_act : the Activation1d that consumes the output (None: raw output only)

and return (raw or None, activated or None).  Anti-aliased activations (bc_aa_snake_fwd) cannot be
an epilogue; they run as their own kernel on the raw output.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
from torch.nn import Parameter

from . import _lib as L
from . import ops
from .conv import WNConv1d, WNConvTranspose1d
from .modules import Activation1d, SnakeBeta, _DeviceCache, _as_input, _cpu, _pkey

__all__ = ["ResidualUnit", "EncoderBlock", "DecoderBlock", "LSTM", "ResLSTM", "Ragged"]

Flow = Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]


def _fusable(act: Optional[Activation1d]) -> bool:
    return act is not None and not act.antialias


def _conv_of(m):
    """The Conv1dWN behind a WNConv1d (CausalConv1d keeps it under `.conv`)."""
    return m.conv if hasattr(m, "conv") and not hasattr(m, "weight_v") else m


class Ragged:
    """Per-layer lengths of a ragged batch: clips of different lengths zero-padded into one (B, C, Tmax) batch.

    Every non-causal conv zero-pads at the clip's end, so the padded batch computes what each clip computes alone as
    long as every producer's output is exactly zero from the clip's own per-layer length to the padded end
    (DESIGN.md "Ragged batches"): snake(0) = 0 keeps an activated tail zero, the ResidualUnit's inner k = 1 conv is
    pointwise, the unidirectional LSTM never looks ahead and a transposed conv's first len * stride outputs read
    inputs below len only.  The producers that must be masked are therefore: the input, the first conv, every
    ResidualUnit, every strided and transposed conv, the ResLSTM (and the decoder's waveform).

    `chain` lists those producers in flow order as (kind, module), kind in "conv", "convT", "unit", "keep"
    (ragged_chain of the stacks); each row of the table is the lengths behind one of them, from the module's own
    out_len on the host.  The table is uploaded once (one int32 H2D copy, no synchronisation per layer) and mask()
    consumes the rows in order: one bc_zero_tail launch per producer (a dual raw + activated output shares it),
    none when no clip of the batch is shorter than the padded row."""

    def __init__(self, chain, lengths, T: int, what: str = "lengths"):
        lens = np.asarray([int(v) for v in lengths], dtype=np.int64).reshape(-1)
        if lens.size and int(lens.max()) > T:
            raise ValueError(f"{what}: clip {int(lens.argmax())} has length {int(lens.max())} > {T}, the batch's")
        self.rows, self.widths = [lens], [int(T)]
        for kind, m in chain:
            lens, T = self._step(kind, m, lens), int(self._step(kind, m, T))
            if T <= 0 or (lens.size and int(lens.min()) <= 0):
                b = int(lens.argmin()) if lens.size else 0
                raise ValueError(f"{what}: clip {b} ({int(self.rows[0][b]) if lens.size else T}) is too short for "
                                 f"this model (its B = 1 forward fails as well)")
            self.rows.append(lens)
            self.widths.append(T)
        self.i = 0
        self.table = None

    def upload(self, device) -> "Ragged":
        """The whole table to the device: the forward's one H2D copy."""
        self.table = torch.from_numpy(np.stack(self.rows).astype(np.int32)).to(device)
        return self

    @staticmethod
    def _step(kind, m, n):
        if kind == "unit":
            return _conv_of(m.block[3]).out_len(_conv_of(m.block[1]).out_len(n))
        return n if kind == "keep" else _conv_of(m).out_len(n)

    def mask(self, y, y2=None):
        """Zero the tails of the next producer's output(s) in place; returns (y, y2)."""
        i, self.i = self.i, self.i + 1
        t = y if y is not None else y2
        if i >= len(self.rows) or t.shape[-1] != self.widths[i] or t.shape[0] != self.rows[i].size:
            raise RuntimeError(f"ragged flow out of step with its length table at producer {i}: output "
                               f"{tuple(t.shape)}, expected width {self.widths[i] if i < len(self.widths) else None}")
        tail_max = self.widths[i] - int(self.rows[i].min())
        if tail_max > 0:
            a, b = (y, y2) if y is not None else (y2, None)
            ops.load().zero_tail_(a, b, self.table[i], tail_max)
        return y, y2

    def masked_input(self, x):
        """The batch with zeros past each clip's length, in a copy: the caller's tensor keeps its tail."""
        if self.widths[0] - int(self.rows[0].min()) > 0:
            x = x.clone()
        return self.mask(x)[0]


def _masked(rg: Optional[Ragged], out):
    """Zero the ragged tails of a producer's output: a tensor, or a (raw, activated) Flow pair."""
    if rg is None:
        return out
    if isinstance(out, tuple):
        return rg.mask(*out)
    return rg.mask(out)[0]


def produce_conv(conv, inp, residual=None, want_raw=True, next_act: Optional[Activation1d] = None,
                 epilogue: int = 0, rg: Optional[Ragged] = None) -> Flow:
    """Run `conv` on an already-activated input and hand its output to `next_act`'s consumer."""
    if next_act is None:
        return _masked(rg, conv.run(inp, residual, epilogue)), None
    if _fusable(next_act):
        co = next_act.act.coeffs(inp.device)
        if want_raw:
            y, ya = conv.run(inp, residual, epilogue, out_snake=co, dual=True)
            return _masked(rg, (y, ya))
        return None, _masked(rg, conv.run(inp, residual, epilogue, out_snake=co))
    y = _masked(rg, conv.run(inp, residual, epilogue))
    return y, next_act(y)


def produce_convT(conv, inp, want_raw=True, next_act: Optional[Activation1d] = None,
                  rg: Optional[Ragged] = None) -> Flow:
    if next_act is None:
        return _masked(rg, conv.run(inp)), None
    if _fusable(next_act):
        co = next_act.act.coeffs(inp.device)
        if want_raw:
            return _masked(rg, conv.run(inp, out_snake=co, dual=True))
        return None, _masked(rg, conv.run(inp, out_snake=co))
    y = _masked(rg, conv.run(inp))
    return y, next_act(y)


class ResidualUnit(nn.Module):
    """vq/module.py:74-89: x + conv1(act2(conv7_d(act1(x)))).  Two launches: conv7 (epilogue =
    act2), conv1 (epilogue = skip add [+ the next block's Snake])."""

    def __init__(self, dim: int = 16, dilation: int = 1, causal: bool = False, antialias: bool = False):
        super().__init__()
        pad = 0 if causal else ((7 - 1) * dilation) // 2
        self.block = nn.Sequential(
            Activation1d(activation=SnakeBeta(dim, alpha_logscale=True), antialias=antialias),
            WNConv1d(dim, dim, kernel_size=7, dilation=dilation, padding=pad, causal=causal),
            Activation1d(activation=SnakeBeta(dim, alpha_logscale=True), antialias=antialias),
            WNConv1d(dim, dim, kernel_size=1),
        )

    @property
    def first_act(self) -> Activation1d:
        return self.block[0]

    def _fused_cfg(self):
        """cfg of the one-launch unit (bc_resunit_fwd), or -1 (x6 / bf16 / h3 mode, no anti-aliasing, C fits)."""
        mode = L.precision_mode()
        if mode not in (1, 2, 3) or self.block[2].antialias:
            return -1
        conv7 = _conv_of(self.block[1])
        return L.load().bc_resunit_select_cfg(conv7.in_channels, conv7.dilation, mode)

    def snake_on_load(self) -> bool:
        """True when the one-launch kernel applies the first Snake while staging its input
        (bc_resunit_fwd_snake_in): the producer then writes the raw tensor only (x_act=None).
        BIGCODEC_RU_SNAKE_IN=0 restores producer-side activation (dual raw + activated outputs)."""
        if not _fusable(self.first_act) or os.environ.get("BIGCODEC_RU_SNAKE_IN", "1") == "0":
            return False
        return self._fused_cfg() >= 0

    def flow(self, x_raw, x_act, want_raw=True, next_act=None, rg: Optional[Ragged] = None) -> Flow:
        """x_act = self.first_act(x_raw) computed by the producer, or None (snake_on_load).  rg: the unit's OUTPUT
        gets the ragged batch's zero tails (the inner k = 1 conv is pointwise: the k = 7 conv's output needs none)."""
        if next_act is None or _fusable(next_act):
            cfg = self._fused_cfg()
            if cfg >= 0:
                return _masked(rg, self._flow_fused(cfg, x_raw, x_act, want_raw, next_act))
        if x_act is None:
            x_act = self.first_act(x_raw)
        _, h = produce_conv(self.block[1], x_act, None, want_raw=False, next_act=self.block[2])
        return produce_conv(self.block[3], h, residual=x_raw, want_raw=want_raw, next_act=next_act, rg=rg)

    def _flow_fused(self, cfg, x_raw, x_act, want_raw, next_act) -> Flow:
        conv7, conv1 = _conv_of(self.block[1]), _conv_of(self.block[3])
        lazy = x_act is None and _fusable(self.first_act)
        if x_act is None and not lazy:
            x_act = self.first_act(x_raw)
        dev = x_raw.device
        w7, b7 = conv7.packed_as(cfg, dev)
        w1, b1 = conv1.packed_as(cfg, dev)
        s2a, s2b = self.block[2].act.coeffs(dev)
        B, C, T = x_raw.shape
        if not lazy and x_raw.shape != x_act.shape:
            raise ValueError("ResidualUnit: raw and activated inputs differ in shape")
        sa, sb = next_act.act.coeffs(dev) if next_act is not None else (None, None)
        dual = next_act is not None and want_raw
        tm = L.active_timer()
        ev = tm.begin() if tm is not None else None
        s1a, s1b = self.first_act.act.coeffs(dev) if lazy else (None, None)
        out = ops.load().resunit(x_raw, None if lazy else x_act, s1a, s1b, w7, b7, s2a, s2b, w1, b1, sa, sb,
                                 conv7.dilation, conv7.pad_left(), cfg, dual)
        y, y2 = out[0], (out[1] if dual else None)
        if tm is not None:
            flops = 2.0 * B * C * C * T * 8  # k=7 and k=1
            nbytes = 4.0 * x_raw.numel() * ((2 if lazy else 3) + dual)
            tm.end(ev, L.resunit_kernel_name(cfg, C, conv7.dilation), flops, nbytes)
        if next_act is None:
            return y, None
        if dual:
            return y, y2
        return None, y

    def forward(self, x):
        x = _as_input(x)
        return self.flow(x, None if self.snake_on_load() else self.first_act(x))[0]


def input_act(stage) -> Optional[Activation1d]:
    """The activation a producer must apply for `stage` (a ResidualUnit / Encoder- / DecoderBlock);
    None when the stage's first ResidualUnit activates on load (raw output only)."""
    first = stage if isinstance(stage, ResidualUnit) else stage.block[0]
    if isinstance(first, ResidualUnit) and first.snake_on_load():
        return None
    return stage.first_act


class EncoderBlock(nn.Module):
    """vq/module.py:91-113: ResidualUnits -> Activation1d -> strided conv (k=2s) C/2 -> C."""

    def __init__(self, dim: int = 16, stride: int = 1, dilations=(1, 3, 9), causal: bool = False,
                 antialias: bool = False):
        super().__init__()
        runits = [ResidualUnit(dim // 2, dilation=d, causal=causal, antialias=antialias) for d in dilations]
        pad = 0 if causal else (stride // 2 + stride % 2 if stride != 1 else 0)
        self.block = nn.Sequential(
            *runits,
            Activation1d(activation=SnakeBeta(dim // 2, alpha_logscale=True), antialias=antialias),
            WNConv1d(dim // 2, dim, kernel_size=2 * stride if stride != 1 else 1, stride=stride, padding=pad,
                     causal=causal),
        )

    @property
    def first_act(self) -> Activation1d:
        return self.block[0].first_act

    def ragged_chain(self):
        """The block's masked producers in flow order (Ragged)."""
        n = len(self.block)
        return [("unit", self.block[i]) for i in range(n - 2)] + [("conv", self.block[n - 1])]

    def flow(self, x_raw, x_act, want_raw=True, next_act=None, rg: Optional[Ragged] = None) -> Flow:
        n = len(self.block)
        rus = [self.block[i] for i in range(n - 2)]
        for i, ru in enumerate(rus):
            last = i == len(rus) - 1
            nxt = self.block[n - 2] if last else input_act(rus[i + 1])
            x_raw, x_act = ru.flow(x_raw, x_act, want_raw=not last, next_act=nxt, rg=rg)
        return produce_conv(self.block[n - 1], x_act, None, want_raw=want_raw, next_act=next_act, rg=rg)

    def forward(self, x):
        x = _as_input(x)
        return self.flow(x, None if input_act(self) is None else self.first_act(x))[0]


class DecoderBlock(nn.Module):
    """vq/module.py:115-141: Activation1d -> transposed conv (k=2s) -> ResidualUnits."""

    def __init__(self, input_dim: int = 16, output_dim: int = 8, stride: int = 1, dilations=(1, 3, 9),
                 causal: bool = False, antialias: bool = False):
        super().__init__()
        if causal:
            tconv_kwargs = {}
        else:
            tconv_kwargs = {"padding": stride // 2 + stride % 2 if stride != 1 else 0,
                            "output_padding": stride % 2 if stride != 1 else 0}
        self.block = nn.Sequential(
            Activation1d(activation=SnakeBeta(input_dim, alpha_logscale=True), antialias=antialias),
            WNConvTranspose1d(input_dim, output_dim, kernel_size=2 * stride if stride != 1 else 1, stride=stride,
                              causal=causal, **tconv_kwargs),
        )
        self.block.extend([ResidualUnit(output_dim, dilation=d, causal=causal, antialias=antialias)
                           for d in dilations])

    @property
    def first_act(self) -> Activation1d:
        return self.block[0]

    def ragged_chain(self):
        """The block's masked producers in flow order (Ragged)."""
        return [("convT", self.block[1])] + [("unit", self.block[i]) for i in range(2, len(self.block))]

    def flow(self, x_raw, x_act, want_raw=True, next_act=None, rg: Optional[Ragged] = None) -> Flow:
        rus = [self.block[i] for i in range(2, len(self.block))]
        y_raw, y_act = produce_convT(self.block[1], x_act, want_raw=True,
                                     next_act=input_act(rus[0]) if rus else next_act, rg=rg)
        for i, ru in enumerate(rus):
            last = i == len(rus) - 1
            y_raw, y_act = ru.flow(y_raw, y_act, want_raw=(want_raw if last else True),
                                   next_act=next_act if last else input_act(rus[i + 1]), rg=rg)
        return y_raw, y_act

    def forward(self, x):
        x = _as_input(x)
        return self.flow(x, self.first_act(x))[0]


class LSTM(nn.Module):
    """Parameter container with torch.nn.LSTM's names (weight_ih_l{k}, weight_hh_l{k}, bias_ih_l{k},
    bias_hh_l{k}; batch_first) so reference checkpoints load; the recurrence runs in
    bc_reslstm_fwd."""

    def __init__(self, input_size, hidden_size, num_layers=1, bias=True, batch_first=True, dropout=0.0,
                 bidirectional=False):
        super().__init__()
        if not bias or not batch_first or dropout:
            raise NotImplementedError("only bias=True, batch_first=True, dropout=0")
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        self.batch_first, self.bidirectional = batch_first, bidirectional
        ref = nn.LSTM(input_size, hidden_size, num_layers, batch_first=True,
                      bidirectional=bidirectional)  # torch's default init and parameter names
        for name, p in ref.named_parameters():
            setattr(self, name, Parameter(p.detach().clone()))
        self._cache = _DeviceCache()

    def _suffixes(self):
        return ("", "_reverse") if self.bidirectional else ("",)

    def _plist(self):
        out = []
        for l in range(self.num_layers):
            for sfx in self._suffixes():
                out += [getattr(self, f"weight_ih_l{l}{sfx}"), getattr(self, f"weight_hh_l{l}{sfx}"),
                        getattr(self, f"bias_ih_l{l}{sfx}"), getattr(self, f"bias_hh_l{l}{sfx}")]
        return out

    def prepared(self, device):
        """Packed per-layer weights; bidirectional: [forward, backward] per layer (bc_reslstm_bidir_fwd)."""
        def build():
            lib = L.load()
            H = self.hidden_size
            # unidirectional: the residual needs input == hidden; bidirectional: every layer reads the
            # 2H-channel concatenation, so the module input must be 2H as well
            Cin = 2 * H if self.bidirectional else H
            if self.input_size != Cin:
                raise NotImplementedError("ResLSTM requires input_size == hidden_size (x2 when bidirectional)")
            mode = L.lstm_mode()
            cfg = L.conv_cfg(4 * H, Cin, 1, 1, 1, mode)
            wih, whh, bias = [], [], []
            for l in range(self.num_layers):
                for sfx in self._suffixes():
                    w = _cpu(getattr(self, f"weight_ih_l{l}{sfx}")).contiguous()
                    packed = np.empty(L.checked_size(lib.bc_conv1d_packed_floats(4 * H, Cin, 1, cfg),
                                                     "bc_conv1d_packed_floats"), dtype=np.float32)
                    L.call("bc_conv1d_pack", w.numpy().ctypes.data, packed.ctypes.data, 4 * H, Cin, 1, cfg)
                    wih.append(torch.from_numpy(packed).to(device))
                    w = _cpu(getattr(self, f"weight_hh_l{l}{sfx}")).contiguous()
                    packed = np.empty(L.checked_size(lib.bc_lstm_hh_packed_floats(H, mode), "bc_lstm_hh_packed_floats"),
                                      dtype=np.float32)
                    L.call("bc_lstm_pack_hh", w.numpy().ctypes.data, packed.ctypes.data, H, mode)
                    whh.append(torch.from_numpy(packed).to(device))
                    b = _cpu(getattr(self, f"bias_ih_l{l}{sfx}")) + _cpu(getattr(self, f"bias_hh_l{l}{sfx}"))
                    bias.append(b.contiguous().to(device))
            arrs = (L.ptr_array([t.data_ptr() for t in wih]), L.ptr_array([t.data_ptr() for t in bias]),
                    L.ptr_array([t.data_ptr() for t in whh]))
            return (wih, whh, bias), arrs
        return self._cache.get(_pkey(*self._plist()) + (str(device), L.lstm_mode()), build)


class ResLSTM(nn.Module):
    """vq/module.py:143-167: y = LSTM(x^T)^T + x for x (B, F, T)."""

    def __init__(self, dimension: int, num_layers: int = 2, bidirectional: bool = False, skip: bool = True):
        super().__init__()
        if not skip:
            raise NotImplementedError("ResLSTM(skip=False) is not used by the reference models")
        self.skip = skip
        self.lstm = LSTM(dimension, dimension if not bidirectional else dimension // 2, num_layers,
                         batch_first=True, bidirectional=bidirectional)

    def run(self, x, out_snake=None, state=None, return_state: bool = False, lens=None):
        """y = LSTM(x^T)^T + x (then the next Snake when out_snake = (alpha_exp, inv_beta)).  Streaming:
        state = (h0, c0) [num_layers][H][B] device tensors or None (zeros); with return_state the call
        returns (y, (h_n, c_n)) in the same layout (nn.LSTM's final state, unit-major).  lens: an int32 device
        tensor (B,) of steps per clip (bc_reslstm_fwd_state_lens): (h_n, c_n) are then each clip's state after its own
        lens[b] steps, y still holds all T steps; the call returns (y, (h_n, c_n))."""
        x = _as_input(x)
        B, H, T = x.shape
        (wih, whh, bias), _ = self.lstm.prepared(x.device)
        sa, sb = out_snake if out_snake is not None else (None, None)
        if self.lstm.bidirectional:
            if state is not None or return_state or lens is not None:
                raise NotImplementedError("carried state (streaming) needs a unidirectional ResLSTM")
            out = ops.load().reslstm_bidir(x, wih, bias, whh, sa, sb, L.precision_mode())
            L.defer_status(out[1], f"ResLSTM(D={H}, layers={self.lstm.num_layers}, bidirectional, T={T})")
            return out[0]
        h0, c0 = state if state is not None else (None, None)
        if lens is not None:
            out = ops.load().reslstm_lens(x, wih, bias, whh, sa, sb, L.precision_mode(), h0, c0, lens)
            return_state = True
        else:
            out = ops.load().reslstm(x, wih, bias, whh, sa, sb, L.precision_mode(), h0, c0, return_state)
        # include/bigcodec.h: out[1] = the call's count of persistent workgroups that timed out; the
        # codec's forward checks it (L.check_status) before its output can be consumed
        L.defer_status(out[1], f"ResLSTM(H={H}, layers={self.lstm.num_layers}, T={T})")
        if return_state:
            return out[0], (out[2], out[3])
        return out[0]

    def flow(self, x_raw, want_raw=True, next_act=None, rg: Optional[Ragged] = None) -> Flow:
        """rg: a ragged batch.  The forward recurrence never looks ahead, so a clip's own steps are the per-clip ones;
        the steps past its end (the LSTM running on over zeros) get the zero tail."""
        if rg is not None and self.lstm.bidirectional:
            raise NotImplementedError("a ragged batch needs a unidirectional ResLSTM: the reverse direction would "
                                      "have to start at each clip's own end")
        if next_act is None:
            return _masked(rg, self.run(x_raw)), None
        if _fusable(next_act) and not want_raw:
            return None, _masked(rg, self.run(x_raw, out_snake=next_act.act.coeffs(x_raw.device)))
        y = _masked(rg, self.run(x_raw))
        return y, next_act(y)

    def forward(self, x):
        with L.status_scope():
            y = self.run(x)
            L.check_status()
        return y
