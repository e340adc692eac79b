"""Causal streaming encode and decode: a causal BigCodecEncoder (causal=True,
vq/module.py:11-48 CausalConv1d, left padding (K - stride) * dilation) fed chunk by chunk, with the
state a chunk boundary cuts carried on the device:

  * every causal conv keeps the last (K - stride) * dilation samples of its (activated) input and runs
    the next chunk over [context | chunk] with no padding, so each output sample sees exactly the
    inputs it sees in a whole-sequence pass;
  * the ResLSTM carries nn.LSTM's (h, c) per layer through bc_reslstm_fwd_state (the persistent kernel
    starts from the carried state and hands back the final one).

The reference has no streaming mode; its whole-sequence causal encoder defines the result: the
concatenation of the chunks' latents equals the encoder's output on the concatenated audio (bit for
bit in the exact-split x6 precision; in h3 the per-tile block scales differ between the two tilings, so
the outputs agree to fp32 rounding).  Chunks must be a multiple of the hop (prod(up_ratios)) samples.
Anti-aliased activations are not causal (act.py / resample.py look ahead), so antialias=True is refused.
The carried contexts live on the device and every step of the state is one bc_stream_window launch: it writes the
[context | chunk] window (with the stage's Snake applied on the way) and the next context in one pass.  A
ResidualUnit the one-launch kernel serves (bc_resunit_fwd_snake_in: C = 48 / 96 in h3, x6, bf16) runs as ONE
launch over its raw window with its own causal padding: output column P + t sees window columns t … P + t, all
real samples, and its residual is the window's own column P + t; the first P = 6d outputs are dropped by taking the
view [P:] (no copy: the next window reads the strided view).  Other units run conv7 (Snake epilogue) and conv1
(residual add) over their activated window.  No torch compute kernel runs in a push.

StreamingDecoder is the same for a causal BigCodecDecoder (vq/codec_decoder.py:15-94 with causal=True): latent
frames in, waveform out.  Its upsamplers are CausalConvTranspose1d (vq/module.py:50-57: ConvTranspose1d with
k = 2s, stride s, no padding, the last s outputs cropped), so output block t depends on input frames t and t - 1:
each carries its last input frame and runs the chunk over [frame | chunk] with padding s (which drops the s
outputs of the carried frame's own block on the left and the k - s look-ahead outputs on the right).

StreamPool serves many independent sessions, which open, close and skip ticks on their own, with one
batched push: the same stages on a batch of whichever sessions are live, the carried state in per-stage pools on the
device and indexed by slot (bc_stream_window_slots, bc_lstm_state_gather / bc_lstm_state_scatter).  Sessions in one
push may deliver different numbers of hops (`hops=`): the rows are left-aligned in a padded batch, every
window zeroes the columns past its entry's own length (bc_stream_window_slots_lens) and the persistent ResLSTM hands
back its state at each entry's own last step (bc_reslstm_fwd_state_lens).

LookaheadEncoder / LookaheadDecoder stream the NON-causal models (`default`, `base`) as well: a conv with
symmetric padding is a causal conv whose output arrives late, so every stage runs as a lazy valid conv over [carry | new]
(bc_stream_window_la), emits what is final and holds the rest; finish() flushes each layer's own right zero padding.  The
result equals the whole-sequence forward after a fixed look-ahead (lookahead_samples: 2451 samples for `default`).  The
classes above keep refusing non-causal models.

LookaheadPool is StreamPool for those models: every stage's window is left-aligned and ragged per
session (bc_stream_window_slots_la: a carry length, a new length, an input offset and a stored carry per entry), so
sessions in their transient, in steady state and at their flush share one batched push.

One walk of the model (_walk) gives every class above its stages, and the five bc_stream_window* calls are one kernel
(csrc/elementwise.hip window_kernel).  The two pools share their host side (_PoolHost): the slot table, the refusals of
a push, the pinned staging of its index arrays, and the marking of its sessions when it fails.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional

import torch

from . import _lib
from . import ops
from .blocks import DecoderBlock, EncoderBlock, ResLSTM, _conv_of
from .conv import CausalConvTranspose1d, ConvTranspose1dWN
from .modules import _as_input


def _refuse_global_attention(model) -> None:
    """The Conformer-STFT family attends over the whole clip (and its causal variant over the whole past): no bounded
    state to carry, so no streaming class takes it."""
    from .conformer import SelfAttention

    if any(isinstance(m, SelfAttention) for m in model.modules()):
        raise NotImplementedError("the Conformer-STFT family attends over the whole clip: streaming is not built for it")


class StreamingEncoder:
    """Wraps a causal BigCodecEncoder; `push(x (B, 1, n))` returns the latents (B, D, n / hop) of the
    chunk.  `reset()` starts a new stream.  The batch size is fixed per stream."""

    _in_samples = True  # a push takes samples (a multiple of the hop); the decoder's takes frames

    def __init__(self, encoder):
        _refuse_global_attention(encoder)
        convs = [m for m in encoder.modules() if hasattr(m, "causal_pad")]
        # every conv that looks at more than one input sample must be causal (the ResidualUnits' k=1
        # convs are plain, padding 0, in the reference too)
        if not convs or any(m.causal_pad is None and (m.kernel_size > 1 or m.padding) for m in convs):
            raise ValueError("streaming needs a causal encoder (causal=True)")
        if any(getattr(m, "antialias", False) for m in encoder.modules()):
            raise NotImplementedError("anti-aliased activations look ahead: not streamable")
        self.encoder = encoder
        self.hop = int(encoder.hop_length)
        self.stages = _walk(encoder)
        self.reset()

    def reset(self):
        self._ctx: Dict[int, torch.Tensor] = {}
        self._lstm: Dict[int, tuple] = {}
        self.samples = 0
        # the precision the carried state belongs to: the fused and the two-launch ResidualUnit paths keep different
        # context (raw input vs activated input), and which one runs depends on the mode
        self._mode = _lib.precision_mode()

    def _check_mode(self):
        if _lib.precision_mode() != self._mode:
            raise RuntimeError(f"precision changed mid-stream ({self._mode} -> {_lib.precision_mode()}): the carried "
                               "context belongs to the old mode; reset() the stream first")

    def _window(self, key, x, P: int, act=None):
        """[carried context | x] (B, C, P + n), `act` (a Snake Activation1d or None) applied to x, as the input of a
        stage with P columns of causal history; the last P columns become the next chunk's context."""
        sa, sb = act.act.coeffs(x.device) if act is not None else (None, None)
        win, nctx = ops.load().stream_window(x, self._ctx.get(key) if P else None, sa, sb, P)
        if P:
            self._ctx[key] = nctx
        return win

    def _conv(self, wrapper, x, act=None, residual=None, out_snake=None, epilogue: int = 0):
        """A causal conv over [context | act(x)] with no padding: exactly the chunk's outputs."""
        c = _conv_of(wrapper)
        P = c.pad_left()
        if P == 0 and act is None and x.is_contiguous():
            return c.run(x, residual, epilogue, out_snake)
        return c.run(self._window(id(c), x, P, act), residual, epilogue, out_snake, pad_left=0)

    def _dense(self, h):
        """A contiguous copy of a strided chunk view (one launch), for the ops that take dense tensors."""
        return h if h.is_contiguous() else self._window(None, h, 0)

    def _unit(self, ru, h):
        """One ResidualUnit on a chunk: x + conv1(act2(conv7(act1(x)))) (vq/module.py:74-89)."""
        cfg = ru._fused_cfg()
        conv7 = _conv_of(ru.block[1])
        if cfg >= 0 and ru.snake_on_load():
            P = conv7.pad_left()  # 6d: the unit's whole history
            win = self._window(("ru", id(ru)), h, P)
            y = ru._flow_fused(cfg, win, None, True, None)[0]
            return y[:, :, P:]
        t = self._conv(ru.block[1], h, act=ru.block[0], out_snake=ru.block[2].act.coeffs(h.device))
        return self._conv(ru.block[3], t, residual=self._dense(h))

    def _lstm_run(self, m: ResLSTM, h):
        y, state = m.run(h, state=self._lstm.get(id(m)), return_state=True)
        self._lstm[id(m)] = state
        return y

    def push(self, x) -> torch.Tensor:
        self._check_mode()
        with _lib.status_scope():
            return self._push(x)

    def _push(self, x) -> torch.Tensor:
        """One chunk through the model's stages (_walk: the order the look-ahead classes run too)."""
        h = x = _as_input(x)
        if self._in_samples and x.shape[-1] % self.hop:
            raise ValueError(f"chunk of {x.shape[-1]} samples: must be a multiple of the hop ({self.hop})")
        for st in self.stages:
            if st.kind == "conv":
                h = self._conv(st.module, h, act=st.act, epilogue=st.epilogue)
            elif st.kind == "unit":
                h = self._unit(st.module, h)
            elif st.kind == "lstm":
                h = self._lstm_run(st.module, h)
            else:
                h = self._convT(st.module, h, st.act)
        self.samples += x.shape[-1] * (1 if self._in_samples else self.hop)
        _lib.check_status()
        return h

    def graph(self, example) -> "StreamGraph":
        """This stream's push for chunks shaped like `example`, captured once in a HIP graph (StreamGraph)."""
        return StreamGraph(self, example)

    def encode(self, x, chunk: int) -> torch.Tensor:
        """Whole input through `push` in chunks of `chunk` samples (the last may be shorter)."""
        self.reset()
        outs = [self.push(x[..., i:i + chunk]) for i in range(0, x.shape[-1], chunk)]
        return torch.cat(outs, dim=2)


class StreamingDecoder(StreamingEncoder):
    """Wraps a causal BigCodecDecoder; `push(z (B, D, n))` (post-VQ embeddings, n frames) returns the waveform
    (B, 1, n * hop) of the chunk, equal to the whole-sequence causal decode of the concatenated frames.
    `tokens(codes (B, n, Nq) int64 device)` pushes a chunk of index frames (vq2emb first, codec_decoder.py:96-99).
    The carried state: every causal conv's input context, every upsampler's last input frame, the ResLSTM's
    (h, c)."""

    _in_samples = False

    def __init__(self, decoder):
        _refuse_global_attention(decoder)
        convs = [m for m in decoder.modules() if hasattr(m, "causal_pad")]
        if not convs or any(m.causal_pad is None and (m.kernel_size > 1 or m.padding) for m in convs):
            raise ValueError("streaming needs a causal decoder (causal=True)")
        if any(isinstance(m, ConvTranspose1dWN) and not m.causal_crop for m in decoder.modules()):
            raise ValueError("streaming needs a causal decoder (causal=True): its upsamplers must be causal")
        if any(getattr(m, "antialias", False) for m in decoder.modules()):
            raise NotImplementedError("anti-aliased activations look ahead: not streamable")
        self.decoder = decoder
        self.hop = int(decoder.hop_length)
        self.stages = _walk(decoder)
        self.reset()

    def _convT(self, conv, h, act):
        s, K = conv.stride, conv.kernel_size
        c = K // s - 1  # input frames of history an output block needs (_convT_stage: K % s == 0)
        x = self._window(id(conv), h, c, act)
        phases, _, bias, cfg = conv.prepared(x.device, conv.phase_cfg(x.shape[0], x.shape[-1]))
        # full length (n + c - 1) s + K; padding c * s crops c * s on both sides: the n * s outputs of this chunk
        out = ops.load().conv_transpose1d(x, phases, bias, None, None, conv.out_channels, h.shape[-1] * s, K, s, c * s,
                                          cfg, False)
        return out[0]

    def tokens(self, codes) -> torch.Tensor:
        """codes (B, n, Nq) int64 on the device -> waveform chunk (B, 1, n * hop)."""
        return self.push(self.decoder.tokens_to_latent(codes))

    def decode(self, z, chunk: int) -> torch.Tensor:
        """Whole latent sequence through `push` in chunks of `chunk` frames (the last may be shorter)."""
        self.reset()
        outs = [self.push(z[..., i:i + chunk]) for i in range(0, z.shape[-1], chunk)]
        return torch.cat(outs, dim=2)


# ---- look-ahead streaming: non-causal models as exact streams with a fixed algorithmic delay ----------
#
# The whole-sequence forward defines the result: each layer zero-pads its own input at both of its own ends.  A conv with
# symmetric padding is a causal conv whose output arrives late, so every stage runs as a LAZY VALID CONV: it holds a
# carry of the input columns it has not finished with (at the stream's start: its left padding, as zeros), forms
# [carry | new], emits the outputs whose whole receptive field is there and keeps the rest; the flush appends the layer's
# own right zero padding and emits what is left.  All of the arithmetic lives in _stage_row; lookahead_plan tabulates
# it and the classes execute the same rows.

class _Stage:
    """One lazy stage: kind "conv" (a Conv1dWN behind `act`), "unit" (a ResidualUnit: a k = 7 lazy conv over the raw
    input), "lstm" (carried state, no geometry) or "convT" (a transposed conv behind `act`).  k, s, d, pl, pr: kernel,
    stride, dilation and the layer's own left / right zero padding; hist: input frames of history a transposed conv's
    output block needs."""

    def __init__(self, kind, module, act=None, k=1, s=1, d=1, pl=0, pr=0, hist=0, epilogue=0):
        self.kind, self.module, self.act, self.epilogue = kind, module, act, epilogue
        self.k, self.s, self.d, self.pl, self.pr, self.hist = k, s, d, pl, pr, hist

    def start(self):
        """(carry, seen, emitted) at the stream's start: the left padding as carried zeros."""
        return (self.pl if self.kind in ("conv", "unit") else 0, 0, 0)


def _conv_stage(wrapper, act=None, epilogue=0, kind="conv"):
    c = _conv_of(wrapper)
    return _Stage(kind, c, act, c.kernel_size, c.stride, c.dilation, c.pad_left(),
                  0 if c.causal_pad is not None else c.padding, epilogue=epilogue)


def _convT_stage(wrapper, act):
    conv = wrapper.conv if isinstance(wrapper, CausalConvTranspose1d) else wrapper
    if conv.kernel_size % conv.stride:
        raise NotImplementedError(f"streaming transposed conv needs kernel_size % stride == 0 (k={conv.kernel_size}, "
                                  f"s={conv.stride})")
    return _Stage("convT", conv, act, conv.kernel_size, conv.stride, 1, conv.padding, 0,
                  hist=conv.kernel_size // conv.stride - 1)


def _unit_stage(ru):
    st = _conv_stage(ru.block[1], kind="unit")
    st.module = ru
    return st


def _walk(model):
    """The stages of a BigCodecEncoder / BigCodecDecoder in flow order: one per producer of the model's own per-layer
    length table (frame_lengths / sample_lengths with per_layer=True, rows 1 on).  The one walk of the model: every
    streaming class runs this list."""
    stages = []
    if hasattr(model, "tokens_to_latent"):
        m = list(model.model)
        stages.append(_conv_stage(m[0]))
        for st in m[1:-3]:
            if isinstance(st, ResLSTM):
                stages.append(_Stage("lstm", st))
            elif isinstance(st, DecoderBlock):
                sub = list(st.block)
                stages.append(_convT_stage(sub[1], sub[0]))
                stages += [_unit_stage(ru) for ru in sub[2:]]
            else:
                raise NotImplementedError(f"unexpected decoder stage {type(st).__name__}")
        stages.append(_conv_stage(m[-2], m[-3], epilogue=1))  # the decoder's nn.Tanh in the epilogue
    else:
        blk = list(model.block)
        stages.append(_conv_stage(blk[0]))
        for st in blk[1:-2]:
            if isinstance(st, EncoderBlock):
                sub = list(st.block)
                stages += [_unit_stage(ru) for ru in sub[:-2]]
                stages.append(_conv_stage(sub[-1], sub[-2]))
            elif isinstance(st, ResLSTM):
                stages.append(_Stage("lstm", st))
            else:
                raise NotImplementedError(f"unexpected encoder stage {type(st).__name__}")
        stages.append(_conv_stage(blk[-1], blk[-2]))
    return stages


def lookahead_stages(model):
    """The lazy stages of a model (_walk).  Refuses what looks ahead without bound: anti-aliased activations, a
    bidirectional ResLSTM and the Conformer-STFT family."""
    _refuse_global_attention(model)
    if any(getattr(m, "antialias", False) for m in model.modules()):
        raise NotImplementedError("anti-aliased activations replicate-pad at the clip's end: not streamable")
    if any(isinstance(m, ResLSTM) and m.lstm.bidirectional for m in model.modules()):
        raise NotImplementedError("a bidirectional ResLSTM reads the whole clip backwards: not streamable")
    return _walk(model)


def _stage_row(st: _Stage, state, new: int, flush: bool):
    """One push of one stage: ((carry_in, new, right_zeros, outputs, carry_out), next state).  state = (carry, seen,
    emitted): the carried input columns, and for a transposed conv the frames seen and the outputs emitted so far."""
    carry, seen, emitted = state
    if st.kind == "lstm":
        return (0, new, 0, new, 0), (0, seen + new, emitted + new)
    if st.kind == "convT":
        # N frames seen: output o reads frames <= (o + p) // s, so o < N * s - p is final; the flush emits the rest
        N = seen + new
        total = st.module.out_len(N) if N > 0 else 0
        upto = total if flush else min(max(0, N * st.s - st.pl), total)
        keep = 0 if flush else min(st.hist, carry + new)
        return (carry, new, 0, upto - emitted, keep), (keep, N, upto)
    R = st.pr if flush else 0
    span, have = (st.k - 1) * st.d, carry + new + R
    out = 0 if have <= span else (have - span - 1) // st.s + 1
    keep = 0 if flush else have - out * st.s  # the suffix from column out * s on
    return (carry, new, R, out, keep), (keep, seen + new, emitted + out)


def _plan_push(stages, states, n: int, flush: bool):
    """One push of n input columns through every stage: (rows, next states)."""
    rows, nxt = [], []
    for st, state in zip(stages, states):
        row, state = _stage_row(st, state, n, flush)
        rows.append(row)
        nxt.append(state)
        n = row[3]
    return rows, nxt


def lookahead_plan_stages(stages, chunks, last: int = 0):
    """lookahead_plan for a list of stages."""
    states = [st.start() for st in stages]
    plan = []
    for i, n in enumerate(list(chunks) + [last]):
        rows, states = _plan_push(stages, states, int(n), i == len(chunks))
        plan.append(rows)
    return plan


def lookahead_plan(model, chunks, last: int = 0):
    """What a look-ahead stream of `model` does with pushes of `chunks` input columns (samples for an encoder, frames
    for a decoder) and a finish() with `last` more: plan[i][j] = (carry_in, new, right_zeros, outputs, carry_out) of
    stage j (lookahead_stages order) in push i; the last entry is the flush.  Pure host arithmetic; LookaheadEncoder /
    LookaheadDecoder execute these rows."""
    return lookahead_plan_stages(lookahead_stages(model), chunks, last)


def lookahead_samples(model) -> int:
    """The algorithmic look-ahead in samples: how far beyond its own position (a frame's own hop of samples; a sample
    itself) output 0 reads, summed over the stages at their rates.  A conv reaches (k - 1) d - pad_left - (s - 1)
    columns to the right of its output's own s input columns, at its input's rate; a transposed conv with padding p
    reads frames <= (o + p) // s for output o, p columns ahead at its OUTPUT's rate.  An encoder's frame 0 is final once
    look-ahead + hop samples are in, a decoder's sample 0 once look-ahead // hop + 1 frames are.  0 for a causal model."""
    stages = lookahead_stages(model)
    decoder = hasattr(model, "tokens_to_latent")
    rate, total = (int(model.hop_length) if decoder else 1), 0
    for st in stages:
        if st.kind in ("conv", "unit"):
            total += ((st.k - 1) * st.d - st.pl - (st.s - 1)) * rate
            rate *= st.s
        elif st.kind == "convT":
            rate //= st.s
            total += st.pl * rate
    return total


class _LookaheadStream:
    """The stream both look-ahead classes share: the stages, their host-side states and carried tensors, and the
    execution of one plan row per stage and push."""

    _what = "samples"

    def __init__(self, model):
        self.model = model
        self.stages = lookahead_stages(model)
        self.hop = int(model.hop_length)
        self.lookahead = lookahead_samples(model)
        self.reset()

    def reset(self):
        self._states = [st.start() for st in self.stages]
        self._carry: Dict[int, torch.Tensor] = {}
        self._lstm: Dict[int, tuple] = {}
        self._done = False
        self._like = None  # (batch size, device) of the stream, from its first input
        self.samples = 0
        self.rows = None  # the plan rows of the last push (tests compare them with lookahead_plan's)
        self._mode = _lib.precision_mode()

    _check_mode = StreamingEncoder._check_mode

    # ---- the stages ----------------------------------------------------------------------------------------------
    def _window(self, j: int, x, row, act=None, store: bool = True):
        """[carry | act(x) | right zeros] of stage j for plan row `row`; the last carry_out columns are kept."""
        cin, _, R, _, cout = row
        sa, sb = act.act.coeffs(x.device) if act is not None else (None, None)
        win, nctx = ops.load().stream_window_la(x, self._carry.get(j) if cin else None, sa, sb, cin, R,
                                                cout if store else 0)
        if store:
            self._carry[j] = nctx if cout else None
        return win

    def _empty(self, x, channels: int):
        return torch.empty(x.shape[0], channels, 0, device=x.device, dtype=torch.float32)

    def _run_conv(self, j, st, x, row):
        cin, new, R, out, cout = row
        c = st.module
        if not (cin or R or cout) and st.act is None and new and x.is_contiguous():
            return c.run(x, None, st.epilogue)  # no carry, no padding: the conv itself
        if not (new or R):  # nothing arrived and nothing to flush: the carry stays as it is
            return self._empty(x, c.out_channels)
        win = self._window(j, x, row, st.act)
        if not out:
            return self._empty(x, c.out_channels)
        return c.run(win, None, st.epilogue, pad_left=0)

    def _run_unit(self, j, st, x, row, flush: bool):
        cin, new, R, out, cout = row
        ru = st.module
        if not new and (not flush or not out):
            return self._empty(x, _conv_of(ru.block[1]).out_channels)
        cfg = ru._fused_cfg()
        raw = self._window(j, x, (cin, new, 0, out, cout))  # the raw window never carries the padding: see below
        if not out:
            return self._empty(x, raw.shape[1])
        if cfg >= 0 and ru.snake_on_load():
            # one launch with the unit's own padding: column c of the window sees columns c - pl ... c + pr, the
            # residual is the same column; [pl, W - pr) are exact, and at the flush the kernel's own right zero
            # padding is the layer's, so [pl, W) are
            y = ru._flow_fused(cfg, raw, None, True, None)[0]
            return y[:, :, st.pl:st.pl + out]
        conv7, conv1 = _conv_of(ru.block[1]), _conv_of(ru.block[3])
        aw = self._window(j, raw, (0, raw.shape[-1], R, out, 0), ru.block[0], store=False)  # snake(0) = 0
        t = conv7.run(aw, None, 0, ru.block[2].act.coeffs(x.device), pad_left=0)
        res = self._window(j, raw[:, :, st.pl:st.pl + out], (0, out, 0, out, 0), store=False)
        return conv1.run(t, res)

    def _run_convT(self, j, st, x, row):
        cin, new, _, out, cout = row
        conv = st.module
        _, seen, emitted = self._states[j]
        if new:
            win = self._window(j, x, row, st.act)
        else:
            win = self._carry.get(j)
        if not out:
            return self._empty(x, conv.out_channels)
        phases, _, bias, cfg = conv.prepared(win.device, conv.phase_cfg(win.shape[0], win.shape[-1]))
        # the window's first frame is frame seen - cin of the stream and the first new output is `emitted`: in the
        # window's own full (unpadded, uncropped) output that is column emitted + p - (seen - cin) s, which the
        # kernel's crop argument skips; out_len stops before the outputs a later frame still adds to
        crop = emitted + st.pl - (seen - cin) * st.s
        return ops.load().conv_transpose1d(win, phases, bias, None, None, conv.out_channels, out, st.k, st.s, crop, cfg,
                                           False)[0]

    def _run_lstm(self, st, x):
        if not x.shape[-1]:
            return x
        m = st.module
        if not x.is_contiguous():
            x = ops.load().stream_window_la(x, None, None, None, 0, 0, 0)[0]
        y, state = m.run(x, state=self._lstm.get(id(m)), return_state=True)
        self._lstm[id(m)] = state
        return y

    def _flow(self, x, flush: bool):
        rows, states = _plan_push(self.stages, self._states, x.shape[-1], flush)
        h = x
        for j, (st, row) in enumerate(zip(self.stages, rows)):
            if st.kind == "conv":
                h = self._run_conv(j, st, h, row)
            elif st.kind == "unit":
                h = self._run_unit(j, st, h, row, flush)
            elif st.kind == "convT":
                h = self._run_convT(j, st, h, row)
            else:
                h = self._run_lstm(st, h)
            if h.shape[-1] != row[3]:
                raise RuntimeError(f"look-ahead stage {j} ({st.kind}) emitted {h.shape[-1]} columns, its plan row {row}")
        self._states, self.rows = states, rows
        _lib.check_status()
        return h

    def _admit(self, x, flush: bool):
        if self._done:
            raise RuntimeError("the stream was finished: reset() it before the next push")
        self._check_mode()
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != self.stages[0].module.in_channels:
            raise ValueError(f"a look-ahead stream takes (B, {self.stages[0].module.in_channels}, n) tensors")
        if not flush and (x.shape[-1] < 1 or (self._what == "samples" and x.shape[-1] % self.hop)):
            raise ValueError(f"chunk of {x.shape[-1]} {self._what}: must be a positive multiple of the hop "
                             f"({self.hop if self._what == 'samples' else 1}); finish() takes any length")
        if x.is_cuda and x.dtype == torch.float32 and (x.stride(2) == 1 or not x.shape[-1]):
            pass  # a view with unit time stride (a slice of a clip) is read in place by the first window
        else:
            x = _as_input(x)
        if self._like is None:
            self._like = (x.shape[0], x.device)
        elif self._like[0] != x.shape[0]:
            raise ValueError(f"a batch of {x.shape[0]} on a stream of {self._like[0]}: the batch size is fixed per stream")
        return x

    def _count(self, n_in: int, n_out: int):
        self.samples += n_in

    def push(self, x) -> torch.Tensor:
        x = self._admit(x, False)
        with _lib.status_scope():
            y = self._flow(x, False)
        self._count(x.shape[-1], y.shape[-1])
        return y

    def finish(self, x=None) -> torch.Tensor:
        """Flush: an optional last chunk of any length, then every layer's own right zero padding; returns the frames
        (samples) that were still held back.  `x=None` needs at least one earlier push (its batch size and device)."""
        if x is None:
            if self._like is None:
                raise ValueError("finish() without input on a stream that saw none: nothing to flush")
            x = torch.empty(self._like[0], self.stages[0].module.in_channels, 0, device=self._like[1],
                            dtype=torch.float32)
        x = self._admit(x, True)
        with _lib.status_scope():
            y = self._flow(x, True)
        self._count(x.shape[-1], y.shape[-1])
        self._done = True
        return y

    def _chunked(self, x, chunk: int):
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"chunk of {chunk} {self._what}")
        self.reset()
        T = x.shape[-1]
        full = T - T % chunk
        outs = [self.push(x[..., i:i + chunk]) for i in range(0, full, chunk)]
        outs.append(self.finish(x[..., full:]))
        return torch.cat(outs, dim=2)


class LookaheadEncoder(_LookaheadStream):
    """Streams ANY BigCodecEncoder whose look-ahead is finite (causal or non-causal convs, a unidirectional ResLSTM, no
    anti-aliasing), exactly, with the fixed algorithmic delay `lookahead` (samples):

        la = LookaheadEncoder(encoder)
        z = la.push(x)        # x (B, 1, n), n a positive multiple of the hop -> (B, D, f): the f >= 0 frames now final
        z = la.finish(x)      # an optional last chunk of any length >= 0; flushes and returns the remaining frames
        la.reset()            # a new stream; push after finish raises RuntimeError until then
        z = la.encode(x, chunk)   # a whole clip in chunks + finish: the memory of one chunk, not of the clip

    cat(pushes..., finish) equals encoder(x) on the whole input (bit for bit in x6 and bf16; to fp32 rounding in h3,
    whose block scales depend on the tiling).  Every stage is a lazy valid conv over [carry | new] (_stage_row); one
    bc_stream_window_la launch forms the window (the stage's Snake applied on load) and the next carry.  A ResidualUnit
    the one-launch kernel serves runs over its RAW window with its own padding and returns the exact columns as a view;
    the others run conv7 over the activated window and conv1 with the residual from the raw one.  A stage with nothing
    to emit launches no conv.  No torch compute kernel runs in a push.  On a causal model the look-ahead is 0, every push
    returns n / hop frames equal to StreamingEncoder's and finish() returns an empty tensor.  All rows of a stream share
    one length and start together; LookaheadPool serves independent sessions with ragged windows in one batched push.
    HIP-graph capture is not offered."""

    def encode(self, x, chunk: int) -> torch.Tensor:
        """A whole clip through push in chunks of `chunk` samples (a multiple of the hop) and finish for the rest:
        encoder(x), with the activations of one chunk in memory at a time."""
        return self._chunked(x, chunk)


class LookaheadDecoder(_LookaheadStream):
    """LookaheadEncoder's counterpart for any BigCodecDecoder: push(z (B, D, n) post-VQ frames) returns the (B, 1, m)
    samples that are now final, finish(z=None) the rest; cat(pushes..., finish) equals decoder(z, vq=False).
    tokens(codes (B, n, Nq) int64 device) pushes index frames (vq2emb first).  A non-causal transposed conv (k = 2s,
    padding p) carries one input frame: with N frames seen its outputs o < N s - p are final, emitted through
    conv_transpose1d's own output length and crop; the last p come at the flush.  `lookahead` is in samples."""

    _what = "frames"

    def _count(self, n_in: int, n_out: int):
        self.samples += n_out

    def tokens(self, codes) -> torch.Tensor:
        return self.push(self.model.tokens_to_latent(codes))

    def decode(self, z, chunk: int) -> torch.Tensor:
        """A whole latent sequence through push in chunks of `chunk` frames and finish for the rest."""
        return self._chunked(z, chunk)


def plan_rows(entries):
    """The (src, dst) pool rows of one pool push, from (slot, pushes so far) per entry.  A session's state is
    ping-pong: slot s owns rows 2s and 2s + 1; its push number k reads row 2s + (k & 1) (k == 0: -1, a fresh session
    reads zeros) and writes row 2s + ((k + 1) & 1).  With distinct slots the two row sets are disjoint and dst holds
    no row twice, which is what bc_stream_window_slots needs (include/bigcodec.h).  Pure host arithmetic."""
    src = [2 * s + (k & 1) if k else -1 for s, k in entries]
    dst = [2 * s + ((k + 1) & 1) for s, k in entries]
    return src, dst


class SlotTable:
    """The host side of a StreamPool: which slots are open, how many pushes each session has made (its ping-pong
    phase), its sample count, and which sessions a failed push left undefined.  A session id is its slot number."""

    def __init__(self, capacity: int):
        if int(capacity) < 1:
            raise ValueError(f"a session pool needs a capacity of at least 1 (got {capacity})")
        self.capacity = int(capacity)
        self.pushes = [None] * self.capacity  # None: the slot is free
        self.samples = [0] * self.capacity
        self.undefined = set()

    def open(self) -> int:
        for s, k in enumerate(self.pushes):
            if k is None:
                self.pushes[s], self.samples[s] = 0, 0
                return s
        raise RuntimeError(f"the session pool is full ({self.capacity} sessions open)")

    def close(self, sid) -> None:
        self.check([sid], self.capacity, allow_undefined=True)
        self.pushes[sid] = None
        self.undefined.discard(sid)

    def live(self):
        return [s for s, k in enumerate(self.pushes) if k is not None]

    def check(self, sids, most: int, allow_undefined: bool = False):
        """The session ids of one push as a list, or ValueError: empty, more than `most`, unknown or closed, twice in
        one push (two writers of one pool row); RuntimeError for a session an earlier failed push left undefined."""
        sids = list(sids)
        if not sids:
            raise ValueError("a pool push needs at least one session")
        if len(sids) > most:
            raise ValueError(f"{len(sids)} sessions in one push: at most {most}")
        for s in sids:
            if isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < self.capacity or self.pushes[s] is None:
                raise ValueError(f"session {s!r} is not open in this pool")
        if len(set(sids)) != len(sids):
            raise ValueError(f"a session appears twice in one push: {sids}")
        bad = [s for s in sids if s in self.undefined]
        if bad and not allow_undefined:
            raise RuntimeError(f"sessions {bad} were in a push that failed: their state is undefined, close them")
        return sids

    def plan(self, sids):
        return plan_rows([(s, self.pushes[s]) for s in sids])

    def commit(self, sids, samples) -> None:
        """One more push for every session of `sids`; `samples` is one amount for all of them or one per session."""
        amounts = [samples] * len(sids) if isinstance(samples, int) else list(samples)
        if len(amounts) != len(sids):
            raise ValueError(f"{len(amounts)} sample counts for {len(sids)} sessions")
        for s, a in zip(sids, amounts):
            self.pushes[s] += 1
            self.samples[s] += a


class _PoolState:
    """The two places a stream touches its carried state, for a pool: the contexts of a stage live in one
    (2 * capacity, C, P) tensor and the ResLSTM state in two (layers, H, 2 * capacity) tensors, allocated at the
    stage's first push and never zeroed (a fresh session reads zeros through src = -1), and the current push's
    device index arrays `_src` / `_dst` (int32, one pool row per entry) say which rows it reads and writes.  `_hops`
    (int32 per entry, None: every entry fills the chunk) is the push's hops per entry out of `_n_hops`: every stage's
    window and the ResLSTM take it with the stage's own columns per hop."""

    _rows = 0
    _src = _dst = _hops = None
    _n_hops = 0

    def _window(self, key, x, P: int, act=None):
        if not P:  # no history, no state: the plain window (a dense copy of a strided view, or the Snake alone)
            return super()._window(key, x, P, act)
        sa, sb = act.act.coeffs(x.device) if act is not None else (None, None)
        pool = self._ctx.get(key)
        if pool is None:
            pool = self._ctx[key] = torch.empty(self._rows, x.shape[1], P, device=x.device, dtype=torch.float32)
        if self._hops is None:
            return ops.load().stream_window_slots_(x, pool, self._src, self._dst, sa, sb, P)
        return ops.load().stream_window_slots_lens_(x, pool, self._src, self._dst, self._hops,
                                                    x.shape[-1] // self._n_hops, sa, sb, P)

    def _lstm_run(self, m: ResLSTM, h):
        ns = ops.load()
        pools = self._lstm.get(id(m))
        if pools is None:
            shape = (m.lstm.num_layers, h.shape[1], self._rows)
            pools = self._lstm[id(m)] = tuple(torch.empty(shape, device=h.device, dtype=torch.float32) for _ in "hc")
        h0, c0 = ns.lstm_state_gather(pools[0], pools[1], self._src, h.shape[0])
        lens = self._hops
        if lens is not None and h.shape[-1] != self._n_hops:  # (no preset: their ResLSTMs run at one step per hop)
            lens = lens * (h.shape[-1] // self._n_hops)
        y, (hT, cT) = m.run(h, state=(h0, c0), return_state=True, lens=lens)
        ns.lstm_state_scatter_(pools[0], pools[1], hT, cT, self._dst)
        return y


class _PoolEncoder(_PoolState, StreamingEncoder):
    pass


class _PoolDecoder(_PoolState, StreamingDecoder):
    pass


class _PoolHost:
    """The host side StreamPool and LookaheadPool share: the slot table and its session calls, every refusal of a push
    that needs no look at the model, the pinned staging of a push's index arrays, and the rule that a push which
    raises after its admission leaves ITS sessions undefined.  A pool sets table, decoder, hop, capacity, channels."""

    _mode = None  # the precision of the pool's first push: the one its carried state belongs to
    _pinned = _event = None
    _chunk_hint = ""  # what a pool with a finish() adds to the refusal of a bad chunk length

    # ---- sessions ------------------------------------------------------------------------------------------------
    def close(self, sid) -> None:
        self.table.close(sid)

    def live(self):
        """The open session ids, ascending."""
        return self.table.live()

    def samples(self, sid) -> int:
        """Samples session `sid` has consumed (encoder pools) or produced (decoder pools) so far."""
        self.table.check([sid], 1, allow_undefined=True)
        return self.table.samples[sid]

    # ---- pushes --------------------------------------------------------------------------------------------------
    @property
    def _started(self) -> bool:
        return self._mode is not None

    def _start(self) -> None:
        if self._mode is None:
            self._mode = _lib.precision_mode()

    def _admit(self, sids, shape, flush: bool = False, most=None, channels=None):
        """Every host-side refusal of a push (nothing is launched before it passes); returns the ids as a list.
        flush: a finish() takes chunks of any length."""
        sids = self.table.check(sids, most or self.capacity)
        channels = self.channels if channels is None else channels
        if len(shape) != 3 or shape[0] != len(sids):
            raise ValueError(f"input of shape {tuple(shape)} for {len(sids)} sessions: row i belongs to sids[i]")
        if channels and shape[1] != channels:
            raise ValueError(f"input of shape {tuple(shape)}: expected {channels} channels")
        if not flush and (shape[2] < 1 or (not self.decoder and shape[2] % self.hop)):
            raise ValueError(f"chunk of {shape[2]} samples: must be a positive multiple of the hop ({self.hop})"
                             + self._chunk_hint)
        if self._mode is not None and _lib.precision_mode() != self._mode:
            raise RuntimeError(f"precision changed ({self._mode} -> {_lib.precision_mode()}): the pool's carried state "
                               "belongs to the mode of its first push")
        return sids

    @staticmethod
    def _ints(values, entries: int, lo: int, hi: int, what: str):
        """One int in [lo, hi] per entry as a list, or ValueError."""
        values = list(values)
        if len(values) != entries:
            raise ValueError(f"{len(values)} {what} for {entries} sessions: entry i belongs to sids[i]")
        for v in values:
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"{what} entry {v!r}: an int from {lo} to {hi}")
        return values

    def _admit_tokens(self, sids, codes):
        """tokens(): codes (len(sids), n, Nq) admitted as n frames of any width; returns (sids, n)."""
        if not self.decoder:
            raise TypeError("tokens() needs a pool over a decoder")
        shape = (codes.shape[0], 0, codes.shape[1]) if codes.dim() == 3 else codes.shape
        return self._admit(sids, shape, channels=0), shape[2]

    def _stage(self, values, out, room: int = 0) -> None:
        """`values` into the int32 device tensor `out`: pinned staging (at least `room` ints at its first use) and a
        copy the host does not wait for (the wait on the previous copy's event has nothing left to wait for once that
        push's status was read)."""
        if self._pinned is None or self._pinned.numel() < len(values):
            self._pinned = torch.empty(max(len(values), room), dtype=torch.int32, pin_memory=out.is_cuda)
            self._event = torch.cuda.Event() if out.is_cuda else None
        elif self._event is not None:
            self._event.synchronize()
        self._pinned[:len(values)] = torch.tensor(values, dtype=torch.int32)
        out.copy_(self._pinned[:len(values)], non_blocking=True)
        if self._event is not None:
            self._event.record(torch.cuda.current_stream(out.device))

    @contextlib.contextmanager
    def _marking(self, sids):
        """Launches may have been queued when anything raises in here: the state of `sids` is undefined from then on."""
        try:
            yield
        except BaseException:
            self.table.undefined.update(sids)
            raise


class StreamPool(_PoolHost):
    """Many independent causal streams in one batched push: a pool of per-session state on the device.

        pool = StreamPool(model, capacity)   # a causal BigCodecEncoder or BigCodecDecoder (StreamingEncoder's refusals)
        sid = pool.open()                    # the lowest free slot; RuntimeError when the pool is full
        y = pool.push(sids, x)               # x (len(sids), 1, n) samples / (len(sids), D, n) frames: row i is sids[i]'s
        y = pool.push(sids, x, hops=[1, 3])  # a chunk length per session: row i holds hops[i] hops, left-aligned
        wav = pool.tokens(sids, codes)       # decoder pools: codes (len(sids), n, Nq) int64 on the device
        pool.close(sid)                      # the slot is free again; nothing is zeroed

    Each session gets exactly what its own B = 1 StreamingEncoder / StreamingDecoder would have produced (bit for bit
    in x6; to fp32 rounding in h3, whose block scales depend on the tiling), whatever else is in the push: sessions
    open, close and sit out ticks independently, the order of `sids` is free, and the chunk length n (a multiple of the
    hop) may differ between calls and, with `hops`, between the sessions of one call: hops[i] (an int, 1 <= hops[i] <=
    n_hops = n / hop samples or n frames) says how many hops of row i are session sids[i]'s; the rest of the row is
    never read (it may hold anything).  The result has the padded shape: entry i's first hops[i] hops are its output,
    the rest is exactly zero (one bc_zero_tail), and samples(sid) advances by the session's own amount.  Every window
    then zeroes the columns past its entry's length and stores the context that ends there
    (bc_stream_window_slots_lens), and the ResLSTM stores each entry's state at its own last step
    (bc_reslstm_fwd_state_lens); hops rides in the same staged copy as the row indices.  hops=None launches exactly
    what it always did.  A model whose first stage carries no history has no window to keep the input's tail out, and
    `hops` is refused for it (NotImplementedError; no preset is such a model).  The push runs StreamingEncoder's / StreamingDecoder's own stages on
    the batch; only the state access differs: one bc_stream_window_slots launch per stage that carries history, one
    bc_lstm_state_gather and one bc_lstm_state_scatter per ResLSTM, all indexed by one (src, dst) pair of pool rows
    per entry (plan_rows: ping-pong rows, so no launch reads a row it writes).  The pair is built on the host, written
    to pinned memory and copied without a wait; no torch compute kernel runs in a push.

    Refused on the host before any launch: an unknown, closed or repeated session id, an empty push, a batch
    dimension other than len(sids), a chunk that is no multiple of the hop, `hops` of another length than `sids`, with
    an entry that is no int or lies outside [1, n_hops] (ValueError); a precision other than the one of the pool's first
    push (RuntimeError).  When a push raises later than that, launches may have been queued
    and the state of ITS sessions is undefined: further pushes for them raise RuntimeError until they are closed."""

    def __init__(self, model, capacity: int):
        self.table = SlotTable(capacity)
        self.decoder = hasattr(model, "tokens_to_latent")
        self._stream = (_PoolDecoder if self.decoder else _PoolEncoder)(model)
        self._stream._rows = 2 * self.table.capacity
        self.capacity, self.hop = self.table.capacity, self._stream.hop
        conv0 = _conv_of((model.model if self.decoder else model.block)[0])
        self.channels = int(conv0.in_channels)  # of a push's input: 1 (samples) or the latent width
        self._first_history = conv0.pad_left() > 0  # the first stage's window keeps a ragged input's tail out

    def open(self) -> int:
        return self.table.open()

    def state_bytes(self) -> int:
        """Bytes of device state the pool holds (both ping-pong rows of every slot; 0 before the first push)."""
        s = self._stream
        return sum(t.numel() * 4 for t in s._ctx.values()) + sum(t.numel() * 4 for v in s._lstm.values() for t in v)

    # ---- pushes --------------------------------------------------------------------------------------------------
    def _n_hops(self, n: int) -> int:
        return n if self.decoder else n // self.hop

    def _check_hops(self, hops, entries: int, n_hops: int):
        """`hops` of a push as a list of ints (None: None), or ValueError; nothing is launched before it passes."""
        if hops is None:
            return None
        hops = self._ints(hops, entries, 1, n_hops, "hops")
        if not self._first_history:
            raise NotImplementedError("a chunk length per session needs a first stage with causal history")
        return hops

    def _start(self) -> None:
        super()._start()
        self._stream._mode = self._mode  # (the stream checks it again in its own push)

    def push(self, sids, x, hops=None) -> torch.Tensor:
        sids = self._admit(sids, x.shape)
        n_hops = self._n_hops(x.shape[-1])
        hops = self._check_hops(hops, len(sids), n_hops)
        src, dst = self.table.plan(sids)
        self._start()
        s, m = self._stream, len(sids)
        try:
            with self._marking(sids):
                x = _as_input(x)
                if hops is None:
                    idx = torch.empty(2 * m, dtype=torch.int32, device=x.device)
                    self._stage(src + dst, idx, 4 * self.capacity)
                    s._src, s._dst = idx[:m], idx[m:]
                    y = s.push(x)
                else:  # the hops and the output lengths ride in the same staged copy as the rows
                    unit = self.hop if self.decoder else 1  # output columns per hop
                    idx = torch.empty(4 * m, dtype=torch.int32, device=x.device)
                    self._stage(src + dst + hops + [h * unit for h in hops], idx, 4 * self.capacity)
                    s._src, s._dst, s._hops, s._n_hops = idx[:m], idx[m:2 * m], idx[2 * m:3 * m], n_hops
                    y = s.push(x)
                    ops.load().zero_tail_(y, None, idx[3 * m:], (n_hops - min(hops)) * unit)
        finally:
            s._hops = None
        if hops is None:
            self.table.commit(sids, y.shape[-1] if self.decoder else x.shape[-1])
        else:
            self.table.commit(sids, [h * self.hop for h in hops])
        return y

    def tokens(self, sids, codes, hops=None) -> torch.Tensor:
        """codes (len(sids), n, Nq) int64 on the device -> waveform chunks (len(sids), 1, n * hop); `hops` as in push
        (the index frames past an entry's own are never decoded into its output)."""
        sids, n = self._admit_tokens(sids, codes)
        self._check_hops(hops, len(sids), n)
        return self.push(sids, self._stream.decoder.tokens_to_latent(codes), hops)

    def graph(self, B: int, n: int) -> "PoolGraph":
        """One pool push of up to B sessions and chunks of n samples (encoder) / frames (decoder) as a HIP graph."""
        return PoolGraph(self, B, n)


# ---- look-ahead session pool: many non-causal streams in one batched push -----------------------------
#
# §23's window is dense: [carry | new | right zeros] with one carry length for the whole batch, which is why its rows
# must start together.  Here every stage's window is LEFT-ALIGNED AND RAGGED per entry: entry b's row is its own carry,
# its own new columns and zeros up to the widest row.  The zeros behind a short entry and a flushing entry's right zero
# padding are the same literal zeros, so sessions in their transient, in steady state and at their flush share every
# launch; they differ in how many output columns the host claims for them (_stage_row, per entry).

class LookaheadSlots:
    """The host side of a LookaheadPool, for any list of lazy stages (tests run it on a toy stack without a GPU): the
    slot table, each session's per-stage stream states (_stage_row's) and per-stage ping-pong phases, and the plan of
    one push: per stage the index arrays bc_stream_window_slots_la / the ResLSTM gather, scatter and lens take.

    The phase is kept per slot AND per stage (None: nothing stored yet, the stage reads zeros through src = -1): a
    stage that receives nothing for an entry this push stores nothing (dst = -1) and keeps its phase, so its carry
    stays where it is.  Slot s owns pool rows 2s and 2s + 1 of every stage; a stage's src rows are the current phases
    and its dst rows the other ones, so with distinct slots the two sets are disjoint and dst holds no row twice."""

    def __init__(self, stages, capacity: int):
        self.stages = list(stages)
        if not self.stages or self.stages[-1].kind == "convT":
            raise NotImplementedError("a look-ahead pool needs a model that ends in a conv (a transposed conv's crop "
                                      "differs per entry and is resolved by the next stage's window)")
        if any(a.kind == "convT" and b.kind == "lstm" for a, b in zip(self.stages, self.stages[1:])):
            raise NotImplementedError("a ResLSTM directly behind a transposed conv: its rows would not be left-aligned")
        self.table = SlotTable(capacity)
        self.states = [None] * self.table.capacity
        self.phases = [None] * self.table.capacity

    def pitch(self, j: int) -> int:
        """Pmax of stage j's pool rows: the largest carry it can hold ((k - 1) d columns; hist frames)."""
        st = self.stages[j]
        return max(1, st.hist if st.kind == "convT" else (st.k - 1) * st.d)

    def open(self) -> int:
        s = self.table.open()
        self.states[s] = [st.start() for st in self.stages]
        self.phases[s] = [None] * len(self.stages)
        return s

    def plan(self, sids, lens, flush):
        """One push of lens[i] input columns for session sids[i] (flush[i]: then its flush).  Pure: nothing changes
        until commit().  Returns a namespace: stages[j] (kind, launch, the per-entry lists src, dst, cin, n, xoff, keep,
        cout, out, and W, Wraw, crop, tout), rows[i][j] (_stage_row's rows of entry i), counts[i] (the last stage's
        outputs), and the next states and phases."""
        import types

        m = len(sids)
        new, xoff = [int(n) for n in lens], [0] * m
        states = [list(self.states[s]) for s in sids]
        phases = [list(self.phases[s]) for s in sids]
        rows, out_stages = [[] for _ in sids], []
        for j, st in enumerate(self.stages):
            p = types.SimpleNamespace(kind=st.kind, launch=False, src=[-1] * m, dst=[-1] * m, cin=[0] * m, n=[0] * m,
                                      xoff=[0] * m, keep=[0] * m, cout=[0] * m, out=[0] * m, W=0, Wraw=0, crop=0, tout=0)
            crops = [0] * m
            for b, s in enumerate(sids):
                carry, seen, emitted = states[b][j]
                row, states[b][j] = _stage_row(st, states[b][j], new[b], bool(flush[b]))
                rows[b].append(row)
                cin, nb, R, out, cout = row
                p.out[b] = out
                if not (nb or out):  # nothing arrived and nothing to flush: a padding row; carry and phase stay
                    continue
                p.launch = True
                ph = phases[b][j]
                if st.kind == "lstm":
                    p.src[b] = -1 if ph is None else 2 * s + ph
                    ph = phases[b][j] = 0 if ph is None else 1 - ph
                    p.dst[b], p.n[b] = 2 * s + ph, nb
                    continue
                p.src[b] = 2 * s + ph if ph is not None and cin else -1
                p.cin[b], p.n[b], p.xoff[b], p.cout[b] = cin, nb, xoff[b], cout
                p.keep[b] = cin + nb - cout if st.kind == "convT" else out * st.s
                if cout:
                    ph = phases[b][j] = 0 if ph is None else 1 - ph
                    p.dst[b] = 2 * s + ph
                p.Wraw, p.W = max(p.Wraw, cin + nb), max(p.W, cin + nb + R)
                if st.kind == "convT" and out:  # (_LookaheadStream._run_convT: the window's own column of output `emitted`)
                    crops[b] = emitted + st.pl - (seen - cin) * st.s
            if st.kind == "convT" and any(p.out):
                p.crop = min(c for c, o in zip(crops, p.out) if o)
                p.tout = max(c + o for c, o in zip(crops, p.out) if o) - p.crop
                xoff = [c - p.crop if o else 0 for c, o in zip(crops, p.out)]
            else:
                p.tout, xoff = max(p.out), [0] * m
            new = list(p.out)
            out_stages.append(p)
        return types.SimpleNamespace(sids=list(sids), lens=[int(n) for n in lens], flush=[bool(f) for f in flush],
                                     stages=out_stages, rows=rows, counts=new, states=states, phases=phases)

    def commit(self, plan, samples) -> None:
        """The plan was executed: its states and phases become the sessions'; flushed sessions are closed."""
        self.table.commit(plan.sids, samples)
        for b, s in enumerate(plan.sids):
            self.states[s], self.phases[s] = plan.states[b], plan.phases[b]
            if plan.flush[b]:
                self.table.close(s)


class LookaheadPool(_PoolHost):
    """Many independent look-ahead streams of a NON-causal (or causal) model in one batched push: StreamPool for the
    models LookaheadEncoder / LookaheadDecoder accept.

        pool = LookaheadPool(model, capacity)      # lookahead_stages' refusals
        sid = pool.open(); pool.close(sid); pool.live(); pool.samples(sid); pool.state_bytes(); pool.lookahead
        y, counts = pool.push(sids, x, hops=None)  # x (m, 1, n) samples / (m, D, n) frames; hops as StreamPool's
        y, counts = pool.tokens(sids, codes, hops=None)   # decoder pools: codes (m, n, Nq) int64 on the device
        y, counts = pool.finish(sids, x=None, lens=None)  # optional last chunks of ANY length >= 0, then the flush

    y has the padded shape: entry i's first counts[i] columns are the frames / samples now FINAL for sids[i] (counts[i]
    may be 0: the look-ahead holds them back), the rest is exactly zero (one bc_zero_tail).  counts is a host list
    taken from the plan: no device read.  Per session, cat(y[i, :, :counts[i]] over its pushes and its finish) equals
    the whole-sequence forward on its own data and its own B = 1 look-ahead stream (bit for bit in x6; to fp32
    rounding in h3), whatever else is in the push: sessions open at any tick, sit ticks out, deliver their own number
    of hops, and one in its transient shares the launch with one in steady state and one at its flush.  finish()
    closes its sessions: their slots are free again.  push(..., finish=[...]) (one bool per entry) flushes the marked
    entries after their hops in the same launches as the others' push; finish() is that for every entry, with lengths
    that need not be multiples of the hop.

    Every stage runs ONCE per push on the batch: one bc_stream_window_slots_la launch forms the left-aligned ragged
    windows [carry | new | zeros] and stores each entry's next carry to its pool row, then the stage's own kernel runs
    over the dense batch (Conv1dWN.run without padding; the one-launch ResidualUnit over the raw window with its own
    padding, its exact columns handed on as a view; conv_transpose1d with the smallest crop of the batch, each entry's
    own crop becoming the next window's input offset; the ResLSTM between one state gather and one scatter, with each
    entry's own length).  All index arrays of all stages ride in one pinned buffer and one non-blocking copy per push.
    A stage no entry feeds launches nothing.  All per-session arithmetic is _stage_row (LookaheadSlots.plan).

    Refused on the host before any launch, as in StreamPool: an unknown, closed or repeated session id, an empty push,
    a batch dimension other than len(sids), a wrong channel count, a chunk that is no positive multiple of the hop,
    `hops` / `lens` / `finish` of another length or with a bad entry (ValueError); a precision other than the one of the
    pool's first push (RuntimeError).  A push that raises later leaves ITS sessions undefined: close them."""

    def __init__(self, model, capacity: int):
        self.model = model
        self.decoder = hasattr(model, "tokens_to_latent")
        self.slots = LookaheadSlots(lookahead_stages(model), capacity)
        self.table, self.stages = self.slots.table, self.slots.stages
        self.capacity, self.hop = self.table.capacity, int(model.hop_length)
        self.lookahead = lookahead_samples(model)
        self.channels = int(self.stages[0].module.in_channels)
        self._pools = {}  # stage -> its (2 * capacity, C, Pmax) carries, or the ResLSTM's two (layers, H, 2 * capacity)
        self.plan = None  # the plan of the last push (tests compare its rows with lookahead_plan's)

    _chunk_hint = "; finish() takes any length"

    def open(self) -> int:
        return self.slots.open()

    def state_bytes(self) -> int:
        """Bytes of device state the pool holds (both ping-pong rows of every slot; 0 before the first push)."""
        return sum(t.numel() * 4 for v in self._pools.values() for t in (v if isinstance(v, tuple) else (v,)))

    # ---- pushes --------------------------------------------------------------------------------------------------
    def _lens(self, sids, n: int, hops):
        """The input columns per entry of a push of n columns with `hops` (StreamPool's: ints in [1, n_hops])."""
        unit = 1 if self.decoder else self.hop
        if hops is None:
            return [n] * len(sids)
        return [h * unit for h in self._ints(hops, len(sids), 1, n // unit, "hops")]

    def _flags(self, sids, finish):
        if finish is None:
            return [False] * len(sids)
        finish = list(finish)
        if len(finish) != len(sids) or not all(isinstance(f, bool) for f in finish):
            raise ValueError(f"finish must hold one bool per session (got {finish!r} for {len(sids)} sessions)")
        return finish

    def push(self, sids, x, hops=None, finish=None):
        sids = self._admit(sids, x.shape)
        lens = self._lens(sids, x.shape[2], hops)
        return self._run(sids, x, lens, self._flags(sids, finish))

    def tokens(self, sids, codes, hops=None, finish=None):
        """codes (len(sids), n, Nq) int64 on the device; `hops` as in push (the index frames past an entry's own are
        never decoded into its output)."""
        sids, n = self._admit_tokens(sids, codes)
        lens = self._lens(sids, n, hops)
        flags = self._flags(sids, finish)
        return self._run(sids, self.model.tokens_to_latent(codes), lens, flags)

    def finish(self, sids, x=None, lens=None):
        """Optional last chunks (entry i delivers lens[i] columns of x, 0 <= lens[i] <= n, any length; None: all n),
        then every layer's own right zero padding: the frames / samples still held back.  Closes the sessions."""
        if x is None:
            sids = list(sids)
            sids = self._admit(sids, (len(sids), self.channels, 0), True)
            if lens is not None:
                self._ints(lens, len(sids), 0, 0, "lens")
            dev = next(self.model.parameters()).device
            x = torch.empty(len(sids), self.channels, 0, device=dev, dtype=torch.float32)
        else:
            sids = self._admit(sids, x.shape, True)
        n = x.shape[2]
        lens = [n] * len(sids) if lens is None else self._ints(lens, len(sids), 0, n, "lens")
        return self._run(sids, x, lens, [True] * len(sids))

    # ---- one push ------------------------------------------------------------------------------------------------
    def _run(self, sids, x, lens, flush):
        plan = self.slots.plan(sids, lens, flush)
        self._start()
        with self._marking(sids):
            if not (x.is_cuda and x.dtype == torch.float32 and (x.stride(2) == 1 or not x.shape[2])):
                x = _as_input(x)  # (a view with unit time stride is read in place by the first window)
            with _lib.status_scope():
                y = self._flow(plan, x)
                _lib.check_status()
        self.slots.commit(plan, plan.counts if self.decoder else plan.lens)
        self.plan = plan
        return y, list(plan.counts)

    def _flow(self, plan, x):
        ns, m, dev = ops.load(), len(plan.sids), x.device
        # every index array of every stage that launches, and the output lengths, in ONE staged copy
        values, where = [], []
        for p in plan.stages:
            names = () if not p.launch else ("src", "dst", "n") if p.kind == "lstm" else \
                ("src", "dst", "cin", "n", "xoff", "keep", "cout")
            where.append({k: len(values) + i * m for i, k in enumerate(names)})
            for k in names:
                values += getattr(p, k)
        counts_at = len(values)
        values += plan.counts
        idx = torch.empty(len(values), dtype=torch.int32, device=dev)
        self._stage(values, idx, 8 * self.capacity * (len(self.stages) + 1))
        h = x
        for j, (st, p) in enumerate(zip(self.stages, plan.stages)):
            arr = {k: idx[o:o + m] for k, o in where[j].items()}
            if st.kind == "lstm":
                h = self._run_lstm(ns, j, st, p, arr, h)
            elif st.kind == "convT":
                h = self._run_convT(ns, j, st, p, arr, h)
            elif st.kind == "unit":
                h = self._run_unit(ns, j, st, p, arr, h)
            else:
                h = self._run_conv(ns, j, st, p, arr, h)
            if h.shape[2] != p.tout:
                raise RuntimeError(f"look-ahead pool stage {j} ({st.kind}) emitted {h.shape[2]} columns, its plan {p.tout}")
        if h.shape[2] and min(plan.counts) < h.shape[2]:
            ns.zero_tail_(h, None, idx[counts_at:], h.shape[2] - min(plan.counts))
        return h

    def _window(self, ns, j, p, arr, x, W: int, act=None):
        pool = self._pools.get(j)
        if pool is None:
            pool = self._pools[j] = torch.empty(2 * self.capacity, x.shape[1], self.slots.pitch(j), device=x.device,
                                                dtype=torch.float32)
        sa, sb = act.act.coeffs(x.device) if act is not None else (None, None)
        return ns.stream_window_slots_la_(x, pool, arr["src"], arr["dst"], arr["cin"], arr["n"], arr["xoff"], arr["keep"],
                                          arr["cout"], sa, sb, W)

    @staticmethod
    def _empty(x, channels: int):
        return torch.empty(x.shape[0], channels, 0, device=x.device, dtype=torch.float32)

    def _run_conv(self, ns, j, st, p, arr, x):
        c = st.module
        if not p.launch:
            return self._empty(x, c.out_channels)
        win = self._window(ns, j, p, arr, x, p.W, st.act)
        if not p.tout:
            return self._empty(x, c.out_channels)
        return c.run(win, None, st.epilogue, pad_left=0)  # entry b's outputs: columns [0, out_b)

    def _run_unit(self, ns, j, st, p, arr, x):
        ru = st.module
        if not p.launch:
            return self._empty(x, x.shape[1])
        raw = self._window(ns, j, p, arr, x, p.Wraw)  # the raw window never carries the padding (_LookaheadStream)
        if not p.tout:
            return self._empty(x, x.shape[1])
        cfg = ru._fused_cfg()
        if cfg >= 0 and ru.snake_on_load():
            # one launch with the unit's own padding: the zeros behind an entry's columns are its right zero padding at
            # the flush and never reach a claimed column otherwise; entry b's outputs are the view's first out_b columns
            y = ru._flow_fused(cfg, raw, None, True, None)[0]
            return y[:, :, st.pl:st.pl + p.tout]
        conv7, conv1 = _conv_of(ru.block[1]), _conv_of(ru.block[3])
        sa, sb = ru.block[0].act.coeffs(x.device)
        aw = ns.stream_window_la(raw, None, sa, sb, 0, p.W - p.Wraw, 0)[0]  # snake(0) = 0: the zeros stay zeros
        t = conv7.run(aw, None, 0, ru.block[2].act.coeffs(x.device), pad_left=0)
        res = ns.stream_window_la(raw[:, :, st.pl:st.pl + p.tout], None, None, None, 0, 0, 0)[0]
        return conv1.run(t, res)

    def _run_convT(self, ns, j, st, p, arr, x):
        conv = st.module
        if not p.launch:
            return self._empty(x, conv.out_channels)
        win = self._window(ns, j, p, arr, x, p.Wraw, st.act)
        if not p.tout:
            return self._empty(x, conv.out_channels)
        phases, _, bias, cfg = conv.prepared(win.device, conv.phase_cfg(win.shape[0], win.shape[2]))
        # one crop argument for the batch: the smallest; entry b's first output is column crop_b - crop of the result,
        # which the next stage's window takes as xoff_b
        return ns.conv_transpose1d(win, phases, bias, None, None, conv.out_channels, p.tout, st.k, st.s, p.crop, cfg,
                                   False)[0]

    def _run_lstm(self, ns, j, st, p, arr, x):
        if not p.launch:
            return x
        m = st.module
        if not x.is_contiguous():
            x = ns.stream_window_la(x, None, None, None, 0, 0, 0)[0]
        pools = self._pools.get(j)
        if pools is None:
            shape = (m.lstm.num_layers, x.shape[1], 2 * self.capacity)
            pools = self._pools[j] = tuple(torch.empty(shape, device=x.device, dtype=torch.float32) for _ in "hc")
        h0, c0 = ns.lstm_state_gather(pools[0], pools[1], arr["src"], x.shape[0])
        # an entry without a frame this push runs one step on whatever its row holds (the kernel clamps lens to 1): its
        # output is never claimed and its state is dropped (dst = -1)
        y, (hT, cT) = m.run(x, state=(h0, c0), return_state=True, lens=arr["n"])
        ns.lstm_state_scatter_(pools[0], pools[1], hT, cT, arr["dst"])
        return y


class PoolGraph:
    """A pool push of B entries of chunk length n captured in a HIP graph (as StreamGraph captures a stream's).  The
    input and the (src, dst) index arrays are static tensors and the pools themselves are the static state: the
    captured kernels write them in place, so there are no copy-back nodes, eager pushes and replays of the same pool
    mix freely, and ONE graph serves any membership: push(sids, x) takes len(sids) <= B sessions, pads the missing
    entries with src = dst = -1 (they read zeros and store nothing) and zero input, replays, and returns the first
    len(sids) rows of the static output (overwritten by the next push: copy it to keep it).  check as in StreamGraph.
    push(sids, x, hops=...) is StreamPool.push's chunk length per session: hops is one more static device array (a
    missing entry stays src = dst = -1), and the launches differ from the equal-length push's (the windows and the
    ResLSTM take the lengths, one bc_zero_tail follows), so they are a second graph over the same static input and
    index arrays, captured at the first push that gives hops; pushes with and without hops mix freely."""

    def __init__(self, pool: StreamPool, B: int, n: int):
        B, n = int(B), int(n)
        if not 1 <= B <= pool.capacity:
            raise ValueError(f"a graph of {B} entries on a pool of capacity {pool.capacity}")
        if n < 1 or (not pool.decoder and n % pool.hop):
            raise ValueError(f"chunk of {n} samples: must be a positive multiple of the hop ({pool.hop})")
        self.pool, self.B = pool, B
        if pool._started:
            pool._stream._check_mode()
        pool._start()
        s = pool._stream
        dev = next(p for p in (s.decoder if pool.decoder else s.encoder).parameters()).device
        self.input = torch.zeros(B, pool.channels, n, device=dev)
        self._dirty = 0  # rows of the static input that hold a session's data
        # static index arrays: src | dst | hops | output lengths, B of each (the last two: the graph with hops only)
        self._n_hops = pool._n_hops(n)
        self._unit = pool.hop if pool.decoder else 1  # output columns per hop
        self._padding = [-1] * (2 * B) + [self._n_hops] * B + [self._n_hops * self._unit] * B
        self._idx = torch.tensor(self._padding, dtype=torch.int32, device=dev)
        self._graph, self.output, self._status = self._capture(False)
        self._ragged = None  # (graph, output, status words) of the push with hops
        self._last = self._status

    def _capture(self, ragged: bool):
        """One push of B entries over the static input and index arrays as a graph: (graph, its static output, its
        status words, rewritten by every replay)."""
        B, s = self.B, self.pool._stream
        self._idx.copy_(torch.tensor(self._padding, dtype=torch.int32))  # (a later capture: no session's rows)
        s._src, s._dst = self._idx[:B], self._idx[B:2 * B]
        if ragged:
            s._hops, s._n_hops = self._idx[2 * B:3 * B], self._n_hops

        def push():
            y = s.push(self.input)
            if ragged:  # sized for the shortest entry there can be: one hop
                ops.load().zero_tail_(y, None, self._idx[3 * B:], (self._n_hops - 1) * self._unit)
            return y

        try:
            # one eager push of padding entries allocates every pool and warms the weight caches; it stores no state
            with torch.no_grad():
                push()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.no_grad(), _lib.deferred_status() as ticket:
                with torch.cuda.graph(graph):
                    output = push()
        finally:
            s._hops = None
        return graph, output, ticket.items

    def push(self, sids, x, hops=None, check: bool = True) -> torch.Tensor:
        pool, B = self.pool, self.B
        sids = pool._admit(sids, x.shape, most=B)
        if x.shape[2] != self.input.shape[2]:
            raise ValueError(f"this graph was captured for chunks of {self.input.shape[2]}, got {x.shape[2]}")
        hops = pool._check_hops(hops, len(sids), self._n_hops)
        src, dst = pool.table.plan(sids)
        m, pad = len(sids), [-1] * (B - len(sids))
        with pool._marking(sids):
            if hops is None:
                graph, output, self._last = self._graph, self.output, self._status
                pool._stage(src + pad + dst + pad, self._idx[:2 * B], 4 * pool.capacity)
            else:
                if self._ragged is None:
                    self._ragged = self._capture(True)
                graph, output, self._last = self._ragged
                pool._stage(src + pad + dst + pad + hops + self._padding[2 * B + m:3 * B]
                            + [h * self._unit for h in hops] + self._padding[3 * B + m:], self._idx, 4 * pool.capacity)
            self.input[:m].copy_(_as_input(x))
            if self._dirty > m:
                self.input[m:self._dirty].zero_()
            self._dirty = m
            graph.replay()
            if check:
                self.check()
        if hops is None:
            pool.table.commit(sids, output.shape[-1] if pool.decoder else x.shape[-1])
        else:
            pool.table.commit(sids, [h * pool.hop for h in hops])
        return output[:m]

    def check(self) -> None:
        """Raise BigCodecLibraryError if the last replay's persistent ResLSTM reported a failure (host wait)."""
        if self._last:
            _lib._raise_bad(self._last, torch.cat([t.reshape(-1) for t, _ in self._last]).cpu().tolist())


class StreamGraph:
    """One push of a fixed chunk shape captured in a HIP graph (torch.cuda.CUDAGraph: hipStreamBeginCapture /
    hipGraphLaunch on ROCm) and replayed per chunk: the dozens of launches of a push (a window, a conv or a
    one-launch ResidualUnit per stage, the persistent ResLSTM) go to the device as ONE graph launch, so a stream
    of short chunks is no longer bound by host-side dispatch.  The carried state lives in static buffers: the
    graph reads them, its stages write the next state into graph-owned tensors, and the graph's last nodes copy
    those back into the static buffers.  The stream's current state is taken over at capture (the warm-up push
    that sizes every buffer is undone), and the stream continues from the graph's state afterwards.

    push(x) copies x into the static input, replays, and returns the graph's static output (overwritten by the next
    push: copy it to keep it).  check=True (the default) reads the ResLSTM status words after the replay (one
    host wait, as StreamingEncoder.push does); check=False skips it and check() reads them later.  The
    results equal the eager stream's bit for bit (tests/test_gpu_streaming.py)."""

    def __init__(self, stream: StreamingEncoder, example):
        example = _as_input(example)
        self.stream = stream
        self.input = example.clone()
        # one eager push sizes every carried state and warms the weight caches; then the state before it returns
        ctx0 = {k: v.clone() for k, v in stream._ctx.items()}
        lstm0 = {k: tuple(t.clone() for t in v) for k, v in stream._lstm.items()}
        samples0 = stream.samples
        with torch.no_grad():
            stream.push(self.input)
        self._ctx = {k: (ctx0[k] if k in ctx0 else torch.zeros_like(v)) for k, v in stream._ctx.items()}
        self._lstm = {k: (lstm0[k] if k in lstm0 else tuple(torch.zeros_like(t) for t in v))
                      for k, v in stream._lstm.items()}
        stream._ctx, stream._lstm, stream.samples = dict(self._ctx), dict(self._lstm), samples0
        torch.cuda.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), _lib.deferred_status() as ticket:
            with torch.cuda.graph(self._graph):
                self.output = stream.push(self.input)
                for k, v in stream._ctx.items():
                    self._ctx[k].copy_(v)
                for k, v in stream._lstm.items():
                    for dst, src in zip(self._lstm[k], v):
                        dst.copy_(src)
        self._status = ticket.items  # the graph's own status words, rewritten by every replay
        stream._ctx, stream._lstm, stream.samples = dict(self._ctx), dict(self._lstm), samples0
        self._n = example.shape[-1] * (stream.hop if isinstance(stream, StreamingDecoder) else 1)

    def push(self, x, check: bool = True) -> torch.Tensor:
        if tuple(x.shape) != tuple(self.input.shape):
            raise ValueError(f"this graph was captured for chunks of shape {tuple(self.input.shape)}, got {tuple(x.shape)}")
        self.input.copy_(x)
        self._graph.replay()
        self.stream.samples += self._n
        if check:
            self.check()
        return self.output

    def reset(self) -> None:
        """Start a new stream on this graph: the static state back to zeros (a fresh stream's context)."""
        for v in self._ctx.values():
            v.zero_()
        for v in self._lstm.values():
            for t in v:
                t.zero_()
        self.stream._ctx, self.stream._lstm, self.stream.samples = dict(self._ctx), dict(self._lstm), 0

    def check(self) -> None:
        """Raise BigCodecLibraryError if the last replay's persistent ResLSTM reported a failure (host wait)."""
        if self._status:
            _lib._raise_bad(self._status, torch.cat([t.reshape(-1) for t, _ in self._status]).cpu().tolist())
