"""BigCodecEncoder / BigCodecDecoder (vq/codec_encoder.py:14-90, vq/codec_decoder.py:15-142) on the
HIP kernels, with the reference's constructor signatures, state_dict keys and call surface.

forward() runs the whole stack as one fused flow (blocks.py): every Snake is computed once in
the epilogue of the kernel producing its input, the ResLSTM writes the final Snake directly, and
the decoder's tanh is the last conv's epilogue."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from .blocks import DecoderBlock, EncoderBlock, Ragged, ResLSTM, input_act, produce_conv
from .conv import WNConv1d
from .modules import FSQ, Activation1d, ResidualVQ, SnakeBeta, _as_input, _zeros


def _length_list(lengths, B, what: str):
    """A ragged batch's `lengths` argument (a list or a CPU integer tensor) as a list of B ints."""
    if isinstance(lengths, torch.Tensor):
        if lengths.is_cuda or lengths.is_floating_point():
            raise ValueError(f"{what}: a list or a CPU integer tensor (a device tensor would cost a synchronisation)")
        lengths = lengths.reshape(-1).tolist()
    lengths = [int(v) for v in lengths]
    if not lengths or (B is not None and len(lengths) != B):
        raise ValueError(f"{what}: {len(lengths)} entries for a batch of {B} clips")
    return lengths


def _refuse_ragged(model) -> None:
    """What a ragged batch cannot express: the anti-aliased activation replicate-pads at the clip's end (the padded
    batch's end is another sample), and a bidirectional ResLSTM's reverse direction starts at each clip's own end."""
    for m in model.modules():
        if isinstance(m, Activation1d) and m.antialias:
            raise NotImplementedError("lengths (a ragged batch) with antialias=True: the anti-aliased activation "
                                      "replicate-pads at each clip's own end")
        if isinstance(m, ResLSTM) and m.lstm.bidirectional:
            raise NotImplementedError("lengths (a ragged batch) with a bidirectional ResLSTM: the reverse direction "
                                      "must start at each clip's own end")


class _Tanh(nn.Module):
    """nn.Tanh (codec_decoder.py:80).  decode() runs it fused in the last conv's epilogue; called on its
    own (decoder.model used as the reference's nn.Sequential) it is bc_tanh_fwd."""

    def forward(self, x):
        return ops.load().tanh(_as_input(x))


class BigCodecEncoder(nn.Module):
    """vq/codec_encoder.py:14-90.  forward(x (B,1,T) f32 device) -> (B, out_channels, T/hop)."""

    def __init__(self, ngf=48, use_rnn=True, rnn_bidirectional=False, causal=False, antialias=False,
                 rnn_num_layers=2, up_ratios=(2, 2, 2, 5, 5), dilations=(1, 3, 9), out_channels=1024):
        super().__init__()
        self.hop_length = np.prod(up_ratios)
        self.ngf = ngf
        self.up_ratios = up_ratios
        if causal:
            assert not rnn_bidirectional
        d_model = ngf
        block = [WNConv1d(1, d_model, kernel_size=7, padding=3, causal=causal)]
        for stride in up_ratios:
            d_model *= 2
            block += [EncoderBlock(d_model, stride=stride, dilations=dilations, causal=causal, antialias=antialias)]
        if use_rnn:
            block += [ResLSTM(d_model, num_layers=rnn_num_layers, bidirectional=rnn_bidirectional)]
        block += [
            Activation1d(activation=SnakeBeta(d_model, alpha_logscale=True), antialias=antialias),
            WNConv1d(d_model, out_channels, kernel_size=3, padding=1, causal=causal),
        ]
        self.block = nn.Sequential(*block)
        self.enc_dim = d_model

    def forward(self, x, lengths=None):
        """lengths (a list or CPU integer tensor, one entry per clip, in samples): a ragged batch.  Clip b's samples
        at t >= lengths[b] are ignored (x is not modified) and latent[b, :, :frame_lengths(lengths)[b]] is what
        encoding x[b:b+1, :, :lengths[b]] alone gives; entries past that extent carry no meaning."""
        with L.status_scope():
            return self._forward(x, lengths)

    def _ragged_chain(self):
        blk = list(self.block)
        chain = [("conv", blk[0])]
        for st in blk[1:-2]:
            chain += st.ragged_chain() if isinstance(st, EncoderBlock) else [("keep", st)]
        return chain + [("conv", blk[-1])]

    def _ragged(self, lengths, B: int, T: int) -> Ragged:
        lengths = _length_list(lengths, B, "encoder lengths")
        _refuse_ragged(self)
        return Ragged(self._ragged_chain(), lengths, T, "encoder lengths")

    def frame_lengths(self, lengths, per_layer: bool = False):
        """Frames of each clip of a ragged batch from its length in samples: every conv's own out_len in turn (a
        causal model gives floor(n / hop), a non-causal one more).  per_layer: the whole table instead, one list per
        masked producer in flow order (row 0 the input, the last row the latent)."""
        lengths = _length_list(lengths, None, "encoder lengths")
        rg = self._ragged(lengths, len(lengths), max(lengths))
        return [r.tolist() for r in rg.rows] if per_layer else rg.rows[-1].tolist()

    def _forward(self, x, lengths=None):
        # (the lengths are checked on the host first: a refusal costs no launch)
        rg = None
        if lengths is not None:
            if not isinstance(x, torch.Tensor) or x.dim() != 3:
                raise ValueError("lengths (a ragged batch) needs a (B, C, T) tensor")
            rg = self._ragged(lengths, x.shape[0], x.shape[2])
        x = _as_input(x)
        if rg is not None:
            x = rg.upload(x.device).masked_input(x)
        blk = list(self.block)
        final_act, last_conv = blk[-2], blk[-1]
        stages = blk[1:-2]  # EncoderBlocks [+ ResLSTM]
        # consumer activation of each stage's output
        def next_act_of(i):
            if i + 1 < len(stages):
                nxt = stages[i + 1]
                return input_act(nxt) if isinstance(nxt, EncoderBlock) else None  # ResLSTM takes raw
            return final_act
        y, ya = produce_conv(blk[0], x, None, want_raw=True, next_act=next_act_of(-1) if stages else final_act, rg=rg)
        for i, st in enumerate(stages):
            nact = next_act_of(i)
            want_raw = i + 1 < len(stages)  # the next stage needs the raw tensor (RU skip / LSTM input)
            if isinstance(st, EncoderBlock):
                y, ya = st.flow(y, ya, want_raw=want_raw, next_act=nact, rg=rg)
            else:
                y, ya = st.flow(y, want_raw=want_raw, next_act=nact, rg=rg)
        # (the latent has no consumer that reads across a clip's end: the VQ is per frame; its tail is left as it is)
        out = produce_conv(last_conv, ya, None, want_raw=True, next_act=None)[0]
        L.check_status()  # a failed persistent ResLSTM launch raises here, before the latent is used
        return out

    def inference(self, x):
        return self.forward(x)

    def remove_weight_norm(self):
        for m in self.modules():
            if m is not self and "weight_v" in m._parameters and hasattr(m, "remove_weight_norm"):
                m.remove_weight_norm()


class BigCodecDecoder(nn.Module):
    """vq/codec_decoder.py:15-142.  forward(x, vq=True) -> (z_q, codes (Nq,B,F), losses (Nq,));
    forward(x, vq=False) -> waveform (B, 1, T)."""

    def __init__(self, in_channels=1024, upsample_initial_channel=1536, ngf=48, use_rnn=True,
                 rnn_bidirectional=False, rnn_num_layers=2, up_ratios=(5, 5, 2, 2, 2), dilations=(1, 3, 9),
                 causal=False, antialias=False, fsq=False, fsq_levels=[4, 4, 4, 8], vq_num_quantizers=1,
                 vq_commit_weight=0.25, vq_weight_init=False, vq_full_commit_loss=False, codebook_size=8192,
                 codebook_dim=8):
        super().__init__()
        self.hop_length = np.prod(up_ratios)
        self.ngf = ngf
        self.up_ratios = up_ratios
        self.fsq = fsq
        if fsq:  # codec_decoder.py:41-47
            self.quantizer = FSQ(levels=fsq_levels, channel_first=True, dim=in_channels)
            assert codebook_size == np.prod(fsq_levels), "codebook_size must be equal to the product of fsq_levels"
        else:
            self.quantizer = ResidualVQ(num_quantizers=vq_num_quantizers, dim=in_channels,
                                        codebook_size=codebook_size, codebook_dim=codebook_dim,
                                        threshold_ema_dead_code=2, commitment=vq_commit_weight,
                                        weight_init=vq_weight_init, full_commit_loss=vq_full_commit_loss)
        channels = upsample_initial_channel
        layers = [WNConv1d(in_channels, channels, kernel_size=7, padding=3, causal=causal)]
        if use_rnn:
            layers += [ResLSTM(channels, num_layers=rnn_num_layers, bidirectional=rnn_bidirectional)]
        output_dim = channels
        for i, stride in enumerate(up_ratios):
            input_dim = channels // 2 ** i
            output_dim = channels // 2 ** (i + 1)
            layers += [DecoderBlock(input_dim, output_dim, stride, dilations, causal=causal, antialias=antialias)]
        layers += [
            Activation1d(activation=SnakeBeta(output_dim, alpha_logscale=True), antialias=antialias),
            WNConv1d(output_dim, 1, kernel_size=7, padding=3, causal=causal),
            _Tanh(),
        ]
        self.model = nn.Sequential(*layers)

    def decode(self, x, lengths=None):
        """self.model(x): fused flow; final Snake in the producer of the last conv's input, tanh in
        the last conv's epilogue.  lengths (a list or CPU integer tensor, one entry per clip, in frames): a ragged
        batch.  Clip b's frames at f >= lengths[b] are ignored (x is not modified), wav[b, :, :sample_lengths(
        lengths)[b]] is what decoding x[b:b+1, :, :lengths[b]] alone gives and the rest of the row is zero."""
        with L.status_scope():
            return self._decode(x, lengths)

    def _ragged_chain(self):
        m = list(self.model)
        chain = [("conv", m[0])]
        for st in m[1:-3]:
            chain += st.ragged_chain() if isinstance(st, DecoderBlock) else [("keep", st)]
        return chain + [("conv", m[-2])]

    def _ragged(self, lengths, B: int, T: int) -> Ragged:
        lengths = _length_list(lengths, B, "decoder lengths")
        _refuse_ragged(self)
        return Ragged(self._ragged_chain(), lengths, T, "decoder lengths")

    def sample_lengths(self, frames, per_layer: bool = False):
        """Samples of each clip of a ragged batch from its length in frames (every transposed conv's own out_len:
        frames * hop).  per_layer: the whole table, one list per masked producer in flow order."""
        frames = _length_list(frames, None, "decoder lengths")
        rg = self._ragged(frames, len(frames), max(frames))
        return [r.tolist() for r in rg.rows] if per_layer else rg.rows[-1].tolist()

    def _decode(self, x, lengths=None):
        # (the lengths are checked on the host first: a refusal costs no launch)
        rg = None
        if lengths is not None:
            if not isinstance(x, torch.Tensor) or x.dim() != 3:
                raise ValueError("lengths (a ragged batch) needs a (B, C, T) tensor")
            rg = self._ragged(lengths, x.shape[0], x.shape[2])
        x = _as_input(x)
        if rg is not None:
            x = rg.upload(x.device).masked_input(x)
        m = list(self.model)
        final_act, last_conv = m[-3], m[-2]
        stages = m[1:-3]  # [ResLSTM] + DecoderBlocks

        def next_act_of(i):
            if i + 1 < len(stages):
                nxt = stages[i + 1]
                return nxt.first_act if isinstance(nxt, DecoderBlock) else None
            return final_act
        first_next = next_act_of(-1) if stages else final_act
        y, ya = produce_conv(m[0], x, None, want_raw=first_next is None, next_act=first_next, rg=rg)
        for i, st in enumerate(stages):
            nact = next_act_of(i)
            want_raw = nact is None
            if isinstance(st, DecoderBlock):
                y, ya = st.flow(y, ya, want_raw=want_raw, next_act=nact, rg=rg)
            else:
                y, ya = st.flow(y, want_raw=want_raw, next_act=nact, rg=rg)
        out = produce_conv(last_conv, ya, None, want_raw=True, next_act=None, epilogue=1, rg=rg)[0]
        L.check_status()
        return out

    def forward(self, x, vq=True, lengths=None):
        """lengths (frames per clip, a ragged batch) applies to the decode (vq=False); the VQ is per frame."""
        if vq is True:
            if self.fsq:  # codec_decoder.py:87-89
                x, q = self.quantizer(x)
                return x, q, _zeros(x.shape[0], x.device)
            return self.quantizer(x)
        return self.decode(x, lengths=lengths)

    def vq2emb(self, vq):
        self.quantizer = self.quantizer.eval()
        return self.quantizer.vq2emb(vq)

    def get_emb(self):
        self.quantizer = self.quantizer.eval()
        return self.quantizer.get_emb()

    def tokens_to_audio(self, vq, lengths=None):
        """Token -> audio: codes (B, T, Nq) int64 on the device (extract_indices' (F, Nq) files, batched)
        -> waveform (B, 1, T * hop): vq2emb (codec_decoder.py:96-99) -> transpose(1, 2) -> self(x, vq=False),
        with the embedding written straight in the decoder's (B, D, T) layout (bc_vq2emb_ct).  fsq=True decoders
        (whose vq2emb raises AttributeError in the reference: FSQ has none) take one index column through
        FSQ.indices_to_codes (finite_scalar_quantization.py:176-192, bc_fsq_codes), then the same decode.
        lengths (frames per clip): a ragged batch, decode(x, lengths); the codes past a clip's end are ignored."""
        return self.decode(self.tokens_to_latent(vq), lengths=lengths)

    def tokens_to_latent(self, vq):
        """codes (B, T, Nq) on the device -> the decoder's input (B, D, T) (see tokens_to_audio)."""
        if self.fsq:
            if vq.dim() != 3 or vq.shape[2] != 1:
                raise ValueError(f"an fsq=True decoder takes (B, T, 1) indices, got {tuple(vq.shape)}")
            return self.quantizer.indices_to_codes(vq[:, :, 0])
        return self.quantizer.vq2emb_ct(vq)

    def inference_vq(self, vq):
        return self.decode(vq[None, :, :])

    def inference_0(self, x):
        x, q, loss = self.quantizer(x)
        return self.decode(x), None

    def inference(self, x):
        return self.decode(x), None

    def remove_weight_norm(self):
        for m in self.modules():
            if m is not self and "weight_v" in m._parameters and hasattr(m, "remove_weight_norm"):
                m.remove_weight_norm()
