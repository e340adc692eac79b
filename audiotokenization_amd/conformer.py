"""The Conformer-STFT codec family (vq/codec_encoder.py:92-209, vq/codec_decoder.py:145-274, 385-509,
vq/module.py:357-547) on the gfx950 kernels: what lightning_module.py:101-116, 140-163 builds for
`type: conformer_stft` / `conformer_istft` (config1/model/base.yaml).

Every class has the reference's name, constructor arguments and parameter / buffer names, so a reference state_dict
loads strictly.  Inference only: eval mode (dropout is the identity), whole clips of one length, no streaming.

Activations stay (B, C, T) fp32 from the STFT to the ISTFT.  Every nn.Linear and 1x1 nn.Conv1d runs on the conv
path (conv.Conv1dWN: the process-wide precision mode, bias and residual add in the epilogue; w1 and w3 of a FeedForward
stacked into one launch); the rest are the kernels of csrc/conformer.hip, fp32 in every precision mode.  What the conv
path gives this family in `bf16` is untested.

A ConformerLayer is 17 launches: 5 RMSNorm, 8 pointwise convs, 2 SwiGLU, 1 GLU + depthwise conv, 1 attention.
The classes whose reference forward takes (B, T, C) (RMSNorm, FeedForward, ISTFTHead) keep that signature for a
standalone call and transpose around the kernels; inside the models the (B, C, T) entry points (`run`) are used."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
from torch.nn import Parameter

from . import _lib as L
from . import ops
from .conv import Conv1dWN
from .modules import FSQ, ResidualVQ, _as_input, _cpu, _DeviceCache, _pkey, _zeros

__all__ = ["RMSNorm", "SelfAttention", "FeedForward", "ConformerConvModule", "ConformerLayer", "ConformerBackbone",
           "STFT", "ConformerEncoderSTFT", "ISTFT", "ISTFTHead", "ConformerDecoderISTFT", "precompute_freqs_cis",
           "stft_basis_t", "istft_basis"]


def _eval_only(m: nn.Module):
    if m.training:
        raise NotImplementedError(f"{type(m).__name__}: inference only, call .eval() first (dropout and the "
                                  f"training-time quantizer paths are not built)")


def _no_lengths(lengths):
    if lengths is not None:
        raise NotImplementedError("the Conformer family takes whole clips of one length: a ragged batch (lengths=) "
                                  "would need a key mask per clip in the attention")


def _on(cache: _DeviceCache, p: torch.Tensor, device) -> torch.Tensor:
    """p as a contiguous fp32 tensor on `device` (itself when it already is one; otherwise uploaded once per version)."""
    if p.device == device and p.dtype == torch.float32 and p.is_contiguous():
        return p.detach()
    return cache.get(_pkey(p) + (str(device),), lambda: _cpu(p).contiguous().to(device))


class _Pointwise(Conv1dWN):
    """nn.Linear (weight (out, in)) or a plain 1x1 nn.Conv1d (weight (out, in, 1)) on the conv path: parameters
    `weight` and `bias`, no weight norm."""

    def __init__(self, in_features, out_features, bias=True, linear=True):
        super().__init__(in_features, out_features, 1, bias=bias)
        w = self.weight_v.detach().clone()
        del self._parameters["weight_g"]
        del self._parameters["weight_v"]
        self.weight = Parameter(w[:, :, 0].contiguous() if linear else w)

    def folded_weight(self) -> torch.Tensor:
        return _cpu(self.weight).reshape(self.out_channels, self.in_channels, 1)

    def remove_weight_norm(self):
        raise ValueError("no weight norm on this module")


class _Stacked(_Pointwise):
    """Two bias-free Linears of one input as one conv: rows [w1; w3].  It owns no parameter (kept out of the owner's
    module tree); its packed weight follows the two source parameters."""

    def __init__(self, a: _Pointwise, b: _Pointwise):
        nn.Module.__init__(self)
        self.in_channels, self.out_channels = a.in_channels, a.out_channels + b.out_channels
        self.kernel_size = self.stride = self.dilation = 1
        self.padding, self.causal_pad = 0, None
        self.register_parameter("bias", None)
        self._src = (a, b)
        self._cache = _DeviceCache()

    def folded_weight(self) -> torch.Tensor:
        return torch.cat([m.folded_weight() for m in self._src], 0)

    def _params(self):
        return tuple(m.weight for m in self._src) + (None,)


# vq/module.py:357-370
class RMSNorm(nn.Module):
    def __init__(self, dim: int, eps: float = 1e-6):
        super().__init__()
        self.eps = eps
        self.weight = Parameter(torch.ones(dim))
        self._cache = _DeviceCache()

    def run(self, x, silu: bool = False):
        """(B, C, T) -> (B, C, T), normalised over C."""
        x = _as_input(x)
        return ops.load().rmsnorm(x, _on(self._cache, self.weight, x.device), float(self.eps), silu)

    def forward(self, x):
        """The reference's call shape: normalised over the LAST dimension of a (B, T, C) tensor."""
        if x.dim() != 3:
            raise ValueError("RMSNorm takes (B, T, C)")
        return self.run(x.transpose(1, 2).contiguous()).transpose(1, 2)


# vq/module.py:372-377, the same torch CPU expressions
def precompute_freqs_cis(dim: int, end: int, theta: float = 10000.0):
    freqs = 1.0 / (theta ** (torch.arange(0, dim, 2)[: (dim // 2)].float() / dim))
    t = torch.arange(end, device=freqs.device, dtype=torch.float32)
    freqs = torch.outer(t, freqs)
    return torch.polar(torch.ones_like(freqs), freqs)


_ROPE = {}


def _rope_table(freqs_cis: torch.Tensor, device) -> torch.Tensor:
    """(max_seq_len, D / 2, 2) fp32 (cos, sin) on `device`: the host table uploaded once."""
    key = (id(freqs_cis), str(device))
    hit = _ROPE.get(key)
    if hit is None or hit[0] is not freqs_cis:
        hit = _ROPE[key] = (freqs_cis, torch.view_as_real(freqs_cis.cpu()).contiguous().to(device))
    return hit[1]


# vq/module.py:399-453
class SelfAttention(nn.Module):
    def __init__(self, dim, n_head=8, dropout=0.1, causal: bool = False):
        super().__init__()
        if dim % n_head or dim // n_head not in (32, 64):
            raise NotImplementedError(f"SelfAttention: head_dim {dim / n_head:g} (dim {dim} / n_head {n_head}): the "
                                      f"attention kernel is built for head dims 32 and 64")
        self.n_head = n_head
        self.head_dim = dim // n_head
        self.causal = causal
        self.qkv_proj = _Pointwise(dim, 3 * dim, bias=False)
        self.out_proj = _Pointwise(dim, dim, bias=False)
        self.dropout = dropout

    def run(self, x, rope, residual=None, trace=None):
        """x (B, C, T) -> out_proj(attention(qkv_proj(x))) [+ residual]; rope: the device table (>= T rows)."""
        _eval_only(self)
        qkv = self.qkv_proj.run(x)
        a = ops.load().attention(qkv, rope, self.n_head, bool(self.causal))
        if trace is not None:
            trace["attn"] = a
        return self.out_proj.run(a, residual=residual)

    def forward(self, x, freqs_cis):
        x = _as_input(x)
        if freqs_cis.shape[0] < x.shape[2]:
            raise ValueError(f"{x.shape[2]} frames, RoPE table of {freqs_cis.shape[0]}")
        return self.run(x, _rope_table(freqs_cis, x.device))


# vq/module.py:455-470
class FeedForward(nn.Module):
    def __init__(self, dim, mult=4, dropout=0.1):
        super().__init__()
        hidden_dim = int(2 * (dim * mult) / 3)
        multiple_of = 256
        hidden_dim = multiple_of * ((hidden_dim + multiple_of - 1) // multiple_of)
        self.w1 = _Pointwise(dim, hidden_dim, bias=False)
        self.w2 = _Pointwise(hidden_dim, dim, bias=False)
        self.w3 = _Pointwise(dim, hidden_dim, bias=False)
        self.dropout = nn.Dropout(dropout)
        object.__setattr__(self, "_w13", _Stacked(self.w1, self.w3))

    def run(self, x, residual=None):
        """x (B, C, T) -> w2(silu(w1 x) * w3 x) [+ residual]."""
        _eval_only(self)
        h = self._w13.run(x)
        return self.w2.run(ops.load().swiglu(h), residual=residual)

    def forward(self, x):
        """The reference's call shape: (B, T, C)."""
        return self.run(_as_input(x).transpose(1, 2).contiguous()).transpose(1, 2)


class _Depthwise(nn.Module):
    """nn.Conv1d(dim, dim, K, groups=dim): parameters weight (dim, 1, K) and bias (dim)."""

    def __init__(self, dim, kernel_size):
        super().__init__()
        ref = nn.Conv1d(dim, dim, kernel_size, groups=dim)
        self.weight = Parameter(ref.weight.detach().clone())
        self.bias = Parameter(torch.zeros(dim))  # (the reference's init_weights zeroes conv biases)
        self.kernel_size = int(kernel_size)
        self._cw, self._cb = _DeviceCache(), _DeviceCache()


class _CausalDepthwise(nn.Module):
    """vq/module.py:11-48 with groups=dim: the conv's parameters under `.conv`, left pad K - 1."""

    def __init__(self, dim, kernel_size):
        super().__init__()
        self.conv = _Depthwise(dim, kernel_size)
        self.padding = kernel_size - 1


# vq/module.py:472-494
class ConformerConvModule(nn.Module):
    def __init__(self, dim, kernel_size=31, dropout=0.1, causal: bool = False):
        super().__init__()
        if not 1 <= kernel_size <= 63:
            raise NotImplementedError(f"ConformerConvModule: depthwise kernel size {kernel_size} (the kernel takes <= 63)")
        self.pointwise_conv1 = _Pointwise(dim, 2 * dim, linear=False)
        self.glu = nn.GLU(dim=1)
        self.depthwise_conv = _CausalDepthwise(dim, kernel_size) if causal else _Depthwise(dim, kernel_size)
        self.conv_norm = RMSNorm(dim)
        self.silu = nn.SiLU()
        self.pointwise_conv2 = _Pointwise(dim, dim, linear=False)
        self.dropout = nn.Dropout(dropout)
        self.causal = causal

    def run(self, x, residual=None):
        _eval_only(self)
        p = self.pointwise_conv1.run(x)
        dw = self.depthwise_conv.conv if self.causal else self.depthwise_conv
        K = dw.kernel_size
        pad_left = K - 1 if self.causal else (K - 1) // 2  # padding='same': torch pads (K - 1) // 2 left, the rest right
        d = ops.load().dwconv_glu(p, _on(dw._cw, dw.weight, p.device), _on(dw._cb, dw.bias, p.device), pad_left)
        return self.pointwise_conv2.run(self.conv_norm.run(d, silu=True), residual=residual)

    def forward(self, x):
        return self.run(_as_input(x))


# vq/module.py:496-526
class ConformerLayer(nn.Module):
    def __init__(self, dim, n_head=8, ffn_mult=4, conv_kernel_size=31, dropout=0.1, conv_first: bool = False,
                 causal: bool = False):
        super().__init__()
        self.ffn1 = FeedForward(dim, mult=ffn_mult, dropout=dropout)
        self.self_attn = SelfAttention(dim, n_head=n_head, dropout=dropout, causal=causal)
        self.conv = ConformerConvModule(dim, kernel_size=conv_kernel_size, dropout=dropout, causal=causal)
        self.ffn2 = FeedForward(dim, mult=ffn_mult, dropout=dropout)
        self.conv_first = conv_first
        self.conv_norm_in = RMSNorm(dim)
        self.ffn1_norm_in = RMSNorm(dim)
        self.attn_norm_in = RMSNorm(dim)
        self.ffn2_norm_in = RMSNorm(dim)
        self.dropout = nn.Dropout(dropout)

    def run(self, x, rope, trace=None):
        """x (B, C, T), rope the device table.  trace (a dict) receives the output of each of the four sub-blocks
        ('conv', 'ffn1', 'attn_out', 'ffn2') and the attention output before out_proj ('attn')."""
        def conv(x):
            return self.conv.run(self.conv_norm_in.run(x), residual=x)

        def attn(x):
            return self.self_attn.run(self.attn_norm_in.run(x), rope, residual=x, trace=trace)

        order = (("conv", conv), ("attn_out", attn)) if self.conv_first else (("attn_out", attn), ("conv", conv))
        x = order[0][1](x)
        if trace is not None:
            trace[order[0][0]] = x
        x = self.ffn1.run(self.ffn1_norm_in.run(x), residual=x)
        if trace is not None:
            trace["ffn1"] = x
        x = order[1][1](x)
        if trace is not None:
            trace[order[1][0]] = x
        x = self.ffn2.run(self.ffn2_norm_in.run(x), residual=x)
        if trace is not None:
            trace["ffn2"] = x
        return x

    def forward(self, x, freqs_cis):
        x = _as_input(x)
        return self.run(x, _rope_table(freqs_cis, x.device))


# vq/module.py:528-547
class ConformerBackbone(nn.Module):
    def __init__(self, dim, n_layers, n_head=8, ffn_mult=4, conv_kernel_size=31, dropout=0.1, max_seq_len=8192,
                 rope_theta=10000.0, conv_first: bool = False, causal: bool = False):
        super().__init__()
        self.layers = nn.ModuleList([
            ConformerLayer(dim, n_head, ffn_mult, conv_kernel_size, dropout, conv_first=conv_first, causal=causal)
            for _ in range(n_layers)
        ])
        self.max_seq_len = max_seq_len
        # built on the CPU with the reference's expressions and uploaded as it is: a plain attribute, not a buffer
        self.freqs_cis = precompute_freqs_cis(dim // n_head, max_seq_len, rope_theta)

    def run(self, x, trace=None):
        _eval_only(self)
        T = x.shape[-1]
        if T > self.freqs_cis.shape[0]:
            raise ValueError(f"{T} frames exceed max_seq_len {self.freqs_cis.shape[0]}")
        rope = _rope_table(self.freqs_cis, x.device)
        for i, layer in enumerate(self.layers):
            x = layer.run(x, rope, trace if i == 0 else None)
        return x

    def forward(self, x):
        return self.run(_as_input(x))


def _hann(window: torch.Tensor) -> np.ndarray:
    return _cpu(window).double().numpy()


def stft_basis_t(window: torch.Tensor, n_fft: int) -> np.ndarray:
    """(n_fft, n_fft + 2) float64: column c < bins is w[n] cos(2 pi c n / n_fft), column bins + c is -w[n] sin(...)
    (torch.stft's sign), w the module's fp32 window buffer.  The angle is reduced in integers."""
    n = np.arange(n_fft, dtype=np.int64)
    c = np.arange(n_fft // 2 + 1, dtype=np.int64)
    ang = 2.0 * np.pi * ((n[:, None] * c[None, :]) % n_fft).astype(np.float64) / n_fft
    w = _hann(window)[:, None]
    return np.concatenate([np.cos(ang) * w, -np.sin(ang) * w], axis=1)


def istft_basis(window: torch.Tensor, n_fft: int) -> np.ndarray:
    """(n_fft + 2, n_fft) float64: irfft (backward norm) times the window as a basis.  Row k < bins multiplies Re S_k:
    c_k cos(2 pi k n / n_fft) w[n] / n_fft; row bins + k multiplies Im S_k: -c_k sin(...) w[n] / n_fft; c_k = 1 for DC
    and Nyquist (whose imaginary rows are exactly zero: irfft ignores those parts), 2 otherwise."""
    bins = n_fft // 2 + 1
    n = np.arange(n_fft, dtype=np.int64)
    k = np.arange(bins, dtype=np.int64)
    ang = 2.0 * np.pi * ((k[:, None] * n[None, :]) % n_fft).astype(np.float64) / n_fft
    ck = np.full((bins, 1), 2.0)
    ck[0, 0] = ck[-1, 0] = 1.0
    w = _hann(window)[None, :] / n_fft
    im = -ck * np.sin(ang) * w
    im[0, :] = im[-1, :] = 0.0
    return np.concatenate([ck * np.cos(ang) * w, im], axis=0)


# vq/codec_encoder.py:92-122
class STFT(nn.Module):
    def __init__(self, hop_length=256, n_fft=1024, window_size=1024, window_fn=torch.hann_window):
        super().__init__()
        if window_size != n_fft:
            raise NotImplementedError(f"STFT: window_size {window_size} != n_fft {n_fft} is not built")
        if n_fft % 2 or not 1 <= hop_length <= n_fft:
            raise NotImplementedError(f"STFT: needs an even n_fft >= hop_length >= 1 (got {n_fft}, {hop_length})")
        self.register_buffer("window", window_fn(window_size))
        self.hop_length = hop_length
        self.n_fft = n_fft
        self.window_size = window_size
        self.pad_mode = "constant"
        self.center = False
        self.return_complex = True
        self._cache = _DeviceCache()

    def frames(self, T: int) -> int:
        """torch.stft's frame count after the (window_size - hop_length) // 2 padding per side."""
        return (T + 2 * ((self.window_size - self.hop_length) // 2) - self.n_fft) // self.hop_length + 1

    def features(self, x):
        """x (B, 1, T) -> (B, 2 * (n_fft // 2 + 1), F): the real rows, then the imaginary rows (what
        ConformerEncoderSTFT.forward concatenates, codec_encoder.py:188-192)."""
        x = _as_input(x)
        if x.dim() != 3 or x.shape[1] != 1:
            raise ValueError("STFT takes (B, 1, T)")
        if x.shape[2] < self.hop_length:
            raise ValueError(f"a clip of {x.shape[2]} samples is shorter than one hop ({self.hop_length})")
        basis = self._cache.get(_pkey(self.window) + (str(x.device),), lambda: torch.from_numpy(
            stft_basis_t(self.window, self.n_fft).astype(np.float32)).contiguous().to(x.device))
        return ops.load().stft_frames(x.reshape(x.shape[0], x.shape[2]), basis, self.n_fft, self.hop_length,
                                      self.window_size)

    def forward(self, x):
        f = self.features(x)
        bins = self.n_fft // 2 + 1
        return torch.complex(f[:, :bins], f[:, bins:])


# vq/codec_encoder.py:124-209
class ConformerEncoderSTFT(nn.Module):
    def __init__(self, hop_length=256, n_fft=1024, window_size=1024, dim=512, n_layers=12, n_head=8, ffn_mult=4,
                 conv_kernel_size=31, dropout=0.1, max_seq_len=8192, rope_theta=10000.0, causal=False,
                 out_channels=1024):
        super().__init__()
        self.hop_length = hop_length
        self.n_fft = n_fft
        self.stft = STFT(hop_length=hop_length, n_fft=n_fft, window_size=window_size)
        stft_dim = n_fft // 2 + 1
        self.input_proj = _Pointwise(2 * stft_dim, dim, linear=False)
        self.input_norm = RMSNorm(dim)
        self.conformer_backbone = ConformerBackbone(dim=dim, n_layers=n_layers, n_head=n_head, ffn_mult=ffn_mult,
                                                    conv_kernel_size=conv_kernel_size, dropout=dropout,
                                                    max_seq_len=max_seq_len, rope_theta=rope_theta, causal=causal,
                                                    conv_first=True)
        self.norm = RMSNorm(dim)
        self.output_proj = Conv1dWN(dim, out_channels, kernel_size=1) if out_channels != dim else nn.Identity()

    def forward(self, x, lengths=None, trace=None):
        """x (B, 1, T) audio -> (B, out_channels, F).  trace (a dict) receives the intermediates of the first layer
        (ConformerLayer.run) plus 'stft' and 'input_norm'."""
        _no_lengths(lengths)
        _eval_only(self)
        if isinstance(x, torch.Tensor) and x.dim() == 3 and x.shape[2] >= self.hop_length:
            frames, limit = self.stft.frames(x.shape[2]), self.conformer_backbone.freqs_cis.shape[0]
            if frames > limit:
                raise ValueError(f"{frames} frames exceed max_seq_len {limit}")
        with L.status_scope():
            f = self.stft.features(x)
            h = self.input_norm.run(self.input_proj.run(f))
            if trace is not None:
                trace["stft"], trace["input_norm"] = f, h
            h = self.norm.run(self.conformer_backbone.run(h, trace))
            return h if isinstance(self.output_proj, nn.Identity) else self.output_proj.run(h)

    def remove_weight_norm(self):
        if not isinstance(self.output_proj, nn.Identity) and "weight_v" in self.output_proj._parameters:
            self.output_proj.remove_weight_norm()


# vq/codec_decoder.py:145-213
class ISTFT(nn.Module):
    """Holds the window buffer and the geometry; the transform itself is fused with the head's exp / cos / sin
    (ISTFTHead.run -> bc_istft_head), so a standalone call on a complex spectrogram is not built."""

    def __init__(self, n_fft: int, hop_length: int, win_length: int, padding: str = "same"):
        super().__init__()
        if padding not in ["center", "same"]:
            raise ValueError("Padding must be 'center' or 'same'.")
        if padding != "same" or win_length != n_fft:
            raise NotImplementedError("ISTFT: only padding='same' with win_length == n_fft is built")
        if n_fft % 2 or not 1 <= hop_length <= n_fft:
            raise NotImplementedError(f"ISTFT: needs an even n_fft >= hop_length >= 1 (got {n_fft}, {hop_length})")
        self.padding = padding
        self.n_fft = n_fft
        self.hop_length = hop_length
        self.win_length = win_length
        self.register_buffer("window", torch.hann_window(win_length))
        self._cache = _DeviceCache()

    def prepared(self, device):
        def build():
            b = torch.from_numpy(istft_basis(self.window, self.n_fft).astype(np.float32)).contiguous().to(device)
            return b, _cpu(self.window).contiguous().to(device)
        return self._cache.get(_pkey(self.window) + (str(device),), build)

    def forward(self, spec):
        raise NotImplementedError("ISTFT runs fused inside ISTFTHead (bc_istft_head); a standalone complex-input call "
                                  "is not built")


# vq/codec_decoder.py:229-274
class ISTFTHead(nn.Module):
    def __init__(self, dim: int, n_fft: int, hop_length: int, padding: str = "same"):
        super().__init__()
        self.out = _Pointwise(dim, n_fft + 2)
        self.istft = ISTFT(n_fft=n_fft, hop_length=hop_length, win_length=n_fft, padding=padding)

    def run(self, x):
        """x (B, dim, F) -> (audio (B, 1, F * hop), x_pred (B, n_fft + 2, F))."""
        x_pred = self.out.run(x)
        basis, window = self.istft.prepared(x_pred.device)
        return ops.load().istft_head(x_pred, basis, window, self.istft.hop_length), x_pred

    def forward(self, x):
        """The reference's call shape: x (B, L, H)."""
        return self.run(_as_input(x).transpose(1, 2).contiguous())


# vq/codec_decoder.py:385-519
class ConformerDecoderISTFT(nn.Module):
    def __init__(self, in_channels=1024, hop_length=256, n_fft=1024, window_size=1024, dim=512, n_layers=12, n_head=8,
                 ffn_mult=4, conv_kernel_size=31, dropout=0.1, max_seq_len=8192, rope_theta=10000.0, causal=False,
                 fsq=False, fsq_levels=[4, 4, 4, 8], vq_num_quantizers=1, vq_commit_weight=0.25, vq_weight_init=False,
                 vq_full_commit_loss=False, codebook_size=8192, codebook_dim=8):
        super().__init__()
        if window_size != n_fft:
            raise NotImplementedError(f"ConformerDecoderISTFT: window_size {window_size} != n_fft {n_fft} is not built")
        self.hop_length = hop_length
        self.n_fft = n_fft
        self.fsq = fsq
        if fsq:
            self.quantizer = FSQ(levels=fsq_levels, channel_first=True, dim=in_channels)
            assert codebook_size == np.prod(fsq_levels), "codebook_size must be equal to the product of fsq_levels"
        else:
            self.quantizer = ResidualVQ(num_quantizers=vq_num_quantizers, dim=in_channels, codebook_size=codebook_size,
                                        codebook_dim=codebook_dim, threshold_ema_dead_code=2,
                                        commitment=vq_commit_weight, weight_init=vq_weight_init,
                                        full_commit_loss=vq_full_commit_loss)
        self.input_proj = Conv1dWN(in_channels, dim, kernel_size=1) if in_channels != dim else nn.Identity()
        self.conformer_backbone = ConformerBackbone(dim=dim, n_layers=n_layers, n_head=n_head, ffn_mult=ffn_mult,
                                                    conv_kernel_size=conv_kernel_size, dropout=dropout,
                                                    max_seq_len=max_seq_len, rope_theta=rope_theta, causal=causal,
                                                    conv_first=False)
        self.norm = RMSNorm(dim)
        self.head = ISTFTHead(dim=dim, n_fft=n_fft, hop_length=hop_length, padding="same")

    def decode(self, x, lengths=None, trace=None):
        """x (B, in_channels, F) -> audio (B, 1, F * hop).  trace: the first layer's intermediates and 'x_pred'."""
        _no_lengths(lengths)
        _eval_only(self)
        x = _as_input(x)
        if x.dim() != 3:
            raise ValueError("the decoder takes (B, C, F)")
        if x.shape[2] > self.conformer_backbone.freqs_cis.shape[0]:
            raise ValueError(f"{x.shape[2]} frames exceed max_seq_len {self.conformer_backbone.freqs_cis.shape[0]}")
        with L.status_scope():
            h = x if isinstance(self.input_proj, nn.Identity) else self.input_proj.run(x)
            h = self.norm.run(self.conformer_backbone.run(h, trace))
            audio, x_pred = self.head.run(h)
            if trace is not None:
                trace["x_pred"] = x_pred
            return audio

    def forward(self, x, vq=True, lengths=None):
        if vq is True:
            _eval_only(self)
            if self.fsq:
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

    def inference_vq(self, vq):
        return self.forward(vq[None, :, :], vq=False)

    def inference_0(self, x):
        x, q, loss = self.forward(x, vq=True)
        return self.forward(x, vq=False), None

    def inference(self, x):
        return self.forward(x, vq=False), None

    def remove_weight_norm(self):
        for m in self.modules():
            if m is not self and "weight_v" in m._parameters and hasattr(m, "remove_weight_norm"):
                m.remove_weight_norm()
