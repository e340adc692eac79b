"""The Conformer-STFT codec family restated as functions of a flat state dict on torch CPU ops: the written
definition the GPU tests compare against, in float32 (equal to the reference modules bit for bit: the fixtures of
tools/make_golden_conformer.py pin that) or in float64 (the error yardstick: a kernel may be off by at most 4 x the
float32 restatement's own distance from the float64 one).

Written from the math of the reference files named at each function; nothing here is used by the package."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import bigcodec_oracle as O


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def rmsnorm(x, eps=1e-6, w=None):
    """vq/module.py:357-370, over the last dimension: (x * rsqrt(mean x^2 + eps)) * w."""
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    return y if w is None else y * w


def freqs_cis(head_dim: int, end: int, theta: float):
    """vq/module.py:372-377 (always built in float32, as the reference does; a float64 run widens the table)."""
    f = 1.0 / (theta ** (torch.arange(0, head_dim, 2)[: head_dim // 2].float() / head_dim))
    ang = torch.outer(torch.arange(end, dtype=torch.float32), f)
    return torch.polar(torch.ones_like(ang), ang)


def rope(x, fc):
    """vq/module.py:387-397: x (B, T, H, D) as D / 2 complex numbers (interleaved pairs) times fc (T, D / 2)."""
    xc = torch.view_as_complex(x.reshape(*x.shape[:-1], -1, 2))
    return torch.view_as_real(xc * fc.view(1, x.shape[1], 1, -1)).flatten(3)


def attention_core(qkv, fc, n_head: int, causal: bool):
    """vq/module.py:421-449, manual branch: qkv (B, T, 3 * dim) -> (B, T, dim)."""
    B, T, C3 = qkv.shape
    D = C3 // 3 // n_head
    q, k, v = qkv.view(B, T, 3, n_head, D).unbind(2)
    q, k = rope(rmsnorm(q), fc), rope(rmsnorm(k), fc)
    q, k, v = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    s = torch.matmul(q, k.transpose(-2, -1)) / (D ** 0.5)
    if causal:
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool, device=s.device).triu(diagonal=1), float("-inf"))
    s = F.softmax(s, dim=-1, dtype=qkv.dtype)
    return torch.matmul(s, v).transpose(1, 2).reshape(B, T, C3 // 3)


def self_attention(sd, p, x, fc, n_head, causal, trace=None):
    """vq/module.py:416-453: x (B, C, T) -> (B, C, T)."""
    a = attention_core(F.linear(x.transpose(1, 2), sd[p + "qkv_proj.weight"]), fc, n_head, causal)
    if trace is not None:
        trace["attn"] = a.transpose(1, 2)
    return F.linear(a, sd[p + "out_proj.weight"]).transpose(1, 2)


def feed_forward(sd, p, x):
    """vq/module.py:467-470: x (B, T, C)."""
    return F.linear(F.silu(F.linear(x, sd[p + "w1.weight"])) * F.linear(x, sd[p + "w3.weight"]), sd[p + "w2.weight"])


def depthwise(x, w, b, causal: bool):
    """vq/module.py:477-480: CausalConv1d (left pad K - 1) or padding='same'."""
    K = w.shape[-1]
    if causal:
        return F.conv1d(F.pad(x, (K - 1, 0)), w, b, groups=x.shape[1])
    return F.conv1d(x, w, b, groups=x.shape[1], padding="same")


def conv_module(sd, p, x, causal):
    """vq/module.py:486-494: x (B, C, T)."""
    o = F.glu(F.conv1d(x, sd[p + "pointwise_conv1.weight"], sd[p + "pointwise_conv1.bias"]), dim=1)
    dp = p + ("depthwise_conv.conv." if causal else "depthwise_conv.")
    o = depthwise(o, sd[dp + "weight"], sd[dp + "bias"], causal)
    o = F.silu(rmsnorm(o.transpose(1, 2), 1e-6, sd[p + "conv_norm.weight"]).transpose(1, 2))
    return F.conv1d(o, sd[p + "pointwise_conv2.weight"], sd[p + "pointwise_conv2.bias"])


def layer(sd, p, x, fc, n_head, causal, conv_first, trace=None):
    """vq/module.py:512-526: x (B, C, T)."""
    def norm(name, x):
        return rmsnorm(x.transpose(1, 2), 1e-6, sd[p + name + ".weight"])

    def conv(x):
        return x + conv_module(sd, p + "conv.", norm("conv_norm_in", x).transpose(1, 2), causal)

    def attn(x):
        return x + self_attention(sd, p + "self_attn.", norm("attn_norm_in", x).transpose(1, 2), fc, n_head, causal, trace)

    steps = (("conv", conv), ("attn_out", attn)) if conv_first else (("attn_out", attn), ("conv", conv))
    t = trace if trace is not None else {}
    x = t[steps[0][0]] = steps[0][1](x)
    x = t["ffn1"] = x + feed_forward(sd, p + "ffn1.", norm("ffn1_norm_in", x)).transpose(1, 2)
    x = t[steps[1][0]] = steps[1][1](x)
    x = t["ffn2"] = x + feed_forward(sd, p + "ffn2.", norm("ffn2_norm_in", x)).transpose(1, 2)
    return x


def backbone(sd, p, x, kw, conv_first, trace=None):
    """vq/module.py:541-547."""
    fc = freqs_cis(kw["dim"] // kw["n_head"], kw["max_seq_len"], kw["rope_theta"])[: x.shape[-1]]
    fc = fc.to(x.device)
    if x.dtype == torch.float64:
        fc = fc.to(torch.complex128)
    for i in range(kw["n_layers"]):
        x = layer(sd, f"{p}layers.{i}.", x, fc, kw["n_head"], kw["causal"], conv_first, trace if i == 0 else None)
    return x


def maybe_wn_conv(sd, p, x):
    """weight_norm(nn.Conv1d(.., 1)) when the keys exist (codec_encoder.py:174-177), the identity otherwise."""
    if p + "weight_v" not in sd:
        return x
    return F.conv1d(x, torch._weight_norm(sd[p + "weight_v"], sd[p + "weight_g"], 0), sd[p + "bias"])


def stft_features(x, window, n_fft, hop):
    """vq/codec_encoder.py:108-122, 188-192: x (B, 1, T) -> (B, n_fft + 2, F), real rows then imaginary rows."""
    pad = (window.numel() - hop) // 2
    s = torch.stft(F.pad(x.squeeze(1), (pad, pad)), n_fft=n_fft, hop_length=hop, window=window, center=False,
                   pad_mode="constant", return_complex=True)
    return torch.cat([s.real, s.imag], dim=1)


def encoder(sd, kw, x, trace=None):
    """vq/codec_encoder.py:181-206."""
    t = trace if trace is not None else {}
    f = t["stft"] = stft_features(x, sd["stft.window"], kw["n_fft"], kw["hop_length"])
    h = F.conv1d(f, sd["input_proj.weight"], sd["input_proj.bias"])
    h = t["input_norm"] = rmsnorm(h.transpose(1, 2), 1e-6, sd["input_norm.weight"]).transpose(1, 2)
    h = backbone(sd, "conformer_backbone.", h, kw, True, trace)
    h = rmsnorm(h.transpose(1, 2), 1e-6, sd["norm.weight"]).transpose(1, 2)
    return maybe_wn_conv(sd, "output_proj.", h)


def istft(spec, window, n_fft, hop):
    """vq/codec_decoder.py:186-213 with padding='same': spec (B, bins, F) complex -> (B, F * hop)."""
    pad = (n_fft - hop) // 2
    Fr = spec.shape[2]
    fr = torch.fft.irfft(spec, n_fft, dim=1, norm="backward") * window[None, :, None]
    size = (Fr - 1) * hop + n_fft
    fold = dict(output_size=(1, size), kernel_size=(1, n_fft), stride=(1, hop))
    y = F.fold(fr, **fold)[:, 0, 0, pad:-pad]
    env = F.fold(window.square().expand(1, Fr, -1).transpose(1, 2), **fold).squeeze()[pad:-pad]
    return y / env


def istft_head(x_pred, window, n_fft, hop):
    """vq/codec_decoder.py:261-274 after self.out: x_pred (B, n_fft + 2, F) -> (B, 1, F * hop)."""
    mag, p = x_pred.chunk(2, dim=1)
    mag = torch.clip(torch.exp(mag), max=1e2)
    return istft(mag * (torch.cos(p) + 1j * torch.sin(p)), window, n_fft, hop).unsqueeze(1)


def decoder(sd, kw, x, trace=None):
    """vq/codec_decoder.py:471-485."""
    t = trace if trace is not None else {}
    h = backbone(sd, "conformer_backbone.", maybe_wn_conv(sd, "input_proj.", x), kw, False, trace)
    h = rmsnorm(h.transpose(1, 2), 1e-6, sd["norm.weight"])
    xp = t["x_pred"] = F.linear(h, sd["head.out.weight"], sd["head.out.bias"]).transpose(1, 2)
    return istft_head(xp, sd["head.istft.window"], kw["n_fft"], kw["hop_length"])


def quantize(sd, latent):
    """The decoder's vq=True call: the project's pinned oracle of the same ResidualVQ (post, codes, loss)."""
    return O.rvq_forward(latent, sd)


# the intermediates of layer 0 recorded in the fixtures, in flow order
ENC_TRACE = ("stft", "input_norm", "conv", "ffn1", "attn", "attn_out", "ffn2")
DEC_TRACE = ("attn", "attn_out", "ffn1", "conv", "ffn2", "x_pred")
