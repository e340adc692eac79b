"""Plain-torch restatements of the waveform decoder's two resampling pieces, in the dtype of their inputs (float64: the
reference of tests/test_gpu_convt_matrix.py and tests/test_gpu_aa_matrix.py; float32: the same arithmetic at the
kernels' width, the yardstick of the activation's bound).  tests/test_convt_matrix_host.py checks them against each
other and against the library's host functions.

ConvTranspose1d (csrc/abi.hip bc_convT1d_fwd / bc_convT1d_fwd_ws).  y[t] = bias + sum_{i, k: s i - p + k = t} W[k] x[i]
for t in [0, Tout), Tout = (Tin - 1) s - 2 p + K + output_padding - crop: output_padding extends the output past the
last tap (bias alone), crop removes the last samples (CausalConvTranspose1d crops s).  Polyphase form: with
Kp = ceil(K / s), output t = s q - p + r of phase r in [0, s) is the stride-1 conv
    y_r[q] = sum_{j' < Kp} W[r + s (Kp - 1 - j')] x[q - (Kp - 1) + j']      (a weight index >= K is a zero tap)
over q in [q_lo, q_lo + n_out), q_lo = ceil((p - r) / s) (never negative), q_hi = floor((Tout - 1 + p - r) / s).
The workspace path keeps every phase's row at Q4 = max n_out rounded up to 4 floats: s * B * Cout * Q4 floats.

Anti-aliased Snake (csrc/elementwise.hip aa_snake_kernel / aa_snake_gen_kernel; modules.py UpSample1d, DownSample1d,
LowPassFilter1d).  Up: replicate pad P = Ku // ru - 1 on both sides, depthwise transposed conv of stride ru, times ru,
crop PL = P ru + (Ku - ru) // 2 on the left and PR = P ru + (Ku - ru + 1) // 2 on the right (length T ru); SnakeBeta;
down: replicate pad (Kd // 2 - [Kd even], Kd // 2), depthwise conv of stride rd.  oracle.upsample2 slices
[PL:-PR], which is empty at PR = 0 (Ku = ru); the crop here is written with the length, which is what the kernel
computes."""
import torch
import torch.nn.functional as F


def ceil_div(a, b):
    return -(-a // b)


def phase_taps(K, s):
    return ceil_div(K, s)


def wn_weight(v, g, dtype):
    """g * v / ||v||, the norm over every dim but 0 (ConvTranspose1dWN: dim 0 = input channels), formed in `dtype`."""
    v, g = v.to(dtype), g.to(dtype)
    n = torch.sqrt((v * v).sum(dim=tuple(range(1, v.dim())), keepdim=True))
    return g * v / n


def out_len(Tin, s, K, p, output_padding, crop):
    return (Tin - 1) * s - 2 * p + K + output_padding - crop


def supported(s, K, p):
    """bc_convT1d_fwd refuses (BC_ERR_UNSUPPORTED) a padding beyond s (Kp - 1): phase 0 would start at q_lo > Kp - 1,
    a negative left pad of its stride-1 conv."""
    return p <= s * (phase_taps(K, s) - 1)


def phases(Tout, s, p):
    """[(q_lo, n_out)] per phase r."""
    out = []
    for r in range(s):
        q_lo = ceil_div(p - r, s) if p > r else 0
        num = Tout - 1 + p - r
        q_hi = num // s if num >= 0 else -1
        out.append((q_lo, max(0, q_hi - q_lo + 1)))
    return out


def q4(Tout, s, p):
    return ceil_div(max(n for _, n in phases(Tout, s, p)), 4) * 4


def workspace_floats(B, Cout, Tout, s, p, dual):
    return s * B * Cout * q4(Tout, s, p) * (2 if dual else 1)


def phase_weight(w, r, s):
    """(Cout, Cin, Kp) stride-1 conv weight of phase r from the transposed conv's (Cin, Cout, K) weight."""
    Cin, Cout, K = w.shape
    Kp = phase_taps(K, s)
    wr = w.new_zeros(Cout, Cin, Kp)
    for jp in range(Kp):
        k = r + s * (Kp - 1 - jp)
        if k < K:
            wr[:, :, jp] = w[:, :, k].t()
    return wr


def _fold(x, w):
    return wn_weight(w[0], w[1], x.dtype) if isinstance(w, (tuple, list)) else w.to(x.dtype)


def convt(x, w, bias, s, p, output_padding, crop):
    """F.conv_transpose1d in the dtype of x; w is the folded (Cin, Cout, K) weight or the weight-norm pair (v, g)."""
    y = F.conv_transpose1d(x, _fold(x, w), None if bias is None else bias.to(x.dtype), s, p, output_padding)
    return y[..., :y.shape[-1] - crop]


def convt_polyphase(x, w, bias, s, p, output_padding, crop):
    """The same values as s stride-1 convs; returns (y, [(q_lo, n_out)] per phase)."""
    wf = _fold(x, w)
    Cin, Cout, K = wf.shape
    B, _, Tin = x.shape
    Kp = phase_taps(K, s)
    Tout = out_len(Tin, s, K, p, output_padding, crop)
    ph = phases(Tout, s, p)
    y = x.new_full((B, Cout, max(Tout, 0)), float("nan"))
    b = None if bias is None else bias.to(x.dtype)
    for r, (q_lo, n) in enumerate(ph):
        if n == 0:
            continue
        xp = F.pad(x, (Kp - 1, max(0, q_lo + n - Tin)))  # conv1d(xp)[q] = sum_j' w_r[j'] x[q - (Kp - 1) + j']
        yr = F.conv1d(xp, phase_weight(wf, r, s), b)[..., q_lo:q_lo + n]
        t0 = s * q_lo - p + r
        y[..., t0:t0 + s * (n - 1) + 1:s] = yr
    return y, ph


def snake(x, alpha, beta):
    """x + beta sin^2(alpha x) per channel, alpha and beta the kernels' operands (SnakeBeta.coeffs: exp(alpha) and
    1 / (exp(beta) + 1e-9), float32 values) cast to the dtype of x."""
    a, b = alpha.to(x.dtype).reshape(1, -1, 1), beta.to(x.dtype).reshape(1, -1, 1)
    return x + b * torch.sin(x * a) ** 2


def aa_out_len(T, ru, rd, kd):
    n = T * ru + (kd // 2 - (1 if kd % 2 == 0 else 0)) + kd // 2 - kd
    return 0 if n < 0 else n // rd + 1


def aa_up(x, fup, ru):
    C, ku = x.shape[1], fup.numel()
    pad = ku // ru - 1
    pl = pad * ru + (ku - ru) // 2
    xp = F.pad(x, (pad, pad), mode="replicate")
    u = ru * F.conv_transpose1d(xp, fup.to(x.dtype).reshape(1, 1, ku).expand(C, 1, ku), stride=ru, groups=C)
    return u[..., pl:pl + x.shape[-1] * ru]


def aa_down(z, fdown, rd):
    C, kd = z.shape[1], fdown.numel()
    zp = F.pad(z, (kd // 2 - (1 if kd % 2 == 0 else 0), kd // 2), mode="replicate")
    return F.conv1d(zp, fdown.to(z.dtype).reshape(1, 1, kd).expand(C, 1, kd), stride=rd, groups=C)


def aa_act(x, alpha, beta, fup, fdown, ru, rd):
    """Activation1d(antialias=True) in the dtype of x; alpha / beta as in snake(), the filters the float32 values the
    kernel receives."""
    return aa_down(snake(aa_up(x, fup, ru), alpha, beta), fdown, rd)
