"""The ResLSTM matrix's cases, references, metric and bound (tests/test_lstm_matrix_host.py proves the bound can tell a
dropped operand plane from fp32 arithmetic; tests/test_gpu_lstm_matrix.py applies it to the kernels, and
tests/test_gpu_lstm_bidir_matrix.py to the bidirectional call: a BiCase next to Case, through the same functions).

The metric is taken on the recurrence's own output h, never on x + h: x ~ N(0, 1) peaks at 4.5 while |h| < 1, so an
error relative to max |x + h| hides a recurrence that lost a whole operand plane.  W_hh is scaled up
(whh_scale 3-4) and T kept short: the recurrent term then carries most of the gate pre-activation, so an operand that
lost its low bits shows, while the map is still far from the chaotic regime (whh_scale 8) where fp32 itself drifts."""
import collections
import functools
import types
import warnings

import numpy as np
import torch
from torch import nn

Case = collections.namedtuple("Case", "H layers B T seed whh_scale state")


class BiCase(collections.namedtuple("BiCase", "D layers B T seed whh_scale mirror")):
    """A bidirectional case: nn.LSTM(D, D / 2, layers, bidirectional=True) on x (B, D, T); no carried state.  mirror:
    the two channel halves of x are equal (tests/test_gpu_lstm_bidir_matrix.py::test_bidir_mirror_identity)."""
    __slots__ = ()
    state = False

    @property
    def H(self):
        return self.D // 2


# The table of cases: H -> (layers, T, whh_scale).  H = 256, 512, 1024, 1536 run the persistent kernel in x6 / h3 and
# lstm_step_frag_kernel in fp32 mode, 128 the latter in every mode, 48, 64 and 768 lstm_step_kernel in every mode.
SHAPES = {48: (2, 24, 3.0), 64: (2, 24, 3.0), 128: (2, 24, 4.0), 256: (2, 24, 4.0), 512: (2, 16, 4.0),
          768: (2, 24, 4.0), 1024: (2, 12, 4.0), 1536: (2, 8, 4.0)}
SEQ_H = (256, 512, 1024, 1536)         # lstm_seq2_x6_kernel<H / 128, P, NTH>
FRAG_H = (128, 256, 512, 1024, 1536)   # lstm_step_frag_kernel<H / 32>
STEP_H = (48, 64, 768)                 # lstm_step_kernel
B_MAIN = 130   # clips of a main case: the largest launch any leg makes (a launch of n clips is compared with ref[:n])
B_STATE = 70   # clips of a carried-state case: the second launch chunk starts at clip 64

# The bidirectional cases: D -> (layers, T, whh_scale), H = D / 2 per direction.  96 runs lstm_step_kernel (H = 48),
# 256 lstm_step_frag_kernel (128), 512 ... 3072 the persistent kernel in x6 / h3 and the frag kernel in fp32 mode, 1536
# (the default preset's width, H = 768) lstm_step_kernel in every mode; "512L" crosses a 32-step tile of the transposes.
BIDIR_SHAPES = {96: (2, 24, 3.0), 256: (2, 24, 4.0), 512: (2, 24, 4.0), 1024: (2, 16, 4.0), 1536: (2, 24, 4.0),
                2048: (2, 12, 4.0), 3072: (2, 8, 4.0), "512L": (2, 33, 4.0)}
BIDIR_SEQ_D = (512, 1024, 2048, 3072)
B_BIDIR = 70   # clips of a bidirectional case: the second launch chunk starts at clip 64

# bound = K[prec] * (error of torch's fp32 CPU LSTM on the same case): twice the largest ratio (kernel error) / cpu32
# measured on the MI355X over the whole matrix: x6 2.27, h3 1.60, fp32 mode 1.59 (DESIGN.md §19 has them per case;
# profiles/lstm_matrix_ratios.txt is the log).  bf16 precision runs the h3 recurrence.
K = {"x6": 4.6, "h3": 3.2, "bf16": 3.2, "fp32": 3.2}
# The bidirectional cases' own K, by the same rule: their largest measured ratios, x6 3.09 and fp32 mode 2.16 (both on
# D = 2048 at n = 65 / 70) and h3 1.62 (D = 3072), exceed K / 2, so K_BIDIR is twice each of them.  None exceeds twice
# the unidirectional ratio of its precision (profiles/lstm_bidir_matrix_ratios.txt is the log).
K_BIDIR = {"x6": 6.18, "h3": 3.24, "bf16": 3.24, "fp32": 4.32}
# Precisions whose bound is proved (tests/test_lstm_matrix_host.py) to sit below half the error of a dropped third
# bf16 plane on every case.  None: native fp32 arithmetic itself comes within 1.6x of cpu32 on the max metric, a dropped
# plane is only 3.3-11x cpu32, so K = 2 x 1.6 cannot leave the factor 2 the proof wants.  Such a
# precision's bound is proved against a single-plane operand instead (three orders of magnitude above it).
LOW_PLANE_PROVEN = ()


def make_case(H, layers, B, T, seed, whh_scale, state=False):
    """Parameters U(+-1 / sqrt(H)) with weight_hh_* multiplied by whh_scale, x ~ N(0, 1) of shape (B, H, T); with state,
    a given h0 = 0.5 U(+-1) and c0 ~ N(0, 1) laid out [layers][H][B].  The key of data(), ref64() and cpu32()."""
    return Case(H, layers, B, T, seed, float(whh_scale), bool(state))


def main_case(H):
    layers, T, s = SHAPES[H]
    return make_case(H, layers, B_MAIN, T, H, s)


def state_case(H):
    layers, T, s = SHAPES[H]
    return make_case(H, layers, B_STATE, T, H, s, state=True)


def bidir_case(key, T=None, layers=None, mirror=False):
    """The bidirectional case of a BIDIR_SHAPES key.  The seed is D and the parameters are drawn before x, layer 0
    first, so every case of one D -- "512L", another T, one layer -- has the same parameters; x is drawn per case."""
    nl, t, s = BIDIR_SHAPES[key]
    D = int(str(key).rstrip("L"))
    return BiCase(D, layers or nl, B_BIDIR, T or t, D, float(s), bool(mirror))


def is_bidir(case):
    return isinstance(case, BiCase)


def bidir_precs(case):
    """Precisions the GPU matrix runs a bidirectional case in."""
    if case.H in SEQ_H:
        return ("x6", "h3", "fp32")
    return ("fp32", "x6") if case.D == 1536 else ("fp32",)


def _torch_module(case):
    if is_bidir(case):
        return nn.LSTM(case.D, case.H, case.layers, batch_first=True, bidirectional=True)
    return nn.LSTM(case.H, case.H, case.layers, batch_first=True)


@functools.lru_cache(maxsize=None)
def data(case):
    """params (torch.nn.LSTM's names), x, h0, c0 of a case; shared and never written."""
    g = torch.Generator().manual_seed(case.seed)
    H = case.H
    params = {}
    for name, p in _torch_module(case).named_parameters():
        v = (torch.rand(p.shape, generator=g) * 2 - 1) / np.sqrt(H)
        params[name] = v * case.whh_scale if name.startswith("weight_hh") else v
    if is_bidir(case):
        x = torch.randn(case.B, case.D, case.T, generator=g)
        if case.mirror:
            x[:, H:] = x[:, :H]
        return types.SimpleNamespace(params=params, x=x, h0=None, c0=None)
    x = torch.randn(case.B, H, case.T, generator=g)
    h0 = c0 = None
    if case.state:
        h0 = 0.5 * (torch.rand(case.layers, H, case.B, generator=g) * 2 - 1)
        c0 = torch.randn(case.layers, H, case.B, generator=g)
    return types.SimpleNamespace(params=params, x=x, h0=h0, c0=c0)


def torch_lstm(case, dtype):
    """torch.nn.LSTM on the CPU in dtype: (h (B, H, T) without the residual, h_n, c_n [layers][H][B]).  On torch's own
    cell loop: the oneDNN RNN primitive an fp32 inference call would otherwise take approximates the nonlinearities and is
    2-4x further from fp64 (3.5e-6 on h_n at H = 1536), which is no measure of fp32 arithmetic."""
    d = data(case)
    m = _torch_module(case).to(dtype)  # (a BiCase: h is (B, D, T), h_n and c_n [2 layers][H][B], forward then reverse)
    m.load_state_dict({k: v.to(dtype) for k, v in d.params.items()})
    st = None if d.h0 is None else (d.h0.to(dtype).transpose(1, 2).contiguous(), d.c0.to(dtype).transpose(1, 2).contiguous())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (flags() warns about a TF32 switch of GPUs this build does not have)
        with torch.no_grad(), torch.backends.mkldnn.flags(enabled=False):
            y, (hn, cn) = m(d.x.to(dtype).transpose(1, 2), st)
    return y.transpose(1, 2).contiguous(), hn.transpose(1, 2).contiguous(), cn.transpose(1, 2).contiguous()


@functools.lru_cache(maxsize=None)
def ref64(case):
    """The reference: torch.nn.LSTM in float64, one per case, shared by every precision and launch size."""
    return torch_lstm(case, torch.float64)


def planes(v, n):
    """The sum of the first n bf16 planes of v (3 planes hold an fp32 value exactly: the x6 operand)."""
    r, s = v.clone(), torch.zeros_like(v)
    for _ in range(n):
        p = r.to(torch.bfloat16).to(v.dtype)
        s, r = s + p, r - p
    return s


def _manual_bidir(case, dtype, f):
    """manual_lstm of a BiCase: per layer the forward direction over the (B, T, D) input and the reverse direction over
    its time reversal, reversed back, concatenated [forward | reverse] (torch's order), h_n / c_n likewise."""
    d, H = data(case), case.H
    inp = d.x.to(dtype).transpose(1, 2)  # (B, T, D)
    hn, cn = [], []
    for l in range(case.layers):
        outs = []
        for sfx, fw, fh in (("", f["fw"], f["fh"]), ("_reverse", f["fw_r"], f["fh_r"])):
            p = {k: d.params[f"{k}_l{l}{sfx}"].to(dtype) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
            wih = torch.cat([p["weight_ih"][:, :H], f["fih"](p["weight_ih"][:, H:])], dim=1)
            xin = inp.flip(1) if sfx else inp
            gx = xin @ wih.t() + (p["bias_ih"] + p["bias_hh"])
            whh = fw(p["weight_hh"]).t()
            h = torch.zeros(case.B, H, dtype=dtype)
            c = torch.zeros(case.B, H, dtype=dtype)
            out = []
            for t in range(case.T):
                i, fg, g, o = (gx[:, t] + fh(h) @ whh).chunk(4, dim=1)
                c = torch.sigmoid(fg) * c + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
                out.append(h)
            y = torch.stack(out, dim=1)
            outs.append(y.flip(1) if sfx else y)
            hn.append(h.t())
            cn.append(c.t())
        inp = torch.cat(outs, dim=2)
    return inp.transpose(1, 2).contiguous(), torch.stack(hn).contiguous(), torch.stack(cn).contiguous()


def manual_lstm(case, dtype, fw=None, fh=None, fw_r=None, fh_r=None, fih=None):
    """The cell loop written out: gx = x W_ih^T + b, g = gx + f_h(h) f_w(W_hh)^T, gates i, f, g, o in torch's order.
    fw / fh degrade the recurrent operands (e.g. lambda v: planes(v, 2)).  A BiCase has five places a fault can sit, each
    degraded on its own: W_hh and h of the forward direction (fw, fh), of the reverse direction (fw_r, fh_r), and the
    [H, 2H) columns of every W_ih (fih: what reads the reverse half of the input and of the previous layer)."""
    d = data(case)
    ident = lambda v: v
    if is_bidir(case):
        return _manual_bidir(case, dtype, {k: v or ident for k, v in
                                           dict(fw=fw, fh=fh, fw_r=fw_r, fh_r=fh_r, fih=fih).items()})
    assert fw_r is None and fh_r is None and fih is None
    fw, fh = fw or ident, fh or ident
    inp = d.x.to(dtype).transpose(1, 2)  # (B, T, H)
    hn, cn = [], []
    for l in range(case.layers):
        p = {k: d.params[f"{k}_l{l}"].to(dtype) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
        gx = inp @ p["weight_ih"].t() + (p["bias_ih"] + p["bias_hh"])
        whh = fw(p["weight_hh"]).t()
        h = torch.zeros(case.B, case.H, dtype=dtype) if d.h0 is None else d.h0[l].t().to(dtype)
        c = torch.zeros(case.B, case.H, dtype=dtype) if d.c0 is None else d.c0[l].t().to(dtype)
        out = []
        for t in range(case.T):
            i, f, g, o = (gx[:, t] + fh(h) @ whh).chunk(4, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            out.append(h)
        inp = torch.stack(out, dim=1)
        hn.append(h.t())
        cn.append(c.t())
    return inp.transpose(1, 2).contiguous(), torch.stack(hn).contiguous(), torch.stack(cn).contiguous()


def rel_h(a, ref, scale=None):
    """max |a - ref| / max |ref| on the recurrence output (for a GPU result: got - x; x is the fp32 input and the
    residual add is one rounding, which cpu32 pays too).  scale: max |ref| of the whole case when a and ref are a slice
    of it (a few clips, the first step), so that the figure stays on the scale the bound was derived on."""
    a, ref = a.double(), ref.double()
    return float((a - ref).abs().max() / (scale if scale is not None else ref.abs().max().clamp_min(1e-30)))


def rel_h_halves(a, ref, scale=None):
    """rel_h of a bidirectional output (B, D, T): (whole, forward half [0, H), reverse half [H, 2H)), all three on the
    whole output's scale."""
    H = ref.shape[1] // 2
    s = scale if scale is not None else float(ref.double().abs().max().clamp_min(1e-30))
    return rel_h(a, ref, s), rel_h(a[:, :H], ref[:, :H], s), rel_h(a[:, H:], ref[:, H:], s)


@functools.lru_cache(maxsize=None)
def scales(case):
    """max |ref| of h, h_n and c_n over the whole case."""
    return tuple(float(r.abs().max()) for r in ref64(case))


def worst(a, ref, dims=("clip", "unit", "step"), bidir=False):
    """Where the largest |a - ref| sits: of an output (clips, units, steps), or of a state with dims (layer, unit, clip);
    bidir: a bidirectional output (B, D, T), and which channel half (direction) the element is in."""
    d = (a.double() - ref.double()).abs()
    i = tuple(int(v) for v in np.unravel_index(int(d.argmax()), d.shape))
    half = f" ({'forward' if i[1] < a.shape[1] // 2 else 'reverse'} half)" if bidir else ""
    return ("worst at " + ", ".join(f"{n} {v}" for n, v in zip(dims, i)) + half +
            f": got {float(a[i])!r}, want {float(ref[i])!r}")


@functools.lru_cache(maxsize=None)
def cpu32(case):
    """Error of torch's fp32 CPU LSTM on the case, residual add and removal included as a GPU result pays them:
    (rel_h of h, of h_n, of c_n)."""
    d = data(case)
    y, hn, cn = torch_lstm(case, torch.float32)
    r = ref64(case)
    return rel_h((y + d.x) - d.x, r[0]), rel_h(hn, r[1]), rel_h(cn, r[2])


def bound(case, prec):
    """The largest rel_h a kernel may show on the case: K[prec] times the larger fp32 CPU error of h, h_n and c_n (the
    three are values of the same recurrence; the final state alone is a noisier, smaller sample of it).  A BiCase takes
    K_BIDIR."""
    return (K_BIDIR if is_bidir(case) else K)[prec] * max(cpu32(case))
