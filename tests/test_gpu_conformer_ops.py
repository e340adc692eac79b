"""The kernels of csrc/conformer.hip on the MI355X, one at a time, against the float64 restatement
(tests/conformer_ref.py), and their torch.ops.bigcodec.* wrappers.

Bound of a kernel case: max |got - ref64| <= min(4 x max |ref32 - ref64|, 1e-4 x max |ref64|), ref32 / ref64 the
restatement in float32 / float64 on the same inputs, recomputed by the case (tests/test_metrics_host.py does the same).
Operands and outputs of the raw C calls sit between NaN guard bands, and outputs start as NaN: a NaN left in an output
(an element never written) or a touched band fails the case."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conformer_ref as R
from audiotokenization_amd import _lib as L
from audiotokenization_amd import conformer as cf
from audiotokenization_amd import ops

pytestmark = pytest.mark.gpu

BAND = 512


def gen(seed):
    return torch.Generator().manual_seed(seed)


class Banded:
    """A contiguous fp32 device tensor of `shape` between two NaN bands (NaN itself unless `src` is given)."""

    def __init__(self, shape, dev, src=None):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * BAND,), float("nan"), device=dev)
        self.t = self.buf[BAND:BAND + self.n].view(shape)
        if src is not None:
            self.t.copy_(src)

    def intact(self):
        return bool(torch.isnan(self.buf[:BAND]).all() and torch.isnan(self.buf[BAND + self.n:]).all())


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def check(out: Banded, ins, ref32, ref64, what):
    got = out.t.detach().cpu().double()
    assert not torch.isnan(got).any(), f"{what}: NaN in the output"
    assert out.intact() and all(i.intact() for i in ins), f"{what}: a guard band was written"
    scale = float(ref64.abs().max())
    own = float((ref32.double() - ref64).abs().max())
    bound = min(4.0 * own, 1e-4 * scale)
    err = float((got - ref64).abs().max())
    print(f"{what}: err {err:.3e}, float32 restatement {own:.3e}, bound {bound:.3e}, max|ref| {scale:.3e}")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"
    return got


def tiles():
    q, k = (np.zeros(1, np.int32) for _ in range(2))
    L.call("bc_attention_tiles", q.ctypes.data, k.ctypes.data)
    return int(q[0]), int(k[0])


# ---- STFT ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop", [(800, 200), (32, 8)])
@pytest.mark.parametrize("T", [200, 400, 1000, 1199])
def test_stft_frames(dev, T, n_fft, hop):
    B = 2
    x = torch.rand(B, 1, T, generator=gen(T + n_fft)) - 0.5
    w = torch.hann_window(n_fft)
    ref32 = R.stft_features(x, w, n_fft, hop)
    ref64 = R.stft_features(x.double(), w.double(), n_fft, hop)
    Fr = ref64.shape[2]
    assert Fr == 1 + (T + n_fft - hop - n_fft) // hop
    xi = Banded((B, T), dev, x[:, 0])
    bi = Banded((n_fft, n_fft + 2), dev, torch.from_numpy(cf.stft_basis_t(w, n_fft).astype(np.float32)))
    out = Banded((B, n_fft + 2, Fr), dev)
    L.call("bc_stft_frames", xi.t.data_ptr(), bi.t.data_ptr(), out.t.data_ptr(), B, T, n_fft, hop, n_fft, stream(dev))
    check(out, (xi, bi), ref32, ref64, f"stft T={T} n_fft={n_fft}")


# ---- RMSNorm ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["gain", "plain", "silu"])
@pytest.mark.parametrize("T", [1, 7, 129])
@pytest.mark.parametrize("C", [40, 64, 256])
def test_rmsnorm(dev, C, T, variant):
    B = 2
    x = torch.randn(B, C, T, generator=gen(C * 1000 + T)) * 3.0
    x[0, :, 0] = 0.0  # an all-zero column: rsqrt(eps) times zero
    w = None if variant == "plain" else torch.rand(C, generator=gen(C)) * 0.5 + 0.75

    def ref(x, w):
        y = R.rmsnorm(x.transpose(1, 2), 1e-6, w).transpose(1, 2)
        return F.silu(y) if variant == "silu" else y

    ref32, ref64 = ref(x, w), ref(x.double(), None if w is None else w.double())
    assert float(ref64[0, :, 0].abs().max()) == 0.0
    xi, out = Banded((B, C, T), dev, x), Banded((B, C, T), dev)
    wi = Banded((C,), dev, w) if w is not None else None
    L.call("bc_rmsnorm_fwd", xi.t.data_ptr(), wi.t.data_ptr() if wi else None, out.t.data_ptr(), B, C, T, 1e-6,
           1 if variant == "silu" else 0, stream(dev))
    check(out, (xi,) + ((wi,) if wi else ()), ref32, ref64, f"rmsnorm C={C} T={T} {variant}")


# ---- GLU + depthwise conv --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("C", [40, 64])
@pytest.mark.parametrize("T", [1, 5, 31, 200, 257])  # (257: a second tile of the row)
@pytest.mark.parametrize("K", [4, 5, 31])
def test_dwconv_glu(dev, K, T, C, causal):
    B = 2
    g = gen(K * 100000 + T * 100 + C)
    x = torch.randn(B, 2 * C, T, generator=g) * 2.0
    w = (torch.rand(C, 1, K, generator=g) - 0.5) * (2.0 / math.sqrt(K))
    b = torch.rand(C, generator=g) - 0.5

    def ref(x, w, b):
        return R.depthwise(F.glu(x, dim=1), w, b, causal)

    ref32, ref64 = ref(x, w, b), ref(x.double(), w.double(), b.double())
    xi, wi, bi, out = Banded(x.shape, dev, x), Banded(w.shape, dev, w), Banded(b.shape, dev, b), Banded((B, C, T), dev)
    L.call("bc_dwconv_glu_fwd", xi.t.data_ptr(), wi.t.data_ptr(), bi.t.data_ptr(), out.t.data_ptr(), B, C, T, K,
           K - 1 if causal else (K - 1) // 2, stream(dev))
    check(out, (xi, wi, bi), ref32, ref64, f"dwconv K={K} T={T} C={C} causal={causal}")


# ---- SwiGLU ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,T", [(256, 1), (768, 33), (40, 129)])
def test_swiglu(dev, H, T):
    B = 2
    h = torch.randn(B, 2 * H, T, generator=gen(H + T)) * 4.0

    def ref(h):
        return F.silu(h[:, :H]) * h[:, H:]

    hi, out = Banded(h.shape, dev, h), Banded((B, H, T), dev)
    L.call("bc_swiglu_fwd", hi.t.data_ptr(), out.t.data_ptr(), B, H, T, stream(dev))
    check(out, (hi,), ref(h), ref(h.double()), f"swiglu H={H} T={T}")


# ---- attention -------------------------------------------------------------------------------------------------------
def attention_lengths():
    try:
        q, k = tiles()
    except Exception:  # collection without the library (no GPU): the kernel's sizes as built
        q, k = 128, 64
    return sorted({1, 2, 200, q - 1, q, q + 1, 2 * q + 1, k - 1, k, k + 1, 2 * k + 1})


def attention_case(dev, D, T, causal, seed=0):
    B, H = 2, 2
    dim = H * D
    g = gen(seed + D * 1000 + T)
    qkv = torch.randn(B, 3 * dim, T, generator=g)
    # raw q / k magnitudes from 1e-3 to 1e3 per (b, head, t): the RMS norm has work to do
    scale = 10.0 ** (torch.rand(B, 2 * H, 1, T, generator=g) * 6.0 - 3.0)
    qkv[:, :2 * dim] = (qkv[:, :2 * dim].view(B, 2 * H, D, T) * scale).view(B, 2 * dim, T)
    fc = R.freqs_cis(D, 512, 500.0)
    btc = qkv.transpose(1, 2).contiguous()
    ref32 = R.attention_core(btc, fc[:T], H, causal).transpose(1, 2)
    ref64 = R.attention_core(btc.double(), fc[:T].to(torch.complex128), H, causal).transpose(1, 2)
    qi = Banded(qkv.shape, dev, qkv)
    ri = Banded((512, D // 2, 2), dev, torch.view_as_real(fc))
    out = Banded((B, dim, T), dev)
    L.call("bc_attention_fwd", qi.t.data_ptr(), ri.t.data_ptr(), out.t.data_ptr(), B, H, D, T, int(causal), stream(dev))
    got = check(out, (qi, ri), ref32, ref64, f"attention D={D} T={T} causal={causal}")
    return qi, ri, got


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("T", attention_lengths())
@pytest.mark.parametrize("D", [32, 64])
def test_attention(dev, D, T, causal):
    qi, ri, got = attention_case(dev, D, T, causal)
    if causal:  # row 0 sees one key: the non-causal result of the first frame alone, bit for bit
        B, dim = qi.t.shape[0], qi.t.shape[1] // 3
        first = Banded((B, 3 * dim, 1), dev, qi.t[:, :, :1])
        one = Banded((B, dim, 1), dev)
        L.call("bc_attention_fwd", first.t.data_ptr(), ri.t.data_ptr(), one.t.data_ptr(), B, 2, D, 1, 0, stream(dev))
        assert torch.equal(one.t.cpu().double(), got[:, :, :1])
        assert torch.equal(one.t.cpu(), qi.t[:, 2 * dim:, :1].cpu())  # softmax over one key is 1: the value itself


# ---- ISTFT head ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,Fr", [(800, 200, f) for f in (1, 2, 3, 4, 5, 9, 50)] + [(32, 8, 9), (32, 8, 1)])
def test_istft_head(dev, n_fft, hop, Fr):
    B, bins = 3, n_fft // 2 + 1
    g = gen(n_fft + Fr)
    mag = torch.rand(B, bins, Fr, generator=g) * 9.0 - 3.0  # exp() from 0.05 to 400: below and above the clip at 100
    ph = (torch.rand(B, bins, Fr, generator=g) * 2.0 - 1.0) * 1e4
    ph[:, :, 0] *= 1e-4  # small phases too
    xp = torch.cat([mag, ph], 1)
    w = torch.hann_window(n_fft)
    ref32 = R.istft_head(xp, w, n_fft, hop)
    ref64 = R.istft_head(xp.double(), w.double(), n_fft, hop)
    assert ref64.shape == (B, 1, Fr * hop) and float(mag.max()) > math.log(100.0) > float(mag.min())
    xi = Banded(xp.shape, dev, xp)
    bi = Banded((n_fft + 2, n_fft), dev, torch.from_numpy(cf.istft_basis(w, n_fft).astype(np.float32)))
    wi = Banded((n_fft,), dev, w)
    out = Banded((B, 1, Fr * hop), dev)
    L.call("bc_istft_head", xi.t.data_ptr(), bi.t.data_ptr(), wi.t.data_ptr(), out.t.data_ptr(), B, Fr, n_fft, hop,
           stream(dev))
    check(out, (xi, bi, wi), ref32, ref64, f"istft_head n_fft={n_fft} F={Fr}")


# ---- the conv path at Cin = 802 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 33, 200])
def test_pointwise_conv_takes_802_input_channels(dev, T):
    """input_proj reads 2 * 401 channels, no multiple of the conv path's channel chunk: its own zero padding of the
    last chunk must hold (DESIGN.md section 4's 1e-4 of max|ref| for a conv against float64)."""
    g = gen(T)
    conv = cf._Pointwise(802, 64, linear=False)
    with torch.no_grad():
        conv.bias.copy_(torch.rand(64, generator=g) - 0.5)
    x = torch.randn(2, 802, T, generator=g)
    ref64 = F.conv1d(x.double(), conv.weight.detach().double(), conv.bias.detach().double())
    got = conv.run(x.to(dev)).cpu().double()
    err = float((got - ref64).abs().max() / ref64.abs().max())
    print(f"pointwise 802 -> 64, T={T}: rel err {err:.3e}")
    assert err <= 1e-4


# ---- torch.ops.bigcodec.* --------------------------------------------------------------------------------------------
def op_cases(dev):
    g = gen(7)
    w32 = torch.hann_window(32)
    fc = torch.view_as_real(R.freqs_cis(32, 128, 500.0)).contiguous().to(dev)
    qkv = torch.randn(2, 192, 70, generator=g).to(dev)
    xp = (torch.randn(2, 34, 5, generator=g)).to(dev)
    basis_t = torch.from_numpy(cf.stft_basis_t(w32, 32).astype(np.float32)).to(dev)
    basis_i = torch.from_numpy(cf.istft_basis(w32, 32).astype(np.float32)).to(dev)
    x = torch.randn(2, 64, 70, generator=g).to(dev)
    return {
        "stft_frames": ((torch.randn(2, 100, generator=g).to(dev), basis_t, 32, 8, 32),
                        lambda a, y: L.call("bc_stft_frames", a[0].data_ptr(), a[1].data_ptr(), y.data_ptr(), 2, 100, 32, 8, 32, stream(dev))),
        "rmsnorm": ((x, torch.rand(64, generator=g).to(dev), 1e-6, True),
                    lambda a, y: L.call("bc_rmsnorm_fwd", a[0].data_ptr(), a[1].data_ptr(), y.data_ptr(), 2, 64, 70, 1e-6, 1, stream(dev))),
        "dwconv_glu": ((x, torch.randn(32, 1, 31, generator=g).to(dev), torch.randn(32, generator=g).to(dev), 15),
                       lambda a, y: L.call("bc_dwconv_glu_fwd", a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), y.data_ptr(), 2, 32, 70, 31, 15, stream(dev))),
        "swiglu": ((x,), lambda a, y: L.call("bc_swiglu_fwd", a[0].data_ptr(), y.data_ptr(), 2, 32, 70, stream(dev))),
        "attention": ((qkv, fc, 2, True),
                      lambda a, y: L.call("bc_attention_fwd", a[0].data_ptr(), a[1].data_ptr(), y.data_ptr(), 2, 2, 32, 70, 1, stream(dev))),
        "istft_head": ((xp, basis_i, w32.to(dev), 8),
                       lambda a, y: L.call("bc_istft_head", a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), y.data_ptr(), 2, 5, 32, 8, stream(dev))),
    }


@pytest.mark.parametrize("name", ["stft_frames", "rmsnorm", "dwconv_glu", "swiglu", "attention", "istft_head"])
def test_op_passes_opcheck_and_equals_the_raw_call(dev, name):
    args, raw = op_cases(dev)[name]
    op = getattr(ops.load(), name)
    y = op(*args)
    z = torch.full_like(y, float("nan"))
    raw(args, z)
    torch.cuda.synchronize()
    assert not torch.isnan(y).any() and torch.equal(y, z)
    torch.library.opcheck(op.default, args)


def test_ops_refuse_bad_arguments_before_launching(dev):
    ns = ops.load()
    x = torch.zeros(2, 96, 8, device=dev)
    with pytest.raises((RuntimeError, ValueError)):
        ns.attention(x, torch.zeros(8, 8, 2, device=dev), 2, False)  # head_dim 16
    with pytest.raises((RuntimeError, ValueError)):
        ns.attention(torch.zeros(2, 192, 8, device=dev), torch.zeros(4, 16, 2, device=dev), 2, False)  # rope too short
    with pytest.raises((RuntimeError, ValueError)):
        ns.dwconv_glu(torch.zeros(2, 8, 4, device=dev), torch.zeros(4, 1, 64, device=dev), None, 0)  # K > 63
    with pytest.raises((RuntimeError, ValueError)):
        ns.stft_frames(torch.zeros(2, 100, device=dev), torch.zeros(32, 34, device=dev), 32, 8, 16)  # win != n_fft
    with pytest.raises((RuntimeError, ValueError)):
        ns.rmsnorm(torch.zeros(2, 8, 4), None, 1e-6, False)  # a host tensor
