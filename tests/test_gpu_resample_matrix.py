"""Both kernels of csrc/resample.hip on the MI355X against the float64 restatement (tests/resample_ref.py).

resample_sinc_launch stages the filter bank in LDS when new * K <= 32 768 floats (resample_sinc_kernel<true>) and reads
it through the caches otherwise (<false>).  Every case asserts from new * K which of the two it runs: the six rate pairs
of tests/test_ingest.py all take the LDS kernel (22050 -> 24000 with 103 040 bytes of it), 44100 -> 16000 and 22050 ->
16000 take the cache kernel, and random filter banks of 128 x 256 and 129 x 255 floats sit on the limit and just above.

Bound of a case (the rule of tests/test_gpu_conformer_ops.check): max |got - ref64| <= min(4 x max |oracle32 - ref64|,
1e-4 x max |ref64|), ref64 the direct float64 sum of the kernel's own statement and oracle32 the float32 oracle
(oracle/resample_oracle.resample: conv1d) on the same input, recomputed and printed by the case.  Inputs, filters and
outputs of the raw C call sit between NaN guard bands and outputs start as NaN: a read outside a row multiplies a weight
by NaN and shows, an element never written shows too."""
import numpy as np
import pytest
import torch

import resample_ref as R
from audiotokenization_amd import _lib as L
from audiotokenization_amd import ingest
from oracle import resample_oracle as RO
from test_gpu_conformer_ops import Banded, check, stream

pytestmark = pytest.mark.gpu

# (orig_freq, new_freq) -> the kernel it takes (True: filters in LDS)
PAIRS = {(16000, 24000): True, (44100, 24000): True, (24000, 16000): True, (22050, 24000): True, (8000, 24000): True,
         (48000, 24000): True, (44100, 16000): False, (22050, 16000): False}


def raw(dev, x, kern, lout, orig, width, pitch=None):
    """bc_resample_sinc on banded operands; returns (output Banded (B, pitch), [input Bandeds])."""
    B, lin = x.shape
    new, K = kern.shape
    pitch = lout if pitch is None else pitch
    xi, ki, out = Banded((B, lin), dev, x), Banded((new, K), dev, kern), Banded((B, pitch), dev)
    L.call("bc_resample_sinc", xi.t.data_ptr(), out.t.data_ptr(), ki.t.data_ptr(), B, lin, lout, pitch, orig, new, K,
           width, stream(dev))
    torch.cuda.synchronize()
    return out, [xi, ki]


def lengths(orig, new, K):
    """1, K - 1 (every output in the edge branch), K and K + 1 (around the fast path's s + K <= Lin), 3 orig + 5, and
    the lengths whose outputs end around the 256-thread workgroup's edge (255 / 256 / 257 where the ratio reaches
    them, the next reachable length otherwise)."""
    ls = [1, K - 1, K, K + 1, 3 * orig + 5] + [R.lin_for_lout(t, orig, new) for t in (255, 256, 257)]
    return sorted(set(ls))


@pytest.mark.parametrize("orig_freq,new_freq", list(PAIRS))
def test_rate_pair_against_float64(dev, orig_freq, new_freq):
    kern, width, orig, new = ingest.sinc_resample_kernel(orig_freq, new_freq)
    K = kern.shape[1]
    assert K == 2 * width + orig
    assert R.takes_lds_kernel(new, K) == PAIRS[(orig_freq, new_freq)], (new, K, new * K)
    print(f"{orig_freq} -> {new_freq}: {new} phases x {K} taps = {new * K} floats, "
          f"{'LDS' if R.takes_lds_kernel(new, K) else 'cache'} kernel")
    louts = set()
    for lin in lengths(orig, new, K):
        x = torch.rand(2, lin, generator=torch.Generator().manual_seed(lin + orig_freq)) * 2 - 1
        lout = R.out_len(lin, orig, new)
        louts.add(lout)
        ref32 = RO.resample(x, orig_freq, new_freq)
        ref64 = torch.from_numpy(R.direct64(x.numpy(), kern, orig, width, lout))
        assert tuple(ref32.shape) == (2, lout)
        out, ins = raw(dev, x, torch.from_numpy(kern), lout, orig, width)
        got = check(out, ins, ref32, ref64, f"{orig_freq} -> {new_freq} Lin {lin} Lout {lout}")
        y = ingest.Resampler.get(orig_freq, new_freq, dev)(x.to(dev))  # the torch op over the same call
        assert tuple(y.shape) == (2, lout) and torch.equal(y.cpu().double(), got)
    assert min(louts) < 256 and any(255 <= v <= 256 for v in louts) and any(v > 256 for v in louts), louts


@pytest.mark.parametrize("orig_freq,new_freq", [(16000, 24000), (22050, 24000), (44100, 16000), (22050, 16000)])
def test_rows_are_independent(dev, orig_freq, new_freq):
    """B = 3 with row 1 entirely NaN: rows 0 and 2 are finite and bit-identical to their B = 1 results."""
    rs = ingest.Resampler.get(orig_freq, new_freq, dev)
    assert R.takes_lds_kernel(rs.new, rs.taps) == PAIRS[(orig_freq, new_freq)]
    lin = 2 * rs.orig + rs.taps + 3
    x = torch.rand(3, lin, generator=torch.Generator().manual_seed(orig_freq)) * 2 - 1
    x[1] = float("nan")
    y = rs(x.to(dev)).cpu()
    assert tuple(y.shape) == (3, rs.out_len(lin))
    assert torch.isnan(y[1]).all()  # every output of the NaN row has a NaN tap or the NaN x 0 of the padding branch
    for b in (0, 2):
        one = rs(x[b:b + 1].to(dev)).cpu()
        assert torch.isfinite(y[b]).all() and torch.equal(y[b], one[0]), b


@pytest.mark.parametrize("orig_freq,new_freq", [(16000, 24000), (22050, 24000), (44100, 16000), (22050, 16000)])
def test_row_pitch_above_the_output_length(dev, orig_freq, new_freq):
    """pitch > Lout through Resampler(..., pad_to=): the pitch - Lout tail of every row is exactly zero and the samples
    in front of it are bit-identical to the unpadded call; the raw call leaves the tail it is given untouched."""
    rs = ingest.Resampler.get(orig_freq, new_freq, dev)
    assert R.takes_lds_kernel(rs.new, rs.taps) == PAIRS[(orig_freq, new_freq)]
    lin = rs.taps + 2 * rs.orig + 1
    lout = rs.out_len(lin)
    x = torch.rand(3, lin, generator=torch.Generator().manual_seed(new_freq)) * 2 - 1
    plain = rs(x.to(dev)).cpu()
    for pad in (lout + 1, lout + 200, 2 * lout + 77):
        y = rs(x.to(dev), pad_to=pad).cpu()
        assert tuple(y.shape) == (3, pad)
        assert torch.equal(y[:, :lout], plain) and bool((y[:, lout:] == 0).all()), pad
    assert torch.equal(rs(x.to(dev), pad_to=lout - 5).cpu(), plain)  # pad_to below Lout: pitch = Lout
    out, ins = raw(dev, x, rs.kern.cpu(), lout, rs.orig, rs.width, pitch=lout + 37)
    assert out.intact() and all(i.intact() for i in ins)
    got = out.t.cpu()
    assert torch.equal(got[:, :lout], plain) and torch.isnan(got[:, lout:]).all()


@pytest.mark.parametrize("new,K", [(128, 256), (129, 255)])
def test_the_lds_limit_itself(dev, new, K):
    """Random filter banks of exactly 32 768 floats (the LDS kernel with all of its 128 KiB) and of 32 895 (the cache
    kernel) through the raw call, which takes any (orig, new, K, width): between the two only the kernel changes."""
    orig, width = 97, 70
    assert R.takes_lds_kernel(new, K) == (new * K == 32768) and abs(new * K - 32768) <= 127
    g = torch.Generator().manual_seed(new)
    kern = (torch.rand(new, K, generator=g) * 2 - 1) / K ** 0.5
    for lin in (1, K - 1, K + 1, 5 * orig + 3):
        x = torch.rand(2, lin, generator=g) * 2 - 1
        lout = R.out_len(lin, orig, new)
        ref32 = R.conv32(x, kern, orig, width, lout)
        ref64 = torch.from_numpy(R.direct64(x.numpy(), kern.numpy(), orig, width, lout))
        out, ins = raw(dev, x, kern, lout, orig, width)
        check(out, ins, ref32, ref64, f"{new} x {K} bank ({'LDS' if R.takes_lds_kernel(new, K) else 'cache'}) Lin {lin}")


def test_refusals_come_before_any_launch(dev):
    """B = 0 and Lout = 0 return OK; y_pitch < Lout, orig < 1 and null pointers BC_ERR_ARG (1); B > 65535
    BC_ERR_UNSUPPORTED (3); none of them writes: the output's NaN and every guard band stay intact."""
    kern, width, orig, new = ingest.sinc_resample_kernel(16000, 24000)
    K, lin = kern.shape[1], 40
    lout = R.out_len(lin, orig, new)
    xi = Banded((2, lin), dev, torch.rand(2, lin))
    ki = Banded((new, K), dev, torch.from_numpy(kern))
    out = Banded((2, lout), dev)
    f = L.load().bc_resample_sinc
    x, y, k, st = xi.t.data_ptr(), out.t.data_ptr(), ki.t.data_ptr(), stream(dev)
    cases = {
        "B = 0": ((x, y, k, 0, lin, lout, lout, orig, new, K, width, st), 0),
        "Lout = 0": ((x, y, k, 2, lin, 0, lout, orig, new, K, width, st), 0),
        "Lin = 0, Lout = 0": ((x, y, k, 2, 0, 0, 0, orig, new, K, width, st), 0),
        "y_pitch < Lout": ((x, y, k, 2, lin, lout, lout - 1, orig, new, K, width, st), 1),
        "orig = 0": ((x, y, k, 2, lin, lout, lout, 0, new, K, width, st), 1),
        "orig < 0": ((x, y, k, 2, lin, lout, lout, -2, new, K, width, st), 1),
        "new = 0": ((x, y, k, 2, lin, lout, lout, orig, 0, K, width, st), 1),
        "taps = 0": ((x, y, k, 2, lin, lout, lout, orig, new, 0, width, st), 1),
        "width < 0": ((x, y, k, 2, lin, lout, lout, orig, new, K, -1, st), 1),
        "B < 0": ((x, y, k, -1, lin, lout, lout, orig, new, K, width, st), 1),
        "Lin < 0": ((x, y, k, 2, -1, lout, lout, orig, new, K, width, st), 1),
        "Lout < 0": ((x, y, k, 2, lin, -1, lout, orig, new, K, width, st), 1),
        "null x": ((None, y, k, 2, lin, lout, lout, orig, new, K, width, st), 1),
        "null y": ((x, None, k, 2, lin, lout, lout, orig, new, K, width, st), 1),
        "null kern": ((x, y, None, 2, lin, lout, lout, orig, new, K, width, st), 1),
        "B = 65536": ((x, y, k, 65536, lin, lout, lout, orig, new, K, width, st), 3),
    }
    for what, (args, want) in cases.items():
        assert f(*args) == want, what
    torch.cuda.synchronize()
    assert torch.isnan(out.buf).all() and xi.intact() and ki.intact()
    with pytest.raises(L.BigCodecLibraryError):
        ingest.Resampler.get(16000, 24000, dev)(torch.rand(2, 40))  # a host tensor: no fallback
