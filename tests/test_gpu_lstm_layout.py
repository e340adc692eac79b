"""The layout kernels around every ResLSTM call, exactly: bc_btc_to_ctb (x[B][C][T] -> y[C][T][B]) and bc_ctb_to_btc_add
(out = transpose(y) + skip), raw calls on NaN-pre-filled buffers between NaN guard bands.

Their tiles are 32 time steps by 64 clips, one channel per blockIdx.y: B in {1, 3, 63, 64, 65, 130} and
T in {1, 31, 32, 33, 65} put every edge of both tile dimensions inside, on it and one past it, C in {1, 5, 48} the
channel stride.  A transpose moves bits and the add is one IEEE fp32 add, so both are compared bit for bit with torch
on the CPU, on inputs that hold +-0, denormals, +-Inf (never opposite infinities in one sum: the outputs must come out
free of NaN, which is what the buffers are pre-filled with), the largest finite value, and pairs of opposite sign that
cancel exactly.  A zero-size dimension returns 0 and writes nothing; null pointers and negative sizes return 1 before
any launch."""
import itertools

import numpy as np
import pytest
import torch

from audiotokenization_amd import _lib as L

pytestmark = pytest.mark.gpu

BS = (1, 3, 63, 64, 65, 130)
TS = (1, 31, 32, 33, 65)
CS = (1, 5, 48)
GUARD = 512
NAN_BITS = 0x7FC00000
SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -5.9e-39, np.inf, -np.inf, 3.4028235e38, 1.0, -1.0,
                    2.0 ** -126], np.float32)


def _values(B, C, T, seed):
    """(B, C, T) N(0, 1) with the special values strewn in at fixed strides."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B * C * T, generator=g)
    idx = torch.arange(0, v.numel(), 7)
    v[idx] = torch.from_numpy(SPECIAL)[torch.arange(idx.numel()) % len(SPECIAL)]
    return v.view(B, C, T)


def _pair(B, C, T):
    """y (C, T, B) and skip (B, C, T) of one add: specials on both sides, no Inf against an Inf, and every third
    element of skip the exact negative of its partner."""
    y = _values(B, C, T, 1000 * B + 10 * T + C).permute(1, 2, 0).contiguous()
    skip = _values(B, C, T, 7 + 1000 * B + 10 * T + C).roll(3)
    yt = y.permute(2, 0, 1)
    skip = torch.where(torch.isinf(yt) & torch.isinf(skip), torch.full_like(skip, 0.5), skip)
    flat, ytf = skip.reshape(-1).clone(), yt.reshape(-1)
    sel = (torch.arange(flat.numel()) % 3 == 0) & torch.isfinite(ytf)
    flat[sel] = -ytf[sel]
    return y, flat.view(B, C, T)


def _guarded(dev, n, src=None):
    buf = torch.full((GUARD + n + GUARD,), float("nan"), device=dev)
    view = buf[GUARD:GUARD + n]
    if src is not None:
        view.copy_(src.reshape(-1))
    return buf, view, buf.data_ptr() + 4 * GUARD


def _bands_intact(g):
    bits = g[0].view(torch.int32)
    return bool((bits[:GUARD] == NAN_BITS).all()) and bool((bits[GUARD + g[1].numel():] == NAN_BITS).all())


def _host(what, *tensors):
    """Device -> host; a device fault ends the whole run (nothing more is started on a faulted GPU)."""
    try:
        return [t.cpu() for t in tensors]
    except RuntimeError as e:
        pytest.exit(f"device error after {what}: {e}", returncode=3)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("B", BS)
def test_btc_to_ctb(dev, B):
    lib, st, fails = L.load(), torch.cuda.current_stream().cuda_stream, []
    for T, C in itertools.product(TS, CS):
        what = f"btc_to_ctb B {B} C {C} T {T}"
        x = _values(B, C, T, B + 131 * T + C)
        xg, yg = _guarded(dev, x.numel(), x.to(dev)), _guarded(dev, x.numel())
        rc = lib.bc_btc_to_ctb(xg[2], yg[2], B, C, T, st)
        got, xb = _host(what, yg[1], xg[1])
        want = x.permute(1, 2, 0).contiguous()
        if rc != 0 or not torch.equal(_bits(got), _bits(want.reshape(-1))):
            bad = int((_bits(got) != _bits(want.reshape(-1))).sum())
            fails.append(f"{what}: rc {rc}, {bad} of {x.numel()} elements differ, {int(torch.isnan(got).sum())} NaN left")
        if not (_bands_intact(xg) and _bands_intact(yg)) or not torch.equal(_bits(xb), _bits(x.reshape(-1))):
            fails.append(f"{what}: a band or the input was written")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B", BS)
def test_ctb_to_btc_add(dev, B):
    lib, st, fails = L.load(), torch.cuda.current_stream().cuda_stream, []
    for T, C in itertools.product(TS, CS):
        what = f"ctb_to_btc_add B {B} C {C} T {T}"
        y, skip = _pair(B, C, T)
        want = y.permute(2, 0, 1) + skip  # torch's fp32 CPU add: one IEEE add per element
        assert not torch.isnan(want).any()
        assert y.numel() < 8 or bool(((want == 0) & (skip != 0)).any())  # the exact cancellations are there
        yg, sg, og = _guarded(dev, y.numel(), y.to(dev)), _guarded(dev, y.numel(), skip.to(dev)), _guarded(dev, y.numel())
        rc = lib.bc_ctb_to_btc_add(yg[2], sg[2], og[2], B, C, T, st)
        got, yb, sb = _host(what, og[1], yg[1], sg[1])
        if rc != 0 or not torch.equal(_bits(got), _bits(want.reshape(-1))):
            bad = int((_bits(got) != _bits(want.reshape(-1))).sum())
            fails.append(f"{what}: rc {rc}, {bad} of {y.numel()} elements differ, {int(torch.isnan(got).sum())} NaN left")
        if not (_bands_intact(yg) and _bands_intact(sg) and _bands_intact(og)):
            fails.append(f"{what}: a band was written")
        if not torch.equal(_bits(yb), _bits(y.reshape(-1))) or not torch.equal(_bits(sb), _bits(skip.reshape(-1))):
            fails.append(f"{what}: an input was written")
    assert not fails, "\n".join(fails)


def test_layout_empty_and_refused(dev):
    """A zero-size dimension returns 0 and writes nothing; null pointers and negative sizes return 1 (BC_ERR_ARG), a
    host-side refusal before any launch."""
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    a, b, c = (_guarded(dev, 64, torch.ones(64)) for _ in range(3))
    o = _guarded(dev, 64)
    for B, C, T in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (0, 0, 0)):
        assert lib.bc_btc_to_ctb(a[2], o[2], B, C, T, st) == 0
        assert lib.bc_ctb_to_btc_add(a[2], b[2], o[2], B, C, T, st) == 0
    for B, C, T in ((-1, 4, 4), (4, -1, 4), (4, 4, -1)):
        assert lib.bc_btc_to_ctb(a[2], o[2], B, C, T, st) == 1
        assert lib.bc_ctb_to_btc_add(a[2], b[2], o[2], B, C, T, st) == 1
    assert lib.bc_btc_to_ctb(None, o[2], 4, 4, 4, st) == 1
    assert lib.bc_btc_to_ctb(a[2], None, 4, 4, 4, st) == 1
    assert lib.bc_ctb_to_btc_add(None, b[2], o[2], 4, 4, 4, st) == 1
    assert lib.bc_ctb_to_btc_add(a[2], None, o[2], 4, 4, 4, st) == 1
    assert lib.bc_ctb_to_btc_add(a[2], b[2], None, 4, 4, 4, st) == 1
    out, = _host("the refused layout calls", o[0])
    assert bool((out.view(torch.int32) == NAN_BITS).all())
    for g in (a, b, c):
        assert _bands_intact(g) and bool((g[1] == 1).all())
