"""Every ResLSTM kernel variant against fp64 on the MI355X, on the recurrence's own output.

Everything goes through blocks.ResLSTM.run; the cases, the fp64 reference (one per H, shared by every precision and
launch size: clips are independent, so a launch of n clips is compared with ref[:n]), the metric rel_h on got - x and
the bound K[prec] * cpu32 (K: twice the largest kernel error / cpu32 measured) come from
tests/lstm_ref.py.  tests/test_lstm_matrix_host.py shows on the CPU what this bound separates from fp32 arithmetic: a
recurrence on single-plane operands by three orders of magnitude; one that lost only the third bf16 plane of an operand
lies 0.7-3.5 x the bound away, so most legs see it but none is guaranteed to.

  test_persistent   lstm_seq2_x6_kernel<H / 128, P, NTH> for H in {256, 512, 1024, 1536} x {x6, h3} at the launch-size
                    edges (NTH switch 32 / 33, half boundaries 16 / 17 and 32 / 33, launch chunks 64 / 65, 97 = 64 + a
                    33-clip remainder); for n <= 64 the launch timer must have recorded the expected instantiation
  test_t_edges      T = 1 (nothing published, no flag set) and T = 2, against the prefix of the longer reference
  test_state        a given nonzero (h0, c0), the returned (h_n, c_n) of every layer, state in the second launch chunk,
                    and chunked passes with the state fed forward (bit-identical to the whole pass in x6)
  test_fp32_mode    lstm_step_frag_kernel<4, 8, 16, 32, 48> and lstm_step_kernel across their blockIdx.y groups
  the module's last test checks that the timer saw all 16 persistent instantiations."""
import contextlib
import functools

import pytest
import torch

from audiotokenization_amd import _lib as L
from audiotokenization_amd import blocks as BL
from audiotokenization_amd import modules as M
from lstm_ref import (FRAG_H, K, SEQ_H, STEP_H, bound, cpu32, data, main_case, ref64, rel_h, scales, state_case,
                      torch_lstm, worst)
from oracle import bigcodec_oracle as O

pytestmark = pytest.mark.gpu

NS = (1, 15, 16, 17, 32, 33, 63, 64, 65, 97)
FP32_NS = (1, 63, 64, 65, 130)
LAUNCHED = set()  # persistent instantiations the launch timer recorded, checked by the module's last test
STATE_DIMS = ("layer", "unit", "clip")


@pytest.fixture(autouse=True)
def _no_timed_out_wait(dev):
    yield
    assert L.load().bc_lstm_status(1) == 0


@contextlib.contextmanager
def _precision(name):
    old = L.precision_mode()
    L.set_precision(name)
    try:
        yield
    finally:
        L._mode = old


@functools.lru_cache(maxsize=None)
def _module(H):
    """The ResLSTM of width H with the case's parameters (main_case and state_case share them), on the device."""
    case = main_case(H)
    m = BL.ResLSTM(H, num_layers=case.layers)
    m.lstm.load_state_dict(data(case).params)
    return m.to(torch.device("cuda", 0))


def _host(what, *tensors):
    """Device -> host; a device fault ends the whole run (nothing more is started on a faulted GPU)."""
    try:
        return [t.cpu() for t in tensors]
    except RuntimeError as e:
        pytest.exit(f"device error after {what}: {e}", returncode=3)


def _run(dev, H, prec, x, what, state=None, return_state=False, out_snake=None, timed=False):
    """ResLSTM.run under a precision: (y, h_n, c_n, {kernel: launches} recorded by the launch timer) on the host."""
    m = _module(H)
    tm = L.KernelTimer() if timed else None
    with _precision(prec):
        if state is not None:
            state = tuple(s.contiguous().to(dev) for s in state)
        if timed:
            L.set_timer(tm)
        try:
            with L.status_scope():
                out = m.run(x.contiguous().to(dev), out_snake=out_snake, state=state, return_state=return_state)
                L.check_status()
        finally:
            if timed:
                L.set_timer(None)
    y, (hn, cn) = out if return_state else (out, (None, None))
    host = _host(what, *[t for t in (y, hn, cn) if t is not None])
    names = {k: d["launches"] for k, d in tm.summary().items()} if timed else {}
    return (host + [None, None])[:3] + [names]


def _check(fails, got, want, case, prec, what, q=0):
    """rel_h of quantity q (0: h, 1: h_n, 2: c_n) of a slice of the case, on the whole case's scale; prints the figure
    (and its ratio to the fp32 CPU error), then collects a failure."""
    lim, c32, dims = bound(case, prec), max(cpu32(case)), STATE_DIMS if q else ("clip", "unit", "step")
    e = rel_h(got, want, scales(case)[q])
    print(f"LSTM-MATRIX {what}: rel_h {e:.3e} cpu32 {c32:.3e} ratio {e / c32:.2f} bound {lim:.3e}")
    if not torch.isfinite(got).all() or e > lim:
        fails.append(f"{what}: rel_h {e:.3e} > {lim:.3e}; {worst(got, want, dims)}")


def _seq_name(H, prec, n):
    return f"lstm_seq2_x6_kernel<{H // 128}, {3 if prec == 'x6' else 2}, {1 if n <= 32 else 2}>"


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("prec", ["x6", "h3"])
@pytest.mark.parametrize("H", SEQ_H)
def test_persistent(dev, H, prec, n):
    case = main_case(H)
    x, ref = data(case).x[:n], ref64(case)[0][:n]
    what = f"persistent H {H} {prec} n {n}"
    y, _, _, names = _run(dev, H, prec, x, what, timed=n <= 64)
    fails = []
    _check(fails, y - x, ref, case, prec, what)
    if n <= 64:  # above 64 the recorded name is the first chunk's only
        name = _seq_name(H, prec, n)
        assert names.get(name) == case.layers, (name, names)
        LAUNCHED.add(name)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("prec", ["x6", "h3"])
@pytest.mark.parametrize("H", SEQ_H)
def test_t_edges(dev, H, prec):
    """A causal recurrence's prefix is its own answer: T = 1 and T = 2 calls against the first steps of the reference."""
    case = main_case(H)
    fails = []
    for T in (1, 2):
        for n in (33, 5):
            x, ref = data(case).x[:n, :, :T], ref64(case)[0][:n, :, :T]
            what = f"T edge H {H} {prec} T {T} n {n}"
            y = _run(dev, H, prec, x, what)[0]
            _check(fails, y - x, ref, case, prec, what)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n", [5, 33, 70])
@pytest.mark.parametrize("prec", ["x6", "h3"])
@pytest.mark.parametrize("H", SEQ_H)
def test_state(dev, H, prec, n):
    """bc_reslstm_fwd_state from a given nonzero (h0, c0): y, h_n and c_n of every layer against fp64, and three chunks
    (1, 5, T - 6 steps) with the returned state fed forward against the whole pass: bit-identical in x6 (exact operand
    splits: a step's arithmetic does not depend on where the call started); in h3 the input projection's block scales
    span the columns of a call, so the chunked pass is held to the bound instead."""
    case = state_case(H)
    d, (ry, rh, rc) = data(case), ref64(case)
    x, st = d.x[:n], (d.h0[:, :, :n], d.c0[:, :, :n])
    want = (ry[:n], rh[:, :, :n], rc[:, :, :n])
    what = f"state H {H} {prec} n {n}"
    fails = []

    def compare(y, hn, cn, tag):
        _check(fails, y - x, want[0], case, prec, f"{what} {tag} y")
        _check(fails, hn, want[1], case, prec, f"{what} {tag} h_n", 1)
        _check(fails, cn, want[2], case, prec, f"{what} {tag} c_n", 2)

    y, hn, cn, _ = _run(dev, H, prec, x, what, state=st, return_state=True)
    compare(y, hn, cn, "whole")
    ys, t0, s = [], 0, st
    for steps in (1, 5, case.T - 6):
        yc, hc, cc, _ = _run(dev, H, prec, x[:, :, t0:t0 + steps], what, state=s, return_state=True)
        ys.append(yc)
        t0, s = t0 + steps, (hc, cc)
    assert t0 == case.T
    yc = torch.cat(ys, dim=2)
    if prec == "x6":
        for name, a, b in (("y", yc, y), ("h_n", s[0], hn), ("c_n", s[1], cn)):
            if not torch.equal(a, b):
                fails.append(f"{what}: chunked {name} differs from the whole pass by {float((a - b).abs().max()):.3e}")
    else:
        compare(yc, s[0], s[1], "chunked")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("H,prec", [(256, "fp32"), (768, "x6")])
def test_state_without_the_persistent_kernel_raises(dev, H, prec):
    """Carried state exists in the persistent kernel only: the per-step kernels (fp32 mode; H = 768 in every mode) must
    refuse it (BC_ERR_UNSUPPORTED), given or asked for, and never run stateless in silence."""
    case = main_case(H)
    x = data(case).x[:3].to(dev)
    z = torch.zeros(case.layers, H, 3, device=dev)
    with _precision(prec):
        with pytest.raises(RuntimeError, match="code 3"), L.status_scope():
            _module(H).run(x, state=(z, z.clone()), return_state=True)
        with pytest.raises(RuntimeError, match="code 3"), L.status_scope():
            _module(H).run(x, return_state=True)
    torch.cuda.synchronize()


def test_bf16_precision_runs_the_h3_recurrence(dev):
    """lstm_mode maps bf16 (2) to h3 (3), projection and recurrence: the outputs are the same bits."""
    case = main_case(512)
    x = data(case).x[:33]
    a = _run(dev, 512, "bf16", x, "bf16 H 512")[0]
    b = _run(dev, 512, "h3", x, "h3 H 512")[0]
    assert torch.equal(a, b), float((a - b).abs().max())
    fails = []
    _check(fails, a - x, ref64(case)[0][:33], case, "bf16", "bf16 H 512 n 33")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n", FP32_NS)
@pytest.mark.parametrize("H", sorted(FRAG_H + STEP_H))
def test_fp32_mode(dev, H, n):
    """lstm_step_frag_kernel<H / 32> (H % 128 == 0) and lstm_step_kernel (48, 64, 768), one launch per step: one to three
    blockIdx.y groups of 64 clips, full and ragged (the b < B guards)."""
    case = main_case(H)
    x, ref = data(case).x[:n], ref64(case)[0][:n]
    what = f"fp32 H {H} n {n}"
    fails = []
    y = _run(dev, H, "fp32", x, what)[0]
    _check(fails, y - x, ref, case, "fp32", what)
    if n == 65:  # one T = 1 call: a single launch that reads no h and no c
        y = _run(dev, H, "fp32", x[:, :, :1], what + " T 1")[0]
        _check(fails, y - x[:, :, :1], ref[:, :, :1], case, "fp32", what + " T 1")
    assert not fails, "\n".join(fails)


@functools.lru_cache(maxsize=None)
def _snake_case(H, n):
    """Snake parameters, the fp64 Snake of x + h and the fp32 CPU pipeline's error, on the recurrence's scale."""
    case = main_case(H)
    g = torch.Generator().manual_seed(H + 1)
    alpha, beta = torch.rand(H, generator=g) - 0.5, torch.rand(H, generator=g) - 0.5
    x, r = data(case).x[:n], ref64(case)[0][:n]
    want = O.snake_beta(x.double() + r, alpha.double(), beta.double())
    y32 = torch_lstm(case, torch.float32)[0][:n]
    s32 = O.snake_beta(y32 + x, alpha, beta)
    scale = scales(case)[0]
    return alpha, beta, want, scale, float((s32.double() - want).abs().max()) / scale


@pytest.mark.parametrize("H,prec", [(256, "x6"), (512, "h3"), (128, "fp32"), (64, "fp32")])
def test_fused_output_snake(dev, H, prec):
    """The Snake fused into the output transpose, one leg per kernel family: max |got - snake64(x + h64)| / max |h64|
    (the recurrence's error as it leaves the Snake) within K[prec] times the same figure of the fp32 CPU pipeline."""
    n = 33
    case = main_case(H)
    alpha, beta, want, scale, c32 = _snake_case(H, n)
    s = M.SnakeBeta(H, alpha_logscale=True)
    with torch.no_grad():
        s.alpha.copy_(alpha)
        s.beta.copy_(beta)
    y = _run(dev, H, prec, data(case).x[:n], f"snake H {H} {prec}", out_snake=s.to(dev).coeffs(dev))[0]
    e = float((y.double() - want).abs().max()) / scale
    lim = K[prec] * c32
    print(f"LSTM-MATRIX snake H {H} {prec} n {n}: rel_h {e:.3e} cpu32 {c32:.3e} ratio {e / c32:.2f} bound {lim:.3e}")
    assert torch.isfinite(y).all() and e <= lim, (e, lim, worst(y, want))


def test_every_persistent_instantiation_ran():
    want = {_seq_name(H, prec, n) for H in SEQ_H for prec in ("x6", "h3") for n in (32, 33)}
    assert len(want) == 16 and LAUNCHED == want, sorted(want - LAUNCHED)
