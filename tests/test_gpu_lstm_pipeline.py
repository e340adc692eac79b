"""The persistent recurrence's pipelined hand-off (csrc/lstm_seq.hip, "Software pipeline": early flag store, early
look at the next half-step's flags, h prefetch in the tail) against the schedule it replaced and against fp64.

Everything goes through blocks.ResLSTM.run; data, the fp64 reference and the bound come from tests/lstm_ref.py.  The
two schedules sum the same products in the same order, so they are compared with torch.equal (x6 and h3 alike); the
old one is selected with the diagnostic bc_debug_set_lstm_pipeline(0).  The early flag store runs in every
instantiation; the look and the prefetch are compiled into the long MFMA phases only (H 1536, x6, n >= 33 here;
DESIGN.md §25), so H 256 checks the early store alone.

  test_schedules_bit_identical   H 256 (KS 2: ring of 2, a one-k-step prefetch) and 1536 (KS 12, the register-tightest)
                                 x {x6, h3} x n in {5 (NTH 1, half 1 empty), 17, 33 (NTH 2, half 1 partly filled), 64,
                                 65 (a second launch on the same flags and hseq)} x T in {1, 2, 3, the case's} x
                                 {no state, a given nonzero (h0, c0)}: y, h_n, c_n equal; the new schedule's outputs
                                 within bound(case, prec) of fp64
  test_lens_bit_identical        the state taken at each clip's own last step
  test_chunked_bit_identical     1, 5 and T - 6 steps with the state fed forward equal the whole pass (x6, new schedule)
  test_setter_round_trip         the setter returns the previous value; the recorded kernel names do not change"""
import contextlib
import functools

import pytest
import torch

from audiotokenization_amd import _lib as L
from audiotokenization_amd import blocks as BL
from lstm_ref import bound, cpu32, data, main_case, ref64, rel_h, scales, state_case, worst

pytestmark = pytest.mark.gpu

HS = (256, 1536)
NS = (5, 17, 33, 64, 65)
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


@contextlib.contextmanager
def _schedule(pipelined):
    setter = L.load().bc_debug_set_lstm_pipeline
    old = setter(1 if pipelined else 0)
    try:
        yield
    finally:
        setter(old)


@functools.lru_cache(maxsize=None)
def _module(H):
    case = main_case(H)  # (state_case shares the parameters: same seed, drawn first)
    m = BL.ResLSTM(H, num_layers=case.layers)
    m.lstm.load_state_dict(data(case).params)
    return m.to(torch.device("cuda", 0))


def _run(dev, H, prec, pipelined, x, what, state=None, lens=None, timed=False):
    """ResLSTM.run with the final state, under a precision and a schedule: [y, h_n, c_n] on the host (+ the kernel
    names the launch timer recorded)."""
    m = _module(H)
    tm = L.KernelTimer() if timed else None
    with _precision(prec), _schedule(pipelined):
        if state is not None:
            state = tuple(s.contiguous().to(dev) for s in state)
        if timed:
            L.set_timer(tm)
        try:
            with L.status_scope():
                y, (hn, cn) = m.run(x.contiguous().to(dev), state=state, return_state=True,
                                    lens=None if lens is None else lens.to(dev))
                L.check_status()
        finally:
            if timed:
                L.set_timer(None)
    try:
        out = [t.cpu() for t in (y, hn, cn)]
    except RuntimeError as e:  # a device fault ends the whole run (nothing more is started on a faulted GPU)
        pytest.exit(f"device error after {what}: {e}", returncode=3)
    return out + ([sorted(k for k in tm.summary() if k.startswith("lstm_seq"))] if timed else [])


def _same(fails, new, old, what):
    for name, a, b in zip(("y", "h_n", "c_n"), new, old):
        if not torch.equal(a, b):
            fails.append(f"{what}: {name} of the two schedules differs by {float((a - b).abs().max()):.3e}")


def _check(fails, got, want, case, prec, what, q=0):
    lim, c32 = bound(case, prec), max(cpu32(case))
    e = rel_h(got, want, scales(case)[q])
    print(f"LSTM-PIPE {what}: rel_h {e:.3e} cpu32 {c32:.3e} ratio {e / c32:.2f} bound {lim:.3e}")
    if not torch.isfinite(got).all() or e > lim:
        fails.append(f"{what}: rel_h {e:.3e} > {lim:.3e}; {worst(got, want, STATE_DIMS if q else ('clip', 'unit', 'step'))}")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("prec", ["x6", "h3"])
@pytest.mark.parametrize("H", HS)
def test_schedules_bit_identical(dev, H, prec, n):
    fails = []
    for given in (False, True):
        case = state_case(H) if given else main_case(H)
        d, (ry, rh, rc) = data(case), ref64(case)
        for T in (1, 2, 3, case.T):
            x = d.x[:n, :, :T]
            st = (d.h0[:, :, :n], d.c0[:, :, :n]) if given else None
            what = f"H {H} {prec} n {n} T {T} {'h0' if given else 'zero state'}"
            new = _run(dev, H, prec, True, x, what, state=st)
            old = _run(dev, H, prec, False, x, what, state=st)
            _same(fails, new, old, what)
            _check(fails, new[0] - x, ry[:n, :, :T], case, prec, what + " y")  # (a causal recurrence's prefix)
            if T == case.T:
                _check(fails, new[1], rh[:, :, :n], case, prec, what + " h_n", 1)
                _check(fails, new[2], rc[:, :, :n], case, prec, what + " c_n", 2)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("prec", ["x6", "h3"])
def test_lens_bit_identical(dev, prec):
    """A chunk length per clip: y holds all T steps, (h_n, c_n) each clip's state after its own lens[b] steps."""
    H, n = 1536, 33
    case = state_case(H)
    d = data(case)
    g = torch.Generator().manual_seed(7)
    lens = torch.randint(1, case.T + 1, (n,), generator=g, dtype=torch.int32)
    lens[0], lens[n - 1] = 1, case.T
    x, st = d.x[:n], (d.h0[:, :, :n], d.c0[:, :, :n])
    what = f"lens H {H} {prec} n {n}"
    new = _run(dev, H, prec, True, x, what, state=st, lens=lens)
    old = _run(dev, H, prec, False, x, what, state=st, lens=lens)
    fails = []
    _same(fails, new, old, what)
    _check(fails, new[0] - x, ref64(case)[0][:n], case, prec, what + " y")
    # a clip that ran all T steps leaves the whole pass's final state
    whole = _run(dev, H, prec, True, x, what, state=st)
    full = lens == case.T
    for name, a, b in (("h_n", new[1], whole[1]), ("c_n", new[2], whole[2])):
        if not torch.equal(a[:, :, full], b[:, :, full]):
            fails.append(f"{what}: {name} of the clips with lens = T differs from the whole pass")
    assert not fails, "\n".join(fails)


def test_chunked_bit_identical(dev):
    """1, 5 and T - 6 steps with the returned state fed forward (as test_gpu_lstm_matrix.test_state does): in x6 a step's
    arithmetic does not depend on where the call started, so the chunks equal the whole pass, under the new schedule."""
    H, n, prec = 1536, 33, "x6"
    case = state_case(H)
    d = data(case)
    x, st = d.x[:n], (d.h0[:, :, :n], d.c0[:, :, :n])
    what = f"chunked H {H} {prec} n {n}"
    y, hn, cn = _run(dev, H, prec, True, x, what, state=st)
    ys, t0, s = [], 0, st
    for steps in (1, 5, case.T - 6):
        yc, hc, cc = _run(dev, H, prec, True, x[:, :, t0:t0 + steps], what, state=s)
        ys.append(yc)
        t0, s = t0 + steps, (hc, cc)
    assert t0 == case.T
    fails = []
    _same(fails, (torch.cat(ys, dim=2), s[0], s[1]), (y, hn, cn), what + " (chunks, whole)")
    assert not fails, "\n".join(fails)


def test_setter_round_trip(dev):
    setter = L.load().bc_debug_set_lstm_pipeline
    first = setter(0)
    try:
        assert first in (0, 1)
        assert setter(1) == 0
        assert setter(5) == 1  # any nonzero value is "on"
        assert setter(0) == 1
    finally:
        assert setter(first) == 0
    case = main_case(256)
    for n, nth in ((17, 1), (33, 2)):
        x = data(case).x[:n]
        for prec, planes in (("x6", 3), ("h3", 2)):
            want = [f"lstm_seq2_x6_kernel<2, {planes}, {nth}>"]
            for pipelined in (True, False):
                names = _run(dev, 256, prec, pipelined, x, f"names n {n} {prec}", timed=True)[3]
                assert names == want, (pipelined, names)
