"""The five stream_window ops against tests/window_ref.py, bit for bit.

All five are instantiations of one kernel body (csrc/elementwise.hip window_kernel), so the sibling comparisons of the
other files (slots against stream_window, slots_la against _la, lens against slots) cannot see a mistake in that body:
it cancels.  Here every op is compared with the formula in plain torch indexing: the bit patterns of the window, of the
stored carry, and of every pool row that must stay untouched (pre-filled with NaNs of a distinct payload).  x holds NaN
wherever an entry must not read it.  The Snake goes through the product's own snake op first, so values move by copies
alone.  Shapes are the smallest that can still go wrong: one and several channels, a carry of 1 / 6 / 54 columns, 1 new
column, one fewer than the carry (the next carry reaches back into the old one), 300 (more than one 256-lane block per
row), none at all for the two look-ahead ops, right zeros, a fresh entry (src = -1) and an unstored one (dst = -1)."""
import pytest
import torch

from window_ref import bits, window_ref

pytestmark = pytest.mark.gpu

B = 3
SRC, DST, POOL_ROWS = [0, -1, 2], [1, 3, -1], 6  # disjoint row sets; rows 4 and 5 belong to nobody
CASES = [(C, act, strided) for C in (1, 5) for act in (False, True) for strided in (False, True)]
case = pytest.mark.parametrize("C,act,strided", CASES)


def nans(shape, payload):
    """float32 NaNs with a payload of their own per leading row: 0x7fc00000 | payload + row."""
    rows = torch.arange(shape[0], dtype=torch.int32).view(-1, *([1] * (len(shape) - 1)))
    return (rows + (0x7FC00000 | payload)).expand(*shape).contiguous().view(torch.float32)


def new_columns(P, least=1):
    return sorted({n for n in (0, 1, P - 1, 300) if n >= least})


class Inputs:
    """x (B, C, xn) on the device, dense or as the view [:, :, 3:] of a wider tensor, NaN outside the columns
    [xo[b], xo[b] + n[b]) of entry b; the Snake coefficients; xa = act(x) on the CPU."""

    def __init__(self, ns, dev, C, act, strided, xn, xo, n, seed):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(B, C, xn, generator=g)
        for b in range(B):
            x[b, :, :xo[b]] = float("nan")
            x[b, :, xo[b] + n[b]:] = float("nan")
        self.a = torch.rand(C, generator=g).add(0.5).to(dev) if act else None
        self.ib = torch.rand(C, generator=g).add(0.5).to(dev) if act else None
        xd = x.to(dev)
        if strided:
            wide = torch.full((B, C, xn + 3), float("nan"), device=dev)
            wide[:, :, 3:] = xd
            self.x = wide[:, :, 3:]
        else:
            self.x = xd
        self.xa = ns.snake(xd, self.a, self.ib).cpu() if act and xn else x
        self.g = g


def ints(dev, v):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(bits(got), bits(want)), what


@pytest.fixture(scope="module")
def ns():
    from audiotokenization_amd import ops

    return ops.load()


# ---- dense carries: bc_stream_window, bc_stream_window_la -----------------------------------------------------------
@case
def test_stream_window(dev, ns, C, act, strided):
    for P in (1, 6, 54):
        for n in new_columns(P):
            for first in (False, True):
                what = f"stream_window P={P} n={n} first={first}"
                i = Inputs(ns, dev, C, act, strided, n, [0] * B, [n] * B, P * 1000 + n)
                ctx = None if first else torch.randn(B, C, P, generator=i.g)
                win, nctx = ns.stream_window(i.x, None if first else ctx.to(dev), i.a, i.ib, P)
                rows = list(range(B))
                want, wctx = window_ref(i.xa, ctx, [-1] * B if first else rows, nans((B, C, P), 0x100), rows, [P] * B,
                                        [n] * B, [0] * B, [n] * B, [P] * B, P + n)
                same(win, want, what + " window")
                same(nctx, wctx, what + " carry")


@case
def test_stream_window_la(dev, ns, C, act, strided):
    for Pin in (1, 6, 54):
        for n in new_columns(Pin, least=0):
            for R in (0, 3):
                for Pout in sorted({0, Pin, Pin + n}):
                    for first in (False, True):
                        what = f"stream_window_la Pin={Pin} n={n} R={R} Pout={Pout} first={first}"
                        i = Inputs(ns, dev, C, act, strided, n, [0] * B, [n] * B, Pin * 1000 + n)
                        ctx = None if first else torch.randn(B, C, Pin, generator=i.g)
                        win, nctx = ns.stream_window_la(i.x, None if first else ctx.to(dev), i.a, i.ib, Pin, R, Pout)
                        rows = list(range(B))
                        want, wctx = window_ref(i.xa, ctx, [-1] * B if first else rows, nans((B, C, Pout), 0x100), rows,
                                                [Pin] * B, [n] * B, [0] * B, [Pin + n - Pout] * B, [Pout] * B,
                                                Pin + n + R)
                        same(win, want, what + " window")
                        same(nctx, wctx, what + " carry")


# ---- pool rows: bc_stream_window_slots, _slots_lens, _slots_la ------------------------------------------------------
def make_pool(C, pitch, g):
    """Every row NaNs of its own payload; the rows that are read (SRC) hold numbers."""
    pool = nans((POOL_ROWS, C, pitch), 0x200)
    for s in SRC:
        if s >= 0:
            pool[s] = torch.randn(C, pitch, generator=g)
    return pool


@case
def test_stream_window_slots(dev, ns, C, act, strided):
    for P in (1, 6, 54):
        for n in new_columns(P):
            what = f"stream_window_slots_ P={P} n={n}"
            i = Inputs(ns, dev, C, act, strided, n, [0] * B, [n] * B, P * 1000 + n)
            pool = make_pool(C, P, i.g)
            dpool = pool.to(dev)
            win = ns.stream_window_slots_(i.x, dpool, ints(dev, SRC), ints(dev, DST), i.a, i.ib, P)
            want, wpool = window_ref(i.xa, pool, SRC, pool, DST, [P] * B, [n] * B, [0] * B, [n] * B, [P] * B, P + n)
            same(win, want, what + " window")
            same(dpool, wpool, what + " pool")


@case
def test_stream_window_slots_lens(dev, ns, C, act, strided):
    for P in (1, 6, 54):
        for n in new_columns(P):
            for unit in (1, 3):
                # one entry past the chunk (clamped to it), one short (with P > 1 it reaches back into the old
                # carry), one with nothing
                lens = [n // unit + 1, (n // 2) // unit, 0]
                L = [min(max(v * unit, 0), n) for v in lens]
                what = f"stream_window_slots_lens_ P={P} n={n} unit={unit} L={L}"
                i = Inputs(ns, dev, C, act, strided, n, [0] * B, L, P * 1000 + n)
                pool = make_pool(C, P, i.g)
                dpool = pool.to(dev)
                win = ns.stream_window_slots_lens_(i.x, dpool, ints(dev, SRC), ints(dev, DST), ints(dev, lens), unit,
                                                   i.a, i.ib, P)
                want, wpool = window_ref(i.xa, pool, SRC, pool, DST, [P] * B, L, [0] * B, L, [P] * B, P + n)
                same(win, want, what + " window")
                same(dpool, wpool, what + " pool")


@case
def test_stream_window_slots_la(dev, ns, C, act, strided):
    for P in (1, 6, 54):
        Pmax = P + 4  # the row pitch: a carry may grow past the one that came in
        for nn in new_columns(P, least=0):
            for R in (0, 3):
                for mode in ("none", "in", "all"):
                    ci = [P, P // 2, P]
                    n = [nn, max(nn - 1, 0), nn // 2]
                    xo = [2, 0, 1]
                    co = [0 if mode == "none" else min(c_, Pmax) if mode == "in" else min(c_ + n_, Pmax)
                          for c_, n_ in zip(ci, n)]
                    co = [min(v, c_ + n_) for v, c_, n_ in zip(co, ci, n)]
                    keep = [c_ + n_ - o_ for c_, n_, o_ in zip(ci, n, co)]
                    W = max(max(c_ + n_ for c_, n_ in zip(ci, n)) + R, 1)
                    what = f"stream_window_slots_la_ P={P} n={n} R={R} cout={co}"
                    i = Inputs(ns, dev, C, act, strided, nn + 2 if nn else 0, xo if nn else [0] * B, n, P * 1000 + nn)
                    pool = make_pool(C, Pmax, i.g)
                    dpool = pool.to(dev)
                    xo_ = xo if nn else [0] * B
                    win = ns.stream_window_slots_la_(i.x, dpool, ints(dev, SRC), ints(dev, DST), ints(dev, ci),
                                                     ints(dev, n), ints(dev, xo_), ints(dev, keep), ints(dev, co), i.a,
                                                     i.ib, W)
                    want, wpool = window_ref(i.xa, pool, SRC, pool, DST, ci, n, xo_, keep, co, W)
                    same(win, want, what + " window")
                    same(dpool, wpool, what + " pool")
