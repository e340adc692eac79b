"""LookaheadPool (streaming.py) without a GPU: the pool's scheme -- LookaheadSlots.plan's index arrays,
left-aligned ragged windows, per-stage ping-pong rows, one crop per transposed conv and batch -- executed in float64
with torch.nn.functional on test_lookahead_host.py's toy stack with integer weights (every sum exact, so every session
must equal its whole-sequence forward to the bit), the window restated from the header's formula, the refusals, and the
new ABI entry point and torch op."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from audiotokenization_amd import _lib as L
from audiotokenization_amd import streaming as S
from helpers import build_models
from lookahead_pool_ref import CAPACITY, ORDER, TICKS, run_schedule, totals
from test_lookahead_host import act, toy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ---- the toy stack: test_lookahead_host's five stages, a recurrent stand-in, a closing conv ---------------------------
def stack(stride, C=3):
    """conv7 -> two units -> act + strided conv -> recurrent stage -> act + transposed conv -> act + conv3 (a pool's
    model ends in a conv).  The recurrent stand-in: c_t = act(c_{t-1} + x_t), y_t = x_t + c_t, state c per channel."""
    st, par = toy(stride, C)
    g = torch.Generator().manual_seed(100 + stride)
    stages = st[:4] + [S._Stage("lstm", None), st[4], S._Stage("conv", None, act, 3, 1, 1, 1, 1)]
    params = par[:4] + [None, par[4], (torch.randint(-2, 3, (1, C, 3), generator=g).double(),
                                        torch.randint(-2, 3, (1,), generator=g).double())]
    return stages, params


def recur(x, c):
    ys, cs = [], []
    for t in range(x.shape[-1]):
        c = act(c + x[..., t])
        ys.append(x[..., t] + c)
        cs.append(c)
    return torch.stack(ys, dim=-1), cs


def whole(stages, par, x):
    h = F.conv1d(x, *par[0], padding=3)
    for j in (1, 2):
        w7, b7, w1, b1 = par[j]
        h = h + F.conv1d(act(F.conv1d(act(h), w7, b7, padding=3 * stages[j].d, dilation=stages[j].d)), w1, b1)
    s, p = stages[3].s, stages[3].pl
    h = F.conv1d(act(h), *par[3], stride=s, padding=p)
    h = recur(h, torch.zeros(h.shape[:2], dtype=h.dtype))[0]
    h = F.conv_transpose1d(act(h), *par[5], stride=s, padding=p, output_padding=s % 2)
    return F.conv1d(act(h), *par[6], padding=1)


# ---- the window, restated from include/bigcodec.h ---------------------------------------------------------------------
def window(x, pool, p, W, fn=None):
    """win[b][c][j] = j < cin ? pool[src][c][j] (src < 0: 0) : j - cin < n ? act(x[b][c][xoff + j - cin]) : 0;
    pool[dst][c][i] = win[b][c][keep + i], i < cout (dst >= 0).  Checks the caller's duties on the way."""
    m, C = len(p.src), pool.shape[1]
    win = torch.zeros(m, C, W, dtype=torch.float64)
    for b in range(m):
        cin, n, xo = p.cin[b], p.n[b], p.xoff[b]
        assert 0 <= cin <= pool.shape[2] and 0 <= p.cout[b] <= pool.shape[2] and 0 <= n <= W - cin
        assert p.keep[b] + p.cout[b] <= cin + n, "the carry reaches into the zeros"
        assert p.src[b] < 0 or cin > 0
        if p.src[b] >= 0:
            win[b, :, :cin] = pool[p.src[b], :, :cin]
        new = x[b, :, xo:xo + n]
        assert new.shape[-1] == n
        win[b, :, cin:cin + n] = fn(new) if fn is not None else new
    reads, writes = {r for r in p.src if r >= 0}, [r for r in p.dst if r >= 0]
    assert not reads & set(writes), (p.src, p.dst)
    assert len(set(writes)) == len(writes), p.dst
    for b in range(m):
        if p.dst[b] >= 0 and p.cout[b]:
            pool[p.dst[b], :, :p.cout[b]] = win[b, :, p.keep[b]:p.keep[b] + p.cout[b]]
    assert not torch.isnan(win).any(), "a NaN of an input tail or of a foreign pool row reached a window"
    return win


class ToyPool:
    """LookaheadPool._flow in float64: the same plan, the same launches stage by stage, torch.nn.functional for the
    kernels.  The pools start as NaN and are never zeroed, as on the device."""

    def __init__(self, stages, par, capacity):
        self.slots, self.par = S.LookaheadSlots(stages, capacity), par
        self.pools = {}
        self.plans = []

    def pool(self, j, C):
        if j not in self.pools:
            self.pools[j] = torch.full((2 * self.slots.table.capacity, C, self.slots.pitch(j)), NAN, dtype=torch.float64)
        return self.pools[j]

    def run(self, sids, x, lens, flush):
        plan = self.slots.plan(sids, lens, flush)
        m, h = len(sids), x
        for j, (q, p) in enumerate(zip(self.slots.stages, plan.stages)):
            par = self.par[j]
            if q.kind == "lstm":
                C = h.shape[1]
                if p.launch:
                    pool = self.pool(j, C)[:, :, 0]
                    reads, writes = {r for r in p.src if r >= 0}, [r for r in p.dst if r >= 0]
                    assert not reads & set(writes) and len(set(writes)) == len(writes)
                    c0 = torch.stack([pool[r] if r >= 0 else torch.zeros(C, dtype=torch.float64) for r in p.src])
                    h, cs = recur(h, c0)
                    for b in range(m):
                        if p.dst[b] >= 0:
                            pool[p.dst[b]] = cs[max(p.n[b], 1) - 1][b]  # the state at the entry's own last step
            elif not p.launch:
                h = h.new_zeros(m, par[0].shape[1 if q.kind == "convT" else 0], 0)
            elif q.kind == "convT":
                win = window(h, self.pool(j, h.shape[1]), p, p.Wraw, q.act)
                h = F.conv_transpose1d(win, *par, stride=q.s)[..., p.crop:p.crop + p.tout]
            elif q.kind == "unit":
                raw = window(h, self.pool(j, h.shape[1]), p, p.Wraw)
                w7, b7, w1, b1 = par
                # the one-launch kernel: its own padding around the raw window, the residual from the same column
                y = raw + F.conv1d(act(F.conv1d(act(F.pad(raw, (q.pl, q.pr))), w7, b7, dilation=q.d)), w1, b1)
                h = y[..., q.pl:q.pl + p.tout]
            else:
                win = window(h, self.pool(j, h.shape[1]), p, p.W, q.act)
                h = F.conv1d(win, *par, stride=q.s) if p.tout else h.new_zeros(m, par[0].shape[0], 0)
            assert h.shape[-1] == p.tout, (j, q.kind, h.shape, p.tout)
        for b in range(m):
            h[b, :, plan.counts[b]:] = 0
        self.slots.commit(plan, plan.lens)
        self.plans.append(plan)
        return h, list(plan.counts)


# ---- the schedule (lookahead_pool_ref.TICKS) --------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [4, 5])
def test_pool_scheme_in_float64_equals_every_whole_sequence(stride):
    stages, par = stack(stride)
    hop = stride
    T, order = totals(hop), list(ORDER)
    assert len(set(T.values())) == 5 and len(TICKS) == 12  # five sessions of different lengths
    g = torch.Generator().manual_seed(stride)
    data = {s: torch.randint(-3, 4, (1, 1, T[s]), generator=g).double() for s in order}
    pool = ToyPool(stages, par, CAPACITY)

    def push(sids, x, hops, flags):
        return pool.run(sids, x, [h * hop for h in hops], flags)

    def finish(sids, x, lens):
        if x is None:
            x, lens = torch.zeros(len(sids), 1, 0, dtype=torch.float64), [0] * len(sids)
        return pool.run(sids, x, lens, [True] * len(sids))

    outs, chunks, sid = run_schedule(data, hop, pool.slots.open, push, finish)
    assert sid["D"] == sid["A"] and sid["E"] == sid["C"]  # slots are reused
    assert pool.slots.table.live() == []  # every finish closed its session
    early = 0
    for s in order:
        want = whole(stages, par, data[s])
        got = torch.cat(outs[s], dim=2)
        assert got.shape == want.shape and torch.equal(got, want), (stride, s)
        rows = S.lookahead_plan_stages(stages, chunks[s][:-1], chunks[s][-1])
        assert [o.shape[-1] for o in outs[s]] == [r[-1][3] for r in rows], (stride, s)
        early += sum(o.shape[-1] for o in outs[s][:-1])
    assert early > 0  # the pool hands frames out while the sessions run
    # one push held a session in its transient (carry still growing) next to a steady one (carry in == carry out)
    def steady(plan, b):
        return all(r[0] == r[4] and r[3] > 0 for r, q in zip(plan.rows[b], stages) if q.kind != "lstm")
    assert any(any(steady(p, b) for b in range(len(p.sids))) and not all(steady(p, b) for b in range(len(p.sids)))
               and not any(p.flush) for p in pool.plans)
    # and one a flushing session next to steady ones
    assert any(any(p.flush) and not all(p.flush) for p in pool.plans)


def test_a_stage_without_input_keeps_its_phase_and_launches_nothing():
    """A fresh session's first hop reaches the first stages only: every later stage gets dst = -1 and keeps its phase
    (None), and a stage no entry feeds does not launch."""
    stages, par = stack(4)
    slots = S.LookaheadSlots(stages, 2)
    a = slots.open()
    plan = slots.plan([a], [4], [False])
    fed = [p.launch for p in plan.stages]
    assert fed[0] and not all(fed) and fed == sorted(fed, reverse=True)
    for p, ph in zip(plan.stages, plan.phases[0]):
        assert (ph is None) == (p.dst[0] < 0)
    assert slots.states[a] == [q.start() for q in stages] and slots.phases[a] == [None] * len(stages)  # plan() is pure
    slots.commit(plan, [4])
    plan2 = slots.plan([a], [8], [False])
    for j, (p, p2) in enumerate(zip(plan.stages, plan2.stages)):
        if p.dst[0] >= 0 and p2.launch:
            assert p2.src[0] == p.dst[0] and p2.dst[0] == (p.dst[0] ^ 1), j  # ping-pong within the slot's two rows
    assert S.LookaheadSlots(stages, 2).pitch(2) == 18 and slots.pitch(5) == 1  # (k - 1) d; hist


def test_models_a_pool_cannot_serve():
    st, _ = toy(4)
    with pytest.raises(NotImplementedError):
        S.LookaheadSlots(st, 2)  # ends in a transposed conv
    with pytest.raises(NotImplementedError):
        S.LookaheadSlots(st + [S._Stage("lstm", None), st[0]], 2)  # a recurrent stage directly behind one
    for kw in (dict(antialias=True), dict(rnn_bidirectional=True)):
        e2, d2 = build_models("base", **kw)[:2]
        with pytest.raises(NotImplementedError):
            S.LookaheadPool(e2, 2)
        with pytest.raises(NotImplementedError):
            S.LookaheadPool(d2, 2)


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals_raise_before_any_state_changes():
    import audiotokenization_amd

    assert audiotokenization_amd.LookaheadPool is S.LookaheadPool
    enc, dec = build_models("debug")[:2]
    with pytest.raises(ValueError):
        S.StreamPool(enc, 2)  # the causal pool keeps refusing a non-causal model
    with pytest.raises(ValueError):
        S.LookaheadPool(enc, 0)
    pool, dpool = S.LookaheadPool(enc, 2), S.LookaheadPool(dec, 2)
    assert pool.hop == 320 and pool.lookahead == S.lookahead_samples(enc) and dpool.lookahead == S.lookahead_samples(dec)
    assert pool.state_bytes() == 0 and pool.live() == []
    a, b = pool.open(), pool.open()
    with pytest.raises(RuntimeError):
        pool.open()  # full
    before = ([list(s) for s in pool.slots.states], [list(p) for p in pool.slots.phases])
    x = torch.zeros(2, 1, 2 * pool.hop)
    for hops in ([1], [1, 2, 1], [0, 1], [1, 3], [1, 2.0], [True, 1], [1, None]):
        with pytest.raises(ValueError):
            pool.push([a, b], x, hops=hops)
    for sids in ([], [a, a], [a, 2], [a, -1], [a, True], [a, b, a]):
        with pytest.raises(ValueError):
            pool.push(sids, x)
    for bad in (torch.zeros(1, 1, 640), torch.zeros(2, 2, 640), torch.zeros(2, 1, 641), torch.zeros(2, 1, 0),
                torch.zeros(2, 640)):
        with pytest.raises(ValueError):
            pool.push([a, b], bad)
    for fin in ([True], [True, 1], "ab"):
        with pytest.raises(ValueError):
            pool.push([a, b], x, finish=fin)
    for lens in ([1], [1, 641], [-1, 3], [1, 2.0], [True, 1]):
        with pytest.raises(ValueError):
            pool.finish([a, b], torch.zeros(2, 1, 640), lens=lens)
    with pytest.raises(ValueError):
        pool.finish([a, b], None, lens=[0, 1])
    with pytest.raises(ValueError):
        pool.finish([a, 5])
    with pytest.raises(TypeError):
        pool.tokens([a], torch.zeros(1, 2, 1, dtype=torch.int64))  # an encoder pool
    c = dpool.open()
    with pytest.raises(ValueError):
        dpool.tokens([c], torch.zeros(2, 3, 1, dtype=torch.int64))
    with pytest.raises(ValueError):
        dpool.push([c], torch.zeros(1, 3, 4))  # the latent width
    assert ([list(s) for s in pool.slots.states], [list(p) for p in pool.slots.phases]) == before
    assert pool.table.pushes[:2] == [0, 0] and not pool.table.undefined and pool.samples(a) == 0 and pool.plan is None
    pool.close(a)
    assert pool.live() == [b] and pool.open() == a


# ---- the new entry point --------------------------------------------------------------------------------------------
def test_library_exports_stream_window_slots_la():
    lib = L.load()
    assert L.ABI_VERSION == 18 and lib.bc_abi_version() == 18  # additive: the ABI version stays
    header = open(os.path.join(REPO, "include", "bigcodec.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    name = "bc_stream_window_slots_la"
    assert name in L.EXPORTED and hasattr(lib, name) and name in set(re.findall(r"\b(bc_[A-Za-z0-9_]+)\s*\(", txt))
    doc = re.sub(r"[\s*]+", " ", re.search(r"/\* bc_stream_window_slots_la:.*?\*/", header, flags=re.S).group(0))
    assert "CALLER guarantees" in doc and "no pool row is both in src and in dst of one call" in doc
    assert "dst names no row twice" in doc  # the caller's disjointness duty, as for bc_stream_window_slots


def test_stream_window_slots_la_argument_checks():
    """Null or inconsistent arguments return 1, sizes beyond 2^31 - 1 return 3, B == 0 returns 0: all without a launch
    (the pointers are fake)."""
    lib = L.load()

    def win(x=1, xbs=12, xT=4, xn=4, pool=1, src=1, dst=1, cin=1, n=1, xoff=1, keep=1, cout=1, sa=None, sb=None, w=1, B=0,
            C=3, W=9, Pmax=6, rows=4):
        return lib.bc_stream_window_slots_la(x, xbs, xT, xn, pool, src, dst, cin, n, xoff, keep, cout, sa, sb, w, B, C, W,
                                             Pmax, rows, None)

    assert win() == 0 and win(sa=1, sb=1) == 0
    assert win(x=None, xn=0, xT=0, xbs=0) == 0  # a push in which this stage only flushes: x is not needed
    for kw in (dict(x=None), dict(pool=None), dict(src=None), dict(dst=None), dict(cin=None), dict(n=None),
               dict(xoff=None), dict(keep=None), dict(cout=None), dict(w=None), dict(sa=1), dict(sb=1), dict(B=-1),
               dict(C=0), dict(W=0), dict(Pmax=0), dict(rows=0), dict(xn=-1), dict(xT=3), dict(xbs=11)):
        assert win(**kw) == 1, kw
    assert win(C=1 << 20, B=1 << 12, xbs=1 << 40) == 3
    assert win(C=1 << 20, rows=1 << 12, xbs=1 << 40) == 3


def test_stream_window_slots_la_op_schema_and_fake():
    from audiotokenization_amd import ops

    ns = ops.load()
    assert "stream_window_slots_la_" in ops.OPS
    assert str(ns.stream_window_slots_la_.default._schema) == (
        "bigcodec::stream_window_slots_la_(Tensor x, Tensor(a!) pool, Tensor src, Tensor dst, Tensor cin, Tensor n, "
        "Tensor xoff, Tensor keep, Tensor cout, Tensor? alpha_exp, Tensor? inv_beta, int W) -> Tensor")
    m = lambda *s: torch.empty(*s, device="meta")  # noqa: E731
    i3 = torch.empty(3, dtype=torch.int32, device="meta")
    win = ns.stream_window_slots_la_(m(3, 48, 100), m(10, 48, 18), i3, i3, i3, i3, i3, i3, i3, m(48), m(48), 111)
    assert win.shape == (3, 48, 111) and win.dtype == torch.float32
    assert ns.stream_window_slots_la_(m(3, 5, 0), m(8, 5, 54), i3, i3, i3, i3, i3, i3, i3, None, None, 7).shape == (3, 5, 7)
