"""Look-ahead streaming of non-causal models (streaming.py LookaheadEncoder / LookaheadDecoder) without a
GPU: the plan's totals against the models' own per-layer length tables, its steady state, the look-ahead against a closed
form written from the configs alone, the plan executed in float64 on a toy stack with integer weights (every sum exact,
so stream == whole sequence must hold to the bit), the refusals, and the new ABI entry point and torch op."""
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from audiotokenization_amd import _lib as L
from audiotokenization_amd import config as cfgmod
from audiotokenization_amd import streaming as S
from helpers import build_models

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESETS = ("debug", "base", "default")
# derived in DESIGN.md §23 (samples); the closed form below reproduces them from the configs
LOOKAHEAD = {"debug": (3887, 4591), "base": (2293, 2741), "default": (2451, 2899)}


@pytest.fixture(scope="module")
def models():
    return {name: build_models(name)[:2] for name in PRESETS}


def chunkings(total, unit):
    """The two chunkings of the issue: [1, 3, 2 units, the rest at finish] and [everything at finish]."""
    return [([unit, 3 * unit, 2 * unit], total - 6 * unit), ([], total)]


# ---- plan totals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PRESETS)
def test_plan_totals_match_the_whole_sequence_lengths(models, name):
    enc, dec = models[name]
    hop = int(enc.hop_length)
    la_e, la_d = S.lookahead_samples(enc), S.lookahead_samples(dec)
    short_e = 6 * hop + 13
    assert short_e < la_e and 9 * hop < la_d  # both "shorter than the look-ahead" totals really are
    cases = [(enc, 7 * hop + 13, hop, enc.frame_lengths), (enc, short_e, hop, enc.frame_lengths),
             (dec, 9, 1, dec.sample_lengths), (dec, 6, 1, dec.sample_lengths)]
    for model, total, unit, lengths in cases:
        table = lengths([total], per_layer=True)
        for chunks, last in chunkings(total, unit):
            plan = S.lookahead_plan(model, chunks, last)
            assert len(plan) == len(chunks) + 1 and all(len(rows) == len(table) - 1 for rows in plan)
            for j in range(len(table) - 1):
                assert sum(rows[j][1] for rows in plan) == table[j][0], (name, total, chunks, j)  # what it was fed
                assert sum(rows[j][3] for rows in plan) == table[j + 1][0], (name, total, chunks, j)  # what it emitted
            assert sum(rows[-1][3] for rows in plan) == lengths([total])[0]
            for rows in plan:  # a stage's outputs are the next stage's new columns; carries chain from push to push
                assert all(rows[j][3] == rows[j + 1][1] for j in range(len(rows) - 1))
            for a, b in zip(plan, plan[1:]):
                assert all(ra[4] == rb[0] for ra, rb in zip(a, b))
            assert all(r[2] == 0 for rows in plan[:-1] for r in rows) and all(r[4] == 0 for r in plan[-1])


@pytest.mark.parametrize("name", PRESETS)
def test_plan_steady_state(models, name):
    """Equal chunks give equal rows once every stage has emitted: a stage that has emitted keeps a carry in
    (span - s, span] that depends on its input per push alone, so by induction along the flow the rows repeat from the
    push after the one in which the LAST stage first emits."""
    enc, dec = models[name]
    for model, unit in ((enc, int(enc.hop_length)), (dec, 1)):
        for per_push in (1, 3):
            plan = S.lookahead_plan(model, [per_push * unit] * 60, 0)[:-1]
            first = next(i for i, rows in enumerate(plan) if rows[-1][3] > 0)
            assert first + 1 < 40
            assert all(rows == plan[first + 1] for rows in plan[first + 1:]), (name, per_push)
            assert all(r[0] == r[4] for r in plan[-1])  # the carry length has settled
            out_unit = 1 if model is enc else int(dec.hop_length)
            assert plan[-1][-1][3] == per_push * out_unit


# ---- the look-ahead ------------------------------------------------------------------------------------------------
def closed_form(name):
    """The look-ahead from the preset's numbers alone.  Encoder: the k = 7 input conv reaches 3 samples, block i (at
    rate r_i = the strides before it) 3 (d1 + d2 + d3) columns for its units and floor(s / 2) for its k = 2s conv with
    padding ceil(s / 2), the k = 3 output conv one frame.  Decoder: the k = 7 input conv 3 frames; block i, at the rate
    behind its upsampler, ceil(s / 2) columns for the upsampler's padding (output o reads frames up to (o + p) // s) and
    3 (d1 + d2 + d3) for its units; the k = 7 output conv 3 samples."""
    p = cfgmod.PRESETS[name]
    e, d = p["codec_encoder"], p["codec_decoder"]
    rate, enc = 1, 3
    for s in e["up_ratios"]:
        enc += rate * (3 * sum(e["dilations"]) + s // 2)
        rate *= s
    enc += rate
    hop = 1
    for s in d["up_ratios"]:
        hop *= s
    rate, dec = hop, 3 * hop
    for s in d["up_ratios"]:
        rate //= s
        dec += rate * (3 * sum(d["dilations"]) + (s + 1) // 2)
    return enc, dec + 3


@pytest.mark.parametrize("name", PRESETS)
def test_lookahead_samples(models, name):
    enc, dec = models[name]
    got = (S.lookahead_samples(enc), S.lookahead_samples(dec))
    assert got == closed_form(name) == LOOKAHEAD[name]
    # what it means for the encoder: frame 0 is final exactly when look-ahead + hop samples are in
    hop = int(enc.hop_length)
    assert S.lookahead_plan(enc, [got[0] + hop - 1], 0)[0][-1][3] == 0
    assert S.lookahead_plan(enc, [got[0] + hop], 0)[0][-1][3] == 1
    # and for the decoder: sample 0 is final once the frame that covers sample `look-ahead` is in
    need = got[1] // hop + 1
    assert S.lookahead_plan(dec, [need - 1], 0)[0][-1][3] == 0 and S.lookahead_plan(dec, [need], 0)[0][-1][3] > 0


def test_lookahead_is_zero_for_causal_models():
    enc, dec = build_models("debug", causal=True)[:2]
    assert S.lookahead_samples(enc) == 0 and S.lookahead_samples(dec) == 0
    hop = int(enc.hop_length)
    plan = S.lookahead_plan(enc, [hop, 3 * hop, 2 * hop], 0)
    assert [rows[-1][3] for rows in plan] == [1, 3, 2, 0]
    plan = S.lookahead_plan(dec, [1, 4, 2], 0)
    assert [rows[-1][3] for rows in plan] == [hop, 4 * hop, 2 * hop, 0]


# ---- the plan executed in float64 on a toy stack --------------------------------------------------------------------
def act(x):
    return x.clamp(-3, 4)  # act(0) = 0, integers stay integers and bounded


def toy(stride, C=3, seed=0):
    """conv7 -> two dilated ResidualUnits -> act + strided conv (k = 2s) -> act + transposed conv (k = 2s): the toy's
    stages (as streaming._Stage, in flow order) and its integer weights."""
    g = torch.Generator().manual_seed(seed + stride)
    w = lambda *s: torch.randint(-2, 3, s, generator=g).double()  # noqa: E731
    s, p = stride, stride // 2 + stride % 2
    st = [S._Stage("conv", None, None, 7, 1, 1, 3, 3), S._Stage("unit", None, None, 7, 1, 1, 3, 3),
          S._Stage("unit", None, None, 7, 1, 3, 9, 9), S._Stage("conv", None, act, 2 * s, s, 1, p, p),
          S._Stage("convT", types.SimpleNamespace(out_len=lambda N: N * s), act, 2 * s, s, 1, p, 0, hist=1)]
    par = [(w(C, 1, 7), w(C)), (w(C, C, 7), w(C), w(C, C, 1), w(C)), (w(C, C, 7), w(C), w(C, C, 1), w(C)),
           (w(2 * C, C, 2 * s), w(2 * C)), (w(2 * C, C, 2 * s), w(C))]
    return st, par


def toy_whole(st, par, x):
    h = F.conv1d(x, *par[0], padding=3)
    for j in (1, 2):
        w7, b7, w1, b1 = par[j]
        h = h + F.conv1d(act(F.conv1d(act(h), w7, b7, padding=3 * st[j].d, dilation=st[j].d)), w1, b1)
    s, p = st[3].s, st[3].pl
    h = F.conv1d(act(h), *par[3], stride=s, padding=p)
    return F.conv_transpose1d(act(h), *par[4], stride=s, padding=p, output_padding=s % 2)


def toy_stream(st, par, x, chunks, last):
    """Execute the plan rows: every stage sees only [carry | new | its own right zeros]."""
    states = [q.start() for q in st]
    carry = [x.new_zeros(1, par[j][0].shape[0 if q.kind == "convT" else 1], q.start()[0]) for j, q in enumerate(st)]
    outs, pos = [], 0
    for i, n in enumerate(list(chunks) + [last]):
        flush = i == len(chunks)
        rows, nxt = S._plan_push(st, states, n, flush)
        h, pos = x[..., pos:pos + n], pos + n
        for j, (q, row) in enumerate(zip(st, rows)):
            cin, new, R, out, cout = row
            assert carry[j].shape[-1] == cin and h.shape[-1] == new
            if q.kind == "convT":
                held = torch.cat([carry[j], act(h)], dim=2)
                y = held.new_zeros(1, par[j][0].shape[1], 0)
                if out:
                    full = F.conv_transpose1d(held, *par[j], stride=q.s)
                    crop = states[j][2] + q.pl - (states[j][1] - cin) * q.s
                    y = full[..., crop:crop + out]
            else:
                held = torch.cat([carry[j], h if q.kind == "unit" or q.act is None else q.act(h)], dim=2)
                win = F.pad(held, (0, R))
                if not out:
                    y = held.new_zeros(1, par[j][0].shape[0], 0)
                elif q.kind == "conv":
                    y = F.conv1d(win, *par[j], stride=q.s)
                else:
                    w7, b7, w1, b1 = par[j]
                    y = win[..., q.pl:q.pl + out] + F.conv1d(act(F.conv1d(act(win), w7, b7, dilation=q.d)), w1, b1)
            assert y.shape[-1] == out
            carry[j] = held[..., held.shape[-1] - cout:]
            h = y
        states = nxt
        outs.append(h)
    return torch.cat(outs, dim=2), [o.shape[-1] for o in outs]


@pytest.mark.parametrize("stride", [4, 5])
@pytest.mark.parametrize("T", [97, 41])
def test_plan_executed_in_float64_equals_the_whole_sequence(stride, T):
    st, par = toy(stride)
    x = torch.randint(-3, 4, (1, 1, T), generator=torch.Generator().manual_seed(T)).double()
    want = toy_whole(st, par, x)
    assert want.shape[-1] == (T // stride if stride % 2 == 0 else (T + 1) // stride) * stride
    for chunks, last in (([7, 20, 3, 1], T - 31), ([], T), ([16, T - 16], 0)):  # the last: finish() with no new input
        got, counts = toy_stream(st, par, x, chunks, last)
        assert got.shape == want.shape and torch.equal(got, want), (stride, T, chunks)
        assert counts == [rows[-1][3] for rows in S.lookahead_plan_stages(st, chunks, last)]
    # the stream does hold back and does emit early: neither everything at finish nor everything at once
    _, counts = toy_stream(st, par, x, [16, T - 16], 0)
    assert counts[-1] > 0 and sum(counts[:-1]) > 0


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals_and_acceptance():
    enc, dec = build_models("debug")[:2]
    with pytest.raises(ValueError):
        S.StreamingEncoder(enc)  # the causal stream keeps refusing a non-causal model
    with pytest.raises(ValueError):
        S.StreamingDecoder(dec)
    with pytest.raises(ValueError):
        S.StreamPool(enc, 2)
    la, ld = S.LookaheadEncoder(enc), S.LookaheadDecoder(dec)  # ... and the look-ahead stream accepts it
    assert la.lookahead == LOOKAHEAD["debug"][0] and ld.lookahead == LOOKAHEAD["debug"][1] and la.hop == ld.hop == 320
    with pytest.raises(ValueError):
        la.push(torch.zeros(1, 1, 321))  # not a multiple of the hop
    with pytest.raises(ValueError):
        la.push(torch.zeros(1, 1, 0))
    with pytest.raises(ValueError):
        ld.push(torch.zeros(1, 512, 0))
    with pytest.raises(ValueError):
        la.finish()  # nothing was ever pushed
    for kw in (dict(antialias=True), dict(rnn_bidirectional=True)):
        e2, d2 = build_models("base", **kw)[:2]
        with pytest.raises(NotImplementedError):
            S.LookaheadEncoder(e2)
        with pytest.raises(NotImplementedError):
            S.LookaheadDecoder(d2)
        with pytest.raises(NotImplementedError):
            S.lookahead_plan(e2, [200], 0)
    ec, dc = build_models("debug", causal=True)[:2]
    assert S.LookaheadEncoder(ec).lookahead == 0 and S.LookaheadDecoder(dc).lookahead == 0


# ---- the new entry point -------------------------------------------------------------------------------------------
def test_library_exports_stream_window_la():
    lib = L.load()
    assert L.ABI_VERSION == 18 and lib.bc_abi_version() == 18  # additive: the ABI version stays
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bigcodec.h")).read(), flags=re.S)
    assert "bc_stream_window_la" in L.EXPORTED and hasattr(lib, "bc_stream_window_la")
    assert "bc_stream_window_la" in set(re.findall(r"\b(bc_[A-Za-z0-9_]+)\s*\(", txt))


def test_stream_window_la_argument_checks():
    """Null or inconsistent arguments return 1, sizes beyond 2^31 - 1 return 3, B == 0 returns 0: all without a launch
    (the pointers are fake)."""
    lib = L.load()

    def win(x=1, ctx=1, sa=None, sb=None, w=1, out=1, B=0, C=3, n=4, Pin=5, R=2, Pout=6, xbs=12, xT=4):
        return lib.bc_stream_window_la(x, xbs, xT, ctx, sa, sb, w, out, B, C, n, Pin, R, Pout, None)

    assert win() == 0 and win(ctx=None) == 0 and win(sa=1, sb=1) == 0
    assert win(x=None, n=0, xT=0, xbs=0, Pout=5) == 0  # a flush without new input: x is not needed
    assert win(Pout=0, out=None) == 0 and win(Pin=0, Pout=4, R=0) == 0 and win(Pout=9) == 0  # Pout up to Pin + n
    for kw in (dict(x=None), dict(w=None), dict(sa=1), dict(sb=1), dict(B=-1), dict(C=0), dict(n=-1), dict(Pin=-1),
               dict(R=-1), dict(Pout=-1), dict(xT=3), dict(xbs=11), dict(Pout=10), dict(out=None), dict(Pout=0),
               dict(n=0, Pin=0, R=0, Pout=0, out=None), dict(n=0, Pin=5, Pout=6)):
        assert win(**kw) == 1, kw
    assert win(C=1 << 20, B=1 << 12, xbs=1 << 40) == 3
    assert win(n=0x7fffffff, xT=1 << 40, xbs=1 << 50) == 3 and win(R=0x7fffffff) == 3


def test_stream_window_la_op_schema_and_fake():
    from audiotokenization_amd import ops

    ns = ops.load()
    assert "stream_window_la" in ops.OPS
    assert str(ns.stream_window_la.default._schema) == (
        "bigcodec::stream_window_la(Tensor x, Tensor? ctx, Tensor? alpha_exp, Tensor? inv_beta, int Pin, int R, int Pout)"
        " -> Tensor[]")
    m = lambda *s: torch.empty(*s, device="meta")  # noqa: E731
    win, ctx = ns.stream_window_la(m(2, 48, 100), m(2, 48, 3), m(48), m(48), 3, 0, 6)
    assert win.shape == (2, 48, 103) and ctx.shape == (2, 48, 6) and win.dtype == torch.float32
    win, ctx = ns.stream_window_la(m(2, 5, 0), m(2, 5, 6), None, None, 6, 3, 0)
    assert win.shape == (2, 5, 9) and ctx.shape == (2, 5, 0)
