"""A chunk length per session in one pool push (streaming.py StreamPool.push(..., hops=)) without a GPU:
the two new ABI entry points and torch ops, every refusal `hops` adds (all before any launch, the table untouched), the
slot table's per-session accounting, and the window formula of bc_stream_window_slots_lens as a torch model."""
import os
import random
import re

import pytest
import torch

from audiotokenization_amd import _lib as L
from audiotokenization_amd.streaming import SlotTable, StreamPool
from helpers import build_models
from window_ref import window_equal, window_lens

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bc_stream_window_slots_lens", "bc_reslstm_fwd_state_lens")


def declared_symbols():
    txt = open(os.path.join(REPO, "include", "bigcodec.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(bc_[A-Za-z0-9_]+)\s*\(", txt))


def test_library_exports_the_ragged_entry_points():
    lib = L.load()
    assert L.ABI_VERSION == 18 and lib.bc_abi_version() == 18  # additive: the ABI version stays
    for name in NEW:
        assert name in L.EXPORTED and name in declared_symbols() and hasattr(lib, name), name


def test_ragged_ops_schemas_and_fakes():
    from audiotokenization_amd import ops

    ns = ops.load()
    want = {
        "stream_window_slots_lens_": "bigcodec::stream_window_slots_lens_(Tensor x, Tensor(a!) pool, Tensor src, Tensor dst, "
                                     "Tensor lens, int unit, Tensor? alpha_exp, Tensor? inv_beta, int P) -> Tensor",
        "reslstm_lens": "bigcodec::reslstm_lens(Tensor x, Tensor[] w_ih_packed, Tensor[] bias, Tensor[] w_hh_packed, "
                        "Tensor? out_alpha_exp, Tensor? out_inv_beta, int mode, Tensor? h0, Tensor? c0, Tensor lens) -> Tensor[]",
    }
    for name, schema in want.items():
        assert name in ops.OPS
        assert str(getattr(ns, name).default._schema) == schema
    m = lambda *s, dt=torch.float32: torch.empty(*s, device="meta", dtype=dt)  # noqa: E731
    i3 = m(3, dt=torch.int32)
    win = ns.stream_window_slots_lens_(m(3, 48, 100), m(10, 48, 18), i3, i3, i3, 25, m(48), m(48), 18)
    assert win.shape == (3, 48, 118) and win.dtype == torch.float32
    assert ns.stream_window_slots_lens_(m(3, 5, 20), m(8, 5, 54), i3, i3, i3, 4, None, None, 54).shape == (3, 5, 74)
    w = m(10)
    y, st, hT, cT = ns.reslstm_lens(m(3, 512, 6), [w, w], [w, w], [w, w], None, None, 1, None, None, i3)
    assert y.shape == (3, 512, 6) and st.shape == (1,) and st.dtype == torch.int32 and hT.shape == cT.shape == (2, 512, 3)
    y, st, hT, cT = ns.reslstm_lens(m(3, 256, 2), [w], [w], [w], m(256), m(256), 3, m(1, 256, 3), m(1, 256, 3), i3)
    assert y.shape == (3, 256, 2) and hT.shape == cT.shape == (1, 256, 3)


def test_ragged_abi_argument_checks():
    """Null or inconsistent arguments return 1, shapes of the per-step ResLSTM kernels 3, B == 0 windows 0: all without
    a launch (the pointers are fake)."""
    lib = L.load()

    def win(x=1, pool=1, src=1, dst=1, lens=1, unit=2, sa=None, sb=None, w=1, B=2, C=3, n=4, P=5, rows=6, xbs=12, xT=4):
        return lib.bc_stream_window_slots_lens(x, xbs, xT, pool, src, dst, lens, unit, sa, sb, w, B, C, n, P, rows, None)

    for kw in (dict(x=None), dict(pool=None), dict(src=None), dict(dst=None), dict(lens=None), dict(w=None), dict(sa=1),
               dict(sb=1), dict(B=-1), dict(C=0), dict(n=0), dict(P=0), dict(P=-3), dict(rows=0), dict(xT=3),
               dict(xbs=11), dict(unit=0), dict(unit=-2)):
        assert win(**kw) == 1, kw
    assert win(B=0) == 0 and win(B=0, sa=1, sb=1) == 0
    assert win(B=0, C=1 << 20, rows=1 << 12, xbs=1 << 40) == 3 and win(B=0, n=0x7fffffff, xT=1 << 40, xbs=1 << 50) == 3

    def lstm(x=1, out=1, B=2, H=256, T=4, layers=2, wih=1, bias=1, whh=1, sa=None, sb=None, ws=1, mode=1, h0=None,
             c0=None, hT=1, cT=1, lens=1):
        return lib.bc_reslstm_fwd_state_lens(x, out, B, H, T, layers, wih, bias, whh, sa, sb, ws, mode, h0, c0, hT, cT,
                                             lens, None)

    for kw in (dict(x=None), dict(out=None), dict(wih=None), dict(bias=None), dict(whh=None), dict(ws=None), dict(B=-1),
               dict(H=0), dict(H=250), dict(T=-1), dict(layers=0), dict(mode=4), dict(mode=-1), dict(h0=1), dict(c0=1),
               dict(hT=None), dict(cT=None)):
        assert lstm(**kw) == 1, kw
    # the per-step kernels carry no state (H = 768 and 48 in every mode, fp32 mode at any H): 3, as bc_reslstm_fwd_state
    for kw in (dict(H=768), dict(H=48), dict(mode=0), dict(H=768, mode=3), dict(H=1536, mode=0)):
        assert lstm(**kw) == 3, kw


# ---- the pool's refusals, all on the host (the models stay on the CPU: a launch would raise another error) ---------
@pytest.fixture(scope="module")
def models():
    enc, dec, *_ = build_models("debug", causal=True)
    return enc, dec


BAD_HOPS = ([2], [1, 2, 1], [], [0, 1], [1, 4], [-1, 2], [1, 2.0], [1, True], [False, 1], [1, None], [1, "2"])


def test_hops_refusals_before_any_launch(models):
    enc, dec = models
    pool = StreamPool(enc, 3)
    a, b = pool.open(), pool.open()
    x = torch.zeros(2, 1, 3 * pool.hop)  # n_hops = 3
    for hops in BAD_HOPS:
        with pytest.raises(ValueError):
            pool.push([a, b], x, hops=hops)
    with pytest.raises(ValueError):
        pool.push([a, b], x[:, :, :pool.hop], hops=[1, 2])  # two hops in a chunk of one
    with pytest.raises(ValueError):
        pool.push([a, a], x, hops=[1, 2])  # the existing refusals still come first
    # a refused push leaves the table untouched
    assert pool.table.pushes == [0, 0, None] and pool.table.samples[:2] == [0, 0] and not pool.table.undefined
    assert not pool._started and pool.samples(a) == 0 and pool.samples(b) == 0 and pool.live() == [a, b]

    dpool = StreamPool(dec, 2)
    d, e = dpool.open(), dpool.open()
    z = torch.zeros(2, dpool.channels, 3)
    codes = torch.zeros(2, 3, 1, dtype=torch.int64)
    for hops in BAD_HOPS:
        with pytest.raises(ValueError):
            dpool.push([d, e], z, hops=hops)
        with pytest.raises(ValueError):
            dpool.tokens([d, e], codes, hops=hops)
    assert dpool.table.pushes == [0, 0] and dpool.table.samples == [0, 0] and not dpool.table.undefined
    assert not dpool._started
    with pytest.raises(TypeError):
        pool.tokens([a], codes[:1], hops=[1])  # an encoder pool


def test_failed_ragged_push_marks_its_sessions(models):
    """A push with good hops passes the host checks; on the CPU its first launch raises, and its sessions, only they,
    are undefined: no sample is counted."""
    enc, _ = models
    pool = StreamPool(enc, 3)
    a, b, c = pool.open(), pool.open(), pool.open()
    old = L.precision_mode()
    try:
        L.set_precision("x6")
        with pytest.raises(L.BigCodecLibraryError):
            pool.push([a, c], torch.zeros(2, 1, 2 * pool.hop), hops=[1, 2])
    finally:
        L._mode = old
    assert pool.table.undefined == {a, c} and pool.table.pushes == [0, 0, 0] and pool.table.samples == [0, 0, 0]
    assert pool._stream._hops is None  # the push's hops do not outlive it


# ---- the slot table ------------------------------------------------------------------------------------------------
def test_commit_takes_one_amount_or_one_per_session():
    t = SlotTable(3)
    a, b, c = t.open(), t.open(), t.open()
    t.commit([a, b], 320)            # the present signature
    t.commit([c, a], [100, 7])       # one amount per session, in the order of sids
    t.commit([b], (5,))
    assert t.samples == [327, 325, 100] and t.pushes == [2, 2, 1]
    for bad in ([1], [1, 2, 3]):
        with pytest.raises(ValueError):
            t.commit([a, b], bad)
    assert t.samples == [327, 325, 100] and t.pushes == [2, 2, 1]


@pytest.mark.parametrize("capacity", [1, 2, 5])
def test_random_ragged_schedules_account_per_session(capacity):
    """Open / push a subset with its own hops per session / close, at random: every session's sample count is the sum
    of its own amounts, its push count the number of its pushes, and the ping-pong rows stay disjoint."""
    hop = 200
    for seed in range(200):
        rng = random.Random(seed * 11 + capacity)
        t = SlotTable(capacity)
        mine = {}  # open session -> [pushes, samples]
        for _ in range(40):
            op, live = rng.random(), t.live()
            if op < 0.3 and len(live) < capacity:
                mine[t.open()] = [0, 0]
            elif op < 0.45 and live:
                s = rng.choice(live)
                t.close(s)
                del mine[s]
            elif live:
                sids = rng.sample(live, rng.randint(1, len(live)))
                hops = [rng.randint(1, 5) for _ in sids]
                src, dst = t.plan(t.check(sids, capacity))
                assert not set(src) & set(dst) and len(set(dst)) == len(dst)
                assert src == [-1 if not mine[s][0] else 2 * s + (mine[s][0] & 1) for s in sids]
                t.commit(sids, [h * hop for h in hops])
                for s, h in zip(sids, hops):
                    mine[s][0] += 1
                    mine[s][1] += h * hop
            for s, (k, n) in mine.items():
                assert t.pushes[s] == k and t.samples[s] == n


# ---- the window formula ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 6, 18, 54])
def test_ragged_pieces_carry_the_context_of_equal_length_pushes(P):
    """A session's audio pushed in ragged pieces L_1, L_2, ... (each padded with NaN to the tick's n; L < P, L == P, L
    > P and L == n all occur) carries, piece by piece, the context the same pieces carry through the equal-length
    formula; its window is that formula's window followed by zeros; no NaN of the padding is ever read."""
    g = torch.Generator().manual_seed(P)
    rng = random.Random(P)
    pieces = [1, P, P + 3, max(1, P - 1), 2, 1, 3 * P, max(1, P // 2)] + [rng.randint(1, 2 * P + 2) for _ in range(12)]
    audio = torch.randn(sum(pieces), generator=g)
    ca = cb = torch.zeros(P)  # a fresh session reads zeros
    pos = 0
    for L_ in pieces:
        n = L_ + rng.choice([0, 0, 1, 5, P])  # the tick's padded length
        x = torch.full((n,), float("nan"))
        x[:L_] = audio[pos:pos + L_]
        wa, ca = window_lens(ca, x, L_)
        wb, cb = window_equal(cb, audio[pos:pos + L_])
        assert torch.equal(wa[:P + L_], wb) and torch.equal(ca, cb)
        assert wa.numel() == P + n and not torch.isnan(wa).any() and int(wa[P + L_:].abs().sum()) == 0
        whole = torch.cat([torch.zeros(P), audio[:pos + L_]])  # the causal pass's zero padding and all audio so far
        assert torch.equal(ca, whole[-P:])
        pos += L_
    assert pos == audio.numel()
