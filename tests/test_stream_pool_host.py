"""The streaming session pool (audiotokenization_amd/streaming.py StreamPool) without a GPU: the three
new ABI entry points and torch ops, and the host side of the pool: the slot table, the ping-pong row planning whose
disjointness bc_stream_window_slots relies on, and every refusal a push makes before it launches anything."""
import random

import pytest
import torch

from audiotokenization_amd import _lib as L
from audiotokenization_amd.streaming import SlotTable, StreamPool, plan_rows
from helpers import build_models

NEW = ("bc_stream_window_slots", "bc_lstm_state_gather", "bc_lstm_state_scatter")


def test_library_exports_the_pool_entry_points():
    lib = L.load()
    assert L.ABI_VERSION == 18 and lib.bc_abi_version() == 18  # additive: the ABI version stays
    for name in NEW:
        assert name in L.EXPORTED and hasattr(lib, name), name


def test_pool_ops_schemas_and_fakes():
    from audiotokenization_amd import ops

    ns = ops.load()
    want = {
        "stream_window_slots_": "bigcodec::stream_window_slots_(Tensor x, Tensor(a!) pool, Tensor src, Tensor dst, "
                                "Tensor? alpha_exp, Tensor? inv_beta, int P) -> Tensor",
        "lstm_state_gather": "bigcodec::lstm_state_gather(Tensor h_pool, Tensor c_pool, Tensor src, int B) -> Tensor[]",
        "lstm_state_scatter_": "bigcodec::lstm_state_scatter_(Tensor(a!) h_pool, Tensor(b!) c_pool, Tensor hT, Tensor cT, "
                               "Tensor dst) -> ()",
    }
    for name, schema in want.items():
        assert name in ops.OPS
        assert str(getattr(ns, name).default._schema) == schema
    m = lambda *s, dt=torch.float32: torch.empty(*s, device="meta", dtype=dt)  # noqa: E731
    i3 = m(3, dt=torch.int32)
    win = ns.stream_window_slots_(m(3, 48, 100), m(10, 48, 18), i3, i3, m(48), m(48), 18)
    assert win.shape == (3, 48, 118) and win.dtype == torch.float32
    assert ns.stream_window_slots_(m(3, 5, 20), m(8, 5, 54), i3, i3, None, None, 54).shape == (3, 5, 74)
    h0, c0 = ns.lstm_state_gather(m(2, 512, 10), m(2, 512, 10), i3, 3)
    assert h0.shape == c0.shape == (2, 512, 3)
    assert ns.lstm_state_scatter_(m(2, 512, 10), m(2, 512, 10), m(2, 512, 3), m(2, 512, 3), i3) is None


def test_pool_abi_argument_checks():
    """Null or inconsistent arguments return 1 and B == 0 returns 0, both without a launch (the pointers are fake)."""
    lib = L.load()

    def win(x=1, pool=1, src=1, dst=1, sa=None, sb=None, w=1, B=2, C=3, n=4, P=5, rows=6, xbs=12, xT=4):
        return lib.bc_stream_window_slots(x, xbs, xT, pool, src, dst, sa, sb, w, B, C, n, P, rows, None)

    for kw in (dict(x=None), dict(pool=None), dict(src=None), dict(dst=None), dict(w=None), dict(sa=1), dict(sb=1),
               dict(B=-1), dict(C=0), dict(n=0), dict(P=0), dict(P=-3), dict(rows=0), dict(xT=3), dict(xbs=11)):
        assert win(**kw) == 1, kw
    assert win(B=0) == 0 and win(B=0, sa=1, sb=1) == 0
    assert win(B=0, C=1 << 20, rows=1 << 12, xbs=1 << 40) == 3 and win(B=0, n=0x7fffffff, xT=1 << 40, xbs=1 << 50) == 3  # over 2^31

    for fn in (lib.bc_lstm_state_gather, lib.bc_lstm_state_scatter):
        good = dict(a=1, b=1, i=1, c=1, d=1, layers=2, H=128, B=3, rows=6)

        def call(**kw):
            v = dict(good, **kw)
            return fn(v["a"], v["b"], v["i"], v["c"], v["d"], v["layers"], v["H"], v["B"], v["rows"], None)

        for kw in (dict(a=None), dict(b=None), dict(i=None), dict(c=None), dict(d=None), dict(layers=0), dict(H=0),
                   dict(B=-1), dict(rows=0)):
            assert call(**kw) == 1, kw
        assert call(B=0) == 0
        assert call(layers=1 << 10, H=1 << 20, B=1 << 10) == 3


# ---- the slot table and the row planning ---------------------------------------------------------------------------
def test_open_returns_the_lowest_free_slot_and_close_reuses_it():
    t = SlotTable(3)
    assert [t.open(), t.open(), t.open()] == [0, 1, 2]
    with pytest.raises(RuntimeError):
        t.open()
    t.commit([1], 320)
    t.commit([1], 320)
    assert t.plan([1]) == ([2], [3]) and t.samples[1] == 640
    t.close(1)
    assert t.live() == [0, 2]
    assert t.open() == 1  # the lowest free slot, reused ...
    assert t.plan([1]) == ([-1], [3]) and t.samples[1] == 0  # ... as a fresh session: it reads zeros
    t.close(0)
    t.close(2)
    assert t.open() == 0 and t.open() == 2
    with pytest.raises(ValueError):
        SlotTable(0)


def test_ping_pong_rows_alternate_per_session():
    assert plan_rows([(0, 0), (4, 1), (2, 2), (1, 7)]) == ([-1, 9, 4, 3], [1, 8, 5, 2])
    t = SlotTable(2)
    a, b = t.open(), t.open()
    seen = []
    for tick in range(6):
        sids = [a, b] if tick % 3 == 0 else [a]  # b sits most ticks out: its rows advance with ITS pushes only
        src, dst = t.plan(sids)
        seen.append((src, dst))
        t.commit(sids, 1)
    assert seen == [([-1, -1], [1, 3]), ([1], [0]), ([0], [1]), ([1, 3], [0, 2]), ([0], [1]), ([1], [0])]


@pytest.mark.parametrize("capacity", [1, 2, 5])
def test_random_schedules_never_read_and_write_one_row(capacity):
    """For any schedule of open / push a subset / close: the src and dst row sets of a push are disjoint, dst has no
    duplicates, every row is inside the pool, a session reads the row it wrote last, a fresh one reads -1."""
    for seed in range(300):
        rng = random.Random(seed * 7 + capacity)
        t = SlotTable(capacity)
        last = {}  # open session -> the row its state is in
        for _ in range(40):
            op = rng.random()
            live = t.live()
            if op < 0.3 and len(live) < capacity:
                s = t.open()
                assert s == min(set(range(capacity)) - set(live))
                last[s] = -1
            elif op < 0.45 and live:
                s = rng.choice(live)
                t.close(s)
                del last[s]
            elif live:
                sids = rng.sample(live, rng.randint(1, len(live)))
                src, dst = t.plan(t.check(sids, capacity))
                assert len(src) == len(dst) == len(sids)
                assert not set(src) & set(dst) and len(set(dst)) == len(dst)
                assert all(0 <= d < 2 * capacity for d in dst) and all(-1 <= r < 2 * capacity for r in src)
                assert src == [last[s] for s in sids]
                assert all(d // 2 == s for s, d in zip(sids, dst))
                t.commit(sids, 1)
                last.update(zip(sids, dst))


# ---- the pool's refusals, all on the host (the models stay on the CPU: a launch would raise another error) ---------
@pytest.fixture(scope="module")
def models():
    enc, dec, *_ = build_models("debug", causal=True)
    return enc, dec


def test_pool_refusals_before_any_launch(models):
    enc, dec = models
    pool = StreamPool(enc, 3)
    hop = pool.hop
    assert pool.capacity == 3 and pool.channels == 1 and pool.state_bytes() == 0 and pool.live() == []
    a, b = pool.open(), pool.open()
    x2 = torch.zeros(2, 1, 2 * hop)
    for sids in ([a, 2], [a, 7], [a, -1], [a, "b"], [a, True]):  # never opened / outside the pool / not an id
        with pytest.raises(ValueError):
            pool.push(sids, x2)
    with pytest.raises(ValueError):
        pool.push([a, a], x2)  # twice in one push
    with pytest.raises(ValueError):
        pool.push([], torch.zeros(0, 1, hop))
    with pytest.raises(ValueError):
        pool.push([a], x2)  # the batch dimension is not len(sids)
    with pytest.raises(ValueError):
        pool.push([a, b], torch.zeros(2, 1, hop + 1))  # not a multiple of the hop
    with pytest.raises(ValueError):
        pool.push([a, b], torch.zeros(2, 1, 0))
    c = pool.open()
    with pytest.raises(RuntimeError):
        pool.open()  # full
    pool.close(c)
    with pytest.raises(ValueError):
        pool.push([c], torch.zeros(1, 1, hop))  # closed
    with pytest.raises(ValueError):
        pool.close(c)
    with pytest.raises(ValueError):
        pool.samples(c)
    with pytest.raises(TypeError):
        pool.tokens([a], torch.zeros(1, 2, 1, dtype=torch.int64))  # an encoder pool
    assert pool.table.pushes[:2] == [0, 0] and not pool.table.undefined and not pool._started  # nothing happened
    assert pool.samples(a) == 0 and pool.live() == [a, b]

    dpool = StreamPool(dec, 2)
    d = dpool.open()
    assert dpool.channels > 1
    with pytest.raises(ValueError):
        dpool.push([d], torch.zeros(2, dpool.channels, 3))
    with pytest.raises(ValueError):
        dpool.push([d], torch.zeros(1, dpool.channels + 1, 3))
    with pytest.raises(ValueError):
        dpool.tokens([d, d], torch.zeros(2, 3, 1, dtype=torch.int64))
    with pytest.raises(ValueError):
        dpool.tokens([d], torch.zeros(2, 3, 1, dtype=torch.int64))


def test_failed_push_marks_its_sessions_and_pins_the_precision(models):
    """A push that passes the host checks pins the pool's precision; when it then raises (here: the input is not on
    a HIP device, so nothing was launched, but the pool cannot know), its sessions are undefined until closed, the
    others are untouched, and a push in another precision is refused."""
    enc, _ = models
    pool = StreamPool(enc, 3)
    a, b = pool.open(), pool.open()
    x = torch.zeros(1, 1, pool.hop)
    old = L.precision_mode()
    try:
        L.set_precision("x6")
        with pytest.raises(L.BigCodecLibraryError):
            pool.push([a], x)
        assert pool.table.undefined == {a} and pool.table.pushes[a] == 0
        with pytest.raises(RuntimeError, match="undefined"):
            pool.push([a], x)
        with pytest.raises(RuntimeError, match="undefined"):
            pool.push([b, a], torch.zeros(2, 1, pool.hop))
        assert pool.table.undefined == {a}
        L.set_precision("h3")
        with pytest.raises(RuntimeError, match="precision changed"):
            pool.push([b], x)
        assert pool.table.undefined == {a}  # refused on the host: b is still good
        L.set_precision("x6")
        pool.close(a)
        assert pool.open() == a and not pool.table.undefined
    finally:
        L._mode = old


def test_pool_refuses_non_streamable_models():
    enc, dec, *_ = build_models("debug")
    with pytest.raises(ValueError):
        StreamPool(enc, 2)
    with pytest.raises(ValueError):
        StreamPool(dec, 2)
    enc_aa, *_ = build_models("debug", causal=True, antialias=True)
    with pytest.raises(NotImplementedError):
        StreamPool(enc_aa, 2)
    enc_c, *_ = build_models("debug", causal=True)
    with pytest.raises(ValueError):
        StreamPool(enc_c, 0)
