"""The streaming session pool (audiotokenization_amd/streaming.py StreamPool) on the MI355X.

Kernels: bc_stream_window_slots against the existing bc_stream_window run per entry on that entry's own context, and
bc_lstm_state_gather / bc_lstm_state_scatter against torch indexing, all bit for bit, with every pool row pre-filled
with its own NaN payload so that a read of a wrong row shows in the values and a write to one shows in the bits.

Pool: five sessions of different lengths on a pool of three slots, opened, pushed in changing subsets and orders with
changing chunk lengths, closed and their slots reused; every session's concatenated output equals its own B = 1
StreamingEncoder / StreamingDecoder and the whole-sequence causal pass (bit for bit in x6, <= 1e-5 in h3: the rule
of test_gpu_streaming.py).  PoolGraph: replays with changing membership equal the eager pool bit for bit.
"""
import pytest
import torch

from audiotokenization_amd import _lib as L
from audiotokenization_amd import ops, synth
from audiotokenization_amd.streaming import StreamingDecoder, StreamingEncoder, StreamPool
from helpers import build_models, max_rel_err

pytestmark = pytest.mark.gpu


def nan_rows(rows, *shape, dev, axis=0):
    """A float32 tensor whose slice `r` along `axis` holds the quiet NaN with payload r + 1."""
    bits = (0x7FC00000 + 1 + torch.arange(rows, dtype=torch.int32)).view([-1 if i == axis else 1 for i in range(len(shape))])
    return bits.expand(*shape).contiguous().view(torch.float32).to(dev)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- kernels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("B,C,P,n", [(3, 5, 18, 100), (4, 7, 54, 20), (2, 48, 6, 1), (1, 3, 1, 7)])
def test_stream_window_slots_kernel(dev, B, C, P, n, act, strided):
    ns = ops.load()
    g = torch.Generator().manual_seed(1000 * B + 10 * P + n + int(act))
    rows = 2 * B + 3
    perm = torch.randperm(rows, generator=g).tolist()
    # entry i: 1 (mod 3) is a fresh session (src = -1), 2 (mod 3) is discarded (dst = -1), the others carry and store
    src = [-1 if i % 3 == 1 else perm[i] for i in range(B)]
    dst = [-1 if i % 3 == 2 else perm[B + i] for i in range(B)]
    pool = nan_rows(rows, rows, C, P, dev=dev)
    for r in src:
        if r >= 0:
            pool[r] = torch.randn(C, P, generator=g).to(dev)
    before = pool.clone()
    base = torch.randn(B, C, P + n, generator=g).to(dev)
    x = base[:, :, P:] if strided else base[:, :, P:].contiguous()
    assert x.is_contiguous() != strided or B * C == 1
    a = torch.rand(C, generator=g).add(0.5).to(dev) if act else None
    ib = torch.rand(C, generator=g).add(0.5).to(dev) if act else None
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    win = ns.stream_window_slots_(x, pool, i32(src), i32(dst), a, ib, P)
    assert win.shape == (B, C, P + n)
    for i in range(B):
        ctx = before[src[i]].unsqueeze(0) if src[i] >= 0 else None
        w1, c1 = ns.stream_window(x[i:i + 1], ctx, a, ib, P)
        assert torch.equal(win[i:i + 1], w1), f"entry {i}: window"
        assert not torch.isnan(win[i]).any()
        if dst[i] >= 0:
            assert torch.equal(pool[dst[i]], win[i, :, n:]) and torch.equal(pool[dst[i]], c1[0]), f"entry {i}: next context"
    keep = [r for r in range(rows) if r not in dst]
    assert torch.equal(bits(pool[keep]), bits(before[keep])), "a pool row no entry names in dst changed"


@pytest.mark.parametrize("layers,H,rows,B", [(2, 128, 7, 3), (1, 512, 2, 1), (2, 1536, 9, 5)])
def test_lstm_state_gather_scatter_kernels(dev, layers, H, rows, B):
    ns = ops.load()
    g = torch.Generator().manual_seed(H + rows)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    perm = torch.randperm(rows, generator=g).tolist()[:B]
    cases = [perm, [-1 if i % 2 else r for i, r in enumerate(perm)], [-1] * B]
    for idx in cases:
        # gather: only the rows src names are data, every other row is a NaN nothing may read
        hp, cp = (nan_rows(rows, layers, H, rows, dev=dev, axis=2) for _ in "hc")
        for r in idx:
            if r >= 0:
                hp[:, :, r] = torch.randn(layers, H, generator=g).to(dev)
                cp[:, :, r] = torch.randn(layers, H, generator=g).to(dev)
        h_before, c_before = hp.clone(), cp.clone()
        h0, c0 = ns.lstm_state_gather(hp, cp, i32(idx), B)
        assert h0.shape == c0.shape == (layers, H, B) and h0.is_contiguous() and c0.is_contiguous()
        for b, r in enumerate(idx):
            want_h = h_before[:, :, r] if r >= 0 else torch.zeros(layers, H, device=dev)
            want_c = c_before[:, :, r] if r >= 0 else torch.zeros(layers, H, device=dev)
            assert torch.equal(h0[:, :, b], want_h) and torch.equal(c0[:, :, b], want_c), (idx, b)
        assert torch.equal(bits(hp), bits(h_before)) and torch.equal(bits(cp), bits(c_before))
        # scatter: the rows dst names take the entries' state, every other row keeps its bits
        hT, cT = torch.randn(layers, H, B, generator=g).to(dev), torch.randn(layers, H, B, generator=g).to(dev)
        hp, cp = (nan_rows(rows, layers, H, rows, dev=dev, axis=2) for _ in "hc")
        h_before, c_before = hp.clone(), cp.clone()
        assert ns.lstm_state_scatter_(hp, cp, hT, cT, i32(idx)) is None
        for b, r in enumerate(idx):
            if r >= 0:
                assert torch.equal(hp[:, :, r], hT[:, :, b]) and torch.equal(cp[:, :, r], cT[:, :, b]), (idx, b)
        keep = [r for r in range(rows) if r not in idx]
        assert torch.equal(bits(hp[:, :, keep]), bits(h_before[:, :, keep]))
        assert torch.equal(bits(cp[:, :, keep]), bits(c_before[:, :, keep]))


# ---- the pool against single-session streams -----------------------------------------------------------------------
HOPS = {"A": 12, "B": 7, "C": 9, "D": 5, "E": 6}  # session lengths in hops (frames)
CAPACITY = 3
# (sessions opened before the push, the push's sessions in order, hops per session in this push, sessions closed after)
SCHEDULE = [
    ("A", "A", 2, ""),
    ("B", "BA", 3, ""),
    ("C", "ABC", 1, ""),
    ("", "CA", 2, ""),      # B sits this tick out
    ("", "BCA", 3, "B"),    # B ends; D gets its slot
    ("D", "DAC", 1, "A"),   # A ends; E gets its slot
    ("E", "CE", 2, "C"),
    ("", "ED", 3, ""),
    ("", "DE", 1, "DE"),
]
REUSE = {"D": "B", "E": "A"}  # who must get whose session id


def run_schedule(pool, inputs, unit, push=None):
    """SCHEDULE on `pool`: inputs[s] (1, C, HOPS[s] * unit) is session s's whole input, cut along the last axis in
    pieces of hops * unit columns; returns each session's concatenated output.  `push(sids, x)`: pool.push unless
    given (the token entry)."""
    push = push or pool.push
    sid, pos, out, closed_id = {}, {s: 0 for s in HOPS}, {s: [] for s in HOPS}, {}
    sizes, stale = set(), {}  # stale[s]: the bits of a closed session's pool rows
    for opened, members, hops, closed in SCHEDULE:
        for s in opened:
            sid[s] = pool.open()
            if s in REUSE:  # the slot of a closed session, whose state is still in the pool (nothing was zeroed)
                assert sid[s] == closed_id[REUSE[s]], (s, sid[s], closed_id)
                rows = slice(2 * sid[s], 2 * sid[s] + 2)
                assert all(torch.equal(bits(t[rows]), old) for t, old in zip(pool._stream._ctx.values(), stale[REUSE[s]]))
        assert len(pool.live()) <= CAPACITY
        n = hops * unit
        x = torch.cat([inputs[s][..., pos[s]:pos[s] + n] for s in members], dim=0)
        y = push([sid[s] for s in members], x)
        assert y.shape[0] == len(members)
        for i, s in enumerate(members):
            out[s].append(y[i:i + 1].clone())
            pos[s] += n
        sizes.add(len(members))
        for s in closed:
            assert pos[s] == inputs[s].shape[-1], f"session {s} closed before its input ended"
            rows = slice(2 * sid[s], 2 * sid[s] + 2)
            stale[s] = [bits(t[rows]).clone() for t in pool._stream._ctx.values()]
            pool.close(sid[s])
            closed_id[s] = sid[s]
    assert sizes == {1, 2, 3} and pool.live() == []
    return {s: torch.cat(v, dim=2) for s, v in out.items()}


def clip(s, hop, dev):
    n = HOPS[s] * hop
    return torch.from_numpy(synth.synth_clips(1, n, clip0=50 + ord(s))).unsqueeze(1).to(dev)


def compare(what, got, alone, whole, sprec):
    assert got.shape == alone.shape == whole.shape, (what, got.shape, alone.shape, whole.shape)
    e1, e2 = max_rel_err(got, alone), max_rel_err(got, whole)
    print(f"{what} [{sprec}]: pool vs its own B=1 stream {e1:.2e}, vs the whole-sequence pass {e2:.2e}")
    if sprec == "x6":
        assert torch.equal(got, alone), f"{what}: pool != B=1 stream ({e1:.3e})"
        assert torch.equal(got, whole), f"{what}: pool != whole-sequence pass ({e2:.3e})"
    else:
        assert e1 <= 1e-5 and e2 <= 1e-5, (what, e1, e2)


@pytest.mark.parametrize("model,sprec", [("base", "x6"), ("base", "h3"), ("debug", "x6"), ("debug", "h3"),
                                         ("default", "x6")])
def test_pool_encode_equals_single_streams(dev, model, sprec):
    old = L.precision_mode()
    try:
        L.set_precision(sprec)
        enc, *_ = build_models(model, device=dev, causal=True)
        hop = int(enc.hop_length)
        x = {s: clip(s, hop, dev) for s in HOPS}
        with torch.no_grad():
            pool = StreamPool(enc, CAPACITY)
            got = run_schedule(pool, x, hop)
            torch.cuda.synchronize()
            assert pool.state_bytes() > 0
            for s in HOPS:
                compare(f"encode {model} session {s}", got[s], StreamingEncoder(enc).encode(x[s], 2 * hop), enc(x[s]), sprec)
    finally:
        L._mode = old


@pytest.mark.parametrize("model,sprec,tokens", [("base", "x6", False), ("base", "h3", False), ("debug", "x6", False),
                                                ("debug", "h3", False), ("base", "x6", True), ("debug", "h3", True)])
def test_pool_decode_equals_single_streams(dev, model, sprec, tokens):
    old = L.precision_mode()
    try:
        L.set_precision(sprec)
        enc, dec, *_ = build_models(model, device=dev, causal=True)
        hop = int(enc.hop_length)
        with torch.no_grad():
            z, whole, alone = {}, {}, {}
            for s in HOPS:
                post, codes, _ = dec(enc(clip(s, hop, dev)), vq=True)
                sd = StreamingDecoder(dec)
                if tokens:  # (1, F, Nq) index frames; the schedule cuts frames, so they go last for run_schedule
                    tok = codes.permute(1, 2, 0).contiguous()
                    z[s] = tok.permute(0, 2, 1).contiguous()
                    whole[s] = dec(dec.tokens_to_latent(tok), vq=False)
                    alone[s] = torch.cat([sd.tokens(tok[:, i:i + 2]) for i in range(0, tok.shape[1], 2)], dim=2)
                else:
                    z[s] = post
                    whole[s] = dec(post, vq=False)
                    alone[s] = sd.decode(post, 2)
            pool = StreamPool(dec, CAPACITY)
            push = (lambda sids, t: pool.tokens(sids, t.permute(0, 2, 1).contiguous())) if tokens else None
            got = run_schedule(pool, z, 1, push)
            torch.cuda.synchronize()
        for s in HOPS:
            assert got[s].shape == (1, 1, HOPS[s] * hop)
            compare(f"decode {model}{' tokens' if tokens else ''} session {s}", got[s], alone[s], whole[s], sprec)
    finally:
        L._mode = old


# ---- one graph for any membership -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sprec", ["h3", "x6"])
def test_pool_graph_equals_eager_pool(dev, sprec):
    """pool.graph(3, n): replays with 3, 2 and 1 live entries and changing membership and order equal the eager pool
    bit for bit, encode and decode; an eager push afterwards (another chunk length) continues from the graph's
    state; a chunk of another length and more sessions than entries are refused; the status words are read."""
    old = L.precision_mode()
    try:
        L.set_precision(sprec)
        enc, dec, *_ = build_models("base", device=dev, causal=True)
        hop = int(enc.hop_length)
        ticks = [(0, 1, 2), (2, 0), (1,), (1, 2, 0), (2,), (0, 1)]
        with torch.no_grad():
            x = torch.from_numpy(synth.synth_clips(3, 12 * hop, clip0=71)).unsqueeze(1).to(dev)
            z = dec(enc(x), vq=True)[0]
            for model, data, unit in ((enc, x, hop), (dec, z, 1)):
                n = 2 * unit
                pe, pg = StreamPool(model, 3), StreamPool(model, 4)
                g = pg.graph(3, n)
                se, sg = [pe.open() for _ in range(3)], [pg.open() for _ in range(3)]
                pos = [0, 0, 0]
                for members in ticks:
                    xin = torch.cat([data[m:m + 1, :, pos[m]:pos[m] + n] for m in members], dim=0)
                    want = pe.push([se[m] for m in members], xin)
                    got = g.push([sg[m] for m in members], xin).clone()
                    assert got.shape == want.shape and torch.equal(got, want), (members, max_rel_err(got, want))
                    for m in members:
                        pos[m] += n
                assert pos == [8 * unit] * 3 and [pg.samples(s) for s in sg] == [pe.samples(s) for s in se]
                with pytest.raises(ValueError):
                    g.push(sg[:1], data[:1, :, :unit])  # another chunk length
                extra = pg.open()
                with pytest.raises(ValueError):
                    g.push(sg + [extra], torch.cat([data, data[:1]], dim=0)[:, :, :n])  # four sessions, three entries
                tail = data[:, :, 8 * unit:11 * unit]  # eager, three hops: continues from the state the graph left
                assert torch.equal(pg.push(sg, tail), pe.push(se, tail))
                torch.cuda.synchronize()
                assert g._status, "the graph holds the ResLSTM status words"
                g.check()
    finally:
        L._mode = old


# ---- refusals on the device model ------------------------------------------------------------------------------------
def test_pool_refusals_on_the_device(dev):
    enc, dec, *_ = build_models("debug", device=dev)
    with pytest.raises(ValueError):
        StreamPool(enc, 2)
    with pytest.raises(ValueError):
        StreamPool(dec, 2)
    enc_aa, dec_aa, *_ = build_models("debug", device=dev, causal=True, antialias=True)
    with pytest.raises(NotImplementedError):
        StreamPool(enc_aa, 2)
    with pytest.raises(NotImplementedError):
        StreamPool(dec_aa, 2)
    enc_c, *_ = build_models("debug", device=dev, causal=True)
    pool = StreamPool(enc_c, 2)
    a, b = pool.open(), pool.open()
    with pytest.raises(RuntimeError):
        pool.open()
    with pytest.raises(ValueError):
        pool.push([a, b], torch.zeros(2, 1, pool.hop + 1, device=dev))
    with pytest.raises(ValueError):
        pool.graph(2, pool.hop + 1)
    with pytest.raises(ValueError):
        pool.graph(3, pool.hop)
    with torch.no_grad():  # none of the refusals touched the sessions
        y = pool.push([b, a], torch.zeros(2, 1, pool.hop, device=dev))
    assert y.shape[0] == 2 and y.shape[2] == 1 and pool.samples(a) == pool.samples(b) == pool.hop
