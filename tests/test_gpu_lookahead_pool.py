"""LookaheadPool (streaming.py) on the MI355X.

Window kernel: bc_stream_window_slots_la against bc_stream_window_la run per entry on that entry's own carry and its own
columns, bit for bit, with NaN everywhere the kernel must not read; the two degenerate cases against
bc_stream_window_slots and bc_stream_window_la; opcheck.

Pool: the host test's schedule (lookahead_pool_ref.TICKS: five sessions on three slots, in transient, steady and flushing
side by side) on real models.  Each session's claimed columns, concatenated, must equal its own B = 1 look-ahead stream
and the whole-sequence forward on its own data,
  x6 and fp32: BIT FOR BIT (an output column is a fixed-order sum over its own input columns, wherever it sits);
  h3 (per-tile block scales): max |a - b| / max |b| <= 1e-5, the bound §18 and §23 hold their h3 streams to.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from audiotokenization_amd import _lib as L
from audiotokenization_amd import ops
from audiotokenization_amd import streaming as S
from audiotokenization_amd import synth
from helpers import max_rel_err
from lookahead_pool_ref import CAPACITY, ORDER, run_schedule, totals
from test_gpu_lookahead import agree, models, precision

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_timed_out_wait(dev):
    yield
    assert L.load().bc_lstm_status(1) == 0


def nan_like(*shape, dev):
    """A float32 tensor of quiet NaNs whose payload is the element's own index (a moved NaN is a visible change)."""
    n = 1
    for s in shape:
        n *= s
    return (0x7FC00001 + torch.arange(n, dtype=torch.int32) % 0x100000).view(torch.float32).reshape(shape).to(dev)


def bits(t):
    return t.contiguous().view(torch.int32)


def i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


# ---- 1. the window kernel -------------------------------------------------------------------------------------------
def entries(Pmax, C):
    """Six entries (cin, n, xoff, keep, cout, fresh, stored): a fresh session (src = -1; its cin columns are zeros), a
    carry shorter than the pitch with a stored carry that is no suffix of the row, no new column, an input offset, a
    new carry that reaches back into the old one (n < cout), and cout = 0; one of them is a padding entry (dst = -1)."""
    half, few = Pmax // 2, min(1, Pmax - 1)
    e = [(half, 7, 0, half + 7 - min(Pmax, half + 7), min(Pmax, half + 7), True, True),
         (max(Pmax - 2, 0), 20, 0, 3, Pmax, False, True),
         (Pmax, 0, 0, Pmax - (Pmax + 1) // 2, (Pmax + 1) // 2, False, True),
         (Pmax, 9, 5, 9, Pmax, False, True),
         (Pmax, few, 2, few, Pmax, False, True),
         (Pmax, 13, 1, 4, 0, False, True)]
    pad = 3 if C == 3 else 1
    e[pad] = e[pad][:6] + (False,)
    return e


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("Pmax", [1, 6, 8, 54])
@pytest.mark.parametrize("C", [3, 5])
def test_stream_window_slots_la_kernel(dev, C, Pmax, act, strided):
    ns = ops.load()
    B, W, xn = 6, Pmax + 20, 25
    ent = entries(Pmax, C)
    g = torch.Generator().manual_seed(100 * Pmax + 10 * C + int(act))
    rows = 2 * B + 3
    perm = torch.randperm(rows, generator=g).tolist()
    src = [-1 if e[5] else perm[i] for i, e in enumerate(ent)]
    dst = [perm[B + i] if e[6] else -1 for i, e in enumerate(ent)]
    pool = nan_like(rows, C, Pmax, dev=dev)  # NaN in every foreign row and in a source row's columns beyond cin
    base = nan_like(B, C, xn + 11, dev=dev)  # NaN outside every [xoff, xoff + n)
    for i, (cin, n, xo, keep, cout, fresh, stored) in enumerate(ent):
        assert keep + cout <= cin + n <= W and xo + n <= xn  # the caller's duty, and the test's own shapes
        if src[i] >= 0:
            pool[src[i], :, :cin] = torch.randn(C, cin, generator=g).to(dev)
        base[i, :, 11 + xo:11 + xo + n] = torch.randn(C, n, generator=g).to(dev)
    before = pool.clone()
    x = base[:, :, 11:] if strided else base[:, :, 11:].contiguous()
    assert x.is_contiguous() != strided
    a = torch.rand(C, generator=g).add(0.5).to(dev) if act else None
    ib = torch.rand(C, generator=g).add(0.5).to(dev) if act else None
    col = lambda k: i32([e[k] for e in ent], dev)  # noqa: E731
    win = ns.stream_window_slots_la_(x, pool, i32(src, dev), i32(dst, dev), col(0), col(1), col(2), col(3), col(4), a, ib, W)
    assert win.shape == (B, C, W)
    assert not torch.isnan(win).any(), "a NaN of an input tail, of a pool row's tail or of a foreign row reached a window"
    for i, (cin, n, xo, keep, cout, fresh, stored) in enumerate(ent):
        ctx = before[src[i], :, :cin].unsqueeze(0).contiguous() if src[i] >= 0 and cin else None
        suffix = keep == cin + n - cout
        w1, c1 = ns.stream_window_la(x[i:i + 1, :, xo:xo + n], ctx, a, ib, cin, W - cin - n, cout if suffix else 0)
        assert torch.equal(bits(win[i:i + 1]), bits(w1)), f"entry {i}: window"
        assert int(bits(win[i, :, cin + n:]).abs().max()) == 0, f"entry {i}: the tail is not +0.0"
        if dst[i] >= 0:
            row = pool[dst[i]]
            assert torch.equal(bits(row[:, :cout]), bits(win[i, :, keep:keep + cout])), f"entry {i}: stored carry"
            if suffix and cout:
                assert torch.equal(bits(row[:, :cout]), bits(c1[0])), f"entry {i}: carry != bc_stream_window_la's"
            assert torch.equal(bits(row[:, cout:]), bits(before[dst[i], :, cout:])), f"entry {i}: wrote past cout"
    written = [r for r, e in zip(dst, ent) if r >= 0 and e[4]]
    keep_rows = [r for r in range(rows) if r not in written]
    assert torch.equal(bits(pool[keep_rows]), bits(before[keep_rows])), "a pool row no entry stores to changed"


@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("C,P,n", [(3, 6, 13), (5, 54, 7), (5, 1, 20), (3, 8, 3)])
def test_degenerate_cases_reproduce_the_neighbours(dev, C, P, n, act):
    ns = ops.load()
    g = torch.Generator().manual_seed(P * 7 + n)
    B, rows = 4, 11
    a = torch.rand(C, generator=g).add(0.5).to(dev) if act else None
    ib = torch.rand(C, generator=g).add(0.5).to(dev) if act else None
    x = torch.randn(B, C, n, generator=g).to(dev)
    pool0 = torch.randn(rows, C, P, generator=g).to(dev)
    src, dst = [0, -1, 5, 7], [1, 2, -1, 9]
    # every cin == cout == Pmax, n == W - Pmax, xoff == 0, keep == n: bc_stream_window_slots
    p1, p2 = pool0.clone(), pool0.clone()
    full = lambda v: i32([v] * B, dev)  # noqa: E731
    w1 = ns.stream_window_slots_la_(x, p1, i32(src, dev), i32(dst, dev), full(P), full(n), full(0), full(n), full(P), a, ib,
                                    P + n)
    w2 = ns.stream_window_slots_(x, p2, i32(src, dev), i32(dst, dev), a, ib, P)
    assert torch.equal(bits(w1), bits(w2)) and torch.equal(bits(p1), bits(p2))
    # one entry, a fresh session (src = -1) or a dense carry in its pool row: bc_stream_window_la
    one = lambda v: i32([v], dev)  # noqa: E731
    for fresh, R, Pout in ((True, 0, P), (False, 3, min(P, 2)), (False, 0, P), (True, 5, 0)):
        p3 = pool0.clone()
        w3 = ns.stream_window_slots_la_(x[:1], p3, one(-1 if fresh else 4), one(6), one(P), one(n), one(0),
                                        one(P + n - Pout), one(Pout), a, ib, P + n + R)
        w4, c4 = ns.stream_window_la(x[:1], None if fresh else pool0[4:5].contiguous(), a, ib, P, R, Pout)
        assert torch.equal(bits(w3), bits(w4)) and torch.equal(bits(p3[6, :, :Pout]), bits(c4[0])), (fresh, R, Pout)
        assert torch.equal(bits(p3[6, :, Pout:]), bits(pool0[6, :, Pout:]))


def test_opcheck_stream_window_slots_la(dev):
    ns = ops.load()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 5, 12, generator=g).to(dev)
    pool = torch.randn(8, 5, 6, generator=g).to(dev)
    a, ib = torch.rand(5, generator=g).add(0.5).to(dev), torch.rand(5, generator=g).add(0.5).to(dev)
    args = (x, pool, i32([0, -1, 3], dev), i32([1, 2, -1], dev), i32([6, 3, 4], dev), i32([12, 5, 0], dev),
            i32([0, 2, 0], dev), i32([12, 2, 1], dev), i32([6, 6, 3], dev))
    torch.library.opcheck(ns.stream_window_slots_la_.default, args + (a, ib, 20))
    torch.library.opcheck(ns.stream_window_slots_la_.default, args + (None, None, 18))


# ---- 2. the pool on real models -------------------------------------------------------------------------------------
SCALE = 2  # real hops per hop of the schedule: the presets' look-ahead is 11.5 to 14.3 hops, the toy's is 5, and the
# sessions must run past it (7 to 12 schedule hops are 14 to 24 real ones: frames come out while the sessions run)


def drive(pool, data, unit, decoder, tokens=None, tail=float("nan")):
    """run_schedule on a LookaheadPool (`unit`: input columns per SCHEDULE hop), with samples(sid) and the counts'
    bookkeeping checked after every call."""
    moved = {}

    def book(sids, lens, counts, closed):
        for s, n, c in zip(sids, lens, counts):
            moved[s] = moved.get(s, 0) + (c if decoder else n)
            if not closed:
                assert pool.samples(s) == moved[s], (s, pool.samples(s), moved[s])
        for s in sids if closed else ():
            moved.pop(s)
            assert s not in pool.live()

    def push(sids, x, hops, flags):
        fin = flags if any(flags) else None
        hops = [h * SCALE for h in hops]
        if tokens is not None:
            y, counts = pool.tokens(sids, x.permute(0, 2, 1).contiguous(), hops=hops, finish=fin)
        else:
            y, counts = pool.push(sids, x, hops=hops, finish=fin)
        assert counts == pool.plan.counts
        live = [s for s, f in zip(sids, flags) if not f]
        book(live, [h * unit // SCALE for h, f in zip(hops, flags) if not f], [c for c, f in zip(counts, flags) if not f], False)
        for s, f in zip(sids, flags):
            if f:
                moved.pop(s, None)
                assert s not in pool.live()
        return y, counts

    def finish(sids, x, lens):
        if x is not None and tokens is not None:
            x = tokens(x.permute(0, 2, 1).contiguous())  # finish() takes frames: the -1 indices become NaN columns
        y, counts = pool.finish(sids, x, lens)
        book(sids, lens or [0] * len(sids), counts, True)
        return y, counts

    return run_schedule(data, unit, pool.open, push, finish, tail=tail)


def compare(what, outs, alone, whole, prec):
    got = torch.cat(outs, dim=2)
    assert got.shape == whole.shape, (what, got.shape, whole.shape)
    agree(got, alone, prec, what + " vs its own B = 1 stream")
    agree(got, whole, prec, what + " vs the whole pass")


def own_stream(stream, x, chunks, push=None):
    """The session's own B = 1 look-ahead stream with the pool's chunking: (outputs per call, concatenated)."""
    push = push or stream.push
    outs, pos = [], 0
    for n in chunks[:-1]:
        outs.append(push(x[..., pos:pos + n]))
        pos += n
    outs.append(stream.finish(x[..., pos:]))
    return outs


def encoder_case(dev, model, prec):
    enc, _ = models(model, dev)
    hop = int(enc.hop_length)
    T = totals(SCALE * hop)
    x = {s: torch.from_numpy(synth.synth_clips(1, T[s], clip0=40 + ord(s))).unsqueeze(1).to(dev) for s in ORDER}
    with precision(prec), torch.no_grad():
        pool = S.LookaheadPool(enc, CAPACITY)
        outs, chunks, _ = drive(pool, x, SCALE * hop, False)
        torch.cuda.synchronize()
        assert pool.live() == [] and pool.state_bytes() > 0
        early = 0
        for s in ORDER:
            plan = S.lookahead_plan(enc, chunks[s][:-1], chunks[s][-1])
            assert [o.shape[-1] for o in outs[s]] == [rows[-1][3] for rows in plan], s
            alone = torch.cat(own_stream(S.LookaheadEncoder(enc), x[s], chunks[s]), dim=2)
            compare(f"pool encoder {model} session {s}", outs[s], alone, enc(x[s]), prec)
            early += sum(o.shape[-1] for o in outs[s][:-1])
        assert early > 0  # frames come out while the sessions run
    return {s: torch.cat(outs[s], dim=2) for s in ORDER}


@pytest.mark.parametrize("prec", ["x6", "h3"])
def test_pool_encoder_equals_single_streams_and_whole_pass(dev, prec):
    encoder_case(dev, "base", prec)


def test_pool_fp32_encoder_two_launch_units(dev):
    """fp32: the ResidualUnits take the two-launch path over the same raw windows; bit for bit with the whole pass."""
    encoder_case(dev, "debug", "fp32")


@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("prec", ["x6", "h3"])
def test_pool_decoder_equals_single_streams_and_whole_pass(dev, prec, tokens):
    enc, dec = models("debug", dev)
    hop = int(dec.hop_length)
    F_ = totals(SCALE)
    with precision(prec), torch.no_grad():
        z, whole, alone = {}, {}, {}
        for s in ORDER:
            clip = torch.from_numpy(synth.synth_clips(1, F_[s] * hop, clip0=70 + ord(s))).unsqueeze(1).to(dev)
            post, codes, _ = dec(enc(clip), vq=True)
            assert post.shape[-1] == F_[s]
            if tokens:
                tok = codes.permute(1, 2, 0).contiguous()  # (1, F, Nq)
                z[s] = tok.permute(0, 2, 1).contiguous()  # laid out (1, Nq, F) for the schedule's batches
                whole[s] = dec(dec.tokens_to_latent(tok), vq=False)
            else:
                z[s] = post
                whole[s] = dec(post, vq=False)
        pool = S.LookaheadPool(dec, CAPACITY)
        if tokens:  # an index of -1 behind every entry's own frames: the decoder's NaN column
            outs, chunks, _ = drive(pool, z, SCALE, True, tokens=dec.tokens_to_latent, tail=-1)
        else:
            outs, chunks, _ = drive(pool, z, SCALE, True)
        torch.cuda.synchronize()
        early = 0
        for s in ORDER:
            plan = S.lookahead_plan(dec, chunks[s][:-1], chunks[s][-1])
            assert [o.shape[-1] for o in outs[s]] == [rows[-1][3] for rows in plan], s
            ld = S.LookaheadDecoder(dec)
            if tokens:
                lat = dec.tokens_to_latent(z[s].permute(0, 2, 1).contiguous())
                one = own_stream(ld, lat, chunks[s])
            else:
                one = own_stream(ld, z[s], chunks[s])
            assert sum(o.shape[-1] for o in outs[s]) == F_[s] * hop
            compare(f"pool decoder debug{' tokens' if tokens else ''} session {s}", outs[s], torch.cat(one, dim=2),
                    whole[s], prec)
            early += sum(o.shape[-1] for o in outs[s][:-1])
        assert early > 0


def test_one_push_mixes_a_flushing_a_fresh_and_a_steady_session(dev):
    """P is in steady state (20 hops in, the look-ahead is 11.5), Q flushes after one more hop, R is fresh: one push."""
    enc, _ = models("base", dev)
    hop = int(enc.hop_length)
    lens = {"P": 23 * hop, "Q": 16 * hop, "R": 2 * hop}
    x = {s: torch.from_numpy(synth.synth_clips(1, n, clip0=90 + ord(s))).unsqueeze(1).to(dev) for s, n in lens.items()}
    outs = {s: [] for s in lens}

    def claim(names, y, counts):
        assert y.shape[2] == max(counts)
        for i, s in enumerate(names):
            assert not y[i, :, counts[i]:].numel() or int(bits(y[i, :, counts[i]:]).abs().max()) == 0
            outs[s].append(y[i:i + 1, :, :counts[i]].clone())

    with precision("x6"), torch.no_grad():
        pool = S.LookaheadPool(enc, 3)
        p, q = pool.open(), pool.open()
        for i in range(3):
            lo, hi = 5 * i * hop, 5 * (i + 1) * hop
            claim("PQ", *pool.push([p, q], torch.cat([x["P"][..., lo:hi], x["Q"][..., lo:hi]])))
        claim("P", *pool.push([p], x["P"][..., 15 * hop:20 * hop]))  # Q sits this one out
        r = pool.open()
        batch = torch.full((3, 1, 3 * hop), float("nan"), device=dev)
        batch[0, :, :hop] = x["Q"][0, :, 15 * hop:]
        batch[1] = x["P"][0, :, 20 * hop:]
        batch[2, :, :2 * hop] = x["R"][0]
        y, counts = pool.push([q, p, r], batch, hops=[1, 3, 2], finish=[True, False, False])
        claim("QPR", y, counts)
        assert pool.live() == [p, r]
        assert all(row[0] == row[4] for row in pool.plan.rows[1]) and counts[1] == 3  # P: steady, 3 hops in, 3 frames out
        assert counts[0] > 3 and counts[2] == 0  # Q's flush hands out what was held back; R is inside its look-ahead
        y, counts = pool.finish([r, p])
        claim("RP", y, counts)
        torch.cuda.synchronize()
        for s in lens:
            got, want = torch.cat(outs[s], dim=2), enc(x[s])
            assert got.shape == want.shape and torch.equal(got, want), (s, max_rel_err(got, want))


# ---- 3. no torch compute kernel in a push ---------------------------------------------------------------------------
def test_no_torch_compute_kernel_in_a_pool_push(dev):
    """§23's dispatch-level recorder around a steady push and a finish: every operator is a bigcodec op, an allocation,
    a view, the staging of the int32 index arrays (host fill, one pinned copy) or the status read."""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Recorder(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.ops = set()

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = str(func)
            if name == "aten.cat.default" and all(t.dtype == torch.int32 and t.numel() == 1 for t in args[0]):
                name = "status.cat"  # _lib.check_status gathers the ResLSTM's int32 status words for ONE host copy
            if name == "aten.copy_.default" and args[0].dtype == torch.int32 and args[0].dim() == 1:
                name = "index.copy"  # the index arrays: host list -> pinned buffer -> device, int32 only
            self.ops.add(name)
            return func(*args, **(kwargs or {}))

    harmless = {"empty", "empty_like", "empty_strided", "new_empty", "slice", "select", "view", "_unsafe_view", "reshape",
                "as_strided", "alias", "detach", "unsqueeze", "squeeze", "expand", "_to_copy", "_local_scalar_dense",
                "lift_fresh", "_pin_memory", "is_pinned"}
    enc, dec = models("base", dev)
    hop = int(enc.hop_length)
    x = torch.from_numpy(synth.synth_clips(2, 20 * hop + 7, clip0=63)).unsqueeze(1).to(dev)
    z = torch.randn(2, 512, 22, generator=torch.Generator().manual_seed(6)).to(dev)
    with precision("x6"), torch.no_grad():
        for model, data, unit in ((enc, x, hop), (dec, z, 1)):
            pool = S.LookaheadPool(model, 2)
            sids = [pool.open(), pool.open()]
            for i in range(4):  # the transient, and the caches of packed weights and Snake coefficients
                pool.push(sids, data[..., 4 * i * unit:4 * (i + 1) * unit], hops=[4, 3])
            steady = data[..., 16 * unit:20 * unit].contiguous()
            last = data[..., 20 * unit:].contiguous()
            with Recorder() as rec:
                y, counts = pool.push(sids, steady, hops=[4, 2])
                tail, tcounts = pool.finish(sids, last)
            assert min(counts) > 0 and min(tcounts) > 0 and counts[0] > counts[1]
            other = sorted(o for o in rec.ops if not o.startswith(("bigcodec.", "status.", "index.")) and
                           o.split(".")[1] not in harmless)
            print(sorted(rec.ops))
            assert not other, other


# ---- 4. the bounds-checked debug build ------------------------------------------------------------------------------
CHILD = r"""
import json, sys, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
from audiotokenization_amd import _lib as L
from audiotokenization_amd import streaming as S
from audiotokenization_amd import synth
from helpers import build_models
from lookahead_pool_ref import CAPACITY, ORDER, run_schedule, totals
L.load()
assert L.lib_path().endswith("_debug/libbigcodec_hip.so"), L.lib_path()
dev = torch.device("cuda", 0)
enc, dec, *_ = build_models("base", device=dev)
hop = int(enc.hop_length)
T = totals(2 * hop)
x = {{s: torch.from_numpy(synth.synth_clips(1, T[s], clip0=40 + ord(s))).unsqueeze(1).to(dev) for s in ORDER}}
z = {{s: torch.randn(1, 512, totals(2)[s], generator=torch.Generator().manual_seed(ord(s))).to(dev) for s in ORDER}}
out = {{}}
with torch.no_grad():
    for name, model, data, unit in (("lat", enc, x, 2 * hop), ("wav", dec, z, 2)):
        pool = S.LookaheadPool(model, CAPACITY)
        push = lambda sids, b, hops, flags: pool.push(sids, b, hops=[2 * h for h in hops], finish=flags if any(flags) else None)
        outs, _, _ = run_schedule(data, unit, pool.open, push, pool.finish)
        out[name] = {{s: torch.cat(outs[s], dim=2).cpu() for s in ORDER}}
status = L.debug_status()
torch.save(out, {dump!r})
print("DEBUG_RESULT " + json.dumps(status))
"""


def test_pool_under_the_debug_build(dev, tmp_path):
    """The schedule on a `base` encoder and decoder pool (x6) in a child process on the bounds-checked library: 0 failed
    index checks (bc_stream_window_slots_la's pool, x and carry-into-the-zeros guards among them), and the product
    build's bits."""
    from audiotokenization_amd import build_lib

    dlib = os.path.join(build_lib.DEBUG_DIR, "libbigcodec_hip.so")
    assert os.path.exists(dlib), "debug library not built (python audiotokenization_amd/build_lib.py --debug)"
    dump = str(tmp_path / "la_pool_dbg.pt")
    code = CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), dump=dump)
    env = dict(os.environ, BIGCODEC_DEBUG="1", BIGCODEC_PRECISION="x6")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DEBUG_RESULT ")][-1]
    assert json.loads(line[len("DEBUG_RESULT "):]) == [0, 0], line
    enc, dec = models("base", dev)
    hop = int(enc.hop_length)
    T = totals(SCALE * hop)
    x = {s: torch.from_numpy(synth.synth_clips(1, T[s], clip0=40 + ord(s))).unsqueeze(1).to(dev) for s in ORDER}
    z = {s: torch.randn(1, 512, totals(SCALE)[s], generator=torch.Generator().manual_seed(ord(s))).to(dev) for s in ORDER}
    d = torch.load(dump, weights_only=True)
    with precision("x6"), torch.no_grad():
        for name, model, data, unit in (("lat", enc, x, SCALE * hop), ("wav", dec, z, SCALE)):
            pool = S.LookaheadPool(model, CAPACITY)
            push = lambda sids, b, hops, flags: pool.push(sids, b, hops=[SCALE * h for h in hops],  # noqa: E731
                                                          finish=flags if any(flags) else None)
            outs, _, _ = run_schedule(data, unit, pool.open, push, pool.finish)
            for s in ORDER:
                got = torch.cat(outs[s], dim=2)
                want = enc(x[s]) if model is enc else dec(z[s], vq=False)
                assert torch.equal(got, want), (name, s)
                assert torch.equal(d[name][s], got.cpu()), (name, s)
