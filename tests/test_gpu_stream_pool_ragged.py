"""A chunk length per session in one pool push (streaming.py StreamPool.push(..., hops=)) on the MI355X.

Window kernel: bc_stream_window_slots_lens against bc_stream_window run per entry on that entry's own context and its
own L_b columns, bit for bit; x holds NaN at and past every L_b, every pool row is pre-filled with its own NaN payload.
ResLSTM: bc_reslstm_fwd_state_lens against the existing state path run once per distinct length on the truncated
batch (x6: bit for bit; h3: y bit for bit against the dense call, the state within tests/lstm_ref.py's bound against
fp64, since the input projection of a truncated T may tile differently).
Pool: the schedule of tests/pool_ragged_ref.py (pushes of one to three sessions with different hops per entry, NaN in
the input tails) against each session's own B = 1 stream and the whole-sequence causal pass (bit for bit in x6,
<= 1e-5 in h3: the rule of test_gpu_streaming.py), exactly-zero output tails, pool.samples, a PoolGraph replay of the
same schedule, and the same schedule on the bounds-checked debug build in a child process.
"""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

from audiotokenization_amd import _lib as L
from audiotokenization_amd import blocks as BL
from audiotokenization_amd import ops
from audiotokenization_amd.streaming import StreamingDecoder, StreamingEncoder, StreamPool
from helpers import build_models, max_rel_err
from lstm_ref import SHAPES, bound, data, make_case, ref64, rel_h, scales, worst
from pool_ragged_ref import CAPACITY, HOPS, N_MAX, clip, run_schedule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_timed_out_wait(dev):
    yield
    assert L.load().bc_lstm_status(1) == 0


def nan_rows(rows, *shape, dev, axis=0):
    """A float32 tensor whose slice `r` along `axis` holds the quiet NaN with payload r + 1."""
    bits = (0x7FC00000 + 1 + torch.arange(rows, dtype=torch.int32)).view([-1 if i == axis else 1 for i in range(len(shape))])
    return bits.expand(*shape).contiguous().view(torch.float32).to(dev)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- the window kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("B,C,P,n_hops,unit", [(3, 5, 18, 4, 25), (4, 7, 54, 5, 4), (2, 48, 6, 1, 1), (1, 3, 1, 7, 1)])
def test_stream_window_slots_lens_kernel(dev, B, C, P, n_hops, unit, act, strided):
    ns = ops.load()
    n = n_hops * unit
    g = torch.Generator().manual_seed(1000 * B + 10 * P + n + int(act))
    rows = 2 * B + 3
    perm = torch.randperm(rows, generator=g).tolist()
    # entry i: 1 (mod 3) is a fresh session (src = -1), 2 (mod 3) is discarded (dst = -1), the others carry and store
    src = [-1 if i % 3 == 1 else perm[i] for i in range(B)]
    dst = [-1 if i % 3 == 2 else perm[B + i] for i in range(B)]
    lens = [(1, n_hops, (n_hops + 1) // 2, max(1, n_hops - 1))[i % 4] for i in range(B)]  # 1, all, and between
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731

    def fresh_pool():
        pool = nan_rows(rows, rows, C, P, dev=dev)
        gp = torch.Generator().manual_seed(7 + P)
        for r in src:
            if r >= 0:
                pool[r] = torch.randn(C, P, generator=gp).to(dev)
        return pool

    pool = fresh_pool()
    before = pool.clone()
    base = torch.randn(B, C, P + n, generator=g).to(dev)
    a = torch.rand(C, generator=g).add(0.5).to(dev) if act else None
    ib = torch.rand(C, generator=g).add(0.5).to(dev) if act else None
    dense = base[:, :, P:] if strided else base[:, :, P:].contiguous()

    # every length == n_hops: the existing kernel's window and pool, bit for bit
    pool_full = fresh_pool()
    win_full = ns.stream_window_slots_lens_(dense, pool_full, i32(src), i32(dst), i32([n_hops] * B), unit, a, ib, P)
    pool_old = fresh_pool()
    win_old = ns.stream_window_slots_(dense, pool_old, i32(src), i32(dst), a, ib, P)
    assert torch.equal(bits(win_full), bits(win_old)) and torch.equal(bits(pool_full), bits(pool_old))

    for i in range(B):  # NaN at and past every entry's own length: never read
        base[i, :, P + lens[i] * unit:] = float("nan")
    x = base[:, :, P:] if strided else base[:, :, P:].contiguous()
    assert x.is_contiguous() != strided or B * C == 1
    win = ns.stream_window_slots_lens_(x, pool, i32(src), i32(dst), i32(lens), unit, a, ib, P)
    assert win.shape == (B, C, P + n)
    assert not torch.isnan(win).any(), "a NaN of an input tail or of a foreign pool row reached a window"
    for i in range(B):
        Lb = lens[i] * unit
        ctx = before[src[i]].unsqueeze(0) if src[i] >= 0 else None
        w1, c1 = ns.stream_window(x[i:i + 1, :, :Lb], ctx, a, ib, P)
        assert torch.equal(bits(win[i:i + 1, :, :P + Lb]), bits(w1)), f"entry {i}: window"
        assert int(bits(win[i, :, P + Lb:]).abs().max()) == 0 if Lb < n else True, f"entry {i}: the tail is not +0.0"
        if dst[i] >= 0:
            assert torch.equal(bits(pool[dst[i]]), bits(c1[0])), f"entry {i}: next context"
            assert torch.equal(bits(pool[dst[i]]), bits(win[i, :, Lb:Lb + P])), f"entry {i}: context != window columns"
            assert not torch.isnan(pool[dst[i]]).any()
    keep = [r for r in range(rows) if r not in dst]
    assert torch.equal(bits(pool[keep]), bits(before[keep])), "a pool row no entry names in dst changed"


# ---- the persistent ResLSTM ----------------------------------------------------------------------------------------
T_LENS = 6


def _case(H):
    return make_case(H, 2, 70, T_LENS, H, SHAPES[H][2], state=True)


@functools.lru_cache(maxsize=None)
def _module(H):
    m = BL.ResLSTM(H, num_layers=2)
    m.lstm.load_state_dict(data(_case(H)).params)
    return m.to(torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def _states64(H):
    """fp64 (h_n, c_n) [layers][H][B] of the case after 1 ... T_LENS steps: torch.nn.LSTM one step at a time with the
    state fed forward (computed once per H, shared by every precision and launch size, never written)."""
    case = _case(H)
    d = data(case)
    m = nn.LSTM(H, H, 2, batch_first=True).double()
    m.load_state_dict({k: v.double() for k, v in d.params.items()})
    st = (d.h0.double().transpose(1, 2).contiguous(), d.c0.double().transpose(1, 2).contiguous())
    out = []
    with torch.no_grad(), torch.backends.mkldnn.flags(enabled=False):
        for t in range(T_LENS):
            _, st = m(d.x[:, :, t:t + 1].double().transpose(1, 2), st)
            out.append((st[0].transpose(1, 2).contiguous(), st[1].transpose(1, 2).contiguous()))
    return out


def _run(dev, H, prec, x, state, lens=None):
    m = _module(H)
    old = L.precision_mode()
    L.set_precision(prec)
    try:
        with L.status_scope():
            y, (hn, cn) = m.run(x, state=state, return_state=True, lens=lens)
            L.check_status()
    finally:
        L._mode = old
    return y, hn, cn


@pytest.mark.parametrize("n", [17, 33, 65])  # NTH 1 / NTH 2 past the half boundary / the second launch chunk
@pytest.mark.parametrize("prec", ["x6", "h3"])
@pytest.mark.parametrize("H", [256, 1536])
def test_reslstm_lens(dev, H, prec, n):
    case = _case(H)
    d = data(case)
    fails = []
    for T in (T_LENS, 2, 1):
        x = d.x[:n, :, :T].contiguous().to(dev)
        st = (d.h0[:, :, :n].contiguous().to(dev), d.c0[:, :, :n].contiguous().to(dev))
        lens = [b % T + 1 for b in range(n)]  # cycles over 1 ... T: 1 and T both occur
        lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        what = f"H {H} {prec} n {n} T {T}"
        y, hn, cn = _run(dev, H, prec, x, st, lens_d)
        yd, hd, cd = _run(dev, H, prec, x, st)
        if not torch.equal(bits(y), bits(yd)):
            fails.append(f"{what}: y differs from the dense call by {float((y - yd).abs().max()):.3e}")
        yf, hf, cf = _run(dev, H, prec, x, st, torch.full((n,), T, dtype=torch.int32, device=dev))
        if not (torch.equal(bits(yf), bits(yd)) and torch.equal(bits(hf), bits(hd)) and torch.equal(bits(cf), bits(cd))):
            fails.append(f"{what}: lens all == T differs from the existing op")
        # the existing state path on the batch truncated to each distinct length
        want_h, want_c = torch.empty_like(hn), torch.empty_like(cn)
        for Lc in sorted(set(lens)):
            sel = [b for b in range(n) if lens[b] == Lc]
            _, h1, c1 = (hd, hd, cd) if Lc == T else _run(dev, H, prec, x[:, :, :Lc].contiguous(), st)
            want_h[:, :, sel], want_c[:, :, sel] = h1[:, :, sel], c1[:, :, sel]
        eh, ec = float((hn - want_h).abs().max()), float((cn - want_c).abs().max())
        print(f"RAGGED-LSTM {what}: |h_n - truncated| {eh:.3e} |c_n - truncated| {ec:.3e}")
        if prec == "x6":
            if not (torch.equal(bits(hn), bits(want_h)) and torch.equal(bits(cn), bits(want_c))):
                fails.append(f"{what}: (h_n, c_n) differ from the truncated calls by {eh:.3e} / {ec:.3e}")
        else:  # h3: lstm_ref's bound on h_n (quantity 1) and c_n (quantity 2) against fp64, as test_state holds them
            s64 = _states64(H)
            lim = bound(case, prec)
            for q, got in ((1, hn.cpu()), (2, cn.cpu())):
                ref = torch.stack([s64[lens[b] - 1][q - 1][:, :, b] for b in range(n)], dim=2)
                e = rel_h(got, ref, scales(case)[q])
                print(f"RAGGED-LSTM {what} quantity {q}: rel_h {e:.3e} bound {lim:.3e}")
                if not torch.isfinite(got).all() or e > lim:
                    fails.append(f"{what} quantity {q}: rel_h {e:.3e} > {lim:.3e}; {worst(got, ref, ('layer', 'unit', 'clip'))}")
    assert ref64(case)[0].shape[2] == T_LENS
    assert not fails, "\n".join(fails)


def test_reslstm_lens_without_the_persistent_kernel_raises(dev):
    """Shapes the per-step kernels serve keep answering 3 (H = 768 in every mode), before any launch."""
    m = BL.ResLSTM(768, num_layers=1).to(dev)
    x = torch.zeros(3, 768, 4, device=dev)
    with pytest.raises(RuntimeError, match="code 3"), L.status_scope():
        m.run(x, lens=torch.tensor([1, 2, 4], dtype=torch.int32, device=dev))
    torch.cuda.synchronize()


# ---- the pool against single-session streams -----------------------------------------------------------------------
def compare(what, got, alone, whole, sprec):
    assert got.shape == alone.shape == whole.shape, (what, got.shape, alone.shape, whole.shape)
    e1, e2 = max_rel_err(got, alone), max_rel_err(got, whole)
    print(f"{what} [{sprec}]: ragged pool vs its own B=1 stream {e1:.2e}, vs the whole-sequence pass {e2:.2e}")
    if sprec == "x6":
        assert torch.equal(got, alone), f"{what}: pool != B=1 stream ({e1:.3e})"
        assert torch.equal(got, whole), f"{what}: pool != whole-sequence pass ({e2:.3e})"
    else:
        assert e1 <= 1e-5 and e2 <= 1e-5, (what, e1, e2)


def encode_case(dev, model):
    enc, *_ = build_models(model, device=dev, causal=True)
    hop = int(enc.hop_length)
    return enc, hop, {s: clip(s, hop, dev) for s in HOPS}


def decode_case(dev, model, tokens):
    """(decoder, hop, per-session inputs laid out (1, C, frames), whole-sequence outputs, B = 1 stream outputs)"""
    enc, dec, *_ = build_models(model, device=dev, causal=True)
    hop = int(enc.hop_length)
    z, whole, alone = {}, {}, {}
    for s in HOPS:
        post, codes, _ = dec(enc(clip(s, hop, dev)), vq=True)
        sd = StreamingDecoder(dec)
        if tokens:
            tok = codes.permute(1, 2, 0).contiguous()  # (1, F, Nq)
            z[s] = tok.permute(0, 2, 1).contiguous()
            whole[s] = dec(dec.tokens_to_latent(tok), vq=False)
            alone[s] = torch.cat([sd.tokens(tok[:, i:i + 2]) for i in range(0, tok.shape[1], 2)], dim=2)
        else:
            z[s] = post
            whole[s] = dec(post, vq=False)
            alone[s] = sd.decode(post, 2)
    return dec, hop, z, whole, alone


@pytest.mark.parametrize("sprec", ["x6", "h3"])
def test_ragged_pool_encode_equals_single_streams(dev, sprec):
    old = L.precision_mode()
    try:
        L.set_precision(sprec)
        with torch.no_grad():
            enc, hop, x = encode_case(dev, "base")
            pool = StreamPool(enc, CAPACITY)
            got = run_schedule(pool, x, hop, 1)
            torch.cuda.synchronize()
            for s in HOPS:
                compare(f"encode base session {s}", got[s], StreamingEncoder(enc).encode(x[s], 2 * hop), enc(x[s]), sprec)
    finally:
        L._mode = old


@pytest.mark.parametrize("tokens", [False, True])
@pytest.mark.parametrize("sprec", ["x6", "h3"])
def test_ragged_pool_decode_equals_single_streams(dev, sprec, tokens):
    old = L.precision_mode()
    try:
        L.set_precision(sprec)
        with torch.no_grad():
            dec, hop, z, whole, alone = decode_case(dev, "debug", tokens)
            pool = StreamPool(dec, CAPACITY)
            if tokens:  # an index of -1 behind an entry's own frames: the decoder's NaN column
                got = run_schedule(pool, z, 1, hop, lambda sids, t, h: pool.tokens(sids, t.permute(0, 2, 1).contiguous(), h),
                                   tail=-1)
            else:
                got = run_schedule(pool, z, 1, hop)
            torch.cuda.synchronize()
        for s in HOPS:
            assert got[s].shape == (1, 1, HOPS[s] * hop)
            compare(f"decode debug{' tokens' if tokens else ''} session {s}", got[s], alone[s], whole[s], sprec)
    finally:
        L._mode = old


@pytest.mark.parametrize("sprec", ["x6", "h3"])
def test_ragged_pool_graph_equals_eager_ragged_pool(dev, sprec):
    """PoolGraph(B = 3, n = 3 hops): replays of the schedule with hops equal the eager ragged pool on the same padded
    shape bit for bit, encode and decode; a replay without hops in between still serves the same sessions."""
    old = L.precision_mode()
    try:
        L.set_precision(sprec)
        with torch.no_grad():
            enc, hop, x = encode_case(dev, "base")
            dec, dec_hop, z, _, _ = decode_case(dev, "debug", False)
            for model, data_, unit, out_unit in ((enc, x, hop, 1), (dec, z, 1, dec_hop)):
                pe, pg = StreamPool(model, CAPACITY), StreamPool(model, CAPACITY)
                g = pg.graph(CAPACITY, N_MAX * unit)
                want = run_schedule(pe, data_, unit, out_unit, pad_to=N_MAX)
                got = run_schedule(pg, data_, unit, out_unit, lambda sids, t, h: g.push(sids, t, hops=h), pad_to=N_MAX)
                for s in HOPS:
                    assert torch.equal(bits(got[s]), bits(want[s])), (s, max_rel_err(got[s], want[s]))
                # with and without hops on one graph: a full chunk either way is the same push
                a, b = pg.open(), pe.open()
                chunk = data_["A"][:, :, :N_MAX * unit]
                assert torch.equal(g.push([a], chunk).clone(), pe.push([b], chunk, hops=[N_MAX]))
                assert torch.equal(g.push([a], chunk, hops=[N_MAX]).clone(), pe.push([b], chunk))
                assert pg.samples(a) == pe.samples(b) == 2 * N_MAX * pe.hop
                torch.cuda.synchronize()
                g.check()
    finally:
        L._mode = old


def test_ragged_pool_refusals_leave_the_sessions_alone(dev):
    enc, *_ = build_models("debug", device=dev, causal=True)
    pool = StreamPool(enc, 2)
    a, b = pool.open(), pool.open()
    x = torch.zeros(2, 1, 2 * pool.hop, device=dev)
    for hops in ([1], [1, 2, 1], [0, 1], [1, 3], [1, 2.0], [True, 1], [1, None]):
        with pytest.raises(ValueError):
            pool.push([a, b], x, hops=hops)
    assert pool.table.pushes[:2] == [0, 0] and not pool.table.undefined
    with torch.no_grad():
        y = pool.push([b, a], x, hops=[2, 1])
    assert y.shape == (2, y.shape[1], 2) and pool.samples(b) == 2 * pool.hop and pool.samples(a) == pool.hop
    assert int(bits(y[1, :, 1:]).abs().max()) == 0


# ---- the bounds-checked debug build --------------------------------------------------------------------------------
CHILD = r"""
import json, sys, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
from audiotokenization_amd import _lib as L
from audiotokenization_amd.streaming import StreamPool
from helpers import build_models
from pool_ragged_ref import CAPACITY, HOPS, clip, run_schedule
lib = L.load()
assert L.lib_path().endswith("_debug/libbigcodec_hip.so"), L.lib_path()
dev = torch.device("cuda", 0)
enc, dec, *_ = build_models("base", device=dev, causal=True)
hop = int(enc.hop_length)
out = {{}}
for prec in ("x6", "h3"):
    L.set_precision(prec)
    with torch.no_grad():
        x = {{s: clip(s, hop, dev) for s in HOPS}}
        lat = run_schedule(StreamPool(enc, CAPACITY), x, hop, 1)
        z = {{s: dec(lat[s], vq=True)[0] for s in HOPS}}
        wav = run_schedule(StreamPool(dec, CAPACITY), z, 1, hop)
        torch.cuda.synchronize()
    out[prec] = L.debug_status()
    torch.save({{"lat": {{s: v.cpu() for s, v in lat.items()}}, "wav": {{s: v.cpu() for s, v in wav.items()}}}},
               {dump!r} + prec + ".pt")
print("DEBUG_RESULT " + json.dumps(out))
"""


def test_ragged_pool_in_the_bounds_checked_build(dev, tmp_path):
    """The `base` ragged schedule, encode then decode, in x6 and h3 on the debug library (a child process with
    BIGCODEC_DEBUG=1): no computed index fails its check, and the outputs equal the product build's."""
    from audiotokenization_amd import build_lib

    dlib = os.path.join(build_lib.DEBUG_DIR, "libbigcodec_hip.so")
    assert os.path.exists(dlib), "debug library not built (python audiotokenization_amd/build_lib.py --debug)"
    assert build_lib.lib_digest(dlib) == build_lib._digest(build_lib._paths(True)[2]), "debug library older than the sources"
    dump = str(tmp_path / "ragged_")
    code = CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), dump=dump)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BIGCODEC_DEBUG="1"), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DEBUG_RESULT ")][-1]
    res = json.loads(line[len("DEBUG_RESULT "):])
    print(res)
    assert res["x6"] == [0, 0] and res["h3"] == [0, 0], res
    enc, dec, *_ = build_models("base", device=dev, causal=True)
    hop = int(enc.hop_length)
    old = L.precision_mode()
    try:
        for prec in ("x6", "h3"):
            L.set_precision(prec)
            with torch.no_grad():
                x = {s: clip(s, hop, dev) for s in HOPS}
                lat = run_schedule(StreamPool(enc, CAPACITY), x, hop, 1)
                z = {s: dec(lat[s], vq=True)[0] for s in HOPS}
                wav = run_schedule(StreamPool(dec, CAPACITY), z, 1, hop)
            d = torch.load(dump + prec + ".pt", weights_only=True)
            for s in HOPS:
                assert torch.equal(d["lat"][s], lat[s].cpu()), (prec, s)
                assert torch.equal(d["wav"][s], wav[s].cpu()), (prec, s)
    finally:
        L._mode = old
