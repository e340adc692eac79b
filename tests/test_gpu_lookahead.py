"""Look-ahead streaming of NON-causal models (streaming.py LookaheadEncoder / LookaheadDecoder) on the
MI355X.  The whole-sequence forward defines the result: cat(pushes..., finish) must equal encoder(x) / decoder(z,
vq=False) on the whole input,
  x6 (exact operand splits, tile-independent): BIT FOR BIT;
  h3 (per-tile block scales): max |a - b| / max |b| <= 1e-5, the bound tests/test_gpu_streaming.py applies to its h3
    stream leg;
  fp32 (the `debug` encoder, whose ResidualUnits then take the two-launch path): bit for bit as well -- the native fp32
    conv kernels accumulate each output column over (input channel, tap) in an order that does not depend on where the
    column sits in the launch.  (The fp32 DECODER stream does not exist: bc_reslstm_fwd_state has no fp32 kernel, and
    every preset's decoder has a ResLSTM; that limit is the causal stream's too.)
and the frames / samples each push returns must be the plan's, so hoarding everything until finish() fails.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from audiotokenization_amd import _lib as L
from audiotokenization_amd import streaming as S
from audiotokenization_amd import synth
from helpers import build_models, max_rel_err

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
H3_BOUND = 1e-5  # tests/test_gpu_streaming.py, h3 stream vs whole pass

_models = {}


def models(name, dev, **ov):
    key = (name, tuple(sorted(ov.items())))
    if key not in _models:
        _models[key] = build_models(name, device=dev, **ov)[:2]
    return _models[key]


class precision:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.old = L.precision_mode()
        L.set_precision(self.name)

    def __exit__(self, *exc):
        L._mode = self.old


def agree(got, want, prec, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = max_rel_err(got, want)
    print(f"{what} [{prec}]: max rel diff to the whole pass {err:.2e}, equal {torch.equal(got, want)}")
    if prec == "h3":
        assert err <= H3_BOUND, (what, err)
    else:
        assert torch.equal(got, want), f"{what} [{prec}]: stream != whole pass ({err:.3e})"


# ---- 1. the window kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 65])
@pytest.mark.parametrize("Pin,n,R,Pout,first", [(3, 8, 0, 3, False), (3, 2, 0, 5, False), (0, 5, 0, 2, False),
                                                (6, 4, 3, 0, False), (6, 0, 3, 0, False), (18, 7, 0, 18, True),
                                                (54, 1000, 9, 54, False)])
@pytest.mark.parametrize("act", [False, True])
@pytest.mark.parametrize("strided", [False, True])
def test_stream_window_la_kernel(dev, C, Pin, n, R, Pout, first, act, strided):
    """bc_stream_window_la against a torch composition of the product's own Snake op and plain copies, exact: the
    carry that grows (Pout > Pin), the carry that reaches back into ctx (Pout > n), no carry in, the flush's right
    zeros with and without new input, a missing ctx, more than one block per row; and bc_stream_window's bits when
    Pin == Pout, R == 0."""
    from audiotokenization_amd import ops

    ns = ops.load()
    g = torch.Generator().manual_seed(Pin * 131 + n * 7 + C)
    B = 2
    base = torch.randn(B, C, n + 11, generator=g).to(dev)
    x = base[:, :, 11:] if strided else base[:, :, :n].contiguous()
    ctx = None if first or not Pin else torch.randn(B, C, Pin, generator=g).to(dev)
    a = torch.rand(C, generator=g).add(0.5).to(dev) if act else None
    ib = torch.rand(C, generator=g).add(0.5).to(dev) if act else None
    win, nctx = ns.stream_window_la(x, ctx, a, ib, Pin, R, Pout)
    xa = ns.snake(x.contiguous(), a, ib) if act and n else x
    held = torch.cat([ctx if ctx is not None else torch.zeros(B, C, Pin, device=dev), xa], dim=2)
    assert torch.equal(win, torch.cat([held, torch.zeros(B, C, R, device=dev)], dim=2))
    assert nctx.shape == (B, C, Pout) and torch.equal(nctx, held[:, :, held.shape[2] - Pout:])
    if Pin == Pout and R == 0:
        win0, nctx0 = ns.stream_window(x, ctx, a, ib, Pin)
        assert torch.equal(win, win0) and torch.equal(nctx, nctx0)


# ---- 2. the encoder -------------------------------------------------------------------------------------------------
def run_encoder(enc, x, chunks, prec, what):
    """Stream x through a fresh LookaheadEncoder: pushes of `chunks`, the rest at finish.  Checks the per-push frame
    counts against the plan and the concatenation against encoder(x)."""
    la = S.LookaheadEncoder(enc)
    T, pos, outs = x.shape[-1], 0, []
    plan = S.lookahead_plan(enc, chunks, T - sum(chunks))
    with torch.no_grad():
        want = enc(x)
        for n in chunks:
            outs.append(la.push(x[..., pos:pos + n]))
            pos += n
        outs.append(la.finish(x[..., pos:]))
        torch.cuda.synchronize()
    assert [o.shape[-1] for o in outs] == [rows[-1][3] for rows in plan], what
    assert la.samples == T
    agree(torch.cat(outs, dim=2), want, prec, what)
    return outs


@pytest.mark.parametrize("model,B,prec", [("debug", 1, "x6"), ("debug", 2, "x6"), ("base", 1, "x6"), ("base", 2, "x6"),
                                          ("debug", 1, "h3"), ("debug", 2, "h3"), ("base", 1, "h3"), ("base", 2, "h3"),
                                          ("debug", 1, "fp32"), ("debug", 2, "fp32")])
def test_lookahead_encoder_equals_whole_sequence(dev, model, B, prec):
    enc, _ = models(model, dev)
    hop = int(enc.hop_length)
    T = 7 * hop + 13
    x = torch.from_numpy(synth.synth_clips(B, T, clip0=51)).unsqueeze(1).to(dev)
    with precision(prec):
        run_encoder(enc, x, [hop, 3 * hop, 2 * hop], prec, f"encoder {model} B={B} chunked")
        run_encoder(enc, x, [], prec, f"encoder {model} B={B} finish alone")


@pytest.mark.parametrize("model,prec", [("base", "x6"), ("base", "h3"), ("debug", "fp32")])
def test_lookahead_encoder_emits_before_the_end(dev, model, prec):
    """7 hops + 13 samples are fewer than any preset's look-ahead + 6 hops, so the case above gets every frame at
    finish(); a longer stream must hand frames out while it runs (the plan's counts), its ResLSTM carrying (h, c) from
    push to push, and still equal the whole pass."""
    enc, _ = models(model, dev)
    hop = int(enc.hop_length)
    x = torch.from_numpy(synth.synth_clips(2, 24 * hop + 5, clip0=55)).unsqueeze(1).to(dev)
    with precision(prec):
        outs = run_encoder(enc, x, [4 * hop] * 5 + [hop, 3 * hop], prec, f"encoder {model} 24 hops")
        assert sum(o.shape[-1] > 0 for o in outs[:-1]) >= 2


# ---- 3. further cases -----------------------------------------------------------------------------------------------
def test_lookahead_encoder_further_cases(dev):
    enc, _ = models("default", dev)
    hop = int(enc.hop_length)
    with precision("x6"):
        # a total shorter than the look-ahead: every push returns no frame, finish() all of them
        T = 6 * hop + 13
        assert T < S.lookahead_samples(enc)
        x = torch.from_numpy(synth.synth_clips(1, T, clip0=61)).unsqueeze(1).to(dev)
        outs = run_encoder(enc, x, [hop, 3 * hop, 2 * hop], "x6", "shorter than the look-ahead")
        assert [o.shape[-1] for o in outs[:-1]] == [0, 0, 0] and outs[-1].shape[-1] == 6
        # enough for frames to come out before the end, and finish() with no argument after hop-multiple pushes
        T = 20 * hop
        x = torch.from_numpy(synth.synth_clips(2, T, clip0=62)).unsqueeze(1).to(dev)
        la = S.LookaheadEncoder(enc)
        with torch.no_grad():
            want = enc(x)
            outs = [la.push(x[..., i:i + 4 * hop]) for i in range(0, T, 4 * hop)]
            assert sum(o.shape[-1] for o in outs) > 0
            outs.append(la.finish())
            assert torch.equal(torch.cat(outs, dim=2), want)
            # encode(): chunks + finish in one call, from a fresh state
            assert torch.equal(la.encode(x[..., :T - 7], 5 * hop), enc(x[..., :T - 7]))
        # push after finish
        with pytest.raises(RuntimeError):
            la.push(x[..., :hop])
        with pytest.raises(RuntimeError):
            la.finish()
        la.reset()
        with torch.no_grad():
            la.push(x[..., :hop])
        with pytest.raises(ValueError):
            la.push(x[..., :hop + 1])
        with pytest.raises(ValueError):
            la.push(x[:1, :, :hop])  # the batch size is fixed per stream
        # a precision change mid-stream: the carried state belongs to the old mode
        L.set_precision("h3")
        with pytest.raises(RuntimeError):
            la.push(x[..., :hop])
        with pytest.raises(RuntimeError):
            la.finish()
        L.set_precision("x6")
        with torch.no_grad():
            la.push(x[..., hop:2 * hop])


def test_no_torch_compute_kernel_in_a_push(dev):
    """Every operator a steady-state push and a finish() dispatch is a bigcodec op, an allocation, a view or the read of
    the ResLSTM's int32 status words (every forward's check_status): no torch kernel touches the data (no cat of
    activations, no zeros, add or contiguous copy)."""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Recorder(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.ops = set()

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = str(func)
            if name == "aten.cat.default" and all(t.dtype == torch.int32 and t.numel() == 1 for t in args[0]):
                name = "status.cat"  # _lib.check_status gathers the ResLSTM's int32 status words for ONE host copy
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
        for stream, data, unit in ((S.LookaheadEncoder(enc), x, hop), (S.LookaheadDecoder(dec), z, 1)):
            for i in range(4):  # the transient, and the caches of packed weights and Snake coefficients
                stream.push(data[..., 4 * i * unit:4 * (i + 1) * unit])
            with Recorder() as rec:
                y = stream.push(data[..., 16 * unit:20 * unit])
                tail = stream.finish(data[..., 20 * unit:])
            assert y.shape[-1] > 0 and tail.shape[-1] > 0
            other = sorted(o for o in rec.ops if not o.startswith(("bigcodec.", "status.")) and
                           o.split(".")[1] not in harmless)
            print(sorted(rec.ops))
            assert not other, other


# ---- 4. the decoder -------------------------------------------------------------------------------------------------
def run_decoder(dec, z, chunks, prec, what):
    ld = S.LookaheadDecoder(dec)
    F_, pos, outs = z.shape[-1], 0, []
    plan = S.lookahead_plan(dec, chunks, F_ - sum(chunks))
    with torch.no_grad():
        want = dec(z, vq=False)
        for n in chunks:
            outs.append(ld.push(z[..., pos:pos + n]))
            pos += n
        outs.append(ld.finish(z[..., pos:]))
        torch.cuda.synchronize()
    assert [o.shape[-1] for o in outs] == [rows[-1][3] for rows in plan], what
    assert ld.samples == want.shape[-1] == F_ * int(dec.hop_length)
    agree(torch.cat(outs, dim=2), want, prec, what)
    return outs


@pytest.mark.parametrize("model,B,prec", [("debug", 1, "x6"), ("debug", 2, "x6"), ("base", 1, "x6"), ("base", 2, "x6"),
                                          ("debug", 2, "h3"), ("base", 1, "h3")])
def test_lookahead_decoder_equals_whole_sequence(dev, model, B, prec):
    enc, dec = models(model, dev)
    hop = int(dec.hop_length)
    x = torch.from_numpy(synth.synth_clips(B, 9 * hop, clip0=71)).unsqueeze(1).to(dev)
    with precision(prec):
        with torch.no_grad():
            post, codes, _ = dec(enc(x), vq=True)
        assert post.shape[-1] == 9
        run_decoder(dec, post, [1, 4, 2], prec, f"decoder {model} B={B} chunked")
        run_decoder(dec, post, [], prec, f"decoder {model} B={B} finish alone")
        # tokens(codes) is push(tokens_to_latent(codes)), whatever either returns
        tok = codes.permute(1, 2, 0).contiguous()  # (B, F, Nq)
        a, b = S.LookaheadDecoder(dec), S.LookaheadDecoder(dec)
        with torch.no_grad():
            for lo, hi in ((0, 5), (5, 9)):
                ya, yb = a.tokens(tok[:, lo:hi]), b.push(dec.tokens_to_latent(tok[:, lo:hi]))
                assert torch.equal(ya, yb)
            ya, yb = a.finish(), b.finish()
            assert ya.shape[-1] > 0 and torch.equal(ya, yb)


def test_lookahead_decoder_emits_before_the_end(dev):
    """Nine frames are fewer than the decoder's look-ahead, so the case above returns every sample at finish(); a longer
    stream must hand samples out while it runs, and still equal the whole pass bit for bit."""
    _, dec = models("base", dev)
    z = torch.randn(1, 512, 24, generator=torch.Generator().manual_seed(5)).to(dev)
    with precision("x6"):
        outs = run_decoder(dec, z, [6, 6, 6, 5], "x6", "decoder base 24 frames")
        assert sum(o.shape[-1] for o in outs[:-1]) > 0
        ld = S.LookaheadDecoder(dec)
        with torch.no_grad():
            assert torch.equal(ld.decode(z, 7), dec(z, vq=False))


# ---- 5. causal agreement --------------------------------------------------------------------------------------------
def test_causal_models_stream_as_the_causal_stream(dev):
    enc, dec = models("debug", dev, causal=True)
    hop = int(enc.hop_length)
    x = torch.from_numpy(synth.synth_clips(2, 6 * hop, clip0=81)).unsqueeze(1).to(dev)
    with precision("x6"), torch.no_grad():
        la, se = S.LookaheadEncoder(enc), S.StreamingEncoder(enc)
        assert la.lookahead == 0
        lat = []
        for lo, hi in ((0, hop), (hop, 4 * hop), (4 * hop, 6 * hop)):
            y, y0 = la.push(x[..., lo:hi]), se.push(x[..., lo:hi])
            assert y.shape[-1] == (hi - lo) // hop and torch.equal(y, y0)
            lat.append(y)
        assert la.finish().shape == (2, lat[0].shape[1], 0)
        post = dec(torch.cat(lat, dim=2), vq=True)[0]
        ld, sd = S.LookaheadDecoder(dec), S.StreamingDecoder(dec)
        assert ld.lookahead == 0
        for lo, hi in ((0, 1), (1, 4), (4, 6)):
            y, y0 = ld.push(post[..., lo:hi]), sd.push(post[..., lo:hi])
            assert y.shape[-1] == (hi - lo) * hop and torch.equal(y, y0)
        assert ld.finish().shape == (2, 1, 0)


# ---- 6. the bounds-checked debug build ------------------------------------------------------------------------------
CHILD = r"""
import json, sys, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
from audiotokenization_amd import _lib as L
from audiotokenization_amd import streaming as S
from audiotokenization_amd import synth
from helpers import build_models
L.load()
assert L.lib_path().endswith("_debug/libbigcodec_hip.so"), L.lib_path()
dev = torch.device("cuda", 0)
enc, dec, *_ = build_models("base", device=dev)
hop = int(enc.hop_length)
x = torch.from_numpy(synth.synth_clips(2, 7 * hop + 13, clip0=91)).unsqueeze(1).to(dev)
z = torch.randn(2, 512, 9, generator=torch.Generator().manual_seed(9)).to(dev)
with torch.no_grad():
    la = S.LookaheadEncoder(enc)
    lat = torch.cat([la.push(x[..., :hop]), la.push(x[..., hop:4 * hop]), la.finish(x[..., 4 * hop:])], dim=2)
    ld = S.LookaheadDecoder(dec)
    wav = torch.cat([ld.push(z[..., :1]), ld.push(z[..., 1:5]), ld.finish(z[..., 5:])], dim=2)
status = L.debug_status()
torch.save({{"lat": lat.cpu(), "wav": wav.cpu()}}, {dump!r})
print("DEBUG_RESULT " + json.dumps(status))
"""


def test_lookahead_under_the_debug_build(dev, tmp_path):
    """One encoder and one decoder stream (x6, `base`) in a child process on the bounds-checked library: 0 failed
    index checks (bc_stream_window_la's among them), and the product build's bits."""
    dump = str(tmp_path / "la_dbg.pt")
    code = CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), dump=dump)
    env = dict(os.environ, BIGCODEC_DEBUG="1", BIGCODEC_PRECISION="x6")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DEBUG_RESULT ")][-1]
    assert json.loads(line[len("DEBUG_RESULT "):]) == [0, 0], line
    enc, dec = models("base", dev)
    hop = int(enc.hop_length)
    x = torch.from_numpy(synth.synth_clips(2, 7 * hop + 13, clip0=91)).unsqueeze(1).to(dev)
    z = torch.randn(2, 512, 9, generator=torch.Generator().manual_seed(9)).to(dev)
    d = torch.load(dump, weights_only=True)
    with precision("x6"), torch.no_grad():
        la, ld = S.LookaheadEncoder(enc), S.LookaheadDecoder(dec)
        lat = torch.cat([la.push(x[..., :hop]), la.push(x[..., hop:4 * hop]), la.finish(x[..., 4 * hop:])], dim=2)
        wav = torch.cat([ld.push(z[..., :1]), ld.push(z[..., 1:5]), ld.finish(z[..., 5:])], dim=2)
        assert torch.equal(lat, enc(x)) and torch.equal(wav, dec(z, vq=False))
    assert torch.equal(d["lat"], lat.cpu()) and torch.equal(d["wav"], wav.cpu())
