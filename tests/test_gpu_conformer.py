"""The Conformer-STFT models on the MI355X against the reference's recorded outputs (tests/golden/conformer_*.npz) and
the float64 restatement (tests/conformer_ref.py), in x6 (the default) and h3; the Lightning shim's call shapes; batch
independence at 10 s; the round trip under the bounds-checked debug build.

Bounds: the latent within 1e-4 of max|ref|; no index may differ (the fixtures' smallest top-2 gap
is 10 x helpers.GAP_TOL, so helpers.index_mismatches has no near-tie to forgive); everything else within
min(4 x |float32 restatement - float64 restatement|, 1e-4 max|ref64|), both restatements recomputed here on the same
inputs.  The decoder is fed the reference's post-VQ embedding, the input both restatements decode."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conformer_ref as R
from audiotokenization_amd import _lib as L
from audiotokenization_amd import config as cfgmod
from audiotokenization_amd import synth
from audiotokenization_amd.lightning_shim import CodecLightningModule
from helpers import index_mismatches, max_rel_err
from test_conformer_host import FIXTURES, fixture_clips, fixture_models, load_fixture

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

_cases = {}


def case(tag):
    """The fixture, our modules (on the CPU until a test moves them) and both restatements, computed once."""
    if tag not in _cases:
        z, meta = load_fixture(tag)
        enc, dec, esd, dsd = fixture_models(meta)
        ek, dk = meta["encoder_kwargs"], meta["decoder_kwargs"]
        x = fixture_clips(meta)
        post_ref = torch.from_numpy(z["post"])
        refs = {}
        with torch.no_grad():
            for dt in (torch.float32, torch.float64):
                et, dtr = {}, {}
                lat = R.encoder(R.cast(esd, dt), ek, x.to(dt), et)
                post = R.quantize(R.cast(dsd, dt), lat)[0]
                wav = R.decoder(R.cast(dsd, dt), dk, post_ref.to(dt), dtr)
                refs[dt] = dict(latent=lat, post=post, wav=wav, **{"enc_" + k: v for k, v in et.items()},
                                **{"dec_" + k: v for k, v in dtr.items()})
        _cases[tag] = dict(z=z, meta=meta, enc=enc, dec=dec, x=x, post_ref=post_ref, r32=refs[torch.float32],
                           r64=refs[torch.float64])
    return _cases[tag]


def within(c, name, got, what):
    r32, r64 = c["r32"][name].double(), c["r64"][name]
    own = float((r32 - r64).abs().max())
    scale = float(r64.abs().max())
    bound = min(4.0 * own, 1e-4 * scale)
    err = float((got.detach().cpu().double() - r64).abs().max())
    print(f"{what} {name}: err {err:.3e}, float32 restatement {own:.3e}, bound {bound:.3e}, max|ref| {scale:.3e}")
    return err <= bound, f"{what} {name}: {err:.3e} > {bound:.3e}"


def run(c, dev, trace=False):
    enc, dec = c["enc"].to(dev), c["dec"].to(dev)
    et, dt = ({}, {}) if trace else (None, None)
    with torch.no_grad():
        lat = enc(c["x"].to(dev), trace=et)
        post, codes, loss = dec(lat, vq=True)
        wav = dec.decode(c["post_ref"].to(dev), trace=dt)
    torch.cuda.synchronize()
    return lat, post, codes, wav, et, dt


def model_checks(c, dev, what, trace):
    z = c["z"]
    lat, post, codes, wav, et, dt = run(c, dev, trace)
    err = max_rel_err(lat.cpu(), z["latent"])
    print(f"{what}: latent rel err {err:.3e}")
    assert err <= 1e-4, f"{what}: latent {err:.3e}"
    assert codes.shape == z["codes"].shape
    assert index_mismatches(codes.cpu().numpy(), z["codes"], z["gap"]) == (0, 0.0)
    assert wav.shape == z["wav"].shape and not torch.isnan(wav).any()
    fails = []
    for name, got in (("post", post), ("wav", wav)):
        ok, msg = within(c, name, got, what)
        if not ok:
            fails.append(msg)
    if trace:
        for k in R.ENC_TRACE:
            ok, msg = within(c, "enc_" + k, et[k], what)
            if not ok:
                fails.append(msg)
        for k in R.DEC_TRACE:
            ok, msg = within(c, "dec_" + k, dt[k], what)
            if not ok:
                fails.append(msg)
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("tag", FIXTURES)
def test_model_matches_the_reference(dev, tag):
    assert L.precision_name() == "x6"
    model_checks(case(tag), dev, tag + " x6", trace=tag != "conformer_base")


@pytest.mark.parametrize("tag", FIXTURES)
def test_model_matches_the_reference_in_h3(dev, tag):
    old = L.precision_mode()
    L.set_precision("h3")
    try:
        model_checks(case(tag), dev, tag + " h3", trace=False)
    finally:
        L._mode = old


def synth_lm(name, dev):
    lm = CodecLightningModule(cfgmod.preset(name))
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(lm.state_dict()).items()}
    lm.load_state_dict(sd, strict=True)
    return lm.eval().to(dev)


def test_shim_call_shapes(dev):
    lm = synth_lm("conformer_debug", dev)
    x = torch.from_numpy(synth.synth_clips(2, 3200)).to(dev)
    with torch.no_grad():
        lat = lm.encode(x.unsqueeze(1))
        post, codes, loss, *_ = lm.quantize(lat)
        wav = lm.decode(post)
        rec = lm.inference(x)
        out = lm({"wav": x})
        emb = lm.decoder.vq2emb(codes.permute(1, 2, 0))
        a0, none = lm.decoder.inference_0(lat)
    assert lat.shape == (2, 64, 16) and post.shape == (2, 64, 16) and codes.shape == (1, 2, 16)
    assert codes.dtype == torch.int64 and wav.shape == (2, 1, 3200) and rec.shape == (2, 3200)
    assert torch.equal(rec, wav[:, 0]) and torch.equal(out["gen_wav"], wav) and none is None and torch.equal(a0, wav)
    assert emb.shape == (2, 16, 64) and lm.encoder.hop_length == lm.decoder.hop_length == 200
    assert lm.decoder.get_emb() is not None


def test_batch_of_two_equals_its_clips_alone_at_ten_seconds(dev):
    """`conformer`, 2 x 10 s (F = 800): every launch is per clip, so B = 2 equals the two B = 1 runs bit for bit."""
    lm = synth_lm("conformer", dev)
    x = torch.from_numpy(synth.synth_clips(2, 160000, clip0=3)).unsqueeze(1).to(dev)
    with torch.no_grad():
        lat = lm.encode(x)
        post, codes, *_ = lm.quantize(lat)
        wav = lm.decode(post)
        assert lat.shape == (2, 256, 800) and wav.shape == (2, 1, 160000)
        for b in range(2):
            lat1 = lm.encode(x[b:b + 1])
            post1, codes1, *_ = lm.quantize(lat1)
            assert torch.equal(lat1, lat[b:b + 1]) and torch.equal(codes1, codes[:, b:b + 1])
            assert torch.equal(post1, post[b:b + 1]) and torch.equal(lm.decode(post1), wav[b:b + 1])
    assert not torch.isnan(wav).any()


CHILD = r"""
import json, sys, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
from audiotokenization_amd import _lib as L
from audiotokenization_amd import synth
from test_gpu_conformer import synth_lm
L.load()
assert L.lib_path().endswith("_debug/libbigcodec_hip.so"), L.lib_path()
dev = torch.device("cuda", 0)
lm = synth_lm("conformer_debug", dev)
x = torch.from_numpy(synth.synth_clips(2, 6400, clip0=5)).to(dev)
with torch.no_grad():
    lat = lm.encode(x.unsqueeze(1))
    post, codes, *_ = lm.quantize(lat)
    wav = lm.decode(post)
st = L.debug_status()
torch.save({{"codes": codes.cpu(), "wav": wav.cpu()}}, {dump!r})
print("DEBUG_RESULT " + json.dumps(st))
"""


def test_round_trip_under_the_debug_build(dev, tmp_path):
    """conformer_debug under the bounds-checked library in a fresh process: 0 failed checks, the product's values."""
    from audiotokenization_amd import build_lib

    dlib = os.path.join(build_lib.DEBUG_DIR, "libbigcodec_hip.so")
    assert os.path.exists(dlib), "debug library not built (python audiotokenization_amd/build_lib.py --debug)"
    assert build_lib.lib_digest(dlib) == build_lib._digest(build_lib._paths(True)[2]), "debug library older than the sources"
    dump = str(tmp_path / "dbg.pt")
    code = CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"), dump=dump)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BIGCODEC_DEBUG="1"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("DEBUG_RESULT ")][-1]
    assert json.loads(line[len("DEBUG_RESULT "):]) == [0, 0], line
    lm = synth_lm("conformer_debug", dev)
    x = torch.from_numpy(synth.synth_clips(2, 6400, clip0=5)).to(dev)
    with torch.no_grad():
        post, codes, *_ = lm.quantize(lm.encode(x.unsqueeze(1)))
        wav = lm.decode(post)
    d = torch.load(dump, weights_only=True)
    assert torch.equal(d["codes"], codes.cpu()) and torch.equal(d["wav"], wav.cpu())
