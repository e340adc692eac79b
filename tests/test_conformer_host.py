"""The Conformer-STFT codec family without a GPU: the float32 restatement (tests/conformer_ref.py) reproduces the
reference's recorded outputs bit for bit, the modules have the reference's state_dict, the config / shim / synth wiring,
the refusals, and the library's new symbols."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import conformer_ref as R
from audiotokenization_amd import _lib as L
from audiotokenization_amd import config as cfgmod
from audiotokenization_amd import conformer as cf
from audiotokenization_amd import ops, synth
from audiotokenization_amd.lightning_shim import CodecLightningModule
from helpers import GAP_TOL, build_models, index_mismatches, synth_load, torch_sd

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("conformer_debug", "conformer_debug_causal", "conformer_base")
NEW_SYMBOLS = ("bc_stft_frames", "bc_rmsnorm_fwd", "bc_dwconv_glu_fwd", "bc_swiglu_fwd", "bc_attention_tiles",
               "bc_attention_fwd", "bc_istft_head")
NEW_OPS = ("stft_frames", "rmsnorm", "dwconv_glu", "swiglu", "attention", "istft_head")


def load_fixture(tag):
    z = np.load(os.path.join(GOLD, tag + ".npz"))
    return z, json.loads(str(z["meta"]))


def fixture_models(meta):
    """(encoder, decoder, enc_sd, dec_sd) of a fixture: our modules with the synthetic weights, on the CPU."""
    enc = cf.ConformerEncoderSTFT(**meta["encoder_kwargs"])
    dec = cf.ConformerDecoderISTFT(**meta["decoder_kwargs"])
    esd, dsd = torch_sd(synth_load(enc, "encoder.")), torch_sd(synth_load(dec, "decoder."))
    return enc.eval(), dec.eval(), esd, dsd


def fixture_clips(meta):
    return torch.from_numpy(synth.synth_clips(meta["n_clips"], meta["n_samples"], clip0=meta["clip0"])).unsqueeze(1)


@pytest.mark.parametrize("tag", FIXTURES)
def test_restatement_equals_the_reference_bit_for_bit(tag):
    """conformer_ref in float32 == every recorded array of the reference modules (torch.equal)."""
    z, meta = load_fixture(tag)
    torch.set_num_threads(8)  # (the generator's setting)
    _, _, esd, dsd = fixture_models(meta)
    ek, dk = meta["encoder_kwargs"], meta["decoder_kwargs"]
    x = fixture_clips(meta)
    et, dt = {}, {}
    with torch.no_grad():
        latent = R.encoder(esd, ek, x, et)
        post, codes, _ = R.quantize(dsd, latent)
        wav = R.decoder(dsd, dk, post, dt)
    for name, got in (("latent", latent), ("post", post), ("wav", wav)):
        assert torch.equal(got, torch.from_numpy(z[name])), name
    assert np.array_equal(codes.numpy(), z["codes"])
    assert float(z["gap"].min()) >= 10 * GAP_TOL  # the generator's gap condition: no near-tie allowance is left
    assert index_mismatches(codes.numpy(), z["codes"], z["gap"]) == (0, 0.0)
    if tag != "conformer_base":
        for k in R.ENC_TRACE:
            assert torch.equal(et[k], torch.from_numpy(z["enc_" + k])), "enc " + k
        for k in R.DEC_TRACE:
            assert torch.equal(dt[k], torch.from_numpy(z["dec_" + k])), "dec " + k


@pytest.mark.parametrize("tag", FIXTURES)
def test_state_dict_keys_and_shapes_are_the_references(tag):
    _, meta = load_fixture(tag)
    enc, dec, _, _ = fixture_models(meta)
    for side, m in (("encoder", enc), ("decoder", dec)):
        ours = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert sorted(ours) == sorted(meta["state_dict"][side]), side
    assert "freqs_cis" not in dict(enc.conformer_backbone.named_buffers())


def test_projection_keys_appear_only_when_the_widths_differ():
    enc = cf.ConformerEncoderSTFT(hop_length=8, n_fft=32, window_size=32, dim=64, n_layers=1, n_head=2, out_channels=48)
    dec = cf.ConformerDecoderISTFT(in_channels=48, hop_length=8, n_fft=32, window_size=32, dim=64, n_layers=1, n_head=2)
    for m, p in ((enc, "output_proj"), (dec, "input_proj")):
        keys = set(m.state_dict())
        assert {p + ".weight_g", p + ".weight_v", p + ".bias"} <= keys
    same = cf.ConformerEncoderSTFT(hop_length=8, n_fft=32, window_size=32, dim=64, n_layers=1, n_head=2, out_channels=64)
    assert not any(k.startswith("output_proj") for k in same.state_dict())
    assert {"stft.window", "input_proj.weight", "input_proj.bias", "input_norm.weight", "norm.weight"} <= set(same.state_dict())
    assert "head.istft.window" in dec.state_dict() and "head.out.bias" in dec.state_dict()
    causal = cf.ConformerEncoderSTFT(hop_length=8, n_fft=32, window_size=32, dim=64, n_layers=1, n_head=2,
                                     out_channels=64, causal=True)
    assert "conformer_backbone.layers.0.conv.depthwise_conv.conv.weight" in causal.state_dict()


@pytest.mark.parametrize("name", ["conformer", "conformer_debug"])
def test_strict_round_trip_through_the_lightning_shim(name):
    cfg = cfgmod.preset(name)
    a, b = CodecLightningModule(cfg), CodecLightningModule(cfg)
    assert isinstance(a.encoder, cf.ConformerEncoderSTFT) and isinstance(a.decoder, cf.ConformerDecoderISTFT)
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(a.state_dict()).items()}
    sd["discriminator.x"] = torch.zeros(1)  # training-only keys of a Lightning checkpoint are ignored
    res = b.load_state_dict({"state_dict": sd}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in b.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert a.encoder.hop_length == a.decoder.hop_length == 200


def test_a_conformer_config_dict_builds_and_presets_keep_their_values():
    base = cfgmod.preset("conformer").model
    assert base.codec_encoder.type == "conformer_stft" and base.codec_decoder.type == "conformer_istft"
    assert (base.codec_encoder.dim, base.codec_encoder.n_layers, base.codec_encoder.n_head) == (256, 6, 8)
    assert base.codec_encoder.rope_theta == 500 and base.codec_decoder.fsq_levels == [4, 4, 4, 4, 4, 8]
    dbg = cfgmod.preset("conformer_debug").model
    assert (dbg.codec_encoder.dim, dbg.codec_encoder.n_head, dbg.codec_encoder.n_layers) == (64, 2, 2)
    assert (dbg.codec_decoder.codebook_size, dbg.codec_decoder.codebook_dim) == (8192, 8)
    ek = cfgmod.encoder_kwargs(dict(base.codec_encoder))
    dk = cfgmod.decoder_kwargs(dict(base.codec_decoder))
    assert tuple(ek) == cfgmod.CONFORMER_ENCODER_KEYS and tuple(dk) == cfgmod.CONFORMER_DECODER_KEYS
    assert "type" not in ek and "vq_weight_init" in dk
    lm = CodecLightningModule({"model": {"codec_encoder": dict(base.codec_encoder), "codec_decoder": dict(base.codec_decoder)}})
    want = sum(int(np.prod(s)) for k, s in load_fixture("conformer_base")[1]["state_dict"]["encoder"] if k != "stft.window")
    assert sum(p.numel() for p in lm.encoder.parameters()) == want == 10097920  # (the reference's own count)
    with pytest.raises(ValueError):
        cfgmod.encoder_kwargs({"type": "vocos"})
    assert set(cfgmod.encoder_kwargs(cfgmod.preset("debug").model.codec_encoder)) == set(cfgmod.ENCODER_KEYS)


def test_rope_table_is_the_references():
    for tag in ("conformer_debug", "conformer_base"):
        z, meta = load_fixture(tag)
        enc, _, _, _ = fixture_models(meta)
        fc = enc.conformer_backbone.freqs_cis
        assert fc.dtype == torch.complex64 and fc.shape == (meta["encoder_kwargs"]["max_seq_len"], 16)
        rope = torch.from_numpy(z["rope"])
        assert torch.equal(torch.view_as_real(fc[: rope.shape[0]]), rope)


def test_refusals_happen_on_the_host():
    with pytest.raises(NotImplementedError):
        cf.ConformerEncoderSTFT(hop_length=8, n_fft=32, window_size=16, dim=64, n_layers=1, n_head=2, out_channels=64)
    with pytest.raises(NotImplementedError):
        cf.ConformerDecoderISTFT(in_channels=64, hop_length=8, n_fft=32, window_size=16, dim=64, n_layers=1, n_head=2)
    for dim, heads in ((64, 4), (256, 2), (64, 1 + 2)):
        with pytest.raises(NotImplementedError):
            cf.SelfAttention(dim, n_head=heads)
    enc = cf.ConformerEncoderSTFT(hop_length=8, n_fft=32, window_size=32, dim=64, n_layers=1, n_head=2, out_channels=64,
                                  max_seq_len=16)
    dec = cf.ConformerDecoderISTFT(in_channels=64, hop_length=8, n_fft=32, window_size=32, dim=64, n_layers=1, n_head=2,
                                   max_seq_len=16)
    x = torch.zeros(1, 1, 64)
    with pytest.raises(NotImplementedError):  # training mode (a fresh module)
        enc(x)
    with pytest.raises(NotImplementedError):
        dec(torch.zeros(1, 64, 4), vq=False)
    enc.eval(), dec.eval()
    with pytest.raises(NotImplementedError):  # ragged batches
        enc(x, lengths=[64])
    with pytest.raises(NotImplementedError):
        dec(torch.zeros(1, 64, 4), vq=False, lengths=[4])
    # host tensors never reach a kernel: the library error of every module here
    with pytest.raises(L.BigCodecLibraryError):
        enc(x)
    from audiotokenization_amd import streaming

    for cls, m in ((streaming.StreamingEncoder, enc), (streaming.StreamingDecoder, dec), (streaming.LookaheadEncoder, enc),
                   (streaming.LookaheadDecoder, dec)):
        with pytest.raises(NotImplementedError):
            cls(m)
    for cls in (streaming.StreamPool, streaming.LookaheadPool):
        with pytest.raises(NotImplementedError):
            cls(enc, 2)


def test_length_refusals_come_before_any_launch(monkeypatch):
    """A clip shorter than one hop and more frames than max_seq_len raise ValueError without touching the ops."""
    calls = []
    monkeypatch.setattr(cf, "_as_input", lambda x: x)
    monkeypatch.setattr(ops, "load", lambda: calls.append(1) or (_ for _ in ()).throw(AssertionError("launched")))
    enc = cf.ConformerEncoderSTFT(hop_length=8, n_fft=32, window_size=32, dim=64, n_layers=1, n_head=2, out_channels=64,
                                  max_seq_len=4).eval()
    dec = cf.ConformerDecoderISTFT(in_channels=64, hop_length=8, n_fft=32, window_size=32, dim=64, n_layers=1, n_head=2,
                                   max_seq_len=4).eval()
    with pytest.raises(ValueError, match="shorter than one hop"):
        enc(torch.zeros(1, 1, 7))
    with pytest.raises(ValueError, match="max_seq_len"):
        dec(torch.zeros(1, 64, 5), vq=False)
    with pytest.raises(ValueError, match="max_seq_len"):
        enc(torch.zeros(1, 1, 8 * 5))
    assert not calls


def test_evaluate_answers_no_ragged_support_for_the_family():
    from audiotokenization_amd import evaluate

    assert evaluate._ragged_ok(CodecLightningModule(cfgmod.preset("conformer_debug"))) is False
    assert evaluate._ragged_ok(CodecLightningModule(cfgmod.preset("debug"))) is True


def test_synth_state_dict_is_unchanged_on_the_bigcodec_debug_template():
    """sha256 over the sorted (key, float32 bytes) of synth_state_dict on the `debug` BigCodec encoder and decoder
    templates.  The parent commit's function (before the RMSNorm-gain and .window rules) gives
    4fa355b400276fdd6e3340077183b737e1e863f3ece7bdb0393361096cb30989; so does this one."""
    enc, dec, *_ = build_models("debug")
    h = hashlib.sha256()
    for m, p in ((enc, "encoder."), (dec, "decoder.")):
        out = synth.synth_state_dict({p + k: v for k, v in m.state_dict().items()})
        for k in sorted(out):
            h.update(k.encode())
            h.update(out[k].tobytes())
    assert h.hexdigest() == "4fa355b400276fdd6e3340077183b737e1e863f3ece7bdb0393361096cb30989"


def test_synth_rules_for_the_family():
    tmpl = {"a.norm.weight": (64,), "a.stft.window": torch.hann_window(32), "a.w1.weight": (8, 4)}
    out = synth.synth_state_dict(tmpl)
    g = out["a.norm.weight"]
    assert g.dtype == np.float32 and 0.75 <= g.min() and g.max() <= 1.25 and g.std() > 0.05
    assert np.array_equal(out["a.stft.window"], torch.hann_window(32).numpy())
    assert np.abs(out["a.w1.weight"]).max() <= 0.5


def test_library_and_ops_export_the_new_entry_points():
    lib = L.load()
    assert L.ABI_VERSION == 18 and lib.bc_abi_version() == 18  # additive: the ABI version stays
    for name in NEW_SYMBOLS:
        assert name in L.EXPORTED and hasattr(lib, name), name
    assert "conformer.hip" in __import__("audiotokenization_amd.build_lib", fromlist=["x"]).SOURCES
    ns = ops.load()
    for name in NEW_OPS:
        assert name in ops.OPS and hasattr(ns, name)
    m = lambda *s: torch.empty(*s, device="meta")  # noqa: E731
    assert ns.stft_frames(m(2, 1000), m(800, 802), 800, 200, 800).shape == (2, 802, 5)
    assert ns.rmsnorm(m(2, 64, 9), None, 1e-6, True).shape == (2, 64, 9)
    assert ns.dwconv_glu(m(2, 128, 9), m(64, 1, 31), m(64), 15).shape == (2, 64, 9)
    assert ns.swiglu(m(2, 512, 9)).shape == (2, 256, 9)
    assert ns.attention(m(2, 192, 9), m(16, 16, 2), 2, False).shape == (2, 64, 9)
    assert ns.istft_head(m(2, 802, 5), m(802, 800), m(800), 200).shape == (2, 1, 1000)
    q, k = (np.zeros(1, np.int32) for _ in range(2))
    assert lib.bc_attention_tiles(q.ctypes.data, k.ctypes.data) == 0 and q[0] >= 1 and k[0] >= 1


def test_host_bases_are_the_transforms():
    """The float64 bases the kernels multiply by are the DFT / inverse DFT they stand for."""
    w = torch.hann_window(32)
    x = torch.randn(32, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    got = torch.from_numpy(cf.stft_basis_t(w, 32)).t() @ x
    want = torch.fft.rfft(x * w.double())
    assert torch.allclose(got[:17], want.real, atol=1e-12) and torch.allclose(got[17:], want.imag, atol=1e-12)
    s = torch.randn(17, dtype=torch.complex128, generator=torch.Generator().manual_seed(1))
    got = torch.cat([s.real, s.imag]) @ torch.from_numpy(cf.istft_basis(w, 32))
    assert torch.allclose(got, torch.fft.irfft(s, 32) * w.double(), atol=1e-12)
