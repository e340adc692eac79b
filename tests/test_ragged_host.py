"""Ragged batches (clips of different lengths in one zero-padded batch), the host side: the per-layer length
bookkeeping against the oracle's per-clip shapes, the argument refusals, the extraction's batch plan, the zero_tail_
op's schema, and the masking scheme itself pinned on the CPU oracle (no GPU needed)."""
import numpy as np
import pytest
import torch

from audiotokenization_amd import synth
from audiotokenization_amd.blocks import DecoderBlock, EncoderBlock, ResLSTM
from audiotokenization_amd.extract import plan_batches
from helpers import assert_close_rel, build_models, torch_sd
from oracle import bigcodec_oracle as O

CASES = [("default", {}), ("default", {"causal": True}), ("debug", {})]
IDS = ["default", "default-causal", "debug"]


def ragged_lengths(hop: int):
    """The issue's length mix: a full clip, one sample short of it, mid-hop lengths, a short and a tiny clip."""
    return [24 * hop, 24 * hop - 1, 17 * hop + 73, 9 * hop + 3, 3 * hop, 401]


def ragged_clips(lengths, clip0: int = 11):
    """(B, 1, Tmax) white noise; clip b is x[b, :, :lengths[b]]."""
    return torch.from_numpy(synth.synth_clips(len(lengths), max(lengths), clip0=clip0)).unsqueeze(1)


_MODELS = {}


def models(name, ov):
    key = (name, tuple(sorted(ov.items())))
    if key not in _MODELS:
        enc, dec, esd, dsd, ek, dk = build_models(name, **ov)
        _MODELS[key] = (enc, dec, torch_sd(esd), torch_sd(dsd), ek, dk)
    return _MODELS[key]


@pytest.mark.parametrize("name,ov", CASES, ids=IDS)
def test_lengths_equal_the_oracles_per_clip_shapes(name, ov):
    enc, dec, esd, dsd, ek, dk = models(name, ov)
    lengths = ragged_lengths(int(enc.hop_length))
    x = ragged_clips(lengths)
    frames = enc.frame_lengths(lengths)
    want = [O.encoder_forward(x[b:b + 1, :, :n], esd, ek).shape[-1] for b, n in enumerate(lengths)]
    assert frames == want
    if ov.get("causal"):  # 24 * hop - 1 samples: one frame less than 24 * hop (each causal conv's own floor)
        assert frames[0] == 24 and frames[1] == 23
    table = enc.frame_lengths(lengths, per_layer=True)
    assert table[0] == lengths and table[-1] == frames
    # one row per masked producer: the input, the first conv, 3 units + the strided conv per block, the ResLSTM, and
    # the last conv's (the latent's)
    n_blocks = sum(isinstance(m, EncoderBlock) for m in enc.block)
    assert len(table) == 2 + 4 * n_blocks + sum(isinstance(m, ResLSTM) for m in enc.block) + 1
    n_dblocks = sum(isinstance(m, DecoderBlock) for m in dec.model)
    assert len(dec.sample_lengths(frames, per_layer=True)) == 2 + sum(isinstance(m, ResLSTM) for m in dec.model) + \
        4 * n_dblocks + 1
    samples = dec.sample_lengths(frames)
    D = dk["in_channels"]
    g = torch.Generator().manual_seed(0)
    got = [O.decoder_forward(torch.randn(1, D, f, generator=g) * 0.1, dsd, dk).shape[-1] for f in frames]
    assert samples == got == [f * int(dec.hop_length) for f in frames]
    assert torch.equal(torch.tensor(enc.frame_lengths(torch.tensor(lengths))), torch.tensor(frames))


def test_refusals():
    enc, dec, *_ = models("default", {})
    x = torch.zeros(2, 1, 4800)
    with pytest.raises(ValueError):  # wrong count
        enc(x, lengths=[4800])
    with pytest.raises(ValueError):  # above T
        enc(x, lengths=[4800, 4801])
    with pytest.raises(ValueError):  # below what the B = 1 forward accepts (the last stride-5 conv has no output)
        enc(x, lengths=[4800, 100])
    with pytest.raises(ValueError):
        enc(x, lengths=torch.tensor([4800.0, 4000.0]))
    with pytest.raises(ValueError):
        enc.frame_lengths([0])
    z = torch.zeros(2, 1024, 24)
    with pytest.raises(ValueError):
        dec.decode(z, lengths=[24, 24, 24])
    with pytest.raises(ValueError):
        dec.decode(z, lengths=[24, 25])
    with pytest.raises(ValueError):
        dec(z, vq=False, lengths=[24, 0])
    with pytest.raises(ValueError):
        dec.sample_lengths([])
    aenc, adec, *_ = build_models("debug", antialias=True)
    with pytest.raises(NotImplementedError):
        aenc(torch.zeros(1, 1, 6400), lengths=[6400])
    with pytest.raises(NotImplementedError):
        adec.decode(torch.zeros(1, 512, 20), lengths=[20])
    benc, bdec, *_ = build_models("debug", use_rnn=True, rnn_bidirectional=True)
    with pytest.raises(NotImplementedError):
        benc(torch.zeros(1, 1, 6400), lengths=[6400])
    with pytest.raises(NotImplementedError):
        bdec.decode(torch.zeros(1, 512, 20), lengths=[20])


def test_plan_batches():
    rng = np.random.default_rng(3)
    for n, batch, window in [(0, 4, None), (1, 4, None), (37, 4, None), (100, 16, 32), (65, 8, 64), (10, 1, 3)]:
        lengths = rng.integers(1000, 480000, size=n).tolist()
        groups = plan_batches(lengths, batch, window)
        assert sorted(i for g in groups for i in g) == list(range(n))  # every item exactly once
        assert all(1 <= len(g) <= batch for g in groups)
        w = 8 * batch if window is None else window
        for lo in range(0, n, w):  # within a window: groups in order of length, and no item leaves its window
            mine = [g for g in groups if lo <= g[0] < lo + w]
            assert all(lo <= i < lo + w for g in mine for i in g)
            flat = [lengths[i] for g in mine for i in g]
            assert flat == sorted(flat)
        assert groups == plan_batches(lengths, batch, window)  # a pure function
    assert plan_batches([5, 3, 9, 1], 2) == [[3, 1], [0, 2]]
    with pytest.raises(ValueError):
        plan_batches([1, 2], 0)


def test_zero_tail_schema_and_fake():
    from audiotokenization_amd import ops

    ns = ops.load()
    assert "zero_tail_" in ops.OPS
    schema = str(ns.zero_tail_.default._schema)
    assert schema.startswith("bigcodec::zero_tail_(Tensor(a!) y, Tensor(b!)? y2, Tensor lens, int tail_max)"), schema
    y, y2 = torch.empty(2, 3, 9, device="meta"), torch.empty(2, 3, 9, device="meta")
    lens = torch.empty(2, device="meta", dtype=torch.int32)
    assert ns.zero_tail_(y, y2, lens, 4) is None and ns.zero_tail_(y, None, lens, 4) is None


def test_zero_tail_abi_argument_checks():
    from audiotokenization_amd import _lib as L

    lib = L.load()
    assert L.ABI_VERSION == 18 and "bc_zero_tail" in L.EXPORTED
    assert lib.bc_zero_tail(None, None, 1, 1, 1, 8, 4, None) == 1   # null y
    assert lib.bc_zero_tail(1, None, None, 1, 1, 8, 4, None) == 1   # null lens
    for B, C, T in [(0, 1, 8), (1, 0, 8), (1, 1, 0), (-1, 1, 8)]:
        assert lib.bc_zero_tail(1, None, 1, B, C, T, 4, None) == 1
    assert lib.bc_zero_tail(1, None, 1, 2, 3, 8, 0, None) == 0      # tail_max <= 0: nothing is launched or touched
    assert lib.bc_zero_tail(1, 1, 1, 2, 3, 8, -5, None) == 0


# ---- the scheme itself, on the CPU oracle ----------------------------------------------------------------------
def _mask(t, lens):
    for b, n in enumerate(lens):
        t[b, :, n:] = 0.0
    return t


def masked_encoder(enc, x, esd, ek, table):
    """O.encoder_forward stage by stage on the padded batch, zeroing every clip's tail after each masked producer
    (blocks.Ragged's list: the input, the first conv, every ResidualUnit and strided conv, the ResLSTM) with the
    lengths of enc.frame_lengths(per_layer=True)."""
    causal, dil = ek.get("causal", False), tuple(ek.get("dilations", (1, 3, 9)))
    rows = iter(table)
    x = _mask(x.clone(), next(rows))
    x = _mask(O.conv(x, esd, "block.0.", 7, 1, 3, 1, causal), next(rows))
    i = 0
    for stride in ek["up_ratios"]:
        i += 1
        p = f"block.{i}."
        for j, d in enumerate(dil):
            x = _mask(O.residual_unit(x, esd, f"{p}block.{j}.", d, causal, False), next(rows))
        n = len(dil)
        h = O.activation(x, esd, f"{p}block.{n}.", False)
        pad = 0 if causal else (stride // 2 + stride % 2 if stride != 1 else 0)
        x = _mask(O.conv(h, esd, f"{p}block.{n + 1}.", 2 * stride if stride != 1 else 1, stride, pad, 1, causal), next(rows))
    if ek.get("use_rnn", True):
        i += 1
        x = _mask(O.res_lstm(x, esd, f"block.{i}.", ek.get("rnn_num_layers", 2)), next(rows))
    x = O.activation(x, esd, f"block.{i + 1}.", False)
    out = O.conv(x, esd, f"block.{i + 2}.", 3, 1, 1, 1, causal)
    assert max(next(rows)) == out.shape[-1] and next(rows, None) is None  # the table's last row: the latent's frames
    return out


def masked_decoder(dec, z, dsd, dk, table):
    causal, dil = dk.get("causal", False), tuple(dk.get("dilations", (1, 3, 9)))
    rows = iter(table)
    x = _mask(z.clone(), next(rows))
    x = _mask(O.conv(x, dsd, "model.0.", 7, 1, 3, 1, causal), next(rows))
    i = 0
    if dk.get("use_rnn", True):
        i += 1
        x = _mask(O.res_lstm(x, dsd, f"model.{i}.", dk.get("rnn_num_layers", 2)), next(rows))
    for stride in dk["up_ratios"]:
        i += 1
        p = f"model.{i}."
        x = O.activation(x, dsd, f"{p}block.0.", False)
        x = _mask(O.conv_transpose(x, dsd, f"{p}block.1.", stride, causal), next(rows))
        for j, d in enumerate(dil):
            x = _mask(O.residual_unit(x, dsd, f"{p}block.{j + 2}.", d, causal, False), next(rows))
    x = O.activation(x, dsd, f"model.{i + 1}.", False)
    x = torch.tanh(O.conv(x, dsd, f"model.{i + 2}.", 7, 1, 3, 1, causal))
    out = _mask(x, next(rows))
    assert next(rows, None) is None
    return out


@pytest.mark.parametrize("name,ov", CASES, ids=IDS)
def test_masked_padded_batch_is_the_per_clip_computation(name, ov):
    """Zero tails after every masked producer make the zero-padded batch compute each clip's own forward.  Two fp32
    CPU evaluations of one clip at different padded lengths differ by the BLAS / oneDNN blocking only: the project's
    fp32 model tolerance (1e-4 of the latent's range; 1e-5 absolute on the waveform) bounds that, and a clip reading
    another value than zero across its end misses it by orders of magnitude (the unmasked batch is checked too)."""
    enc, dec, esd, dsd, ek, dk = models(name, ov)
    hop = int(enc.hop_length)
    lengths = ragged_lengths(hop)
    x = ragged_clips(lengths)
    with torch.no_grad():
        lat = masked_encoder(enc, x, esd, ek, enc.frame_lengths(lengths, per_layer=True))
        frames = enc.frame_lengths(lengths)
        alone = [O.encoder_forward(x[b:b + 1, :, :n], esd, ek) for b, n in enumerate(lengths)]
        for b, f in enumerate(frames):
            assert_close_rel(lat[b, :, :f], alone[b][0], 1e-4, f"{name} clip {b} latent")
        if not ov.get("causal"):  # the control: plain zero-padding is NOT the per-clip computation
            plain = O.encoder_forward(_mask(x.clone(), lengths), esd, ek)
            worst = max(float((plain[b, :, :f] - alone[b][0]).abs().max() / alone[b][0].abs().max())
                        for b, f in enumerate(frames) if f < max(frames))
            assert worst > 1e-3, worst
        post = [O.rvq_forward(a, dsd)[0] for a in alone]
        z = torch.randn(len(frames), post[0].shape[1], max(frames), generator=torch.Generator().manual_seed(1))
        for b, f in enumerate(frames):
            z[b, :, :f] = post[b][0]
        wav = masked_decoder(dec, z, dsd, dk, dec.sample_lengths(frames, per_layer=True))
        for b, f in enumerate(frames):
            want = O.decoder_forward(post[b], dsd, dk)[0]
            n = f * int(dec.hop_length)
            assert want.shape[-1] == n
            err = (wav[b, :, :n] - want).abs()
            assert float(err.max()) <= 1e-5 and float((err ** 2).mean()) <= 1e-12, (b, float(err.max()))
            assert not wav[b, :, n:].any()
