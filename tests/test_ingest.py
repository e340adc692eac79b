"""Real-audio ingest (audiotokenization_amd/ingest.py, csrc/resample.hip).

Oracle: oracle/resample_oracle.py, a torch-CPU restatement of torchaudio's Resample and soundfile's read.
Parity is UNPINNED against the reference itself (torchaudio / soundfile are absent from this image); the
oracle is checked here against independent float64 / `wave`-module evaluations instead.

Tolerances: WAV decoding bit-exact; sinc filters equal to the float32 cast of the float64 design within
1 ulp; resampled samples max|d| / max|ref| <= 2e-6 (fp32 sums of 16-171 taps in a different order than
oneDNN's conv); encoder latents 1e-4 and VQ indices equal except certified near-ties (test_gpu_model.py).
"""
import math
import os
import struct
import wave

import numpy as np
import pytest
import torch

from audiotokenization_amd import ingest
from oracle import resample_oracle as RO

RATES = [(16000, 24000), (44100, 24000), (24000, 16000), (22050, 24000), (8000, 24000), (48000, 24000)]


def _write_riff(path, tag, channels, rate, bits, payload: bytes):
    align = channels * bits // 8
    fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(payload)) + payload
    if len(payload) & 1:
        body += b"\0"
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def _pcm16_file(path, x16: np.ndarray, rate=16000, channels=1):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(x16.astype("<i2").tobytes())


def test_read_wav_formats(tmp_path):
    rng = np.random.default_rng(0)
    v16 = rng.integers(-32768, 32768, size=(500, 2)).astype(np.int16)
    _pcm16_file(tmp_path / "a.wav", v16.reshape(-1), channels=2)
    x, sr = ingest.read_wav(str(tmp_path / "a.wav"))
    assert sr == 16000 and x.shape == (2, 500) and x.dtype == np.float32
    assert np.array_equal(x, v16.T.astype(np.float32) / 32768.0)
    v8 = rng.integers(0, 256, size=300).astype(np.uint8)
    _write_riff(tmp_path / "b.wav", 1, 1, 8000, 8, v8.tobytes())
    x, sr = ingest.read_wav(str(tmp_path / "b.wav"))
    assert sr == 8000 and np.array_equal(x[0], (v8.astype(np.float32) - 128) / 128)
    v24 = rng.integers(-(1 << 23), 1 << 23, size=301)
    b24 = b"".join(int(v & 0xFFFFFF).to_bytes(3, "little") for v in v24)
    _write_riff(tmp_path / "c.wav", 1, 1, 24000, 24, b24)
    x, _ = ingest.read_wav(str(tmp_path / "c.wav"))
    assert np.array_equal(x[0], v24.astype(np.float32) / 8388608.0)
    v32 = rng.integers(-(1 << 31), 1 << 31, size=64).astype(np.int32)
    _write_riff(tmp_path / "d.wav", 1, 1, 24000, 32, v32.astype("<i4").tobytes())
    x, _ = ingest.read_wav(str(tmp_path / "d.wav"))
    assert np.array_equal(x[0], v32.astype(np.float32) * np.float32(2.0 ** -31))
    f32 = rng.standard_normal(77).astype(np.float32)
    _write_riff(tmp_path / "e.wav", 3, 1, 44100, 32, f32.astype("<f4").tobytes())
    x, sr = ingest.read_wav(str(tmp_path / "e.wav"))
    assert sr == 44100 and np.array_equal(x[0], f32)
    (tmp_path / "f.flac").write_bytes(b"fLaC\0\0\0\0")
    with pytest.raises(ValueError):  # FLAC goes to the FLAC decoder (tests/test_flac.py), which rejects this stub
        ingest.read_wav(str(tmp_path / "f.flac"))


def test_read_pcm16_wavs_like_wave_module(tmp_path):
    """Files of the format of the recordings the reference ships (VoxCeleb excerpts: mono 16 kHz PCM16 behind the
    canonical 44-byte RIFF header, 4 to 17 s; voice recordings are not stored in this repository) decode like `wave`
    / 32768: seeded, amplitude-modulated tones in noise that reach both ends of the int16 range."""
    rng = np.random.default_rng(3)
    for i, n in enumerate((70401, 78721, 270721)):  # the samples of the shortest, another and the longest excerpt
        t = np.arange(n) / 16000.0
        tone = np.sin(2 * np.pi * (120 + 40 * np.sin(2 * np.pi * 3 * t)) * t)
        sig = 0.5 * tone * (0.6 + 0.4 * np.sin(2 * np.pi * 2 * t))
        x16 = np.clip(np.round((sig + 0.1 * rng.standard_normal(n)) * 32767), -32768, 32767).astype(np.int16)
        x16[:2] = (-32768, 32767)
        p = str(tmp_path / f"utt{i}.wav")
        _pcm16_file(p, x16)
        assert os.path.getsize(p) == 44 + 2 * n
        x, sr = ingest.read_wav(p)
        assert sr == 16000 and x.shape == (1, n)
        assert torch.equal(torch.from_numpy(x), RO.read_wav_pcm16(p))
        assert np.array_equal(x[0], x16.astype(np.float32) / 32768.0)


def _riff(*chunks, size=None):
    """A RIFF/WAVE file of (id, body[, claimed size]) chunks, each padded to an even length as RIFF asks."""
    body = b"WAVE"
    for cid, payload, *claimed in chunks:
        body += cid + struct.pack("<I", claimed[0] if claimed else len(payload)) + payload + b"\0" * (len(payload) & 1)
    return b"RIFF" + struct.pack("<I", len(body) if size is None else size) + body


def _fmt(tag=1, channels=1, rate=16000, bits=16, align=None, extra=b""):
    align = channels * ((bits + 7) // 8) if align is None else align
    return struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits) + extra


_PCM = np.arange(-6, 6, dtype="<i2").tobytes()  # 12 samples
MALFORMED_WAVS = {
    "bits = 0": _riff((b"fmt ", _fmt(bits=0, align=0)), (b"data", _PCM)),
    "bits = 0, align = 2": _riff((b"fmt ", _fmt(bits=0, align=2)), (b"data", _PCM)),
    "align = 0": _riff((b"fmt ", _fmt(align=0)), (b"data", _PCM)),
    "align is not channels * bytes": _riff((b"fmt ", _fmt(channels=2, align=3)), (b"data", _PCM)),
    "align of one channel for two": _riff((b"fmt ", _fmt(channels=2, align=2)), (b"data", _PCM)),
    "channels = 0": _riff((b"fmt ", _fmt(channels=0, align=2)), (b"data", _PCM)),
    "channels = 0, align = 0": _riff((b"fmt ", _fmt(channels=0, align=0)), (b"data", _PCM)),
    "fmt chunk of 14 bytes": _riff((b"fmt ", _fmt()[:14]), (b"data", _PCM)),
    "fmt chunk of 0 bytes": _riff((b"fmt ", b""), (b"data", _PCM)),
    "fmt chunk cut off by the end of the file": _riff((b"data", _PCM), (b"fmt ", _fmt()[:10], 16)),
    "no data chunk": _riff((b"fmt ", _fmt()), (b"LIST", b"INFOxx")),
    "no fmt chunk": _riff((b"data", _PCM)),
    "no chunk at all": _riff(),
    "extensible header of 24 bytes": _riff((b"fmt ", _fmt(tag=0xFFFE, extra=bytes(8))), (b"data", _PCM)),
    "extensible header of 16 bytes": _riff((b"fmt ", _fmt(tag=0xFFFE)), (b"data", _PCM)),
    "17-bit PCM": _riff((b"fmt ", _fmt(bits=17, align=3)), (b"data", _PCM)),
    "unknown format tag": _riff((b"fmt ", _fmt(tag=2)), (b"data", _PCM)),
    "not WAVE": b"RIFF" + struct.pack("<I", 4) + b"AVI ",
    "11 bytes": b"RIFF\0\0\0\0WAV",
    "empty file": b"",
}


@pytest.mark.parametrize("what", list(MALFORMED_WAVS))
def test_read_wav_rejects_malformed_headers(tmp_path, what):
    """Every malformed header is a ValueError (or NotImplementedError for a format that is well formed but not
    read), never a ZeroDivisionError, a struct.error or a numpy reshape error."""
    p = tmp_path / "bad.wav"
    p.write_bytes(MALFORMED_WAVS[what])
    with pytest.raises((ValueError, NotImplementedError)) as e:
        ingest.read_wav(str(p))
    assert type(e.value) in (ValueError, NotImplementedError), type(e.value)  # no subclass from numpy or struct
    assert "bad.wav" in str(e.value)


def test_read_wav_chunk_layouts(tmp_path):
    """Layouts that are read: a data chunk whose size runs past the end of the file (the samples present are read,
    a partial last sample frame is dropped), an odd-sized chunk before `data` (its pad byte is skipped), `fmt ` after
    `data`, a zero-length data chunk, and a 40-byte WAVE_FORMAT_EXTENSIBLE header."""
    want = np.arange(-6, 6, dtype=np.float32)[None] / 32768.0
    cases = {
        "data past the end": (_riff((b"fmt ", _fmt()), (b"data", _PCM, 1 << 20)), want),
        "data past the end, odd": (_riff((b"fmt ", _fmt()), (b"data", _PCM + b"\x7f", 4000))[:-1], want),  # (without the pad)
        "stereo data past the end": (_riff((b"fmt ", _fmt(channels=2)), (b"data", _PCM[:22], 400)),
                                     want[0, :10].reshape(5, 2).T),
        "odd chunk first": (_riff((b"fmt ", _fmt()), (b"LIST", b"INFOabc"), (b"data", _PCM)), want),
        "odd chunks around fmt": (_riff((b"JUNK", b"x"), (b"fmt ", _fmt()), (b"fact", b"12345"), (b"data", _PCM)), want),
        "fmt after data": (_riff((b"data", _PCM), (b"fmt ", _fmt())), want),
        "empty data": (_riff((b"fmt ", _fmt()), (b"data", b"")), np.zeros((1, 0), np.float32)),
        "empty stereo data": (_riff((b"fmt ", _fmt(channels=2)), (b"data", b"")), np.zeros((2, 0), np.float32)),
        "extensible PCM16": (_riff((b"fmt ", _fmt(tag=0xFFFE, extra=struct.pack("<HHIH", 22, 16, 4, 1) + bytes(14))),
                                   (b"data", _PCM)), want),
        "RIFF size wrong": (_riff((b"fmt ", _fmt()), (b"data", _PCM), size=4), want),
    }
    for what, (data, ref) in cases.items():
        p = tmp_path / "ok.wav"
        p.write_bytes(data)
        x, sr = ingest.read_wav(str(p))
        assert sr == 16000 and x.dtype == np.float32 and x.shape == ref.shape, (what, x.shape)
        assert np.array_equal(x, ref), what


def _flac_header_only(total):
    si = struct.pack(">HH", 4096, 4096) + bytes(6) + ((16000 << 44) | (0 << 41) | (15 << 36) | total).to_bytes(8, "big")
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + si + bytes(16)


def test_read_flac_does_not_allocate_for_an_announced_total(monkeypatch):
    """A 42-byte stream whose STREAMINFO announces 2^36 - 1 samples (256 GiB of float32) is rejected before any
    buffer is made: read_flac bounds the announced total by what the bytes can hold (ingest.flac_max_samples)."""
    data = _flac_header_only((1 << 36) - 1)
    assert len(data) == 42
    lib = ingest.L.load()
    buf = np.frombuffer(data, np.uint8)
    total = ingest.ctypes_longlong()
    assert lib.bc_flac_info(buf.ctypes.data, len(data), None, None, None, ingest.ctypes_ref(total)) == 0
    assert total.value == (1 << 36) - 1  # the header itself is well formed: the decoder would be asked to fill it
    assert ingest.flac_max_samples(42) == 5 * 65536 and ingest.flac_max_samples(7) == 0

    sizes = []
    real_empty = np.empty

    def empty(shape, *a, **k):
        sizes.append(int(np.prod(shape)))
        assert sizes[-1] <= 8 * 65536, f"read_flac asks for {sizes[-1]} samples for a 42-byte stream"
        return real_empty(shape, *a, **k)

    monkeypatch.setattr(ingest.np, "empty", empty)
    for as_int in (False, True):
        with pytest.raises(ValueError, match="more than 42 bytes can hold"):
            ingest.read_flac("huge", data, as_int=as_int)
    assert sizes == []
    # one more sample than the bytes can hold is refused, the bound itself goes to the decoder (which finds no frame)
    with pytest.raises(ValueError, match="can hold"):
        ingest.read_flac("over", _flac_header_only(5 * 65536 + 1))
    with pytest.raises(ValueError, match="corrupt"):
        ingest.read_flac("at", _flac_header_only(5 * 65536))
    assert sizes == [5 * 65536]


def test_read_flac_unknown_total_grows_its_buffer(monkeypatch):
    """Total unknown and more samples than max(4096, len(data)): CONSTANT subframes of 4096 samples take 12 bytes a
    frame, so the first buffer is too small and the growth loop (x 4, bounded by flac_max_samples) runs."""
    import flac_writer

    T = 40 * 4096 + 17
    x = np.repeat(np.arange(-20, 21, dtype=np.int64) * 700, 4096)[None, :T]
    data = flac_writer.encode(x, 16000, 16, block_sizes=[4096], plan=lambda fi, c: dict(kind="constant"),
                              total_known=False, extra_meta=False)
    first = max(4096, len(data))
    assert 16 * first < T <= 64 * first, (len(data), T)  # three growth steps
    caps = []
    real_empty = np.empty
    monkeypatch.setattr(ingest.np, "empty", lambda shape, *a, **k: (caps.append(shape[1]), real_empty(shape, *a, **k))[1])
    y, sr = ingest.read_flac("mem", data, as_int=True)
    assert caps == [first, 4 * first, 16 * first, 64 * first]
    assert sr == 16000 and y.shape == (1, T)
    np.testing.assert_array_equal(y.astype(np.int64), x)
    f, _ = ingest.read_flac("mem", data)
    np.testing.assert_array_equal(f, (x / 32768.0).astype(np.float32))


@pytest.mark.parametrize("orig,new", RATES)
def test_sinc_filters_match_oracle_design(orig, new):
    k, width, o, nw = ingest.sinc_resample_kernel(orig, new)
    kr, wr, orr, nr = RO.sinc_kernel(orig, new)
    assert (width, o, nw) == (wr, orr, nr) and k.shape == (nw, 2 * width + o)
    a, b = torch.from_numpy(k), kr[:, 0]
    ulp = torch.nextafter(b.abs(), torch.tensor(float("inf"))) - b.abs()
    assert bool(((a - b).abs() <= ulp).all())


@pytest.mark.parametrize("orig,new", RATES[:3])
def test_oracle_resampler_against_direct_float64(orig, new):
    """The oracle's conv1d formulation against a direct float64 sum of the same filters."""
    x = torch.from_numpy(np.random.default_rng(orig + new).standard_normal((2, 913)).astype(np.float32))
    y = RO.resample(x, orig, new)
    k, width, o, nw = ingest.sinc_resample_kernel(orig, new)
    n = x.shape[1]
    lout = math.ceil(nw * n / o)
    xp = np.pad(x.double().numpy(), ((0, 0), (width, width + o)))
    ref = np.zeros((2, lout))
    for j in range(lout):
        jj, kk = divmod(j, nw)
        ref[:, j] = xp[:, jj * o: jj * o + k.shape[1]] @ k[kk].astype(np.float64)
    assert y.shape == (2, lout)
    assert float(np.abs(y.double().numpy() - ref).max() / np.abs(ref).max()) < 1e-6


def test_oracle_resampler_passes_a_low_tone():
    t = np.arange(16000) / 16000.0
    x = torch.from_numpy(np.sin(2 * np.pi * 440 * t).astype(np.float32))[None]
    y = RO.resample(x, 16000, 24000)[0].double().numpy()
    ref = np.sin(2 * np.pi * 440 * np.arange(24000) / 24000.0)
    assert y.shape == (24000,)
    assert np.abs(y[600:-600] - ref[600:-600]).max() < 2e-3


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("orig,new", RATES)
@pytest.mark.parametrize("n", [1, 5, 3001, 16001])
def test_gpu_resampler_matches_oracle(dev, orig, new, n):
    x = torch.from_numpy(np.random.default_rng(n + orig).standard_normal((3, n)).astype(np.float32))
    ref = RO.resample(x, orig, new)
    y = ingest.Resampler.get(orig, new, dev)(x.to(dev)).cpu()
    assert y.shape == ref.shape
    err = float((y - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    assert err <= 2e-6, err


@pytest.mark.gpu
@pytest.mark.parametrize("duration,stride", [(None, 200), (0.9, None), (1.7, 200)])
def test_gpu_load_item_then_encode_matches_oracle(dev, tmp_path, duration, stride):
    """A 16 kHz PCM16 WAV through load_item (read -> trim/pad -> GPU resample -> pad to stride) and the
    encoder + VQ, against the oracle's load_libritts_item restatement and CPU encoder."""
    from helpers import assert_close_rel, build_models, index_mismatches, top2_gap, torch_sd
    from oracle import bigcodec_oracle as O

    rng = np.random.default_rng(11)
    t = np.arange(int(1.3 * 16000)) / 16000.0
    sig = 0.4 * np.sin(2 * np.pi * (200 + 900 * t) * t) + 0.05 * rng.standard_normal(t.size)
    path = tmp_path / "utt.wav"
    _pcm16_file(path, np.clip(np.round(sig * 32767), -32768, 32767))
    x, sr = ingest.load_item(str(path), 24000, duration=duration, pad_to_stride=stride, device=dev)
    xr, srr = RO.load_item(str(path), 24000, duration=duration, pad_to_stride=stride)
    assert sr == srr == 24000 and tuple(x.shape) == tuple(xr.shape)
    assert float((x.cpu() - xr).abs().max()) <= 2e-6 * float(xr.abs().max())
    enc, dec, esd, dsd, ek, _ = build_models("debug", device=dev)
    with torch.no_grad():
        lat = enc(x[None])
        codes = dec(lat, vq=True)[1].cpu()
        lat_ref = O.encoder_forward(xr[None], torch_sd(esd), ek)
        _, codes_ref, _ = O.rvq_forward(lat_ref, torch_sd(dsd))
        _, _, _, ze_ref = O.fvq_forward(lat_ref, torch_sd(dsd), "quantizer.layers.0.", return_ze=True)
    assert_close_rel(lat.cpu(), lat_ref, 1e-4, "latent of ingested audio")
    gap = top2_gap(ze_ref, torch.from_numpy(dsd["quantizer.layers.0._codebook.weight"]))
    n_bad, worst = index_mismatches(codes.numpy(), codes_ref.numpy(), gap)
    print(f"ingest duration={duration} stride={stride}: {n_bad} / {codes.numel()} index mismatches")
