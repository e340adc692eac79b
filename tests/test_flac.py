"""Host FLAC decoder (csrc/flac.cpp, bc_flac_decode) — the reference's input format (extract_indices.py:
98-106 reads LibriTTS / LibriSpeech .flac through soundfile).  No FLAC file, encoder or decoder exists in
this image or the reference, so every case is a lossless round trip through tests/flac_writer.py (an
independent RFC 9639 encoder that forces each feature): the decoded integers must equal the encoded ones
exactly, and the float32 read must equal int / 2^(bits - 1) (libsndfile's normalised read).  Parity with
libFLAC itself is unpinned; the one vector not written by this project's own encoder is RFC 9639's first example file
(test_rfc9639_example_file).  Damaged input is tests/test_flac_harness.py's subject.  CPU only (host code)."""
import hashlib
import struct

import numpy as np
import pytest

from audiotokenization_amd import _lib as L
from audiotokenization_amd import ingest
import flac_writer
from flac_writer import encode


def _signal(C, T, bps, seed, kind="speechy"):
    rng = np.random.default_rng(seed)
    lim = (1 << (bps - 1)) - 1
    if kind == "noise":
        x = rng.integers(-lim - 1, lim + 1, size=(C, T))
    else:  # smooth (predictable) + noise: exercises the predictors' residuals
        t = np.arange(T)
        base = np.sin(2 * np.pi * t * (0.013 + 0.004 * np.arange(C)[:, None])) * 0.6 * lim
        x = base + rng.normal(0, lim * 0.01, size=(C, T))
    return np.clip(np.round(x), -lim - 1, lim).astype(np.int64)


def _decode(data, as_int=True, check_crc=True, cap=None):
    lib = L.load()
    buf = np.frombuffer(data, np.uint8)
    rate, ch, bits, total = (ingest.ctypes_int(), ingest.ctypes_int(), ingest.ctypes_int(), ingest.ctypes_longlong())
    assert lib.bc_flac_info(buf.ctypes.data, len(data), ingest.ctypes_ref(rate), ingest.ctypes_ref(ch),
                            ingest.ctypes_ref(bits), ingest.ctypes_ref(total)) == 0
    cap = cap or max(int(total.value), 1)
    out = np.zeros((ch.value, cap), np.int32 if as_int else np.float32)
    n = lib.bc_flac_decode(buf.ctypes.data, len(data), out.ctypes.data, int(as_int), cap, int(check_crc))
    return n, out, rate.value, bits.value


KINDS = [dict(kind="verbatim")] + [dict(kind="fixed", order=o) for o in range(5)] + \
        [dict(kind="lpc", order=o, lpc_prec=p) for o, p in ((1, 12), (2, 15), (8, 12), (12, 14), (32, 10))]


@pytest.mark.parametrize("bps", [8, 16, 24])
@pytest.mark.parametrize("C", [1, 2])
def test_roundtrip_every_subframe_type(C, bps):
    T = 30000
    x = _signal(C, T, bps, seed=bps * 10 + C)
    plan_kinds = KINDS + [dict(kind="constant")]
    starts = np.cumsum([0] + [1152, 576, 4096, 192, 300, 4608, 1000] * 5)
    for fi in range(len(starts) - 1):  # constant blocks where the plan asks for CONSTANT subframes
        if any((fi * C + c) % len(plan_kinds) == len(plan_kinds) - 1 for c in range(C)):
            x[:, starts[fi]:starts[fi + 1]] = 7 - fi
    flac_writer.EMITTED.clear()

    def plan(fi, c):
        if fi == "stereo":
            return (1, 8, 9, 10)[c % 4]
        k = dict(plan_kinds[(fi * C + c) % len(plan_kinds)])
        k.update(porder=fi % 5, method=(fi + c) % 2, escape_parts=(1,) if fi % 3 == 0 else ())
        return k

    data = encode(x, 16000, bps, block_sizes=[1152, 576, 4096, 192, 300, 4608, 1000], plan=plan)
    n, out, rate, bits = _decode(data)
    assert (n, rate, bits) == (T, 16000, bps)
    np.testing.assert_array_equal(out.astype(np.int64), x)
    f, sr = ingest.read_flac("mem", data)
    assert sr == 16000 and f.dtype == np.float32 and f.shape == (C, T)
    np.testing.assert_array_equal(f, (x.astype(np.float64) / 2 ** (bps - 1)).astype(np.float32))
    kinds = {(k, o) for k, o, *_ in flac_writer.EMITTED}
    assert {("verbatim", 0), ("constant", 0)} | {("fixed", o) for o in range(5)} <= kinds, kinds
    assert {("lpc", o) for o in (1, 2, 8, 12, 32)} <= kinds, kinds
    assert any(e[2] for e in flac_writer.EMITTED) and {e[3] for e in flac_writer.EMITTED if e[0] == "lpc"} == {0, 1}


@pytest.mark.parametrize("assign", [1, 8, 9, 10])
def test_stereo_decorrelation_and_wasted_bits(assign):
    x = _signal(2, 5000, 16, seed=assign, kind="noise") // 8 * 8  # 3 wasted bits in every channel
    x[1] = np.clip(x[1] // 2 + x[0] // 2, -32768, 32760) // 8 * 8

    def plan(fi, c):
        if fi == "stereo":
            return assign
        return dict(kind=("fixed", "lpc", "verbatim")[fi % 3], order=(2, 6, 0)[fi % 3], wasted=3, porder=2)

    n, out, _, _ = _decode(encode(x, 44100, 16, block_sizes=[1024], plan=plan))
    assert n == 5000
    np.testing.assert_array_equal(out.astype(np.int64), x)


def test_header_codes_variable_blocks_and_unknown_length():
    """Sample-rate codes 12 / 13 / 0 (STREAMINFO), sample size 0 (STREAMINFO), variable block sizes (coded
    sample numbers up to several bytes), no extra metadata, total length unknown."""
    x = _signal(1, 70001, 16, seed=3)
    for rate, kw in ((12000, {}), (12345, {}), (16000, dict(rate_in_header=False, size_in_header=False))):
        data = encode(x, rate, 16, block_sizes=[4096, 333, 16384, 192], variable=True, extra_meta=False,
                      total_known=False, **kw)
        f, sr = ingest.read_flac("mem", data, as_int=True)
        assert sr == rate
        np.testing.assert_array_equal(f[0].astype(np.int64), x[0])


def test_corruption_is_detected():
    x = _signal(1, 3000, 16, seed=5)
    data = bytearray(encode(x, 16000, 16, block_sizes=[1024]))
    first = data.index(b"\xff\xf8")
    for off, want in ((first + 5, -4), (len(data) - 40, -4)):
        bad = bytearray(data)
        bad[off] ^= 0x10
        n, _, _, _ = _decode(bytes(bad))
        assert n in (want, -2), n  # CRC mismatch (or a corrupt field found first)
    n, _, _, _ = _decode(bytes(data[: len(data) - 100]))
    assert n < 0  # truncated stream
    n, _, _, _ = _decode(bytes(data), cap=100)
    assert n == -5  # output too small
    with pytest.raises(ValueError):
        ingest.read_flac("mem", b"fLaC\x00\x00")


def test_read_audio_dispatches_on_content(tmp_path):
    x = _signal(1, 2000, 16, seed=9)
    p = tmp_path / "a_0_0_0.flac"
    p.write_bytes(encode(x, 24000, 16, block_sizes=[4096]))
    y, sr = ingest.read_audio(str(p))
    assert sr == 24000
    np.testing.assert_array_equal(y[0], (x[0] / 32768.0).astype(np.float32))


# RFC 9639, appendix D.1 ("Decoding Example 1"): the whole 57-byte file as the RFC prints it.  STREAMINFO: block size
# 4096, 44 100 Hz, 2 channels, 16 bits, 1 sample, then the MD5 of the samples; one frame of two independent VERBATIM
# subframes with 2 and 4 wasted bits.
RFC9639_EXAMPLE_1 = bytes.fromhex(
    "664c6143 80000022 10001000 00000f00 000f0ac4 42f00000 00013e84 b41807dc"
    "69030758 6a3dad1a 2e0f fff86918 0000bf 0358fd 03128b aa9a".replace(" ", ""))


def test_rfc9639_example_file():
    data = RFC9639_EXAMPLE_1
    assert len(data) == 57
    for check_crc in (True, False):
        n, out, rate, bits = _decode(data, check_crc=check_crc)
        assert (n, rate, bits) == (1, 44100, 16) and out.shape == (2, 1)
        assert out[:, 0].tolist() == [25588, 10416]
    f, sr = ingest.read_flac("rfc", data)
    assert sr == 44100 and f.dtype == np.float32 and f.shape == (2, 1)
    np.testing.assert_array_equal(f[:, 0], np.array([25588 / 32768, 10416 / 32768], np.float32))
    i, sr = ingest.read_flac("rfc", data, as_int=True)
    assert i.dtype == np.int32 and i[:, 0].tolist() == [25588, 10416]
    # the stream's own MD5 (STREAMINFO's last 16 bytes) is over the interleaved little-endian samples
    assert hashlib.md5(struct.pack("<hh", *i[:, 0].tolist())).digest() == data[26:42]


@pytest.mark.parametrize("bps", [12, 20, 32])
@pytest.mark.parametrize("C", [1, 2, 8])
def test_roundtrip_more_sample_sizes_and_eight_channels(C, bps):
    """12 / 20 / 32-bit samples (32-bit stereo with a side channel makes 33-bit subframes) and 8 channels, every
    subframe kind, every assignment for C = 2; the noise rows reach both ends of the range."""
    T = 3000
    x = _signal(C, T, bps, seed=bps + C)
    x[-1] = _signal(1, T, bps, seed=bps, kind="noise")[0]
    x[0, :2] = (-(1 << (bps - 1)), (1 << (bps - 1)) - 1)
    flac_writer.EMITTED.clear()
    assigns = set()

    def plan(fi, c):
        if fi == "stereo":
            assigns.add((1, 8, 9, 10)[c % 4])
            return (1, 8, 9, 10)[c % 4]
        k = dict(KINDS[(fi * C + c) % len(KINDS)])
        k.update(porder=fi % 4, method=1)  # 5-bit Rice parameters: 32-bit noise needs parameters above 14
        return k

    data = encode(x, 48000, bps, block_sizes=[256, 100, 192, 576], plan=plan)
    n, out, rate, bits = _decode(data)
    assert (n, rate, bits) == (T, 48000, bps)
    np.testing.assert_array_equal(out.astype(np.int64), x)
    f, _ = ingest.read_flac("mem", data)
    np.testing.assert_array_equal(f, (x.astype(np.float64) / 2 ** (bps - 1)).astype(np.float32))
    kinds = {(k, o) for k, o, *_ in flac_writer.EMITTED}
    assert {("verbatim", 0)} | {("fixed", o) for o in range(5)} | {("lpc", o) for o in (1, 2, 8, 12, 32)} <= kinds
    assert C != 2 or assigns == {1, 8, 9, 10}


@pytest.mark.parametrize("bps", [8, 16, 24, 32])
@pytest.mark.parametrize("assign", [1, 8, 9, 10])
@pytest.mark.parametrize("phase", ["in", "anti"])
def test_full_scale_stereo(phase, assign, bps):
    """Alternating -2^(bps-1) / 2^(bps-1) - 1 in both channels, in phase and in anti-phase: the largest side channel
    (bps + 1 bits), the largest predictions and residuals of FIXED order 4 and of LPC order 8 with 15-bit coefficients.
    No sample of a losslessly encoded stream may trip the decoder's range checks."""
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    T = 4 * 96
    x = np.empty((2, T), np.int64)
    x[0] = np.where(np.arange(T) % 2 == 0, lo, hi)
    x[1] = x[0] if phase == "in" else np.where(np.arange(T) % 2 == 0, hi, lo)
    x[:, 200:260] = np.random.default_rng(bps).integers(lo, hi + 1, size=(2, 60))  # and an unpredictable stretch
    flac_writer.EMITTED.clear()

    def plan(fi, c):
        if fi == "stereo":
            return assign
        return (dict(kind="verbatim"), dict(kind="fixed", order=4, method=1), dict(kind="lpc", order=8, lpc_prec=15,
                method=1), dict(kind="fixed", order=1, method=1, porder=2))[(fi + c) % 4]

    data = encode(x, 44100, bps, block_sizes=[96], plan=plan)
    n, out, _, _ = _decode(data)
    assert n == T
    np.testing.assert_array_equal(out.astype(np.int64), x)
    assert {(k, o) for k, o, *_ in flac_writer.EMITTED} >= {("verbatim", 0), ("fixed", 4), ("lpc", 8), ("fixed", 1)}
    f, _ = ingest.read_flac("mem", data)
    np.testing.assert_array_equal(f, (x.astype(np.float64) / 2 ** (bps - 1)).astype(np.float32))


@pytest.mark.parametrize("sizes,T", [([16], 16 * 5 + 1), ([65535], 65535 + 1), ([65535, 16], 65535 + 16 + 1)])
def test_smallest_and_largest_blocks_and_a_last_block_of_one(sizes, T):
    """Block sizes 16 (the smallest a stream may announce) and 65 535 (the largest the 16-bit field of block-size code 7
    can hold), and a last block of a single sample."""
    x = _signal(1, T, 8, seed=T)
    data = encode(x, 8000, 8, block_sizes=sizes, plan=lambda fi, c: dict(kind="fixed", order=2, porder=0))
    n, out, _, _ = _decode(data)
    assert n == T
    np.testing.assert_array_equal(out.astype(np.int64), x)


@pytest.mark.parametrize("total_known", [True, False])
def test_trailing_tag_after_the_last_frame(total_known):
    """128 bytes that are no frame (an ID3v1 tag) after the last frame end the stream, with the total known or not."""
    x = _signal(2, 2500, 16, seed=21)
    tag = b"TAG" + bytes(range(125))
    data = encode(x, 22050, 16, block_sizes=[1024], total_known=total_known) + tag
    assert len(tag) == 128
    f, sr = ingest.read_flac("mem", data, as_int=True)
    assert sr == 22050 and f.shape == (2, 2500)
    np.testing.assert_array_equal(f.astype(np.int64), x)
