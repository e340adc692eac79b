"""STOI on the host: the float64 oracle of tests/stoi_ref.py (the written definition csrc/stoi.hip is held to), the host
tables of audiotokenization_amd/metrics.py against it, the op's schema and fake kernel, the C ABI's argument checks and
the Python layer's refusals.  No GPU needed.  tests/test_gpu_stoi.py runs the kernels on the inputs built here.

Input conditions.  The one discrete decision of the measure is the silent-frame mask (a frame is dropped when it is more
than 40 dB below the loudest).  Every test clip keeps each frame's energy at least 0.05 dB away from that threshold
(test_input_conditions asserts it on the oracle; the clips here measure 2.3 dB and more), while the float32 energy error
is about 1e-5 dB, so the float64 reference, the float32 pipeline and the kernels decide every frame alike.
"""
import numpy as np
import pytest
import torch

import stoi_ref as R
from audiotokenization_amd import _lib as L
from audiotokenization_amd import metrics as M

MIN_MARGIN_DB = 0.05


def make_clip(n: int, fs: int, seed: int, gates=()) -> np.ndarray:
    """12 amplitude-modulated tones from 160 Hz to 4.2 kHz over a 1e-3 noise floor; gates: (t0, t1, gain) stretches in
    seconds (gain 0: exact zeros)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / fs
    f = 160.0 * (4200.0 / 160.0) ** (np.arange(12) / 11.0)
    x = np.zeros(n)
    for i in range(12):
        fm, ph, th = rng.uniform(2.0, 9.0), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
        x += (1.0 + 0.8 * np.sin(2 * np.pi * fm * t + ph)) * np.sin(2 * np.pi * f[i] * t + th) / (1.0 + 0.25 * i)
    x = 0.1 * x + 1e-3 * rng.standard_normal(n)
    for t0, t1, g in gates:
        x[(t >= t0) & (t < t1)] *= g
    return x


def add_noise(x: np.ndarray, snr_db: float, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    nz = rng.standard_normal(len(x))
    return x + nz * np.sqrt(np.mean(x ** 2) / np.mean(nz ** 2)) * 10 ** (-snr_db / 20)


# name -> (seed, gates): leading silence, a -50 dB stretch and a zero tail; one gap; no silence
SHAPES = {
    "gated": (101, ((0.0, 0.145, 1e-4), (0.45, 0.575, 3e-3), (0.87, 9.0, 0.0))),
    "gap": (102, ((0.30, 0.468, 1e-4),)),
    "plain": (103, ()),
    "plain2": (104, ()),
}
# per rate: T of the batch buffer and, per clip, (shape, samples, SNR dB, frames, frames kept)
CASES = {
    16000: {"T": 16000, "clips": (("gated", 16000, 20.0, 77, 50), ("gap", 11000, 0.0, 52, 41), ("plain", 7000, 20.0, 33, 33),
                                  ("plain2", 6554, 0.0, 31, 31))},
    10000: {"T": 10000, "clips": (("gated", 10000, 20.0, 77, 50), ("gap", 6875, 0.0, 52, 41), ("plain", 4375, 20.0, 33, 33),
                                  ("plain2", 4097, 0.0, 31, 31))},
}


def build_pair(shape: str, n: int, fs: int, snr_db: float):
    """(clean, processed) float32 arrays (the GPU's inputs; the oracle is given the same rounded values)."""
    seed, gates = SHAPES[shape]
    x = make_clip(n, fs, seed, gates)
    y = add_noise(x, snr_db, 1000 + seed)
    return x.astype(np.float32), y.astype(np.float32)


# edge clips at 16 kHz: name -> (samples, seed, gates, SNR dB, frames, frames kept).  short: 30 frames, 29 STFT frames;
# silenced: too short only after silence removal; k33 / k34: 32 and 33 STFT frames (the last tile of 16 owns 16, then 1);
# loud_last: the loudest frame is the last one; drop2: the first two frames are dropped
EDGE = {
    "short": (6552, 105, (), 10.0, 30, 30),
    "silenced": (8000, 106, ((0.20, 0.32, 1e-4),), 10.0, 38, 30),
    "k33": (7000, 103, (), 20.0, 33, 33),
    "k34": (7200, 107, (), 5.0, 34, 34),
    "loud_last": (9000, 108, ((0.5165, 9.0, 3.0),), 10.0, 42, 42),
    "drop2": (9000, 109, ((0.0, 0.0386, 1e-4),), 10.0, 42, 40),
}


def edge_pair(name: str):
    n, seed, gates, snr, _, _ = EDGE[name]
    x = make_clip(n, 16000, seed, gates)
    return x.astype(np.float32), add_noise(x, snr, 1000 + seed).astype(np.float32)


def make_batch(pairs, fs: int, T=None) -> dict:
    """A ragged batch of (clean, processed) float32 pairs with its oracle: clean / proc (B, T) float32 tensors (zeros
    beyond each clip), lens, and per clip the float64 score, the float32 pipeline's |error| and the oracle's info."""
    B, T = len(pairs), T or max(len(x) for x, _ in pairs)
    clean, proc = np.zeros((B, T), np.float32), np.zeros((B, T), np.float32)
    lens, want, f32_err, info = [], [], [], []
    for b, (x, y) in enumerate(pairs):
        n = len(x)
        clean[b, :n], proc[b, :n] = x, y
        d, inf = R.stoi(x.astype(np.float64), y.astype(np.float64), fs, info=True)
        lens.append(n)
        want.append(d)
        f32_err.append(abs(R.stoi(x, y, fs, dtype=np.float32) - d))
        info.append(inf)
    return {"clean": torch.from_numpy(clean), "proc": torch.from_numpy(proc), "lens": lens, "want": np.array(want),
            "f32_err": np.array(f32_err), "info": info}


_batches = {}


def batch_case(fs: int) -> dict:
    """make_batch of CASES[fs], computed once."""
    if fs not in _batches:
        spec = CASES[fs]
        _batches[fs] = make_batch([build_pair(shape, n, fs, snr) for shape, n, snr, _, _ in spec["clips"]], fs, spec["T"])
    return _batches[fs]


def edge_case(names) -> dict:
    """make_batch of the named EDGE clips (16 kHz), computed once."""
    key = tuple(names)
    if key not in _batches:
        _batches[key] = make_batch([edge_pair(n) for n in names], 16000)
    return _batches[key]


# ---- the oracle ---------------------------------------------------------------------------------------------------
def test_oracle_sanity():
    x = make_clip(12000, 16000, 5)
    assert R.stoi(x, x, 16000) > 1 - 1e-9
    scores = [R.stoi(x, add_noise(x, snr, 6), 16000) for snr in (40.0, 20.0, 5.0, -5.0)]
    print("stoi at 40 / 20 / 5 / -5 dB:", scores)
    assert all(a > b for a, b in zip(scores, scores[1:])) and scores[0] < 1.0 and scores[-1] > 0.0
    y = add_noise(x, 10.0, 7)
    assert abs(R.stoi(x, 7.0 * y, 16000) - R.stoi(x, y, 16000)) <= 1e-12
    assert R.band_ranges() == R.BANDS == ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43),
                                          (43, 55), (55, 69), (69, 87), (87, 109), (109, 138), (138, 174), (174, 219))
    assert R.stoi(x[:6552], x[:6552], 16000) == 1e-5  # 30 frames, 29 STFT frames


def test_oracle_resampler():
    h, p, q, half = R.resample_filter(16000)
    assert (p, q, half, len(h)) == (5, 8, 290, 581)
    rng = np.random.default_rng(0)
    for n in (1000, 1003, 37):
        x = rng.standard_normal(n)
        y = R.resample(x, 16000)
        assert len(y) == -(-5 * n // 8)
        np.testing.assert_allclose(R.resample_direct(x, 16000), y, rtol=0, atol=1e-12)
    x = rng.standard_normal(400)
    np.testing.assert_allclose(R.resample_direct(x, 8000), R.resample(x, 8000), rtol=0, atol=1e-12)  # 5 / 4: upsampling
    assert R.resample(x, 10000) is not None and len(R.resample(x, 10000)) == 400


def test_host_tables_equal_the_oracle():
    for fs in (16000, 8000, 48000):
        np.testing.assert_array_equal(M.stoi_resample_filter_f64(fs), R.resample_filter(fs)[0])
        assert M.stoi_resample_ratio(fs) == R.resample_ratio(fs)
    assert M.stoi_resample_ratio(10000) == (1, 1) and M.stoi_resample_filter_f64(10000).tolist() == [1.0]
    basis = M.stoi_basis_f64()
    assert basis.shape == (448, 256)
    # rows against rfft of the windowed unit impulses: X[r] of w e_n is w[n] exp(-2 pi i r n / 512)
    eye = np.eye(256) * R.window()[None, :]
    spec = np.fft.rfft(eye, n=512, axis=1).T  # (257, 256)
    np.testing.assert_allclose(basis[:224], spec.real[7:231], rtol=0, atol=1e-14)
    np.testing.assert_allclose(basis[224:], spec.imag[7:231], rtol=0, atol=1e-14)
    assert max(b for _, b in R.BANDS) <= 7 + 224 and min(a for a, _ in R.BANDS) == 7
    assert M.stoi_basis("cpu").dtype == torch.float32 and M.stoi_resample_filter(16000, "cpu").shape == (581,)


@pytest.mark.parametrize("fs", [16000, 10000])
def test_input_conditions(fs):
    """Every clip of the GPU tests: the expected frame and kept counts, a mask margin of at least 0.05 dB, and a float32
    pipeline that takes the same decisions (its kept count equals the float64 one)."""
    case = batch_case(fs)
    for (shape, n, snr, frames, kept), inf, d, e in zip(CASES[fs]["clips"], case["info"], case["want"], case["f32_err"]):
        print(f"fs {fs} {shape} {n}: stoi {d:.6f}, float32 pipeline error {e:.2e}, frames {inf['frames']}, kept "
              f"{inf['kept']}, margin {inf['margin_db']:.3f} dB")
        assert (inf["frames"], inf["kept"]) == (frames, kept)
        assert inf["stft_frames"] == kept - 1 >= 30
        assert inf["margin_db"] >= MIN_MARGIN_DB
        assert 0.3 < d < 1.0
    x, y = build_pair("gated", CASES[fs]["clips"][0][1], fs, 20.0)
    assert R.stoi(x, y, fs, dtype=np.float32, info=True)[1]["kept"] == case["info"][0]["kept"]


def test_edge_input_conditions():
    """The edge clips: frame and kept counts, the mask margin, and what each one is there for."""
    case = edge_case(tuple(EDGE))
    by = dict(zip(EDGE, case["info"]))
    for (name, (n, _, _, _, frames, kept)), inf, d in zip(EDGE.items(), case["info"], case["want"]):
        print(f"{name} {n}: stoi {d}, frames {inf['frames']}, kept {inf['kept']}, margin {inf['margin_db']:.3f} dB")
        assert (inf["frames"], inf["kept"], inf["stft_frames"]) == (frames, kept, kept - 1)
        assert inf["margin_db"] >= MIN_MARGIN_DB
        assert (d == 1e-5) == (kept - 1 < 30)
    assert by["loud_last"]["loudest"] == by["loud_last"]["frames"] - 1
    assert by["drop2"]["src"][:2] == [2, 3]


# ---- registry, ABI checks, refusals -------------------------------------------------------------------------------
def test_stoi_op_schema_and_fake():
    from audiotokenization_amd import ops

    ns = ops.load()
    assert "stoi" in ops.OPS
    assert str(ns.stoi.default._schema).startswith(
        "bigcodec::stoi(Tensor clean, Tensor proc, Tensor? lens, Tensor? filt, Tensor basis, int up, int down) -> "
        "(Tensor, Tensor)")
    m = lambda *s, dt=torch.float32: torch.empty(*s, device="meta", dtype=dt)  # noqa: E731
    score, kept = ns.stoi(m(3, 9000), m(3, 9000), m(3, dt=torch.int32), m(581), m(448, 256), 5, 8)
    assert score.shape == (3,) and score.dtype == torch.float32 and kept.shape == (3,) and kept.dtype == torch.int32
    score, kept = ns.stoi(m(3, 9000), m(3, 9000), None, None, m(448, 256), 1, 1)
    assert score.shape == (3,) and kept.dtype == torch.int32
    for name in ("bc_stoi", "bc_stoi_workspace_bytes"):
        assert name in L.EXPORTED
    assert L.ABI_VERSION == 18 and L.load().bc_abi_version() == 18


def test_stoi_abi_argument_checks():
    """Null pointers and non-positive sizes answer 1, a ratio or tap count the kernel is not built for 3, before
    anything is launched (the pointers here are not memory)."""
    lib = L.load()
    #     clean proc lens  filt up down half basis out kept ws  B  T     stream
    ok = [16, 16, None, 16, 5, 8, 290, 16, 16, 16, 16, 2, 9000, None]
    for i in (0, 1, 3, 7, 8, 9, 10):
        bad = list(ok)
        bad[i] = None
        assert lib.bc_stoi(*bad) == 1, i
    for i, v in ((4, 0), (4, -5), (5, 0), (5, -8), (6, 0), (6, -1), (11, 0), (11, -1), (12, 0), (12, -3)):
        bad = list(ok)
        bad[i] = v
        assert lib.bc_stoi(*bad) == 1, (i, v)
    for i in (7, 10):  # basis and workspace: 16-byte aligned
        bad = list(ok)
        bad[i] = 20
        assert lib.bc_stoi(*bad) == 1, i
    for up, down, half in ((100, 441, 290), (10, 16, 290), (5, 8, 2048), (65, 1, 10)):
        bad = list(ok)
        bad[4], bad[5], bad[6] = up, down, half
        assert lib.bc_stoi(*bad) == 3, (up, down, half)
    bad = list(ok)
    bad[11] = 70000  # more clips than one launch's grid holds
    assert lib.bc_stoi(*bad) == 3
    # no filter is needed at 10 kHz, but then the other pointers are still checked
    assert lib.bc_stoi(16, 16, None, None, 1, 1, 0, None, 16, 16, 16, 2, 9000, None) == 1
    assert lib.bc_stoi_workspace_bytes(0, 9000, 5, 8) == -1 and lib.bc_stoi_workspace_bytes(2, 0, 5, 8) == -1
    assert lib.bc_stoi_workspace_bytes(2, 9000, 100, 441) == -1 and lib.bc_stoi_workspace_bytes(2, 9000, 0, 8) == -1
    # 9000 samples at 16 kHz: 5625 at 10 kHz, 42 frames; samples of both signals, energies, kept list, band magnitudes
    up16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
    assert lib.bc_stoi_workspace_bytes(2, 9000, 5, 8) == (up16(2 * 2 * 5625 * 4) + up16(2 * 42 * 8) + up16(2 * 42 * 4)
                                                        + up16(2 * 2 * 15 * 42 * 4))
    assert lib.bc_stoi_workspace_bytes(2, 5625, 1, 1) == up16(2 * 42 * 8) + up16(2 * 42 * 4) + up16(2 * 2 * 15 * 42 * 4)
    assert lib.bc_stoi_workspace_bytes(1, 100, 1, 1) > 0  # no whole frame: still a valid (tiny) workspace


def test_stoi_python_layer_refusals():
    """Checked on the host before any launch, so CPU tensors get that far."""
    x = torch.zeros(2, 1, 9000)
    with pytest.raises(ValueError, match="differ in shape"):
        M.stoi(x, torch.zeros(2, 1, 8999), 16000)
    with pytest.raises(ValueError):
        M.stoi(x, x, 16000, lengths=[9000])  # one length for two clips
    with pytest.raises(ValueError):
        M.stoi(x, x, 16000, lengths=[9000, 9001])  # longer than the batch
    with pytest.raises(ValueError, match="empty clip"):
        M.stoi(x, x, 16000, lengths=[9000, 0])
    with pytest.raises(ValueError, match="not built for"):
        M.stoi(x, x, 44100)
    with pytest.raises(L.BigCodecLibraryError):
        M.stoi(x, x, 16000)  # CPU tensors: there is no CPU path
    with pytest.raises(ValueError, match="stoi_clean"):
        M.RoundTripMetrics(16000, 64, stoi=True, stoi_clean="x")
    with pytest.raises(ValueError, match="not built for"):
        M.RoundTripMetrics(44100, 64, stoi=True)
    m = M.RoundTripMetrics(16000, 64, stoi=True, stoi_clean="rec")
    with pytest.raises(ValueError):
        m.update(x, x, lengths=[9000])
    with pytest.raises(L.BigCodecLibraryError):
        m.update(x, x)
    assert m.clips == 0


def test_defaults_are_untouched():
    """STOI is opt-in: a default RoundTripMetrics has no STOI state, and any rate still constructs."""
    m = M.RoundTripMetrics(16000, 64)
    assert m.stoi is False and m._stoi_sums is None and m._stoi_ratio is None
    assert M.RoundTripMetrics(44100, 64).stoi is False
    import inspect

    from audiotokenization_amd.evaluate import evaluate_round_trip

    sig = inspect.signature(evaluate_round_trip)
    assert sig.parameters["stoi"].default is False and sig.parameters["stoi_clean"].default == "ref"

