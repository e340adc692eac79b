"""Round-trip metrics, host side (no GPU): the float64 oracle the GPU tests compare against (torch.stft in float64,
a mel filterbank recomputed from Slaney's formulas, per-clip slicing), the host-built constants of
audiotokenization_amd/metrics.py, perplexity against a fixture recorded from the reference's calculate_perplexity
(tools/make_golden_perplexity.py), the op registry, the ABI argument checks and the Python layer's refusals.

Tolerances of tests/test_gpu_metrics.py, measured on the CPU by measured_bounds() below on that file's inputs
(seed 7; B = 4, T = 5000 for SI-SNR; B = 3, T = 4133 for the log-mel distance, sample rate 16000):
  SI-SNR: |float32 formula with float64 accumulation of the residual - float64| per clip
          = 6.6e-07, 7.2e-07, 6.9e-06, 9.4e-06 dB at 5, 30, 60, 80 dB; bound = min(4 x 9.36e-06, 0.01) = 3.7e-05 dB
          (SI_SNR_BOUND_DB).
  log-mel L1: |float32 torch.stft pipeline - float64|, the largest of the three clips, per resolution (n_fft 32 ...
          2048) = 2.0e-08, 3.4e-08, 4.2e-08, 1.3e-07, 9.2e-08, 8.0e-08, 4.5e-08 on values of 0.01 ... 1.3; the GPU test
          recomputes them from its inputs (float32_logmel_error) and allows 4 x; DESIGN.md section 16 records them.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from audiotokenization_amd import _lib as L
from audiotokenization_amd import metrics as M

SAMPLE_RATE = 16000
RESOLUTIONS = tuple(zip(M.WINDOW_LENGTHS, M.N_MELS))
SI_SNR_BOUND_DB = 3.7e-5
EPS = 2.0 ** -23


# ---- the float64 oracle -------------------------------------------------------------------------------------------
def slaney_hz_to_mel(f: float) -> float:
    return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / (math.log(6.4) / 27.0)


def slaney_mel_to_hz(m: float) -> float:
    return m * (200.0 / 3.0) if m < 15.0 else 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0))


def oracle_band_edges(sample_rate: int, n_mels: int):
    lo, hi = slaney_hz_to_mel(0.0), slaney_hz_to_mel(float(sample_rate // 2))
    return [slaney_mel_to_hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]


def oracle_mel_filterbank(sample_rate: int, n_fft: int, n_mels: int) -> np.ndarray:
    """(n_mels, bins) float64, written from the definition: filter m is the triangle over (f[m], f[m+1], f[m+2]) of
    height 2 / (f[m+2] - f[m]), sampled at the bin frequencies k (sample_rate // 2) / (bins - 1)."""
    bins = n_fft // 2 + 1
    f = oracle_band_edges(sample_rate, n_mels)
    fb = np.zeros((n_mels, bins))
    for m in range(n_mels):
        lo, c, hi = f[m], f[m + 1], f[m + 2]
        for k in range(bins):
            fk = k * float(sample_rate // 2) / (bins - 1)
            fb[m, k] = max(0.0, min((fk - lo) / (c - lo), (hi - fk) / (hi - c))) * 2.0 / (hi - lo)
    return fb


def _logmel(x: torch.Tensor, fb: torch.Tensor, n_fft: int, eps: float) -> torch.Tensor:
    win = torch.hann_window(n_fft, periodic=True, dtype=x.dtype)
    spec = torch.stft(x, n_fft, hop_length=n_fft // 4, window=win, center=True, pad_mode="reflect",
                      return_complex=True).abs()
    return (fb @ spec).clamp(min=eps).log10()


def oracle_logmel_l1(ref, rec, lens, sample_rate, n_fft, n_mels, eps=1e-5, dtype=torch.float64) -> np.ndarray:
    """Per clip: mean |log10 clamp(mel(ref)) - log10 clamp(mel(rec))| over the clip's own first lens[b] samples
    (float32: the same pipeline in float32, for the tolerance)."""
    fb = torch.from_numpy(oracle_mel_filterbank(sample_rate, n_fft, n_mels)).to(dtype)
    out = []
    for b, n in enumerate(lens):
        r, c = (torch.as_tensor(v[b]).reshape(-1)[:n].cpu().to(dtype) for v in (ref, rec))
        out.append(float((_logmel(r, fb, n_fft, eps) - _logmel(c, fb, n_fft, eps)).abs().double().mean()))
    return np.array(out)


def float32_logmel_error(ref, rec, lens, sample_rate, n_fft, n_mels, eps=1e-5):
    """(float64 oracle values, max |float32 pipeline - float64| over the clips): the reference's own error."""
    want = oracle_logmel_l1(ref, rec, lens, sample_rate, n_fft, n_mels, eps)
    f32 = oracle_logmel_l1(ref, rec, lens, sample_rate, n_fft, n_mels, eps, dtype=torch.float32)
    return want, float(np.abs(f32 - want).max())


def oracle_si_snr(ref, rec, lens) -> np.ndarray:
    out = []
    for b, n in enumerate(lens):
        t, p = (torch.as_tensor(v[b]).reshape(-1)[:n].cpu().double() for v in (ref, rec))
        t, p = t - t.mean(), p - p.mean()
        alpha = ((p * t).sum() + EPS) / ((t * t).sum() + EPS)
        s = alpha * t
        out.append(float(10.0 * torch.log10(((s * s).sum() + EPS) / (((s - p) ** 2).sum() + EPS))))
    return np.array(out)


def float32_si_snr(ref, rec, lens) -> np.ndarray:
    """The same formula in float32, the residual energy (and the signal's) accumulated in float64."""
    out = []
    for b, n in enumerate(lens):
        t, p = (torch.as_tensor(v[b]).reshape(-1)[:n].cpu().float() for v in (ref, rec))
        t, p = t - t.mean(), p - p.mean()
        eps = torch.tensor(EPS, dtype=torch.float32)
        alpha = ((p * t).sum() + eps) / ((t * t).sum() + eps)
        s = alpha * t
        num, den = (s * s).double().sum() + EPS, ((s - p) ** 2).double().sum() + EPS
        out.append(float(10.0 * torch.log10(num / den)))
    return np.array(out)


def make_signals(B: int, T: int, seed: int, snr_db, dc=None):
    """Seeded (ref, rec) float32 (B, T): ref = five sinusoids (80 Hz - 7 kHz) + a -40 dB noise floor, rec = ref + white
    noise at snr_db[b] below the signal (+ dc[b])."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / SAMPLE_RATE
    ref = np.zeros((B, T))
    rec = np.zeros((B, T))
    for b in range(B):
        f = rng.uniform(80.0, 7000.0, 5)
        a = rng.uniform(0.05, 0.4, 5)
        ph = rng.uniform(0, 2 * np.pi, 5)
        x = (a[:, None] * np.sin(2 * np.pi * f[:, None] * t[None, :] + ph[:, None])).sum(0) + 0.003 * rng.standard_normal(T)
        ref[b] = x
        rec[b] = x + x.std() * 10.0 ** (-snr_db[b] / 20.0) * rng.standard_normal(T) + (dc[b] if dc else 0.0)
    return torch.from_numpy(ref.astype(np.float32)), torch.from_numpy(rec.astype(np.float32))


SNR_CASE = dict(B=4, T=5000, lens=[5000, 4999, 1025, 3001], snr_db=[5.0, 30.0, 60.0, 80.0], dc=[0.0, 0.0, 0.5, 0.0])
MEL_CASE = dict(B=3, T=4133, lens=[4133, 2049, 1025], snr_db=[10.0, 25.0, 40.0])


def measured_bounds():
    """The figures of this module's header (python tests/test_metrics_host.py prints them)."""
    ref, rec = make_signals(SNR_CASE["B"], SNR_CASE["T"], 7, SNR_CASE["snr_db"], SNR_CASE["dc"])
    want = oracle_si_snr(ref, rec, SNR_CASE["lens"])
    err = np.abs(float32_si_snr(ref, rec, SNR_CASE["lens"]) - want)
    print("si_snr float64", want, "float32 error", err, "bound", min(4 * err.max(), 0.01))
    ref, rec = make_signals(MEL_CASE["B"], MEL_CASE["T"], 7, MEL_CASE["snr_db"])
    for n_fft, n_mels in RESOLUTIONS:
        want, e = float32_logmel_error(ref, rec, MEL_CASE["lens"], SAMPLE_RATE, n_fft, n_mels)
        print(f"logmel n_fft {n_fft} n_mels {n_mels}: float64 {want}, float32 error {e:.3e}")


# ---- host-built constants -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,n_mels", RESOLUTIONS)
def test_mel_filterbank_properties(n_fft, n_mels):
    fb = M.mel_filterbank_f64(SAMPLE_RATE, n_fft, n_mels)
    bins = n_fft // 2 + 1
    assert fb.shape == (n_mels, bins) and fb.dtype == np.float64
    assert (fb >= 0).all()
    np.testing.assert_allclose(fb, oracle_mel_filterbank(SAMPLE_RATE, n_fft, n_mels), rtol=1e-12, atol=1e-13)
    # each filter is the triangle of height 2 / (f_hi - f_lo) over (f_lo, f_hi): its area is
    # 2 / (f_hi - f_lo) * (f_hi - f_lo) / 2 = 1; no sample exceeds the height, and where the bins are dense (at
    # least 32 inside the band) the sampled area agrees
    edges = np.array(oracle_band_edges(SAMPLE_RATE, n_mels))
    np.testing.assert_allclose(M.mel_points(SAMPLE_RATE, n_mels), edges, rtol=1e-12)
    height = 2.0 / (edges[2:] - edges[:-2])
    np.testing.assert_allclose(height * (edges[2:] - edges[:-2]) / 2.0, 1.0, rtol=1e-15)
    assert (fb <= height[:, None] * (1 + 1e-12)).all()
    df = (SAMPLE_RATE // 2) / (bins - 1)
    dense = (edges[2:] - edges[:-2]) >= 32 * df
    if dense.any():
        np.testing.assert_allclose(fb[dense].sum(1) * df, 1.0, rtol=2e-3)
    t = M.mel_filterbank(SAMPLE_RATE, n_fft, n_mels)
    assert t.dtype == torch.float32 and t.shape == (n_mels, bins) and t.is_contiguous()
    assert t is M.mel_filterbank(SAMPLE_RATE, n_fft, n_mels)  # cached
    assert torch.equal(t, torch.from_numpy(fb.astype(np.float32)))


def test_mel_filterbank_all_zero_filters():
    """A band narrower than the bin spacing (500 Hz at n_fft = 32) that no bin falls into is a row of exact zeros
    (both signals then clamp to eps and contribute 0): the rows that are zero are the oracle's, at n_fft = 32 with
    n_mels = 5 (at 16 kHz every band there catches a bin) and with n_mels = 40, where most of the low bands do not."""
    for n_mels, expect_zero_rows in ((5, False), (40, True)):
        fb = M.mel_filterbank_f64(SAMPLE_RATE, 32, n_mels)
        zero = ~(fb > 0).any(1)
        assert zero.any() == expect_zero_rows and not zero.all(), zero
        assert np.array_equal(zero, ~(oracle_mel_filterbank(SAMPLE_RATE, 32, n_mels) > 0).any(1))
        assert np.isfinite(fb).all() and (fb[zero] == 0).all()
    with pytest.raises(ValueError):
        M.mel_filterbank_f64(SAMPLE_RATE, 32, 0)


@pytest.mark.parametrize("n_fft", [32, 256, 2048])
def test_dft_basis_is_rfft_of_a_windowed_impulse(n_fft):
    basis = M.dft_basis_f64(n_fft)
    bins = n_fft // 2 + 1
    assert basis.shape == (2 * bins, n_fft)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    for n in sorted({0, 1, 5, n_fft // 4 + 1, n_fft // 2, n_fft - 1}):
        imp = np.zeros(n_fft)
        imp[n] = 1.0
        want = np.fft.rfft(win * imp)
        np.testing.assert_allclose(basis[:bins, n], want.real, atol=1e-14)
        np.testing.assert_allclose(basis[bins:, n], want.imag, atol=1e-14)
    t = M.dft_basis(n_fft)
    assert t.dtype == torch.float32 and t.shape == (2 * bins, n_fft) and t is M.dft_basis(n_fft)
    with pytest.raises(ValueError):
        M.dft_basis_f64(40)


def test_oracle_pipeline_equals_the_basis_and_filterbank():
    """The two host-built matrices applied to reflect-padded frames give the oracle's log-mel distance (float64):
    the constants and the frame rule (frames = 1 + len // hop, reflect at the clip's own ends) are the stft's."""
    ref, rec = make_signals(1, 700, 3, [20.0])
    n_fft, n_mels, n = 128, 20, 650
    hop = n_fft // 4
    basis, fb = M.dft_basis_f64(n_fft), M.mel_filterbank_f64(SAMPLE_RATE, n_fft, n_mels)
    bins = n_fft // 2 + 1
    logs = []
    for x in (ref, rec):
        v = np.pad(x[0, :n].double().numpy(), n_fft // 2, mode="reflect")
        frames = np.stack([v[f * hop:f * hop + n_fft] for f in range(1 + n // hop)], 1)
        s = basis @ frames
        logs.append(np.log10(np.maximum(fb @ np.hypot(s[:bins], s[bins:]), 1e-5)))
    got = np.abs(logs[0] - logs[1]).mean()
    np.testing.assert_allclose(got, oracle_logmel_l1(ref, rec, [n], SAMPLE_RATE, n_fft, n_mels)[0], rtol=1e-10)


# ---- perplexity ---------------------------------------------------------------------------------------------------
def test_perplexity_equals_the_reference_fixture(golden):
    g = golden("perplexity_cases.npz")
    size = int(g["codebook_size"])
    for name in ("uniform", "onehot", "skewed"):
        counts, total, want = g[name + "_counts"], int(g[name + "_total"]), g[name + "_expected"]
        got = M.perplexity(counts, size, total=total)
        np.testing.assert_allclose(got, want, rtol=1e-12, err_msg=name)
    assert int(g["skewed_total"]) > int(g["skewed_counts"].sum())  # the fixture has out-of-range keys
    np.testing.assert_allclose(M.perplexity(g["uniform_counts"]), (math.e, float(size)), rtol=1e-12)
    assert M.perplexity(np.zeros(size, np.int64)) == (0.0, 0.0)
    assert M.perplexity(torch.from_numpy(g["onehot_counts"])) == (1.0, 1.0)
    with pytest.raises(ValueError):
        M.perplexity(np.zeros(5), 6)


# ---- registry, ABI checks, refusals -------------------------------------------------------------------------------
def test_metric_ops_schemas_and_fakes():
    from audiotokenization_amd import ops

    ns = ops.load()
    for name in ("si_snr", "logmel_l1", "code_hist_"):
        assert name in ops.OPS
    assert str(ns.si_snr.default._schema).startswith("bigcodec::si_snr(Tensor ref, Tensor rec, Tensor? lens) -> Tensor")
    assert str(ns.logmel_l1.default._schema).startswith(
        "bigcodec::logmel_l1(Tensor ref, Tensor rec, Tensor? lens, Tensor basis, Tensor mel, int n_fft, float clamp_eps)")
    assert str(ns.code_hist_.default._schema).startswith(
        "bigcodec::code_hist_(Tensor(a!) counts, Tensor codes, Tensor? lens) -> ()")
    m = lambda *s, dt=torch.float32: torch.empty(*s, device="meta", dtype=dt)  # noqa: E731
    lens = m(3, dt=torch.int32)
    out = ns.si_snr(m(3, 500), m(3, 500), lens)
    assert out.shape == (3,) and out.dtype == torch.float32
    out = ns.logmel_l1(m(3, 500), m(3, 500), None, m(34, 32), m(5, 17), 32, 1e-5)
    assert out.shape == (3,) and out.dtype == torch.float32
    assert ns.code_hist_(m(64, dt=torch.int64), m(3, 9, dt=torch.int64), lens) is None


def test_metric_abi_argument_checks():
    """Null pointers and non-positive sizes answer 1 (bad argument) before anything is launched."""
    lib = L.load()
    assert L.ABI_VERSION == 18
    for name in ("bc_si_snr", "bc_logmel_l1", "bc_code_hist", "bc_logmel_tile_frames", "bc_logmel_workspace_doubles"):
        assert name in L.EXPORTED
    assert lib.bc_si_snr(None, 1, None, 1, 1, 8, None) == 1
    assert lib.bc_si_snr(1, None, None, 1, 1, 8, None) == 1
    assert lib.bc_si_snr(1, 1, None, None, 1, 8, None) == 1
    for B, T in ((0, 8), (-1, 8), (1, 0), (1, -3)):
        assert lib.bc_si_snr(1, 1, None, 1, B, T, None) == 1
    eps = ctypes.c_float(1e-5)
    ok = [16, 16, None, 16, 16, 16, 16, 2, 4000, 64, 10, eps, None]  # (pointers: non-null and 16-byte aligned)
    for i in (0, 1, 3, 4, 5, 6):
        bad = list(ok)
        bad[i] = None
        assert lib.bc_logmel_l1(*bad) == 1, i
    for i, v in ((7, 0), (7, -2), (8, 0), (8, -1), (9, 0), (9, -64), (9, 40), (10, 0), (10, -1)):
        bad = list(ok)
        bad[i] = v
        assert lib.bc_logmel_l1(*bad) == 1, (i, v)
    bad = list(ok)
    bad[11] = ctypes.c_float(0.0)
    assert lib.bc_logmel_l1(*bad) == 1
    bad = list(ok)
    bad[3] = 20  # a basis that is not 16-byte aligned
    assert lib.bc_logmel_l1(*bad) == 1
    bad = list(ok)
    bad[10] = 321  # more mel bands than the kernel's tiles hold: unsupported
    assert lib.bc_logmel_l1(*bad) == 3
    assert lib.bc_logmel_tile_frames() == M.tile_frames() == 16
    assert lib.bc_logmel_workspace_doubles(2, 4000, 64) == 2 * -(-(1 + 4000 // 16) // 16)
    assert lib.bc_logmel_workspace_doubles(0, 4000, 64) == -1 and lib.bc_logmel_workspace_doubles(2, 4000, 40) == -1
    assert lib.bc_code_hist(None, 64, None, 1, 1, 8, 64, None) == 1
    assert lib.bc_code_hist(1, 64, None, None, 1, 8, 64, None) == 1
    assert lib.bc_code_hist(1, 16, None, 1, 1, 8, 64, None) == 1  # code width
    for B, T, K in ((0, 8, 64), (1, 0, 64), (1, 8, 0), (-1, 8, 64), (1, 8, -4)):
        assert lib.bc_code_hist(1, 64, None, 1, B, T, K, None) == 1
    assert lib.bc_code_hist(1, 64, None, 1, 1, 8, 1 << 20, None) == 3  # a codebook the LDS histogram cannot hold


def test_python_layer_refusals():
    """Shape mismatches and clips shorter than n_fft / 2 + 1 of the largest resolution raise ValueError on the host,
    before any launch (so CPU tensors get that far)."""
    m = M.RoundTripMetrics(SAMPLE_RATE, 64)
    assert m.min_samples == 1025
    x = torch.zeros(2, 1, 3000)
    with pytest.raises(ValueError, match="differ in shape"):
        m.update(x, torch.zeros(2, 1, 2999))
    with pytest.raises(ValueError, match="differ in shape"):
        M.si_snr(torch.zeros(2, 100), torch.zeros(3, 100))
    with pytest.raises(ValueError):
        m.update(torch.zeros(2, 2, 3000), torch.zeros(2, 2, 3000))
    with pytest.raises(L.BigCodecLibraryError):
        m.update(x, x)  # CPU tensors: there is no CPU path
    with pytest.raises(ValueError):
        M.RoundTripMetrics(SAMPLE_RATE, 64, n_mels=(5, 10), window_lengths=(32,))
    with pytest.raises(RuntimeError):
        m.compute()
    with pytest.raises(ValueError, match="shorter than the 1025"):
        m.update(x, x, lengths=[3000, 1024])
    with pytest.raises(ValueError, match="shorter than the 1025"):
        m.update(torch.zeros(1, 1000), torch.zeros(1, 1000))
    with pytest.raises(ValueError, match="n_fft / 2 \\+ 1 = 129"):
        M.logmel_l1(torch.zeros(1, 128), torch.zeros(1, 128), SAMPLE_RATE, 256, 40)
    with pytest.raises(ValueError):
        m.update(x, x, lengths=[3000])  # one length for two clips
    with pytest.raises(ValueError):
        m.update(x, x, lengths=[3000, 3001])  # longer than the batch
    with pytest.raises(ValueError):
        m.update(x, x, codes=torch.zeros(3, 5, dtype=torch.int64))  # codes of another batch size
    with pytest.raises(ValueError):
        m.update(x, x, frame_lengths=[1, 1])
    assert m.clips == 0


if __name__ == "__main__":
    measured_bounds()
