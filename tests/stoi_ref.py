"""STOI (Taal, Hendriks, Heusdens, Jensen 2011: "An algorithm for intelligibility prediction of time-frequency weighted
noisy speech"), the non-extended measure as the pystoi package computes it, written out in float64 numpy + scipy.  This
file is the definition csrc/stoi.hip is held to; parity with the package itself is unpinned.

    resample to 10 kHz (polyphase, Octave-style Kaiser filter)  ->  drop the frames of the clean signal more than 40 dB
    below its loudest frame, rebuild both signals by overlap-add of their kept windowed frames  ->  STFT (256 / 128,
    n = 512)  ->  15 third-octave band magnitudes  ->  per 30-frame segment and band: scale, clip, centre, normalise,
    correlate  ->  the mean correlation.

Every stage takes `dtype`: float64 is the oracle, float32 the pipeline whose own error sets the GPU tolerance.
"""
from math import ceil, gcd

import numpy as np
import scipy.fft
import scipy.signal

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
NUM_BANDS = 15
MIN_FREQ = 150.0
N_SEG = 30
BETA = -15.0
DYN_RANGE = 40.0
EPS = np.finfo(float).eps
TOO_SHORT = 1e-5
# the half-open bin ranges of the 15 bands at FS / NFFT (band_ranges() recomputes them)
BANDS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87),
         (87, 109), (109, 138), (138, 174), (174, 219))


def window() -> np.ndarray:
    """The 256-point Hann window without its zero end points."""
    return np.hanning(N_FRAME + 2)[1:-1]


def band_ranges(fs: int = FS, nfft: int = NFFT, num_bands: int = NUM_BANDS, min_freq: float = MIN_FREQ):
    """Each band's [lo, hi) bins: the bins nearest to the band edges min_freq 2^((2k -+ 1) / 6)."""
    f = np.linspace(0, fs, nfft + 1)[:nfft // 2 + 1]
    k = np.arange(num_bands, dtype=np.float64)
    lo = min_freq * 2.0 ** ((2 * k - 1) / 6)
    hi = min_freq * 2.0 ** ((2 * k + 1) / 6)
    return tuple((int(np.argmin((f - a) ** 2)), int(np.argmin((f - b) ** 2))) for a, b in zip(lo, hi))


def band_matrix() -> np.ndarray:
    """(15, 257) 0 / 1 matrix of BANDS."""
    m = np.zeros((NUM_BANDS, NFFT // 2 + 1))
    for i, (a, b) in enumerate(BANDS):
        m[i, a:b] = 1.0
    return m


def resample_ratio(fs: int):
    """(p, q): FS / fs reduced."""
    g = gcd(FS, int(fs))
    return FS // g, int(fs) // g


def resample_filter(fs: int):
    """(h, p, q, L): the 2 L + 1 taps y[n] = sum_m x[m] h[q n - p m + L] runs over, i.e. resample_poly's `window` times
    p.  fc = 1 / (2 max(p, q)), L = ceil((60 - 8) / (28.714 fc / 10)), Kaiser beta = 0.1102 (60 - 8.7)."""
    p, q = resample_ratio(fs)
    fc = 1.0 / (2 * max(p, q))
    L = int(ceil((60.0 - 8.0) / (28.714 * fc / 10.0)))
    t = np.arange(-L, L + 1, dtype=np.float64)
    h = 2 * p * fc * np.sinc(2 * fc * t) * np.kaiser(2 * L + 1, 0.1102 * (60.0 - 8.7))
    return p * h / h.sum(), p, q, L


def resample(x: np.ndarray, fs: int, dtype=np.float64) -> np.ndarray:
    """x at fs -> 10 kHz, ceil(len p / q) samples (x itself at fs = 10000)."""
    x = np.asarray(x, dtype)
    if int(fs) == FS:
        return x
    h, p, q, _ = resample_filter(fs)
    return scipy.signal.resample_poly(x, p, q, window=(h / p).astype(dtype)).astype(dtype)


def resample_direct(x: np.ndarray, fs: int) -> np.ndarray:
    """The same written out: y[n] = sum_m x[m] h[q n - p m + L], n < ceil(len p / q), x zero outside the clip."""
    x = np.asarray(x, np.float64)
    h, p, q, L = resample_filter(fs)
    n_out = -(-len(x) * p // q)
    y = np.zeros(n_out)
    m = np.arange(len(x))
    for n in range(n_out):
        j = q * n - p * m + L
        ok = (j >= 0) & (j <= 2 * L)
        y[n] = np.dot(x[ok], h[j[ok]])
    return y


def _frames(x: np.ndarray, strict: bool) -> np.ndarray:
    """(frames, 256) at hop 128 while i + 256 <= len (strict: < len)."""
    last = len(x) - N_FRAME - (1 if strict else 0)
    if last < 0:
        return np.zeros((0, N_FRAME), x.dtype)
    starts = np.arange(0, last + 1, HOP)
    return x[starts[:, None] + np.arange(N_FRAME)[None, :]]


def remove_silent_frames(x: np.ndarray, y: np.ndarray, dtype=np.float64):
    """(x rebuilt, y rebuilt, info): frames of the clean x more than 40 dB below its loudest are dropped from both.
    info: frames, kept, margin_db (the smallest |max(e) - 40 - e| over the frames other than the loudest; inf when
    there is no other), the loudest frame's index and the kept frames' indices."""
    w = window().astype(dtype)
    xf, yf = _frames(x, False) * w, _frames(y, False) * w
    nf = len(xf)
    if nf == 0:
        return np.zeros(0, dtype), np.zeros(0, dtype), {"frames": 0, "kept": 0, "margin_db": np.inf, "loudest": -1,
                                                      "src": []}
    e = (20 * np.log10(np.linalg.norm(xf, axis=1) + dtype(EPS))).astype(dtype)
    t = (e.max() - dtype(DYN_RANGE) - e).astype(np.float64)
    mask = t < 0
    others = np.delete(np.abs(t), int(np.argmax(e)))
    xk, yk = xf[mask], yf[mask]
    K = len(xk)
    xs, ys = np.zeros((K - 1) * HOP + N_FRAME, dtype), np.zeros((K - 1) * HOP + N_FRAME, dtype)
    for i in range(K):
        xs[i * HOP:i * HOP + N_FRAME] += xk[i]
        ys[i * HOP:i * HOP + N_FRAME] += yk[i]
    info = {"frames": nf, "kept": K, "margin_db": float(others.min()) if len(others) else np.inf,
            "loudest": int(np.argmax(e)), "src": np.nonzero(mask)[0].tolist()}
    return xs, ys, info


def band_magnitudes(x: np.ndarray, dtype=np.float64) -> np.ndarray:
    """(15, STFT frames): sqrt of the band sums of |rfft(w frame, 512)|^2; K rebuilt frames give K - 1 columns."""
    fr = _frames(x, True) * window().astype(dtype)
    if len(fr) == 0:
        return np.zeros((NUM_BANDS, 0), dtype)
    spec = scipy.fft.rfft(fr.astype(dtype), n=NFFT, axis=1)
    power = (spec.real ** 2 + spec.imag ** 2).astype(dtype)
    return np.sqrt(band_matrix().astype(dtype) @ power.T).astype(dtype)


def segment_score(xb: np.ndarray, yb: np.ndarray, dtype=np.float64) -> float:
    """The mean over J = frames - 29 segments and 15 bands of the clipped, centred, normalised correlation."""
    S = xb.shape[1]
    if S < N_SEG:
        return TOO_SHORT
    J = S - N_SEG + 1
    idx = np.arange(J)[:, None] + np.arange(N_SEG)[None, :]
    xs = xb[:, idx].transpose(1, 0, 2).astype(dtype)  # (J, 15, 30)
    ys = yb[:, idx].transpose(1, 0, 2).astype(dtype)
    eps = dtype(EPS)
    c = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + eps)
    yp = np.minimum(ys * c, xs * dtype(1 + 10 ** (-BETA / 20)))
    yp = yp - yp.mean(axis=2, keepdims=True)
    xs = xs - xs.mean(axis=2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + eps)
    xs = xs / (np.linalg.norm(xs, axis=2, keepdims=True) + eps)
    return float(np.sum(yp * xs, dtype=dtype) / dtype(NUM_BANDS * J))


def stoi(x, y, fs: int = FS, dtype=np.float64, info: bool = False):
    """STOI of the processed y against the clean x (both 1-D, the same length, at fs).  info: also a dict with the
    frame count, the kept count, margin_db and the STFT frame count."""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError("stoi: two 1-D signals of the same length")
    xr, yr = resample(x, fs, dtype), resample(y, fs, dtype)
    xs, ys, inf = remove_silent_frames(xr, yr, dtype)
    xb, yb = band_magnitudes(xs, dtype), band_magnitudes(ys, dtype)
    inf["stft_frames"] = int(xb.shape[1])
    d = segment_score(xb, yb, dtype)
    return (d, inf) if info else d


def float32_error(x, y, fs: int = FS):
    """(float64 score, |float32 pipeline - float64|)."""
    want = stoi(x, y, fs)
    return want, abs(stoi(x, y, fs, dtype=np.float32) - want)
