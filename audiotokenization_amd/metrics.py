"""Round-trip quality metrics on the GPU: what inference_full.py:570-604, 644-647, 723-737 reports
of a reconstruction -- SI-SNR and codebook perplexity -- plus the model's own spectral distance
(criterions/mel_loss.py MultiResolutionMelSpectrogramLoss), computed where the waveforms already are by the kernels
of csrc/metrics.hip (torch.ops.bigcodec.si_snr / logmel_l1 / code_hist_), and on request STOI (csrc/stoi.hip,
torch.ops.bigcodec.stoi).  PESQ is not computed.

    m = RoundTripMetrics(sample_rate=16000, codebook_size=8192)
    m.update(x, x_rec, lengths=lens, codes=codes[0], frame_lengths=frames)
    m.compute()   # {"si_snr", "mel_distance", "norm_perplexity", "raw_perplexity", "clips", "frames"}
    RoundTripMetrics(16000, 8192, stoi=True)   # compute() adds {"stoi", "stoi_short_clips"}
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import ops

N_MELS = (5, 10, 20, 40, 80, 160, 320)                 # criterions/mel_loss.py:13-14
WINDOW_LENGTHS = (32, 64, 128, 256, 512, 1024, 2048)
SI_SNR_EPS = 2.0 ** -23                                # torch.finfo(torch.float32).eps, what torchmetrics adds
STOI_FS = 10000                                        # the rate STOI is defined at
STOI_FRAME, STOI_NFFT = 256, 512
STOI_BIN0, STOI_ROWS = 7, 224                          # the basis holds bins 7 .. 230 (the 15 bands span 7 .. 218)
STOI_SEGMENT = 30                                      # STFT frames per segment; a clip with fewer scores 1e-5
STOI_MAX_RATIO, STOI_MAX_TAPS = 64, 4096               # what bc_stoi's resampler is built for

_cache = {}


def tile_frames() -> int:
    """Frames one workgroup of the log-mel kernel owns (bc_logmel_tile_frames)."""
    return int(L.load().bc_logmel_tile_frames())


def _hz_to_mel(f):
    """Slaney's mel scale (torchaudio.functional._hz_to_mel, mel_scale="slaney"): linear below 1 kHz, log above."""
    f = np.asarray(f, np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3.0, 1000.0, math.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_points(sample_rate: int, n_mels: int) -> np.ndarray:
    """The n_mels + 2 band edges in Hz, f_min = 0 to f_max = sample_rate // 2, equally spaced in Slaney mels."""
    return _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(float(sample_rate // 2)), n_mels + 2))


def mel_filterbank_f64(sample_rate: int, n_fft: int, n_mels: int) -> np.ndarray:
    """torchaudio.functional.melscale_fbanks(n_fft // 2 + 1, 0, sample_rate // 2, n_mels, sample_rate,
    norm="slaney", mel_scale="slaney"), transposed to (n_mels, bins), in float64: triangles between neighbouring
    band edges sampled at the bin frequencies, each scaled by 2 / (f_hi - f_lo).  A filter narrower than the bin
    spacing that no bin falls into is all zeros (n_fft = 32 with n_mels = 5 has some)."""
    if n_fft < 2 or n_mels < 1 or sample_rate < 2:
        raise ValueError("mel_filterbank: n_fft >= 2, n_mels >= 1, sample_rate >= 2")
    bins = n_fft // 2 + 1
    freqs = np.linspace(0.0, float(sample_rate // 2), bins)
    pts = mel_points(sample_rate, n_mels)
    diff = pts[1:] - pts[:-1]
    slopes = pts[None, :] - freqs[:, None]                  # (bins, n_mels + 2)
    down = -slopes[:, :-2] / diff[:-1]
    up = slopes[:, 2:] / diff[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    fb *= (2.0 / (pts[2:] - pts[:-2]))[None, :]
    return np.ascontiguousarray(fb.T)


def dft_basis_f64(n_fft: int) -> np.ndarray:
    """(2 * bins, n_fft) float64: row r < bins is w[n] cos(2 pi r n / n_fft), row bins + r is -w[n] sin(...), w the
    periodic Hann window -- the real and imaginary parts of rfft(w * frame).  The angle is reduced in integers."""
    if n_fft < 16 or n_fft % 16:
        raise ValueError("dft_basis: n_fft must be a multiple of 16")
    n = np.arange(n_fft, dtype=np.int64)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)
    r = np.arange(n_fft // 2 + 1, dtype=np.int64)
    ang = 2.0 * np.pi * ((r[:, None] * n[None, :]) % n_fft).astype(np.float64) / n_fft
    return np.concatenate([np.cos(ang) * w[None, :], -np.sin(ang) * w[None, :]], axis=0)


def _cached(key, device, make):
    device = torch.device(device)
    k = key + (str(device),)
    t = _cache.get(k)
    if t is None:
        t = _cache[k] = torch.from_numpy(make().astype(np.float32)).contiguous().to(device)
    return t


def mel_filterbank(sample_rate: int, n_fft: int, n_mels: int, device="cpu") -> torch.Tensor:
    """mel_filterbank_f64 cast once to float32 on `device` (cached per device)."""
    return _cached(("mel", int(sample_rate), int(n_fft), int(n_mels)), device,
                   lambda: mel_filterbank_f64(sample_rate, n_fft, n_mels))


def dft_basis(n_fft: int, device="cpu") -> torch.Tensor:
    """dft_basis_f64 cast once to float32 on `device` (cached per device)."""
    return _cached(("dft", int(n_fft)), device, lambda: dft_basis_f64(n_fft))


def stoi_resample_ratio(sample_rate: int):
    """(up, down) = 10000 / sample_rate, reduced (16 kHz: 5 / 8)."""
    if int(sample_rate) < 1:
        raise ValueError("stoi: sample_rate >= 1")
    g = math.gcd(STOI_FS, int(sample_rate))
    return STOI_FS // g, int(sample_rate) // g


def _stoi_half_len(up: int, down: int) -> int:
    """L of the resampling filter: ceil((60 - 8) / (28.714 fc / 10)), fc = 1 / (2 max(up, down))."""
    fc = 1.0 / (2 * max(up, down))
    return int(math.ceil((60.0 - 8.0) / (28.714 * fc / 10.0)))


def stoi_resample_filter_f64(sample_rate: int) -> np.ndarray:
    """The 2 L + 1 float64 taps h of y[n] = sum_m x[m] h[down n - up m + L] that bring sample_rate to 10 kHz:
    scipy.signal.resample_poly(x, up, down, window=g / g.sum()) with the Octave-style filter
    g[t] = 2 up fc sinc(2 fc t) kaiser(2 L + 1, 0.1102 (60 - 8.7)), t = -L .. L, fc = 1 / (2 max(up, down)),
    L = ceil((60 - 8) / (28.714 fc / 10)), so h = up g / g.sum() (16 kHz: L = 290, 581 taps).  [1.0] at 10 kHz."""
    up, down = stoi_resample_ratio(sample_rate)
    if up == down:
        return np.ones(1)
    fc, half = 1.0 / (2 * max(up, down)), _stoi_half_len(up, down)
    t = np.arange(-half, half + 1, dtype=np.float64)
    g = 2 * up * fc * np.sinc(2 * fc * t) * np.kaiser(2 * half + 1, 0.1102 * (60.0 - 8.7))
    return up * g / g.sum()


def stoi_basis_f64() -> np.ndarray:
    """(2 * 224, 256) float64: row r < 224 is w[n] cos(2 pi (7 + r) n / 512), row 224 + r is -w[n] sin(...), w the
    256-point Hann window without its zero end points (np.hanning(258)[1:-1]) -- the real and imaginary parts of bins
    7 .. 230 of rfft(w * frame, 512).  The angle is reduced in integers."""
    n = np.arange(STOI_FRAME, dtype=np.int64)
    w = np.hanning(STOI_FRAME + 2)[1:-1]
    r = STOI_BIN0 + np.arange(STOI_ROWS, dtype=np.int64)
    ang = 2.0 * np.pi * ((r[:, None] * n[None, :]) % STOI_NFFT).astype(np.float64) / STOI_NFFT
    return np.concatenate([np.cos(ang) * w[None, :], -np.sin(ang) * w[None, :]], axis=0)


def stoi_resample_filter(sample_rate: int, device="cpu") -> torch.Tensor:
    """stoi_resample_filter_f64 cast once to float32 on `device` (cached per device)."""
    return _cached(("stoi_filt", int(sample_rate)), device, lambda: stoi_resample_filter_f64(sample_rate))


def stoi_basis(device="cpu") -> torch.Tensor:
    """stoi_basis_f64 cast once to float32 on `device` (cached per device)."""
    return _cached(("stoi_basis",), device, stoi_basis_f64)


def _stoi_rate(sample_rate: int):
    """(up, down) of a rate bc_stoi's resampler is built for, or ValueError."""
    up, down = stoi_resample_ratio(sample_rate)
    if max(up, down) > STOI_MAX_RATIO or (up != down and 2 * _stoi_half_len(up, down) + 1 > STOI_MAX_TAPS):
        raise ValueError(f"stoi: the resampler is not built for {sample_rate} Hz -> 10 kHz ({up} / {down}: both at most "
                         f"{STOI_MAX_RATIO}, at most {STOI_MAX_TAPS} taps)")
    return up, down


def _stoi_op(clean, proc, ld, sample_rate: int, up: int, down: int):
    """(scores (B,) float32, kept frames (B,) int32) of torch.ops.bigcodec.stoi."""
    filt = None if up == down else stoi_resample_filter(sample_rate, clean.device)
    return ops.load().stoi(clean, proc, ld, filt, stoi_basis(clean.device), up, down)


def perplexity(counts, codebook_size: Optional[int] = None, total: Optional[int] = None):
    """inference_full.py:570-604 calculate_perplexity from a usage counter (counts[c] for c < codebook_size):
    (normalized, raw) = (exp(H / log(codebook_size)), exp(H)), H the entropy of counts / total.  total defaults to
    counts.sum(); the reference divides by the sum over ALL its counter's keys, the ones it then ignores included, so
    a caller that kept those passes their sum in `total`.  An empty counter gives (0.0, 0.0) (the reference: 0.0)."""
    c = np.asarray(counts.cpu() if isinstance(counts, torch.Tensor) else counts, dtype=np.float64).reshape(-1)
    size = int(codebook_size) if codebook_size is not None else c.size
    if c.size != size:
        raise ValueError(f"perplexity: {c.size} counts for a codebook of {size}")
    total = float(c.sum()) if total is None else float(total)
    if total == 0:
        return 0.0, 0.0
    probs = c / total
    nz = probs[probs > 0]
    entropy = -np.sum(nz * np.log(nz))
    return float(np.exp(entropy / np.log(size))), float(np.exp(entropy))


def _pair(ref, rec):
    if not isinstance(ref, torch.Tensor) or not isinstance(rec, torch.Tensor):
        raise ValueError("metrics: ref and rec must be tensors")
    if ref.shape != rec.shape:
        raise ValueError(f"metrics: ref {tuple(ref.shape)} and rec {tuple(rec.shape)} differ in shape")
    if ref.dim() == 3:
        if ref.shape[1] != 1:
            raise ValueError(f"metrics: (B, 1, T) or (B, T) waveforms, got {tuple(ref.shape)}")
        ref, rec = ref[:, 0], rec[:, 0]
    if ref.dim() != 2 or ref.shape[0] < 1 or ref.shape[1] < 1:
        raise ValueError(f"metrics: (B, 1, T) or (B, T) waveforms, got {tuple(ref.shape)}")
    return ref.float().contiguous(), rec.float().contiguous()


def _need_device(*tensors) -> None:
    """(after the argument checks, so a refusal does not depend on where the tensors live)"""
    if not all(t.is_cuda for t in tensors):
        raise L.BigCodecLibraryError("metrics take device tensors (there is no CPU path)")


def _lengths(lengths, B: int, T: int, what: str):
    """(list of B ints, int32 device tensor or None)."""
    if lengths is None:
        return [T] * B, None
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.reshape(-1).tolist()  # (a device tensor costs a synchronisation: pass a list)
    lens = [int(v) for v in lengths]
    if len(lens) != B:
        raise ValueError(f"{what}: {len(lens)} entries for a batch of {B} clips")
    if min(lens) < 0 or max(lens) > T:
        raise ValueError(f"{what}: every length must lie in [0, {T}], got {lens}")
    return lens, lens


def si_snr(ref, rec, lengths=None) -> torch.Tensor:
    """(B,) SI-SNR in dB of rec against ref over each clip's own first lengths[b] samples (bc_si_snr)."""
    ref, rec = _pair(ref, rec)
    lens, given = _lengths(lengths, ref.shape[0], ref.shape[1], "si_snr lengths")
    if min(lens) < 1:
        raise ValueError("si_snr: an empty clip has no SI-SNR")
    _need_device(ref, rec)
    ld = None if given is None else torch.tensor(lens, dtype=torch.int32).to(ref.device, non_blocking=True)
    return ops.load().si_snr(ref, rec, ld)


def logmel_l1(ref, rec, sample_rate: int, n_fft: int, n_mels: int, lengths=None, clamp_eps: float = 1e-5) -> torch.Tensor:
    """(B,) per-clip mean |log10 mel(ref) - log10 mel(rec)| at one resolution (bc_logmel_l1)."""
    ref, rec = _pair(ref, rec)
    lens, given = _lengths(lengths, ref.shape[0], ref.shape[1], "logmel_l1 lengths")
    if min(lens) < n_fft // 2 + 1:
        raise ValueError(f"logmel_l1: a clip of {min(lens)} samples is shorter than n_fft / 2 + 1 = {n_fft // 2 + 1}: "
                         f"reflect padding is undefined")
    _need_device(ref, rec)
    ld = None if given is None else torch.tensor(lens, dtype=torch.int32).to(ref.device, non_blocking=True)
    return ops.load().logmel_l1(ref, rec, ld, dft_basis(n_fft, ref.device), mel_filterbank(sample_rate, n_fft, n_mels, ref.device),
                                n_fft, float(clamp_eps))


def stoi(clean, processed, sample_rate: int, lengths=None) -> torch.Tensor:
    """(B,) STOI of `processed` against `clean` over each clip's own first lengths[b] samples (bc_stoi; the definition
    is tests/stoi_ref.py).  The measure is asymmetric: the clean signal decides which frames are silent and bounds the
    clipping.  A clip that keeps fewer than 31 frames (30 STFT frames) scores 1e-5."""
    clean, processed = _pair(clean, processed)
    lens, given = _lengths(lengths, clean.shape[0], clean.shape[1], "stoi lengths")
    if min(lens) < 1:
        raise ValueError("stoi: an empty clip has no STOI")
    up, down = _stoi_rate(sample_rate)
    _need_device(clean, processed)
    ld = None if given is None else torch.tensor(lens, dtype=torch.int32).to(clean.device, non_blocking=True)
    return _stoi_op(clean, processed, ld, sample_rate, up, down)[0]


class RoundTripMetrics:
    """Running round-trip metrics of (reference, reconstruction) batches; the defaults are criterions/mel_loss.py's.
    update() launches the kernels and keeps the sums on the device (no host synchronisation); compute() reads them.
    stoi=True adds STOI (off by default: a clip under about 0.41 s keeps fewer than 30 STFT frames and scores 1e-5).
    STOI is asymmetric; stoi_clean says which signal is the clean one: "ref" (the standard order, what
    lightning_module.py:427 feeds torchmetrics) or "rec" (inference_full.py:724, which passes the reconstruction as
    pystoi's clean signal)."""

    def __init__(self, sample_rate: int, codebook_size: int, n_mels: Sequence[int] = N_MELS,
                 window_lengths: Sequence[int] = WINDOW_LENGTHS, clamp_eps: float = 1e-5, stoi: bool = False,
                 stoi_clean: str = "ref"):
        if len(n_mels) != len(window_lengths) or not len(n_mels):
            raise ValueError("RoundTripMetrics: one n_mels per window length")
        if codebook_size < 1:
            raise ValueError("RoundTripMetrics: codebook_size >= 1")
        self.sample_rate, self.codebook_size = int(sample_rate), int(codebook_size)
        self.n_mels, self.window_lengths = tuple(int(v) for v in n_mels), tuple(int(v) for v in window_lengths)
        self.clamp_eps = float(clamp_eps)
        self.min_samples = max(self.window_lengths) // 2 + 1
        if stoi_clean not in ("ref", "rec"):
            raise ValueError(f"RoundTripMetrics: stoi_clean must be \"ref\" or \"rec\", got {stoi_clean!r}")
        self.stoi, self.stoi_clean = bool(stoi), stoi_clean
        self._stoi_ratio = _stoi_rate(self.sample_rate) if self.stoi else None
        self.reset()

    def reset(self) -> None:
        self._sums = None      # device float64 [si_snr sum, mel_distance sum]
        self._stoi_sums = None  # device float64 [stoi sum, clips that scored 1e-5] (stoi=True)
        self._counts = None    # device int64 [codebook_size]
        self._last = None
        self.clips = 0
        self.frames = 0

    def update(self, ref, rec, lengths=None, codes=None, frame_lengths=None) -> None:
        """ref, rec: (B, 1, T) or (B, T) device waveforms; lengths: each clip's own samples (a list or CPU tensor).
        codes: (B, F) or (Nq, B, F) int32 / int64 device codes with frame_lengths (frames per clip), counted into the
        usage histogram."""
        ref, rec = _pair(ref, rec)
        B, T = ref.shape
        lens, given = _lengths(lengths, B, T, "RoundTripMetrics lengths")
        if min(lens) < self.min_samples:
            raise ValueError(f"RoundTripMetrics: a clip of {min(lens)} samples is shorter than the {self.min_samples} "
                             f"that reflect padding at n_fft = {max(self.window_lengths)} needs")
        if codes is not None:
            if not isinstance(codes, torch.Tensor) or codes.dim() not in (2, 3) or codes.shape[-2] != B:
                raise ValueError(f"RoundTripMetrics: codes must be (B, F) or (Nq, B, F) with B = {B}")
        elif frame_lengths is not None:
            raise ValueError("RoundTripMetrics: frame_lengths without codes")
        _need_device(*((ref, rec) if codes is None else (ref, rec, codes)))
        ns = ops.load()
        ld = None if given is None else torch.tensor(lens, dtype=torch.int32).to(ref.device, non_blocking=True)
        snr = ns.si_snr(ref, rec, ld)
        mel = None
        for n_fft, nm in zip(self.window_lengths, self.n_mels):
            d = ns.logmel_l1(ref, rec, ld, dft_basis(n_fft, ref.device),
                             mel_filterbank(self.sample_rate, n_fft, nm, ref.device), n_fft, self.clamp_eps)
            mel = d if mel is None else mel + d
        if self._sums is None:
            self._sums = torch.zeros(2, dtype=torch.float64, device=ref.device)
        self._sums += torch.stack([snr.double().sum(), mel.double().sum()])
        self._last = {"si_snr": snr, "mel_distance": mel}
        if self.stoi:
            clean, proc = (ref, rec) if self.stoi_clean == "ref" else (rec, ref)
            score, kept = _stoi_op(clean, proc, ld, self.sample_rate, *self._stoi_ratio)
            if self._stoi_sums is None:
                self._stoi_sums = torch.zeros(2, dtype=torch.float64, device=ref.device)
            self._stoi_sums += torch.stack([score.double().sum(), (kept <= STOI_SEGMENT).double().sum()])
            self._last["stoi"] = score
        self.clips += B
        if codes is not None:
            F = codes.shape[-1]
            fl, fgiven = _lengths(frame_lengths, B, F, "RoundTripMetrics frame_lengths")
            fd = None if fgiven is None else torch.tensor(fl, dtype=torch.int32).to(ref.device, non_blocking=True)
            if self._counts is None:
                self._counts = torch.zeros(self.codebook_size, dtype=torch.int64, device=ref.device)
            for layer in (codes.unsqueeze(0) if codes.dim() == 2 else codes):
                ns.code_hist_(self._counts, layer.contiguous(), fd)
            self.frames += sum(fl)

    def per_clip(self) -> dict:
        """The last update's (B,) device vectors {"si_snr", "mel_distance"} (and "stoi" with stoi=True)."""
        if self._last is None:
            raise RuntimeError("RoundTripMetrics.per_clip() before update()")
        return dict(self._last)

    def counts(self) -> np.ndarray:
        """The usage histogram so far, int64 [codebook_size] on the host."""
        if self._counts is None:
            return np.zeros(self.codebook_size, np.int64)
        return self._counts.cpu().numpy()

    def compute(self) -> dict:
        """Means over the clips seen (synchronises): mel_distance is the mean over clips of the sum over resolutions of
        the clip's own mean, which for equal-length clips is MultiResolutionMelSpectrogramLoss.forward."""
        if self.clips == 0:
            raise RuntimeError("RoundTripMetrics.compute() before update()")
        s = self._sums.cpu().tolist()
        norm, raw = perplexity(self.counts(), self.codebook_size)
        out = {"si_snr": s[0] / self.clips, "mel_distance": s[1] / self.clips, "norm_perplexity": norm,
               "raw_perplexity": raw, "clips": self.clips, "frames": self.frames}
        if self.stoi:  # the mean over clips, and how many of them were too short for a score (each counted as 1e-5)
            t = self._stoi_sums.cpu().tolist()
            out["stoi"], out["stoi_short_clips"] = t[0] / self.clips, int(t[1])
        return out
