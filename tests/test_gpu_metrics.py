"""Round-trip metrics on the GPU (csrc/metrics.hip, audiotokenization_amd/metrics.py, evaluate.py) against the float64
oracle of tests/test_metrics_host.py; that module's header states how the tolerances were measured.

Measured on an MI355X, GPU |error| against float64 per resolution n_fft 32 ... 2048 (test_logmel_l1_vs_oracle prints
them next to the float32 torch.stft pipeline's own error, of which 4 x is allowed): see DESIGN.md section 16.
"""
import json
import wave

import numpy as np
import pytest
import torch

from audiotokenization_amd import metrics as M
from test_metrics_host import (MEL_CASE, RESOLUTIONS, SAMPLE_RATE, SI_SNR_BOUND_DB, SNR_CASE, float32_logmel_error,
                               make_signals, oracle_si_snr)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def snr_case():
    ref, rec = make_signals(SNR_CASE["B"], SNR_CASE["T"], 7, SNR_CASE["snr_db"], SNR_CASE["dc"])
    return ref, rec, SNR_CASE["lens"], oracle_si_snr(ref, rec, SNR_CASE["lens"])


@pytest.fixture(scope="module")
def mel_case():
    ref, rec = make_signals(MEL_CASE["B"], MEL_CASE["T"], 7, MEL_CASE["snr_db"])
    return ref, rec, MEL_CASE["lens"]


def test_si_snr_vs_oracle(dev, snr_case):
    """5, 30, 60 and 80 dB (the row a single-pass float32 expansion of the residual loses), ragged lengths, a DC
    offset of 0.5 on the 60 dB clip's reconstruction."""
    ref, rec, lens, want = snr_case
    assert np.all(np.abs(want - np.array(SNR_CASE["snr_db"])) < 1.0), want
    got = M.si_snr(ref.to(dev), rec.to(dev), lens).cpu().double().numpy()
    err = np.abs(got - want)
    print("si_snr float64", want, "GPU", got, "|error| dB", err, "bound", SI_SNR_BOUND_DB)
    assert (err <= SI_SNR_BOUND_DB).all(), (got, want, err)
    # (B, 1, T) input and no lengths: every clip over the whole row
    full = M.si_snr(ref.to(dev).unsqueeze(1), rec.to(dev).unsqueeze(1)).cpu().double().numpy()
    assert (np.abs(full - oracle_si_snr(ref, rec, [ref.shape[1]] * ref.shape[0])) <= SI_SNR_BOUND_DB).all()


@pytest.mark.parametrize("n_fft,n_mels", RESOLUTIONS + ((32, 40),))
def test_logmel_l1_vs_oracle(dev, mel_case, n_fft, n_mels):
    """Every resolution of mel_loss.py (and n_fft = 32 with 40 bands, most of them all-zero filters) on lengths that
    are no multiple of any hop, one above a power of two, and the minimum for n_fft = 2048 (both reflect regions
    overlap most of the clip), within 4 x the float32 torch.stft pipeline's own error against float64."""
    ref, rec, lens = mel_case
    want, f32_err = float32_logmel_error(ref, rec, lens, SAMPLE_RATE, n_fft, n_mels)
    got = M.logmel_l1(ref.to(dev), rec.to(dev), SAMPLE_RATE, n_fft, n_mels, lengths=lens).cpu().double().numpy()
    err = np.abs(got - want)
    print(f"logmel n_fft {n_fft} n_mels {n_mels}: float64 {want}, GPU |error| {err}, float32 pipeline error "
          f"{f32_err:.3e}, bound {4 * f32_err:.3e}")
    assert np.isfinite(got).all() and (want > 1e-3).all()
    assert (err <= 4 * f32_err).all(), (n_fft, got, want, err, 4 * f32_err)


@pytest.mark.parametrize("n_fft,n_mels", [(64, 10), (512, 80)])
def test_logmel_l1_at_a_tile_boundary(dev, n_fft, n_mels):
    """T = 3 tile_frames hop + 1: frames = 3 tile_frames + 1, so the last workgroup of the clip owns one frame; a
    second clip one hop shorter ends exactly at the boundary (frames = 3 tile_frames)."""
    tf, hop = M.tile_frames(), n_fft // 4
    T = 3 * tf * hop + 1
    lens = [T, T - hop - 1]
    assert [1 + n // hop for n in lens] == [3 * tf + 1, 3 * tf]
    ref, rec = make_signals(2, T, 11, [15.0, 35.0])
    want, f32_err = float32_logmel_error(ref, rec, lens, SAMPLE_RATE, n_fft, n_mels)
    got = M.logmel_l1(ref.to(dev), rec.to(dev), SAMPLE_RATE, n_fft, n_mels, lengths=lens).cpu().double().numpy()
    err = np.abs(got - want)
    print(f"tile boundary n_fft {n_fft}: GPU |error| {err}, bound {4 * f32_err:.3e}")
    assert (err <= 4 * f32_err).all(), (got, want, err, 4 * f32_err)


def _all_metrics(ref, rec, lens):
    out = [M.si_snr(ref, rec, lens)]
    out += [M.logmel_l1(ref, rec, SAMPLE_RATE, n_fft, n_mels, lengths=lens) for n_fft, n_mels in RESOLUTIONS]
    return torch.stack(out).cpu()


def test_tails_are_not_read(dev, mel_case):
    """NaN beyond each clip's own length in both signals changes no bit of any result."""
    ref, rec, lens = mel_case
    clean = _all_metrics(ref.to(dev), rec.to(dev), lens)
    r2, c2 = ref.clone(), rec.clone()
    for b, n in enumerate(lens):
        r2[b, n:] = float("nan")
        c2[b, n:] = float("nan")
    dirty = _all_metrics(r2.to(dev), c2.to(dev), lens)
    assert torch.isfinite(clean).all()
    assert torch.equal(clean.view(torch.int32), dirty.view(torch.int32))


def test_a_clip_in_a_batch_equals_the_clip_alone(dev, mel_case):
    ref, rec, lens = mel_case
    batch = _all_metrics(ref.to(dev), rec.to(dev), lens)
    for b, n in enumerate(lens):
        alone = _all_metrics(ref[b:b + 1, :n].contiguous().to(dev), rec[b:b + 1, :n].contiguous().to(dev), [n])
        assert torch.equal(alone[:, 0].view(torch.int32), batch[:, b].view(torch.int32)), (b, alone[:, 0], batch[:, b])


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_code_hist(dev, dtype):
    from audiotokenization_amd import ops

    ns = ops.load()
    size, B, F = 64, 5, 37
    rng = np.random.default_rng(5)
    codes = rng.integers(0, size, (B, F))
    codes[0, 3], codes[1, 0], codes[2, 36], codes[4, 10] = size, -1, 10 * size, -7  # ignored
    lens = [37, 36, 37, 1, 20]
    want = np.zeros(size, np.int64)
    for b in range(B):
        row = codes[b, :lens[b]]
        want += np.bincount(row[(row >= 0) & (row < size)], minlength=size)
    counts = torch.zeros(size, dtype=torch.int64, device=dev)
    cd = torch.from_numpy(codes).to(dtype).to(dev)
    ld = torch.tensor(lens, dtype=torch.int32, device=dev)
    ns.code_hist_(counts, cd, ld)
    assert np.array_equal(counts.cpu().numpy(), want)
    ns.code_hist_(counts, cd, ld)  # a second update accumulates
    assert np.array_equal(counts.cpu().numpy(), 2 * want)
    full = torch.zeros(size, dtype=torch.int64, device=dev)
    ns.code_hist_(full, cd, None)
    flat = codes.reshape(-1)
    assert np.array_equal(full.cpu().numpy(), np.bincount(flat[(flat >= 0) & (flat < size)], minlength=size))


def test_ops_refuse_bad_arguments(dev):
    from audiotokenization_amd import ops

    ns = ops.load()
    x = torch.zeros(2, 3000, device=dev)
    lens = torch.tensor([3000, 2000], dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        ns.si_snr(x, x[:, :2999].contiguous(), lens)
    with pytest.raises(ValueError):
        ns.si_snr(x, x, lens[:1])
    with pytest.raises(RuntimeError):
        ns.si_snr(x, x, lens.long())
    with pytest.raises(ValueError):
        ns.logmel_l1(x, x, lens, M.dft_basis(64, dev), M.mel_filterbank(SAMPLE_RATE, 32, 5, dev), 64, 1e-5)
    with pytest.raises(ValueError):
        ns.logmel_l1(x, x, lens, M.dft_basis(64, dev), M.mel_filterbank(SAMPLE_RATE, 64, 10, dev), 64, 0.0)
    with pytest.raises(ValueError):
        ns.code_hist_(torch.zeros(8, dtype=torch.int64, device=dev), torch.zeros(2, 3, 4, dtype=torch.int64, device=dev), None)
    with pytest.raises(ValueError, match="shorter than"):
        M.logmel_l1(x, x, SAMPLE_RATE, 2048, 320, lengths=[3000, 1024])


def _debug_lm(dev):
    from audiotokenization_amd.config import preset
    from audiotokenization_amd.lightning_shim import CodecLightningModule
    from helpers import synth_load

    lm = CodecLightningModule(preset("debug"))
    synth_load(lm.encoder, "encoder.")
    synth_load(lm.decoder, "decoder.")
    return lm.eval().to(dev)


def _mel_distance_oracle(ref, rec, lens):
    """(per-clip float64 sum over the resolutions, bound): the bound is the sum over the resolutions of 4 x the float32
    torch.stft pipeline's own error on these inputs, the per-resolution tolerance of test_logmel_l1_vs_oracle."""
    total, bound = np.zeros(len(lens)), 0.0
    for n_fft, n_mels in RESOLUTIONS:
        want, f32_err = float32_logmel_error(ref, rec, lens, SAMPLE_RATE, n_fft, n_mels)
        total += want
        bound += 4 * f32_err
    return total, bound


def test_round_trip_metrics_on_the_debug_preset(dev):
    """evaluate_round_trip on three ragged clips: compute() equals the oracle applied to the very waveforms and codes
    the device produced (recomputed here by the same ragged round trip), and per_file rows carry each clip's values."""
    from audiotokenization_amd.evaluate import evaluate_round_trip
    from audiotokenization_amd.extract import BigCodecModel

    lm = _debug_lm(dev)
    size = lm.cfg.model.codec_decoder.codebook_size
    ref, _ = make_signals(3, 4800, 21, [20.0, 20.0, 20.0])
    lens = [4800, 3999, 2561]
    clips = [ref[b, :n].clone() for b, n in enumerate(lens)]
    got = evaluate_round_trip(lm, clips, batch=4, sample_rate=SAMPLE_RATE, per_file=True)
    assert {"si_snr", "mel_distance", "norm_perplexity", "raw_perplexity", "clips", "frames", "files"} <= set(got)
    # the same round trip by hand (plan_batches sorts by length: one group of three, shortest first)
    order = sorted(range(3), key=lambda i: lens[i])
    x = torch.zeros(3, 1, max(lens), device=dev)
    for b, i in enumerate(order):
        x[b, 0, :lens[i]] = clips[i].to(dev)
    slens = [lens[i] for i in order]
    out = BigCodecModel(lm, reconstruct=True)(x, lengths=slens)
    frames = [int(f) for f in out["frames"]]
    own = [min(a, b) for a, b in zip(slens, lm.decoder.sample_lengths(frames))]
    codes = out["indices"].cpu().numpy()
    counts = np.zeros(size, np.int64)
    for b, f in enumerate(frames):
        counts += np.bincount(codes[:, b, :f].reshape(-1), minlength=size)
    xr, xc = x[:, 0].cpu(), out["x_rec"][:, 0].cpu()
    snr = oracle_si_snr(xr, xc, own).mean()
    mel, mel_bound = _mel_distance_oracle(xr, xc, own)
    print("round trip", {k: v for k, v in got.items() if k != "files"}, "oracle si_snr", snr, "mel_distance", mel.mean(),
          "mel bound", mel_bound)
    assert got["clips"] == 3 and got["frames"] == sum(frames)
    assert abs(got["si_snr"] - snr) <= SI_SNR_BOUND_DB
    assert abs(got["mel_distance"] - mel.mean()) <= mel_bound
    assert (got["norm_perplexity"], got["raw_perplexity"]) == M.perplexity(counts, size)
    rows = got["files"]
    assert [r["index"] for r in rows] == [0, 1, 2] and [r["samples"] for r in rows] == [own[order.index(i)] for i in range(3)]
    assert abs(np.mean([r["si_snr"] for r in rows]) - got["si_snr"]) < 1e-5


def test_mel_distance_of_equal_lengths_is_the_batch_mean_loss(dev):
    """Equal-length clips: mel_distance equals MultiResolutionMelSpectrogramLoss.forward in its batch-mean form, the
    sum over resolutions of the L1 mean over the whole (B, n_mels, frames) tensor (float64 oracle)."""
    from test_metrics_host import _logmel, oracle_mel_filterbank

    ref, rec = make_signals(3, 3000, 31, [8.0, 18.0, 28.0])
    m = M.RoundTripMetrics(SAMPLE_RATE, 64)
    m.update(ref.unsqueeze(1).to(dev), rec.unsqueeze(1).to(dev))
    loss, (_, bound) = 0.0, _mel_distance_oracle(ref, rec, [3000] * 3)
    for n_fft, n_mels in RESOLUTIONS:
        fb = torch.from_numpy(oracle_mel_filterbank(SAMPLE_RATE, n_fft, n_mels))
        loss += float((_logmel(ref.double(), fb, n_fft, 1e-5) - _logmel(rec.double(), fb, n_fft, 1e-5)).abs().mean())
    got = m.compute()
    print("mel_distance", got["mel_distance"], "batch-mean loss", loss, "bound", bound)
    assert abs(got["mel_distance"] - loss) <= bound
    assert got["clips"] == 3 and got["frames"] == 0 and got["raw_perplexity"] == 0.0
    pc = m.per_clip()
    assert pc["si_snr"].shape == (3,) and pc["mel_distance"].shape == (3,)
    m.reset()
    assert m.clips == 0


def test_cli_smoke(tmp_path, dev, capsys):
    """python -m audiotokenization_amd.evaluate's main() over three seeded WAV files in a LibriTTS-style tree."""
    import yaml

    from audiotokenization_amd import config as cfgmod
    from audiotokenization_amd.evaluate import main
    from helpers import build_models

    rng = np.random.default_rng(2)
    base = tmp_path / "LibriTTS" / "test-clean"
    for i, n in enumerate((4000, 5200, 3100)):
        d = base / "100" / str(2000 + i)
        d.mkdir(parents=True)
        t = np.arange(n) / SAMPLE_RATE
        x = 6000 * np.sin(2 * np.pi * (200 + 150 * i) * t) + rng.normal(0, 800, n)
        with wave.open(str(d / f"100_{2000 + i}_000000_00000{i}.wav"), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(SAMPLE_RATE)
            w.writeframes(np.clip(x, -32768, 32767).astype("<i2").tobytes())
    sp = tmp_path / "run"
    (sp / "hydra").mkdir(parents=True)
    (sp / "pl_log").mkdir()
    cfg = cfgmod.preset("debug")
    with open(sp / "hydra" / "config.yaml", "w") as fh:
        yaml.safe_dump({"model": {k: dict(v) for k, v in cfg.model.items()}}, fh)
    _, _, esd, dsd, *_ = build_models("debug")
    sd = {**{"encoder." + k: torch.from_numpy(v) for k, v in esd.items()},
          **{"decoder." + k: torch.from_numpy(v) for k, v in dsd.items()}}
    torch.save({"state_dict": sd}, sp / "pl_log" / "last.ckpt")
    out = tmp_path / "metrics.json"
    rc = main(["--dataset_root", str(tmp_path), "--save_path", str(sp), "--subsets", "test-clean", "--ext_audio", ".wav",
               "--sample_rate", str(SAMPLE_RATE), "--batch", "4", "--per_file", "--json", str(out)])
    assert rc == 0
    got = json.loads(out.read_text())
    assert {"si_snr", "mel_distance", "norm_perplexity", "raw_perplexity", "clips", "frames"} <= set(got)
    assert got["clips"] == 3 and len(got["files"]) == 3 and np.isfinite(got["si_snr"]) and np.isfinite(got["mel_distance"])
    assert got["frames"] > 0 and 1.0 <= got["raw_perplexity"] <= got["frames"]
